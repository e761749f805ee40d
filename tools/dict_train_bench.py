#!/usr/bin/env python3
"""Dictionary training on one MI355X: 16384 sample messages of 1 KiB and of 4 KiB from the
quality corpus (tests/dicttrainmodel.py corpus(), seed 1), a dictionary of 61440 bytes, segments
of 64 and 256 bytes.  Per case, in one process:

  train     ms of one dict_train call (median of --reps by HIP events around the whole call,
            with min and max; its launches are not timed apart), bytes used and picks; and ms
            of the same call into a dictionary of ONE segment, which counts the same samples
            and scores every slot once, as the full call does, in 5 launches instead of 3 + 2 E
  ratio     of compress_usingCDict and of compress_hc_usingCDict at depth 8 on 16384 HELD-OUT
            messages (seed 2) with the trained dictionary, with the head-of-the-samples
            dictionary of the same size, and without a dictionary (compress_batch; the
            high-ratio call on an empty prepared dictionary)

Message 0 of every output is decoded by the host's decompress_safe_usingDict with the dictionary
it was compressed against.  The corpus takes about a minute to generate, so it is kept as .npy
files under --corpus-dir and loaded from there when present.  Each case runs in a child process
of its own under a time limit; the first failure ends the run.  Prints one JSON line per case
and writes profiles/dict_train.json (--out).
usage: dict_train_bench.py [--reps 5] [--messages 16384] [--out FILE] [--corpus-dir DIR]
                           [--case NAME]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DD = 61440
CASES = {"msg1KiB": 1024, "msg4KiB": 4096}
SEGMENTS = (64, 256)
DEPTH = 8
CASE_TIMEOUT = 400   # seconds per child


def times_ms(torch, fn, reps):
    ts = []
    for _ in range(reps + 1):   # (the first call warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts[1:])


def corpus_rows(np, corpus_dir, nb, L, seed):
    """corpus(nb, L, seed) as a [nb, L] uint8 array, kept under corpus_dir."""
    import dicttrainmodel as M
    path = os.path.join(corpus_dir, "corpus_%dx%d_seed%d.npy" % (nb, L, seed))
    if os.path.exists(path):
        rows = np.load(path)
        assert rows.shape == (nb, L) and rows.dtype == np.uint8, path
        return rows
    rows = np.frombuffer(b"".join(M.corpus(nb, L, seed)), dtype=np.uint8).reshape(nb, L).copy()
    os.makedirs(corpus_dir, exist_ok=True)
    np.save(path, rows)
    return rows


def run_case(name, reps, nb, corpus_dir):
    import numpy as np
    import torch
    import libapenetwork_amd as amd
    L = CASES[name]
    total = nb * L
    samples = torch.from_numpy(corpus_rows(np, corpus_dir, nb, L, 1)).cuda()
    held_rows = corpus_rows(np, corpus_dir, nb, L, 2)
    held = torch.from_numpy(held_rows).cuda()
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    sizes = i32([L] * nb)
    tptr = i64([samples.data_ptr() + i * L for i in range(nb)])
    hptr = i64([held.data_ptr() + i * L for i in range(nb)])
    bound = amd.compressBound(L)
    slot = (bound + 15) // 16 * 16
    out = torch.empty((nb, slot), dtype=torch.uint8, device="cuda")
    dptr = i64([out.data_ptr() + i * slot for i in range(nb)])
    caps, res = i32([bound] * nb), i32([0] * nb)
    obj = torch.empty(amd.cdict_size(), dtype=torch.uint8, device="cuda")
    hobj = torch.empty(amd.hc_cdict_size(), dtype=torch.uint8, device="cuda")
    hscratch = torch.empty(amd.compress_hc_cdict_scratch_size(nb, L), dtype=torch.uint8,
                           device="cuda")
    dec = amd.lib().APE_LZ4_decompress_safe_usingDict
    dec.restype, dec.argtypes = C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int]

    def ratio(dict_host):
        rs = res.cpu().tolist()
        assert min(rs) > 0, min(rs)
        blk = out[0, :rs[0]].cpu().numpy().tobytes()
        o = C.create_string_buffer(L + 64)
        assert dec(blk, o, len(blk), L, dict_host, len(dict_host)) == L and \
            o.raw[:L] == held_rows[0].tobytes(), "host usingDict decode"
        return round(total / sum(rs), 4)

    def ratios(ddev):
        """{fast, hc} ratio of the held-out messages against the dictionary ddev (may be empty)."""
        dict_host = ddev.cpu().numpy().tobytes()
        if ddev.numel():
            amd.cdict_prepare(ddev, L, obj)
            amd.compress_cdict_batch(hptr, sizes, dptr, caps, res, obj)
        else:
            amd.compress_batch(held, sizes, out, res, dst_caps=caps)
        fast = ratio(dict_host)
        amd.hc_cdict_prepare(ddev, L, hobj)
        amd.compress_hc_cdict_batch(hptr, sizes, dptr, caps, res, hobj, L, DEPTH, hscratch)
        return {"compress_usingCDict": fast, "compress_hc_usingCDict_depth8": ratio(dict_host)}

    rec = {"case": name, "samples": nb, "held_out_messages": nb, "message_bytes": L,
           "dict_bytes": DD, "hc_depth": DEPTH,
           "none": ratios(torch.empty(0, dtype=torch.uint8, device="cuda")),
           "head": ratios(samples.view(-1)[:DD].clone()), "trained": {}}
    info = i32([0] * 4)
    for k in SEGMENTS:
        d = torch.empty(DD, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(amd.dict_train_scratch_size(nb, L, k), dtype=torch.uint8,
                              device="cuda")
        ts = times_ms(torch, lambda: amd.dict_train(tptr, sizes, L, d, k, scratch, info), reps)
        used, picks, ignored, _ = info.cpu().tolist()
        # the same samples into a dictionary of one segment: zero, count, ONE round that scores
        # every slot, finish -- the count and the scoring of the whole call in 5 launches
        one = torch.empty(k, dtype=torch.uint8, device="cuda")
        t1 = times_ms(torch, lambda: amd.dict_train(tptr, sizes, L, one, k, scratch, info), reps)
        e = {"train_ms": round(ts[len(ts) // 2], 3), "train_ms_min": round(ts[0], 3),
             "train_ms_max": round(ts[-1], 3), "launches": 3 + 2 * (DD // k),
             "one_round_call_ms": round(t1[len(t1) // 2], 3),
             "bytes_used": used, "picks": picks, "samples_ignored": ignored,
             "scratch_bytes": scratch.numel()}
        e.update(ratios(d))
        for key in ("compress_usingCDict", "compress_hc_usingCDict_depth8"):
            e[key + "_size_vs_head"] = round(rec["head"][key] / e[key], 4)
        rec["trained"]["segment%d" % k] = e
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--messages", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_train.json"))
    ap.add_argument("--corpus-dir", default=os.path.join(ROOT, "bench_out", "dict_train_corpus"))
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, a.reps, a.messages, a.corpus_dir)), flush=True)
        return 0
    recs = []
    for name in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                                "--reps", str(a.reps), "--messages", str(a.messages),
                                "--corpus-dir", a.corpus_dir], capture_output=True, text=True,
                               timeout=CASE_TIMEOUT)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (name, CASE_TIMEOUT), file=sys.stderr)
            return 1
        if p.returncode != 0:
            print("%s: exit %d; stopping\n%s" % (name, p.returncode, p.stderr[-2000:]), file=sys.stderr)
            return 1
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        recs.append(json.loads(line))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/dict_train_bench.py", "reps": a.reps, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
