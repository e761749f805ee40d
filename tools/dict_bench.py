#!/usr/bin/env python3
"""Small independent messages against one shared dictionary on one MI355X: 1 KiB and 4 KiB
messages, a 61440-byte dictionary, both cut from one stream of the `comp` generator
(tests/golden/inputs.py): the dictionary is the stream's first 61440 bytes, the messages are
the 32 KiB that follow, cut every L bytes and repeated across the batch (each copy at its own
address; blocks are independent, so repetition changes no block's work).  Per case, GiB/s of
MESSAGE bytes (median of --reps by HIP events, with min and max) and the ratio of:

  plain     (a) compress_batch_dev, no dictionary
  staged    (b) what a caller could do before: a staging copy [dictionary | message] per
            message (two torch copies), then compress_withPrefix_batch_dev; the copy and the
            encode are timed separately
  cdict     (c) compress_usingCDict_batch_dev on a prepared dictionary, and the one-off
            cdict_prepare time

Each case runs in a child process of its own under a time limit; the first failure ends the
run.  Prints one JSON line per case and writes profiles/dict_compress.json (--out).
usage: dict_bench.py [--reps 5] [--out profiles/dict_compress.json] [--case NAME]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DD = 61440
# (staging of case (b): batch x (DD + L) bytes, 1 GiB at most)
CASES = {"msg1KiB_x16384": (1024, 16384), "msg4KiB_x16384": (4096, 16384)}
CASE_TIMEOUT = 240   # seconds per child


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


def run_case(name, reps):
    import numpy as np
    import torch
    import inputs as I
    import libapenetwork_amd as amd
    L, nb = CASES[name]
    stream = I.make("comp", DD + 32768, seed=7)
    d = stream[:DD]
    distinct = [stream[DD + s:DD + s + L] for s in range(0, 32768, L)]
    k = len(distinct)
    total = nb * L
    dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    ddict = dev(d)
    msgs = dev(b"".join(distinct)).view(k, L).repeat(nb // k, 1).contiguous()
    assert msgs.shape == (nb, L)
    bound = amd.compressBound(L)
    slot = (bound + 15) // 16 * 16
    out = torch.empty((nb, slot), dtype=torch.uint8, device="cuda")
    sizes, caps, res = i32([L] * nb), i32([bound] * nb), i32([0] * nb)
    sptr = i64([msgs.data_ptr() + i * L for i in range(nb)])
    dptr = i64([out.data_ptr() + i * slot for i in range(nb)])
    rec = {"case": name, "messages": nb, "message_bytes": L, "distinct_messages": k,
           "dict_bytes": DD, "window": amd.cdict_window(DD, L)}

    def entry(ts, **more):
        med = ts[len(ts) // 2]
        e = {"ms": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
             "GiBps": round(total / (med * 1e-3) / (1 << 30), 3)}
        e.update(more)
        return e

    def ratio():
        rs = res.cpu().tolist()
        assert min(rs) > 0, min(rs)
        return round(total / sum(rs), 4)

    # (a) no dictionary
    ts = times_ms(torch, lambda: amd.compress_batch(msgs, sizes, out, res, dst_caps=caps), reps)
    rec["plain"] = entry(ts, ratio=ratio())

    # (b) staged [dictionary | message] + withPrefix
    stage = torch.empty((nb, DD + L), dtype=torch.uint8, device="cuda")

    def copy():
        stage[:, :DD] = ddict
        stage[:, DD:] = msgs
    tc = times_ms(torch, copy, reps)
    pp = i64([stage.data_ptr() + i * (DD + L) + DD for i in range(nb)])
    pre = i32([DD] * nb)
    te = times_ms(torch, lambda: amd.compress_prefix_batch(pp, sizes, pre, dptr, caps, res), reps)
    r_staged = ratio()
    rec["staged"] = {"copy": entry(tc), "encode": entry(te, ratio=r_staged),
                     "staging_bytes": stage.numel(),
                     "GiBps_copy_plus_encode": round(
                         total / ((tc[len(tc) // 2] + te[len(te) // 2]) * 1e-3) / (1 << 30), 3)}
    del stage

    # (c) prepared dictionary
    obj = torch.empty(amd.cdict_size(), dtype=torch.uint8, device="cuda")
    tp = times_ms(torch, lambda: amd.cdict_prepare(ddict, L, obj), reps)
    ts = times_ms(torch, lambda: amd.compress_cdict_batch(sptr, sizes, dptr, caps, res, obj), reps)
    rec["cdict"] = entry(ts, ratio=ratio(), prepare_ms=round(tp[len(tp) // 2], 4))
    # the block is valid: message 0 through the host decoder with the original dictionary
    rs = res.cpu().tolist()
    blk = out[0, :rs[0]].cpu().numpy().tobytes()
    o = C.create_string_buffer(L + 64)
    f = amd.lib().APE_LZ4_decompress_safe_usingDict
    f.restype, f.argtypes = C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    assert f(blk, o, len(blk), L, d, DD) == L and o.raw[:L] == distinct[0], "host usingDict decode"

    rec["cdict_vs_staged_encode"] = round(rec["staged"]["encode"]["ms"] / rec["cdict"]["ms"], 3)
    rec["cdict_vs_staged_copy_plus_encode"] = round(
        (rec["staged"]["copy"]["ms"] + rec["staged"]["encode"]["ms"]) / rec["cdict"]["ms"], 3)
    rec["cdict_size_vs_staged"] = round(r_staged / rec["cdict"]["ratio"], 5)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_compress.json"))
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, a.reps)), flush=True)
        return 0
    recs = []
    for name in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                                "--reps", str(a.reps)], capture_output=True, text=True,
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
        json.dump({"tool": "tools/dict_bench.py", "reps": a.reps, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
