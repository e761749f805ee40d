#!/usr/bin/env python3
"""A prepared dictionary per message on one MI355X: 16384 independent messages
of 1 KiB and of 4 KiB, K = 1, 8 and 64 dictionaries of 61440 bytes with different content
(dictionary k is the first 61440 bytes of the `comp` stream of seed 100 + k, its messages the
32 KiB that follow, cut every L bytes and repeated, each copy at its own address).  Messages are
assigned to dictionaries once in runs (`grouped`: message i belongs to dictionary i // (N / K))
and once round-robin (`interleaved`: i % K).  For each of the three encoders that read a prepared
dictionary (fast, hc and hc_opt, the last two at depth 8), per case, K and assignment, in one
process and interleaved repetition by repetition, ms per call by HIP events around --inner calls
(median of --reps, with min and max) of:

  new          one usingCDicts call on the mixed batch, an object pointer per message
  partitioned  the only way before: the four pointer and size arrays grouped by dictionary, then K
               single-dictionary calls, one per group (the K calls are timed; grouping the arrays
               on the host and uploading them is timed once, by the host clock, as partition_ms)
  single       K = 1 only: the single-dictionary call on the caller's arrays as they are

new_over_partitioned is the median of the per-repetition quotients, with their min and max.  The
new call's results and bytes are compared with the partitioned calls', and its output is decoded
on the GPU with decompress_safe_usingDict and each message's own dictionary.  Per K, one batched
prepare is timed against K single prepares in the same way, for both kinds of object.  Each
(case, encoder) runs in a child process of its own under a time limit; the first failure ends the
run.  Prints one JSON line per child and writes profiles/multi_dict.json (--out).
usage: multi_dict_bench.py [--reps 7] [--messages 16384] [--out FILE] [--case NAME --encoder E]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DD = 61440
FOLLOW = 32768
CASES = {"msg1KiB": 1024, "msg4KiB": 4096}
KS = (1, 8, 64)
ENCODERS = ("fast", "hc", "hc_opt", "prepare")
DEPTH = 8
INNER = {"fast": 16, "hc": 4, "hc_opt": 2, "prepare": 4}   # calls per timed window
CHILD_TIMEOUT = 300   # seconds per child


def interleaved_ms(torch, fns, reps, inner):
    """Per function, the ms per call of every repetition in order, the functions taking turns
    within each repetition (the first turn of each warms up and is dropped)."""
    ts = [[] for _ in fns]
    for _ in range(reps + 1):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    return [t[1:] for t in ts]


def stats(ts, total=None):
    s = sorted(ts)
    med = s[len(s) // 2]
    out = {"ms": round(med, 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4)}
    if total:
        out["GiBps"] = round(total / (med * 1e-3) / (1 << 30), 3)
    return out


def quotient(num, den):
    q = sorted(a / b for a, b in zip(num, den))
    return {"median": round(q[len(q) // 2], 4), "min": round(q[0], 4), "max": round(q[-1], 4)}


def run_prepare(torch, amd, ddicts, i32, i64, L, reps):
    """K single prepares against one batched prepare, both kinds, every K."""
    rec = {}
    for kind, size, single, batch in (("cdict", amd.cdict_size(), amd.cdict_prepare,
                                       amd.cdict_prepare_batch),
                                      ("hc_cdict", amd.hc_cdict_size(), amd.hc_cdict_prepare,
                                       amd.hc_cdict_prepare_batch)):
        for K in KS:
            one = torch.zeros(K * size, dtype=torch.uint8, device="cuda")
            all_ = torch.zeros(K * size, dtype=torch.uint8, device="cuda")
            dptr, dsz = i64([d.data_ptr() for d in ddicts[:K]]), i32([DD] * K)
            views = [one[k * size:(k + 1) * size] for k in range(K)]

            def singles():
                for k in range(K):
                    single(ddicts[k], L, views[k])

            ts, tb = interleaved_ms(torch, [singles, lambda: batch(dptr, dsz, L, all_, size)], reps,
                                    INNER["prepare"])
            assert bool(torch.equal(one, all_)), "objects of the batched and the single prepares"
            rec["%s_K%d" % (kind, K)] = {"singles": stats(ts), "batched": stats(tb),
                                         "batched_over_singles": quotient(tb, ts)}
    return rec


def run_case(name, enc, reps, nb):
    import numpy as np
    import torch
    import inputs as I
    import libapenetwork_amd as amd
    L = CASES[name]
    Kmax = max(KS)
    streams = [I.make("comp", DD + FOLLOW, seed=100 + k) for k in range(Kmax)]
    nd = FOLLOW // L
    dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    i32 = lambda xs: torch.tensor(np.asarray(xs, dtype=np.int32), device="cuda")
    i64 = lambda xs: torch.tensor(np.asarray(xs, dtype=np.int64), device="cuda")
    ddicts = [dev(s[:DD]) for s in streams]
    rec = {"case": name, "encoder": enc, "messages": nb, "message_bytes": L, "dict_bytes": DD,
           "distinct_messages_per_dictionary": nd}
    if enc == "prepare":
        rec.update(run_prepare(torch, amd, ddicts, i32, i64, L, reps))
        return rec

    follow = np.stack([np.frombuffer(s[DD:], dtype=np.uint8).reshape(nd, L) for s in streams])
    total = nb * L
    bound = amd.compressBound(L)
    slot = (bound + 15) // 16 * 16
    fast = enc == "fast"
    size = amd.cdict_size() if fast else amd.hc_cdict_size()
    objs = torch.zeros(Kmax * size, dtype=torch.uint8, device="cuda")
    (amd.cdict_prepare_batch if fast else amd.hc_cdict_prepare_batch)(
        i64([d.data_ptr() for d in ddicts]), i32([DD] * Kmax), L, objs, size)
    obj = [objs[k * size:(k + 1) * size] for k in range(Kmax)]
    scratch = None
    if not fast:
        ssize = (amd.compress_hc_cdict_scratch_size if enc == "hc"
                 else amd.compress_hc_opt_cdict_scratch_size)(nb, L)
        scratch = torch.empty(ssize, dtype=torch.uint8, device="cuda")
        rec["scratch_bytes"] = ssize
    new_call, one_call = {"fast": (amd.compress_cdicts_batch, amd.compress_cdict_batch),
                          "hc": (amd.compress_hc_cdicts_batch, amd.compress_hc_cdict_batch),
                          "hc_opt": (amd.compress_hc_opt_cdicts_batch,
                                     amd.compress_hc_opt_cdict_batch)}[enc]
    hc = () if fast else (L, DEPTH, scratch)
    caps_h = np.full(nb, bound, dtype=np.int32)
    sizes_h = np.full(nb, L, dtype=np.int32)
    outs = [torch.empty((nb, slot), dtype=torch.uint8, device="cuda") for _ in range(2)]
    back = torch.empty((nb, L), dtype=torch.uint8, device="cuda")
    bptr = i64(back.data_ptr() + np.arange(nb, dtype=np.int64) * L)
    dres = i32(np.zeros(nb))

    for K in KS:
        for assign in ("grouped", "interleaved"):
            idx = np.arange(nb)
            owner = idx // (nb // K) if assign == "grouped" else idx % K
            msgs = torch.from_numpy(follow[owner, (idx // K) % nd]).cuda()
            sptr_h = msgs.data_ptr() + idx.astype(np.int64) * L
            dptr_h = [o.data_ptr() + idx.astype(np.int64) * slot for o in outs]
            optr_h = objs.data_ptr() + owner.astype(np.int64) * size
            sptr, sizes, caps = i64(sptr_h), i32(sizes_h), i32(caps_h)
            dptr0, optr = i64(dptr_h[0]), i64(optr_h)
            res = [i32(np.zeros(nb)) for _ in range(3)]

            # the only way before: group the caller's four arrays by dictionary, upload them
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            perm = np.argsort(owner, kind="stable")
            count = np.bincount(owner, minlength=K)
            p_sptr, p_sizes = i64(sptr_h[perm]), i32(sizes_h[perm])
            p_dptr, p_caps = i64(dptr_h[1][perm]), i32(caps_h[perm])
            torch.cuda.synchronize()
            partition_ms = (time.perf_counter() - t0) * 1e3
            start = [0] + [int(c) for c in np.cumsum(count)]
            groups = [(p_sptr[a:b], p_sizes[a:b], p_dptr[a:b], p_caps[a:b], res[1][a:b], obj[k])
                      for k, (a, b) in enumerate(zip(start, start[1:]))]

            def new():
                new_call(sptr, sizes, dptr0, caps, res[0], optr, *hc)

            def partitioned():
                for group in groups:
                    one_call(*group, *hc)

            fns = [new, partitioned]
            if K == 1:
                dptr1 = i64(dptr_h[1])
                fns.append(lambda: one_call(sptr, sizes, dptr1, caps, res[2], obj[0], *hc))
            ts = interleaved_ms(torch, fns, reps, INNER[enc])

            rs = res[0].cpu().numpy()
            assert rs.min() > 0, int(rs.min())
            assert np.array_equal(rs[perm], res[1].cpu().numpy()), "results, new and partitioned"
            width = torch.arange(slot, device="cuda")[None, :] < res[0][:, None]
            assert bool(torch.equal(outs[0] * width, outs[1] * width)), "bytes, new and partitioned"
            back.zero_()
            amd.decompress_dict_batch(dptr0, res[0], bptr, sizes,
                                      i64([ddicts[k].data_ptr() for k in owner]), i32([DD] * nb),
                                      dres)
            torch.cuda.synchronize()
            assert bool((dres == L).all()) and bool(torch.equal(back, msgs)), "usingDict round trip"

            e = {"new": stats(ts[0], total), "partitioned": stats(ts[1], total),
                 "partition_ms": round(partition_ms, 3),
                 "new_over_partitioned": quotient(ts[0], ts[1]),
                 "ratio": round(total / int(rs.sum()), 4)}
            if K == 1:
                e["single"] = stats(ts[2], total)
                e["new_over_single"] = quotient(ts[0], ts[2])
            rec["K%d_%s" % (K, assign)] = e
        g, i = rec["K%d_grouped" % K]["new"]["ms"], rec["K%d_interleaved" % K]["new"]["ms"]
        rec["K%d_interleaved_over_grouped" % K] = round(i / g, 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--messages", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_dict.json"))
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    ap.add_argument("--encoder", choices=ENCODERS)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, a.encoder, a.reps, a.messages)), flush=True)
        return 0
    recs = []
    for name in CASES:
        for enc in ENCODERS:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                                    "--encoder", enc, "--reps", str(a.reps), "--messages",
                                    str(a.messages)],
                                   capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                print("%s %s: no result within %d s; stopping" % (name, enc, CHILD_TIMEOUT),
                      file=sys.stderr)
                return 1
            if p.returncode != 0:
                print("%s %s: exit %d; stopping\n%s" % (name, enc, p.returncode, p.stderr[-2000:]),
                      file=sys.stderr)
                return 1
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            recs.append(json.loads(line))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/multi_dict_bench.py", "reps": a.reps, "depth": DEPTH,
                   "calls_per_timed_window": INNER, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
