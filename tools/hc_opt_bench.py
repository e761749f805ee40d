#!/usr/bin/env python3
"""The cost-minimising parse of the high-ratio mode beside the lazy one, on one MI355X and the
three inputs of tools/hc_bench.py (appC, pysrc, sobin), in one process per input and
interleaved call by call:

  blocks   1024 blocks of 64 KiB at depths 8, 64 and 256: compress_hc_ptr_batch (lazy) and
           compress_hc_opt_ptr_batch (opt)
  large    16 inputs of 16 MiB (tools/large_hc_bench.py's) at depths 8 and 64:
           compress_large_hc_ptr_batch and compress_large_hc_opt_ptr_batch

Per call: ms (median of --reps by HIP events, with min and max), GiB/s of input and the ratio;
every output is decoded on the GPU and compared with the input.  Per pair: opt's time and ratio
over lazy's, and "ratio_holds": opt's ratio is at least lazy's.  Each case runs in a child
process of its own under a time limit; the first failure ends the run.  Prints one JSON line per
case and writes profiles/hc_opt.json (--out); the exit status is 1 when a ratio does not hold.

--case NAME --once runs every call of one case exactly once: the run to wrap in a kernel trace
(one call of each kind per depth, so the per-kernel sums compare lz4_hc_opt_parse_kernel with
lz4_hc_parse_kernel directly; its event times include the first call's warm-up).
usage: hc_opt_bench.py [--reps 5] [--out FILE] [--case NAME [--once] [--no-large]]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MB = 1 << 20
N = 65536
NB = 1024
NIN, LN = 16, 16 * MB
CASES = ("appC", "pysrc", "sobin")
DEPTHS = (8, 64, 256)
LARGE_DEPTHS = (8, 64)
CASE_TIMEOUT = 500   # seconds per child


def interleaved_ms(torch, fns, reps):
    """Sorted times of each of fns, called in turn reps + 1 times (the first round warms up)."""
    ts = [[] for _ in fns]
    for _ in range(reps + 1):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [sorted(t[1:] or t) for t in ts]   # (reps 0, --once: the one call there was)


def entry(ts, total, rs):
    med = ts[len(ts) // 2]
    return {"ms": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
            "GiBps": round(total / (med * 1e-3) / (1 << 30), 3), "bytes": sum(rs),
            "ratio": round(total / sum(rs), 4)}


def pair(lazy, opt):
    return {"lazy": lazy, "opt": opt, "time_opt_over_lazy": round(opt["ms"] / lazy["ms"], 4),
            "ratio_opt_over_lazy": round(lazy["bytes"] / opt["bytes"], 4),
            "ratio_holds": opt["bytes"] <= lazy["bytes"]}


def run_blocks(torch, np, amd, name, reps):
    src = torch.empty((NB, N), dtype=torch.uint8, device="cuda")
    if name == "appC":
        amd.synth_blocks(src, N, 0, 1)
    else:
        import ratio_files
        d = ratio_files.datasets()[name]
        distinct = len(d) // N
        assert NB % distinct == 0, (NB, distinct)
        one = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).reshape(distinct, N).copy())
        src.copy_(one.repeat(NB // distinct, 1))
    torch.cuda.synchronize()
    total = NB * N
    bound = amd.compressBound(N)
    slot = (bound + 15) // 16 * 16
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    sizes, caps, dres = i32([N] * NB), i32([bound] * NB), i32([0] * NB)
    sptr = i64([src.data_ptr() + i * N for i in range(NB)])
    out = torch.empty((NB, N), dtype=torch.uint8, device="cuda")
    comp = [torch.empty((NB, slot), dtype=torch.uint8, device="cuda") for _ in range(2)]
    dptr = [i64([c.data_ptr() + i * slot for i in range(NB)]) for c in comp]
    res = [i32([0] * NB), i32([0] * NB)]
    scr = [torch.empty(amd.compress_hc_scratch_size(NB), dtype=torch.uint8, device="cuda"),
           torch.empty(amd.compress_hc_opt_scratch_size(NB), dtype=torch.uint8, device="cuda")]
    calls = (amd.compress_hc_ptr_batch, amd.compress_hc_opt_ptr_batch)

    def decoded(k, what):
        rs = res[k].cpu().tolist()
        assert min(rs) > 0, (what, min(rs))
        out.zero_()
        amd.decompress_batch(comp[k], res[k], out, dres, dst_caps=sizes)
        torch.cuda.synchronize()
        assert bool((dres == N).all()) and bool(torch.equal(out, src)), what + ": round trip"
        return rs

    rec = {"blocks": NB, "block_bytes": N, "scratch_bytes": {"lazy": scr[0].numel(), "opt": scr[1].numel()}}
    for depth in DEPTHS:
        fns = [lambda k=k: calls[k](sptr, sizes, dptr[k], caps, res[k], depth, scr[k]) for k in (0, 1)]
        ts = interleaved_ms(torch, fns, reps)
        rec["depth%d" % depth] = pair(*[entry(ts[k], total, decoded(k, "depth %d call %d" % (depth, k)))
                                        for k in (0, 1)])
    return rec


def run_large(torch, np, amd, name, reps):
    import large_bench
    total = NIN * LN
    flat = torch.empty(total, dtype=torch.uint8, device="cuda")
    large_bench.fill(torch, np, name, flat, 4 * MB if name == "pysrc" else LN)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    bound = amd.compressBound(LN)
    slot = (bound + 15) // 16 * 16
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    sptr = i64([flat.data_ptr() + i * LN for i in range(NIN)])
    bptr = i64([back.data_ptr() + i * LN for i in range(NIN)])
    sizes, caps, dres = i32([LN] * NIN), i32([bound] * NIN), i32([0] * NIN)
    out = [torch.empty(NIN * slot, dtype=torch.uint8, device="cuda") for _ in range(2)]
    dptr = [i64([o.data_ptr() + i * slot for i in range(NIN)]) for o in out]
    res = [i32([0] * NIN), i32([0] * NIN)]
    scr = [torch.empty(amd.compress_large_hc_scratch_size(NIN, LN), dtype=torch.uint8, device="cuda"),
           torch.empty(amd.compress_large_hc_opt_scratch_size(NIN, LN), dtype=torch.uint8, device="cuda")]
    calls = (amd.compress_large_hc_ptr_batch, amd.compress_large_hc_opt_ptr_batch)

    def decoded(k, what):
        rs = res[k].cpu().tolist()
        assert min(rs) > 0, (what, rs)
        back.zero_()
        amd.decompress_ptr_batch(dptr[k], res[k], bptr, sizes, dres)
        torch.cuda.synchronize()
        assert dres.cpu().tolist() == [LN] * NIN and torch.equal(back, flat), what + ": round trip"
        return rs

    rec = {"inputs": NIN, "input_bytes": LN, "slice": amd.compress_large_slice_size(),
           "scratch_bytes": {"lazy": scr[0].numel(), "opt": scr[1].numel()}}
    for depth in LARGE_DEPTHS:
        fns = [lambda k=k: calls[k](sptr, sizes, dptr[k], caps, res[k], LN, depth, scratch=scr[k])
               for k in (0, 1)]
        ts = interleaved_ms(torch, fns, reps)
        rec["depth%d" % depth] = pair(*[entry(ts[k], total, decoded(k, "large depth %d call %d" % (depth, k)))
                                        for k in (0, 1)])
    return rec


def run_case(name, reps, large):
    import numpy as np
    import torch
    import libapenetwork_amd as amd
    rec = {"case": name, "blocks64k": run_blocks(torch, np, amd, name, reps)}
    if large:
        rec["large"] = run_large(torch, np, amd, name, reps)
    return rec


def holds(rec):
    return all(v["ratio_holds"] for part in ("blocks64k", "large") if part in rec
               for k, v in rec[part].items() if k.startswith("depth"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hc_opt.json"))
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    ap.add_argument("--once", action="store_true", help="with --case: one call each, for a trace")
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, 0 if a.once else a.reps, not a.no_large)), flush=True)
        return 0
    recs = []
    for name in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                                "--reps", str(a.reps)] + (["--no-large"] if a.no_large else []),
                               capture_output=True, text=True, timeout=CASE_TIMEOUT)
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
    ok = all(holds(r) for r in recs)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/hc_opt_bench.py", "reps": a.reps, "ratio_holds": ok, "cases": recs},
                  f, indent=1)
        f.write("\n")
    if not ok:
        print("the cost-minimising parse's ratio is BELOW the lazy parse's somewhere", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
