#!/usr/bin/env python3
"""APE_LZ4_compress_large_hc_batch_dev on one MI355X: 16 inputs of 16 MiB of the corpora of
tools/large_bench.py -- device-synthesised App. C blocks laid end to end ("appC"), the torch/lib
slice ("sobin") and the Python sources ("pysrc": the 4 MiB of large_bench.py, four times per
input; the copies lie further apart than any window reaches) -- at depths 8 and 64.  Per case
and depth, in one process:

  large_hc     the whole call: ms (median of --reps by HIP events, with min and max), GiB/s of
               input, ratio; every block decoded on the GPU (decompress_ptr_batch) and compared
  stages_ms    plan / chain / search / parse / offsets / stitch of one call, the passes summed
               (APE_LZ4_compress_large_hc_timed_dev, the best of 3)
  blocks64k_hc the same bytes through compress_hc_ptr_batch as independent 64 KiB blocks at the
               same depth (not one LZ4 block; no history beyond the block), decoded and compared
  ns_per_byte  of the two, and their quotient: what history and the stitch cost per input byte

and once per case

  large_fast   compress_large_ptr_batch on the same inputs (the fast encoder), decoded and compared
  ref_ratio    the reference's compress_default ratio on input 0 (oracle/_ref when it was built,
               else the oracle)

Each case runs in a child process of its own under a time limit; the first failure ends the
run.  Prints one JSON line per case and writes profiles/large_hc.json (--out).
usage: large_hc_bench.py [--reps 5] [--out FILE] [--case NAME]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MB = 1 << 20
NIN, N = 16, 16 * MB
CASES = ("appC", "sobin", "pysrc")
DEPTHS = (8, 64)
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


def run_case(kind, reps):
    import numpy as np
    import torch
    import large_bench
    import libapenetwork_amd as amd
    total = NIN * N
    flat = torch.empty(total, dtype=torch.uint8, device="cuda")
    if kind == "pysrc":
        large_bench.fill(torch, np, kind, flat, 4 * MB)
    else:
        large_bench.fill(torch, np, kind, flat, N)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    bound = amd.compressBound(N)
    slot = (bound + 15) // 16 * 16
    out = torch.empty(NIN * slot, dtype=torch.uint8, device="cuda")
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    sptr = i64([flat.data_ptr() + i * N for i in range(NIN)])
    dptr = i64([out.data_ptr() + i * slot for i in range(NIN)])
    bptr = i64([back.data_ptr() + i * N for i in range(NIN)])
    sizes, caps, res, dres = i32([N] * NIN), i32([bound] * NIN), i32([0] * NIN), i32([0] * NIN)
    scr = torch.empty(amd.compress_large_hc_scratch_size(NIN, N), dtype=torch.uint8, device="cuda")
    rec = {"case": "%s_%dx%dMiB" % (kind, NIN, N // MB), "inputs": NIN, "input_bytes": N,
           "slice": amd.compress_large_slice_size(), "scratch_bytes": scr.numel()}

    def entry(ts, rs):
        med = ts[len(ts) // 2]
        return {"ms": round(med, 3), "ms_min": round(ts[0], 3), "ms_max": round(ts[-1], 3),
                "GiBps": round(total / (med * 1e-3) / (1 << 30), 3),
                "ns_per_byte": round(med * 1e6 / total, 4), "ratio": round(total / sum(rs), 4)}

    def decoded(what):
        """The blocks at dptr / res decode, on the GPU, to the inputs."""
        rs = res.cpu().tolist()
        assert min(rs) > 0, (what, rs)
        back.zero_()
        amd.decompress_ptr_batch(dptr, res, bptr, sizes, dres)
        torch.cuda.synchronize()
        assert dres.cpu().tolist() == [N] * NIN and torch.equal(back, flat), what
        return rs

    ts = times_ms(torch, lambda: amd.compress_large_ptr_batch(sptr, sizes, dptr, caps, res, N,
                                                              scratch=scr), reps)
    rec["large_fast"] = entry(ts, decoded("large_fast"))

    src0 = flat[:N].cpu().numpy().tobytes()
    refp = os.path.join(ROOT, "oracle", "_ref", "libape_lz4_ref.so")
    if os.path.exists(refp):
        name, f = "oracle/_ref", C.CDLL(refp).APE_LZ4_compress_default
    else:
        name, f = "oracle", C.CDLL(os.path.join(ROOT, "oracle", "liblz4_oracle.so")).orc_compress_default
    rec["reference"] = {"from": name, "ratio_input0": round(N / f(src0, C.create_string_buffer(bound), N, bound), 4)}

    # independent 64 KiB blocks of the same bytes
    nb = total // 65536
    bslot = (amd.compressBound(65536) + 15) // 16 * 16
    bout = torch.empty((nb, bslot), dtype=torch.uint8, device="cuda")
    bsz, bcap, bres, bdres = i32([65536] * nb), i32([bslot] * nb), i32([0] * nb), i32([0] * nb)
    bsp = i64([flat.data_ptr() + i * 65536 for i in range(nb)])
    bdp = i64([bout.data_ptr() + i * bslot for i in range(nb)])
    bscr = torch.empty(amd.compress_hc_scratch_size(nb), dtype=torch.uint8, device="cuda")

    timed = amd.lib().APE_LZ4_compress_large_hc_timed_dev
    ms6 = (C.c_float * 6)()
    stream = torch.cuda.current_stream().cuda_stream
    for depth in DEPTHS:
        ts = times_ms(torch, lambda: amd.compress_large_hc_ptr_batch(sptr, sizes, dptr, caps, res, N,
                                                                     depth, scratch=scr), reps)
        e = entry(ts, decoded("large_hc depth %d" % depth))
        best = None
        for _ in range(3):
            rc = timed(sptr.data_ptr(), sizes.data_ptr(), dptr.data_ptr(), caps.data_ptr(),
                       res.data_ptr(), NIN, N, depth, scr.data_ptr(), scr.numel(), 0, stream, ms6)
            assert rc == 0, amd.gpu_last_error()
            if best is None or sum(ms6) < sum(best):
                best = list(ms6)
        e["stages_ms"] = dict(zip(("plan", "chain", "search", "parse", "offsets", "stitch"),
                                  (round(x, 3) for x in best)))
        rec["large_hc_depth%d" % depth] = e

        ts = times_ms(torch, lambda: amd.compress_hc_ptr_batch(bsp, bsz, bdp, bcap, bres, depth, bscr),
                      reps)
        brs = bres.cpu().tolist()
        assert min(brs) > 0
        back.zero_()
        amd.decompress_batch(bout, bres, back.view(nb, 65536), bdres, dst_caps=bsz)
        torch.cuda.synchronize()
        assert bool((bdres == 65536).all()) and torch.equal(back, flat), "blocks64k_hc round trip"
        b = entry(ts, brs)
        rec["blocks64k_hc_depth%d" % depth] = b
        rec["large_vs_blocks64k_depth%d" % depth] = {
            "time_per_byte": round(e["ms"] / b["ms"], 4), "ratio": round(e["ratio"] / b["ratio"], 4)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_hc.json"))
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
        json.dump({"tool": "tools/large_hc_bench.py", "reps": a.reps, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
