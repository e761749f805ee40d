#!/usr/bin/env python3
"""The high-ratio mode on one MI355X: encode time and ratio of APE_LZ4_compress_hc_batch_dev at
depths 8, 64 and 256 beside APE_LZ4_compress_batch_dev, in the same process, on 1024 blocks of
64 KiB of

  appC    SURVEY App. C blocks (the benchmark data, synthesised on the device)
  pysrc   the real-file inputs of tools/ratio_files.py: 64 blocks of Python standard-library
  sobin   source / of a shared library, repeated 16 times across the batch (each copy at its
          own address; blocks are independent, so repetition changes no block's work)

Per case and encoder: ms per call (median of --reps by HIP events, with min and max), GiB/s of
input bytes, the ratio, and the ratio relative to the reference's compress_default on the same
blocks (oracle/_ref when it was built, else the oracle).  Every output is decoded on the GPU
and compared with the input.  Each case runs in a child process of its own under a time limit;
the first failure ends the run.  Prints one JSON line per case and writes
profiles/hc_compress.json (--out).
usage: hc_bench.py [--reps 5] [--blocks 1024] [--out profiles/hc_compress.json] [--case NAME]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N = 65536
CASES = ("appC", "pysrc", "sobin")
DEPTHS = (8, 64, 256)
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


def reference_sizes(data, nb):
    """(name of the checker, compress_default sizes of the nb blocks of data)."""
    refp = os.path.join(ROOT, "oracle", "_ref", "libape_lz4_ref.so")
    if os.path.exists(refp):
        name, f = "oracle/_ref", C.CDLL(refp).APE_LZ4_compress_default
    else:
        name, f = "oracle", C.CDLL(os.path.join(ROOT, "oracle", "liblz4_oracle.so")).orc_compress_default
    bound = N + N // 255 + 16
    o = C.create_string_buffer(bound)
    return name, [f(data[i * N:(i + 1) * N], o, N, bound) for i in range(nb)]


def run_case(name, reps, nb):
    import numpy as np
    import torch
    import libapenetwork_amd as amd
    src = torch.empty((nb, N), dtype=torch.uint8, device="cuda")
    if name == "appC":
        amd.synth_blocks(src, N, 0, 1)
        distinct = nb
    else:
        import ratio_files
        d = ratio_files.datasets()[name]
        distinct = len(d) // N
        assert nb % distinct == 0, (nb, distinct)
        one = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).reshape(distinct, N).copy())
        src.copy_(one.repeat(nb // distinct, 1))
    torch.cuda.synchronize()
    total = nb * N
    checker, rsz = reference_sizes(src[:distinct].cpu().numpy().tobytes(), distinct)
    ref_ratio = distinct * N / sum(rsz)
    bound = amd.compressBound(N)
    slot = (bound + 15) // 16 * 16
    comp = torch.empty((nb, slot), dtype=torch.uint8, device="cuda")
    out = torch.empty((nb, N), dtype=torch.uint8, device="cuda")
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    sizes, caps, res, dres = i32([N] * nb), i32([bound] * nb), i32([0] * nb), i32([0] * nb)
    sptr = i64([src.data_ptr() + i * N for i in range(nb)])
    dptr = i64([comp.data_ptr() + i * slot for i in range(nb)])
    scratch = torch.empty(amd.compress_hc_scratch_size(nb), dtype=torch.uint8, device="cuda")
    rec = {"case": name, "blocks": nb, "block_bytes": N, "distinct_blocks": distinct,
           "reference": {"from": checker, "ratio": round(ref_ratio, 4)},
           "scratch_bytes": scratch.numel()}

    def entry(ts):
        rs = res.cpu().tolist()
        assert min(rs) > 0, min(rs)
        amd.decompress_batch(comp, res, out, dres, dst_caps=sizes)
        torch.cuda.synchronize()
        assert bool((dres == N).all()) and bool(torch.equal(out, src)), "round trip"
        med, ratio = ts[len(ts) // 2], total / sum(rs)
        return {"ms": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                "GiBps": round(total / (med * 1e-3) / (1 << 30), 3), "ratio": round(ratio, 4),
                "ratio_vs_reference": round(ratio / ref_ratio, 4)}

    f = amd.lib().APE_LZ4_compress_batch_dev
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [C.c_void_p(t.data_ptr()) for t in (sptr, sizes, dptr, caps, res)]

    def fast():
        assert f(*args, nb, stream) == 0, amd.gpu_last_error()
    rec["compress_batch_dev"] = entry(times_ms(torch, fast, reps))
    for depth in DEPTHS:
        ts = times_ms(torch, lambda: amd.compress_hc_ptr_batch(sptr, sizes, dptr, caps, res,
                                                               depth, scratch), reps)
        rec["hc_depth%d" % depth] = entry(ts)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hc_compress.json"))
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, a.reps, a.blocks)), flush=True)
        return 0
    recs = []
    for name in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                                "--reps", str(a.reps), "--blocks", str(a.blocks)],
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
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/hc_bench.py", "reps": a.reps, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
