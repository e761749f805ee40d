#!/usr/bin/env python3
"""The LZ4 frame layer on one MI355X (include/ape_lz4f.h): first measurements,
no threshold.  Two shapes of the same kind of data (the benchmark's compressible synthetic
blocks, generated on the device): 16384 inputs of 64 KiB, and 16 inputs of 16 MiB.  Per shape,
in one process:

  xxh32        GiB/s of xxh32_batch over the inputs (one stream per input)
  compress     ms and input GiB/s of lz4f_compress_batch without checksums (flags 4: the
               content size only) and with all of them (flags 7), and the frames' ratio
  decompress   ms and output GiB/s of lz4f_decompress_batch on those frames, without the
               chained launch (flag 2: the frames are block-independent), verifying (flags 2)
               and not verifying (flags 3)
  blocks       beside them, compress_batch and decompress_batch (the plain block calls) on the
               same bytes cut into the same 64 KiB blocks

Times are medians of --reps by HIP events around the whole call, after one warm-up call.  Every
frame's decoded bytes are compared with the input on the device.  Each shape runs in a child
process of its own under a time limit; the first failure ends the run.  Prints one JSON line per
shape and writes profiles/lz4f.json (--out), one line.
usage: lz4f_bench.py [--reps 5] [--out FILE] [--shape NAME]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 65536
SHAPES = {"16384x64KiB": (16384, 1), "16x16MiB": (16, 256)}   # inputs, blocks per input
SHAPE_TIMEOUT = 400   # seconds per child
GIB = float(1 << 30)


def median_ms(torch, fn, reps):
    ts = []
    for _ in range(reps + 1):   # (the first call warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts[1:])[reps // 2]


def run_shape(name, reps):
    import torch
    import libapenetwork_amd as amd
    n, bpf = SHAPES[name]
    size = bpf * BLOCK
    total = n * size
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    blocks = torch.empty((n * bpf, BLOCK), dtype=torch.uint8, device="cuda")
    amd.synth_blocks(blocks, BLOCK, 0, 1)
    src = blocks.view(n, size)
    sptr, sizes = i64([src.data_ptr() + k * size for k in range(n)]), i32([size] * n)
    rate = lambda ms: round(total / GIB / (ms / 1e3), 2)
    rec = {"shape": name, "inputs": n, "input_bytes": size, "reps": reps}

    hashes = i32([0] * n)
    ms = median_ms(torch, lambda: amd.xxh32_batch(sptr, sizes, hashes), reps)
    rec["xxh32"] = {"ms": round(ms, 3), "GiB_s": rate(ms)}

    bound = amd.lz4f_compress_bound(size, 7)
    slot = (bound + 15) // 16 * 16
    frames = torch.empty((n, slot), dtype=torch.uint8, device="cuda")
    fptr, fcap, fres = i64([frames.data_ptr() + k * slot for k in range(n)]), i32([bound] * n), i32([0] * n)
    cscr = torch.empty(amd.lz4f_compress_scratch_size(n, size), dtype=torch.uint8, device="cuda")
    dscr = torch.empty(amd.lz4f_decompress_scratch_size(n, bpf), dtype=torch.uint8, device="cuda")
    back = torch.empty((n, size), dtype=torch.uint8, device="cuda")
    bptr, dres = i64([back.data_ptr() + k * size for k in range(n)]), i32([0] * n)
    for label, cflags in (("plain", 4), ("checksums", 7)):
        ms = median_ms(torch, lambda: amd.lz4f_compress_batch(sptr, sizes, fptr, fcap, fres, size,
                                                              cflags, cscr), reps)
        rs = fres.cpu().tolist()
        assert min(rs) > 0, min(rs)
        e = {"compress_ms": round(ms, 3), "compress_GiB_s": rate(ms),
             "ratio": round(total / sum(rs), 4)}
        for what, dflags in (("decompress_verify", 2), ("decompress_no_verify", 3)):
            back.zero_()
            ms = median_ms(torch, lambda: amd.lz4f_decompress_batch(fptr, fres, bptr, sizes, dres,
                                                                    bpf, dflags, dscr), reps)
            assert dres.cpu().tolist() == [size] * n, (label, what)
            assert torch.equal(back, src), (label, what)
            e[what + "_ms"], e[what + "_GiB_s"] = round(ms, 3), rate(ms)
        rec["frames_" + label] = e

    # the plain block calls on the same 64 KiB blocks
    nb = n * bpf
    bslot = (amd.compressBound(BLOCK) + 15) // 16 * 16
    comp = torch.empty((nb, bslot), dtype=torch.uint8, device="cuda")
    bsizes, csz, bres = i32([BLOCK] * nb), i32([0] * nb), i32([0] * nb)
    ms = median_ms(torch, lambda: amd.compress_batch(blocks, bsizes, comp, csz), reps)
    e = {"compress_ms": round(ms, 3), "compress_GiB_s": rate(ms),
         "ratio": round(total / int(csz.sum().item()), 4)}
    out = back.view(nb, BLOCK)
    out.zero_()
    ms = median_ms(torch, lambda: amd.decompress_batch(comp, csz, out, bres, dst_caps=bsizes), reps)
    assert torch.equal(out, blocks)
    e["decompress_ms"], e["decompress_GiB_s"] = round(ms, 3), rate(ms)
    rec["blocks"] = e
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4f.json"))
    ap.add_argument("--shape", help="run one shape in this process (used by the parent)")
    a = ap.parse_args()
    if a.shape:
        print(json.dumps(run_shape(a.shape, a.reps)), flush=True)
        return 0
    recs = []
    for name in SHAPES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name,
                                "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=SHAPE_TIMEOUT)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (name, SHAPE_TIMEOUT), file=sys.stderr)
            return 1
        if p.returncode != 0:
            print("%s: exit %d; stopping\n%s" % (name, p.returncode, p.stderr[-2000:]),
                  file=sys.stderr)
            return 1
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        recs.append(json.loads(line))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps({"tool": "tools/lz4f_bench.py", "shapes": recs}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
