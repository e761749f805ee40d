#!/usr/bin/env python3
"""The calls of include/ape_lz4f_placed.h on one MI355X, on the benchmark's
compressible synthetic blocks generated on the device.  One process, the two sides of every
comparison alternating call by call, medians of --reps by HIP events around whole calls after a
warm-up call of each side:

  sizer    decompress_size_ptr_batch against decompress_ptr_batch on 16384 blocks of 64 KiB:
           ms of both and their quotient (below 1, or a dry run has no reason to exist)
  full     lz4f_decompress_placed_batch against lz4f_decompress_batch on full-block frames
           without checksums, 16384 x 64 KiB and 16 x 16 MiB (flags 3): the price of generality
  flushed  lz4f_decompress_placed_batch on 16 frames of 16 MiB written in 4 KiB and in 16 KiB
           pieces, one block per piece, independent and linked (matches reach into the pieces
           before): GiB/s of content.  No comparator: the existing call refuses them.
           maxBlocks = pieces per frame; it sets the scratch and, for a batch that may hold
           linked frames, the chained launch, in which one wave per frame walks maxBlocks slots.

Every decoded byte is compared with the input on the device.  Prints one JSON line per part
and writes profiles/lz4f_placed.json (--out), one line.
usage: lz4f_placed_bench.py [--reps 5] [--out FILE]"""
import argparse
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 65536
GIB = float(1 << 30)


def alternate_ms(torch, fns, reps):
    """Medians of `reps` timings of each fn, the fns taking turns; one warm-up turn."""
    ts = [[] for _ in fns]
    for r in range(reps + 1):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                ts[k].append(e0.elapsed_time(e1))
    return [sorted(t)[reps // 2] for t in ts]


def tensors(torch):
    return (lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda"),
            lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda"))


def part_sizer(torch, amd, reps):
    i32, i64 = tensors(torch)
    n = 16384
    blocks = torch.empty((n, BLOCK), dtype=torch.uint8, device="cuda")
    amd.synth_blocks(blocks, BLOCK, 0, 1)
    slot = (amd.compressBound(BLOCK) + 15) // 16 * 16
    comp = torch.empty((n, slot), dtype=torch.uint8, device="cuda")
    sizes, csz = i32([BLOCK] * n), i32([0] * n)
    amd.compress_batch(blocks, sizes, comp, csz)
    out = torch.zeros((n, BLOCK), dtype=torch.uint8, device="cuda")
    cptr = i64([comp.data_ptr() + k * slot for k in range(n)])
    optr = i64([out.data_ptr() + k * BLOCK for k in range(n)])
    dres, sres = i32([0] * n), i32([0] * n)
    ms_size, ms_dec = alternate_ms(torch, [
        lambda: amd.decompress_size_ptr_batch(cptr, csz, sizes, sres),
        lambda: amd.decompress_ptr_batch(cptr, csz, optr, sizes, dres)], reps)
    assert sres.cpu().tolist() == [BLOCK] * n == dres.cpu().tolist()
    assert torch.equal(out, blocks)
    return {"part": "sizer", "blocks": n, "block_bytes": BLOCK, "reps": reps,
            "ratio": round(n * BLOCK / int(csz.sum().item()), 4),
            "size_ms": round(ms_size, 3), "decompress_ms": round(ms_dec, 3),
            "size_over_decompress": round(ms_size / ms_dec, 3)}


def part_full(torch, amd, reps, n, bpf):
    i32, i64 = tensors(torch)
    size = bpf * BLOCK
    total = n * size
    blocks = torch.empty((n * bpf, BLOCK), dtype=torch.uint8, device="cuda")
    amd.synth_blocks(blocks, BLOCK, 0, 1)
    src = blocks.view(n, size)
    sptr, sizes = i64([src.data_ptr() + k * size for k in range(n)]), i32([size] * n)
    bound = amd.lz4f_compress_bound(size, 4)
    slot = (bound + 15) // 16 * 16
    frames = torch.empty((n, slot), dtype=torch.uint8, device="cuda")
    fptr, fcap, fres = i64([frames.data_ptr() + k * slot for k in range(n)]), i32([bound] * n), i32([0] * n)
    cscr = torch.empty(amd.lz4f_compress_scratch_size(n, size), dtype=torch.uint8, device="cuda")
    amd.lz4f_compress_batch(sptr, sizes, fptr, fcap, fres, size, 4, cscr)
    del cscr
    dscr = torch.empty(amd.lz4f_decompress_scratch_size(n, bpf), dtype=torch.uint8, device="cuda")
    pscr = torch.empty(amd.lz4f_decompress_placed_scratch_size(n, bpf), dtype=torch.uint8,
                       device="cuda")
    back = [torch.zeros((n, size), dtype=torch.uint8, device="cuda") for _ in range(2)]
    bptr = [i64([b.data_ptr() + k * size for k in range(n)]) for b in back]
    res = [i32([0] * n), i32([0] * n)]
    ms_placed, ms_grid = alternate_ms(torch, [
        lambda: amd.lz4f_decompress_placed_batch(fptr, fres, bptr[0], sizes, res[0], bpf, 3, pscr),
        lambda: amd.lz4f_decompress_batch(fptr, fres, bptr[1], sizes, res[1], bpf, 3, dscr)], reps)
    for r, b in zip(res, back):
        assert r.cpu().tolist() == [size] * n
        assert torch.equal(b, src)
    rate = lambda ms: round(total / GIB / (ms / 1e3), 2)
    return {"part": "full", "shape": "%dx%s" % (n, "64KiB" if bpf == 1 else "16MiB"), "reps": reps,
            "placed_ms": round(ms_placed, 3), "placed_GiB_s": rate(ms_placed),
            "existing_ms": round(ms_grid, 3), "existing_GiB_s": rate(ms_grid),
            "placed_over_existing": round(ms_placed / ms_grid, 3),
            "scratch_bytes": {"placed": pscr.numel(), "existing": dscr.numel()}}


def flushed_frames(torch, amd, src, n, size, piece, linked):
    """One frame per row of src, one block per piece, assembled on the host from the blocks
    compress_prefix_batch writes (a piece it does not shrink is stored)."""
    i32, i64 = tensors(torch)
    per = size // piece
    nb = n * per
    pos = [j * piece for j in range(per)] * n
    ptrs = i64([src.data_ptr() + f * size + j * piece for f in range(n) for j in range(per)])
    prefix = i32([min(p, BLOCK) if linked else 0 for p in pos])
    slot = (piece + 15) // 16 * 16
    comp = torch.empty((nb, slot), dtype=torch.uint8, device="cuda")
    cptr = i64([comp.data_ptr() + k * slot for k in range(nb)])
    res = i32([0] * nb)
    amd.compress_prefix_batch(ptrs, i32([piece] * nb), prefix, cptr, i32([piece - 1] * nb), res)
    torch.cuda.synchronize()
    rs, rows, content = res.cpu().tolist(), comp.cpu().numpy(), src.cpu().numpy()
    header = bytes.fromhex("04224d18") + (bytes([0x40, 0x40, 0xC0]) if linked else
                                           bytes([0x60, 0x40, 0x82]))
    frames, stored = [], 0
    for f in range(n):
        out = [header]
        for j in range(per):
            r = rs[f * per + j]
            if r > 0:
                out.append(struct.pack("<I", r) + rows[f * per + j, :r].tobytes())
            else:
                stored += 1
                out.append(struct.pack("<I", piece | 0x80000000) +
                           content[f, j * piece:(j + 1) * piece].tobytes())
        out.append(struct.pack("<I", 0))
        frames.append(b"".join(out))
    return frames, stored


def part_flushed(torch, amd, reps, piece, linked):
    import numpy as np
    i32, i64 = tensors(torch)
    n, size = 16, 256 * BLOCK
    per = size // piece
    blocks = torch.empty((n * 256, BLOCK), dtype=torch.uint8, device="cuda")
    amd.synth_blocks(blocks, BLOCK, 0, 1)
    src = blocks.view(n, size)
    frames, stored = flushed_frames(torch, amd, src, n, size, piece, linked)
    offs, at = [], 0
    for fr in frames:
        offs.append(at)
        at += (len(fr) + 15) // 16 * 16
    host = np.zeros(at, dtype=np.uint8)
    for o, fr in zip(offs, frames):
        host[o:o + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    fptr, fsz = i64([dev.data_ptr() + o for o in offs]), i32([len(fr) for fr in frames])
    back = torch.zeros((n, size), dtype=torch.uint8, device="cuda")
    bptr, caps, res = i64([back.data_ptr() + k * size for k in range(n)]), i32([size] * n), i32([0] * n)
    pscr = torch.empty(amd.lz4f_decompress_placed_scratch_size(n, per), dtype=torch.uint8,
                       device="cuda")
    flags = 1 if linked else 3
    (ms,) = alternate_ms(torch, [lambda: amd.lz4f_decompress_placed_batch(
        fptr, fsz, bptr, caps, res, per, flags, pscr)], reps)
    assert res.cpu().tolist() == [size] * n
    assert torch.equal(back, src)
    return {"part": "flushed", "frames": n, "content_bytes": size, "piece_bytes": piece,
            "linked": linked, "max_blocks": per, "stored_blocks": stored, "reps": reps,
            "ratio": round(n * size / sum(len(fr) for fr in frames), 4),
            "placed_ms": round(ms, 3), "content_GiB_s": round(n * size / GIB / (ms / 1e3), 2),
            "scratch_bytes": pscr.numel()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4f_placed.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "medians of at least 5"
    import torch
    import libapenetwork_amd as amd
    recs = []
    for part in ([lambda: part_sizer(torch, amd, a.reps),
                  lambda: part_full(torch, amd, a.reps, 16384, 1),
                  lambda: part_full(torch, amd, a.reps, 16, 256)] +
                 [lambda p=p, l=l: part_flushed(torch, amd, a.reps, p, l)
                  for p in (4096, 16384) for l in (False, True)]):
        recs.append(part())
        print(json.dumps(recs[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps({"tool": "tools/lz4f_placed_bench.py", "parts": recs}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
