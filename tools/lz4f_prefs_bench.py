#!/usr/bin/env python3
"""Framed compress with preferences on one MI355X (include/ape_lz4f_prefs.h): what
the block-size ID and the mode buy in ratio, what the frame layer costs over the bare large-input
call, and what the ID costs the reader.

Input: 16 x 16 MiB of SURVEY App. C data, of the concatenated Python 3.10 standard-library
sources and of the largest shared library under torch/lib from its 50th MiB on (the files of
tools/ratio_files.py; the sources are 4.5 MiB and are repeated to 256 MiB, which no LZ4 match
can see: offsets end at 64 KiB).  For block-size IDs 4..7 x modes {0; 1 and 2 at depth 8}:

  framed     APE_LZ4_lz4f_compress_prefs_batch_dev, flags 4 (content size, no checksums)
  bare       the mode's large-input call on the same block ranges with capacity len - 1, as one
             batch of 16 x 16 MiB / B inputs of B bytes (a block it answers with 0 counts as
             stored in the ratio)
  decode     APE_LZ4_lz4f_decompress_batch_dev, verifying, on the frames produced.  It decodes
             one block per wave, so ID 7 has 64 times fewer waves than ID 4 on the same bytes:
             expect it to be far slower.  The figure is there as advice on choosing the ID.
  existing   at ID 4 mode 0 also APE_LZ4_lz4f_compress_batch_dev beside compress_batch on the
             64 KiB blocks: the yardstick for the frame layer's overhead

One process, the sides of a pair alternating rep by rep, medians of --reps (at least 5) by HIP
events around whole calls.  Prints one JSON line per case and writes --out.
usage: lz4f_prefs_bench.py [--reps 5] [--out profiles/lz4f_prefs.json] [--mib 16] [--frames 16]"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEPTH = 8


def alternate(torch, fns, reps):
    """median ms of each fn, run in turn reps + 1 times (the first round warms up)"""
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
    return [sorted(t)[len(t) // 2] for t in ts]


def datasets(torch, amd, total):
    import numpy as np
    out = {}
    src = torch.empty((total // 65536, 65536), dtype=torch.uint8, device="cuda")
    amd.synth_blocks(src, 65536, 0, 1)
    out["appC"] = src.view(-1)
    py = b"".join(open(f, "rb").read() for f in sorted(glob.glob("/usr/lib/python3.10/*.py")))
    if py:
        out["pysrc"] = torch.from_numpy(np.frombuffer((py * (total // len(py) + 1))[:total],
                                                      dtype=np.uint8).copy()).cuda()
    libs = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "*.so")),
                  key=os.path.getsize)
    if libs and os.path.getsize(libs[-1]) >= (50 << 20) + total:
        with open(libs[-1], "rb") as f:
            f.seek(50 << 20)
            out["sobin"] = torch.from_numpy(np.frombuffer(f.read(total), dtype=np.uint8).copy()).cuda()
    return out


def run(torch, amd, name, src, nframes, n, reps):
    i32 = lambda xs: torch.tensor(list(xs), dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(list(xs), dtype=torch.int64, device="cuda")
    total = nframes * n
    sptr, sizes = i64(src.data_ptr() + f * n for f in range(nframes)), i32([n] * nframes)
    slot = (amd.lz4f_compress_prefs_bound(n, 4, 4) + 15) // 16 * 16
    out = torch.empty(nframes * slot, dtype=torch.uint8, device="cuda")
    optr, caps = i64(out.data_ptr() + f * slot for f in range(nframes)), i32([slot] * nframes)
    fres, dres = i32([0] * nframes), i32([0] * nframes)
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    kptr = i64(back.data_ptr() + f * n for f in range(nframes))
    bout = torch.empty(total, dtype=torch.uint8, device="cuda")
    rows = []
    for bsid in (4, 5, 6, 7):
        B = 1 << (8 + 2 * bsid)
        nb = total // B                    # (n is a multiple of every B)
        bptr, bsz = i64(src.data_ptr() + q * B for q in range(nb)), i32([B] * nb)
        bdst, bcap = i64(bout.data_ptr() + q * B for q in range(nb)), i32([B - 1] * nb)
        bres = i32([0] * nb)
        dscr = torch.empty(amd.lz4f_decompress_scratch_size(nframes, n // B), dtype=torch.uint8,
                           device="cuda")
        for mode, mname in ((0, "fast"), (1, "hc"), (2, "hc_opt")):
            depth = DEPTH if mode else 0
            fscr = torch.empty(amd.lz4f_compress_prefs_scratch_size(nframes, n, bsid, mode, 0),
                               dtype=torch.uint8, device="cuda")
            framed = lambda: amd.lz4f_compress_prefs_batch(sptr, sizes, optr, caps, fres, n, bsid,
                                                           mode, depth, 4, fscr)
            if mode == 0:
                bscr = torch.empty(amd.compress_large_scratch_size(nb, B), dtype=torch.uint8,
                                   device="cuda")
                bare = lambda: amd.compress_large_ptr_batch(bptr, bsz, bdst, bcap, bres, B, 1, bscr)
            else:
                size_fn, f = ((amd.compress_large_hc_scratch_size, amd.compress_large_hc_ptr_batch)
                              if mode == 1 else (amd.compress_large_hc_opt_scratch_size,
                                                 amd.compress_large_hc_opt_ptr_batch))
                bscr = torch.empty(size_fn(nb, B, 0), dtype=torch.uint8, device="cuda")
                bare = lambda: f(bptr, bsz, bdst, bcap, bres, B, DEPTH, scratch=bscr)
            ms = alternate(torch, [framed, bare], reps)
            fr, br = fres.cpu().tolist(), bres.cpu().tolist()
            assert min(fr) > 0 and min(br) >= 0
            decode = lambda: amd.lz4f_decompress_batch(optr, fres, kptr, sizes, dres, n // B, 2, dscr)
            dms = alternate(torch, [decode], reps)[0]
            assert dres.cpu().tolist() == [n] * nframes and torch.equal(back, src[:total])
            row = {"case": "%s_id%d_%s" % (name, bsid, mname), "data": name, "bsid": bsid,
                   "mode": mode, "depth": depth, "framed_ms": ms[0], "bare_ms": ms[1],
                   "overhead": ms[0] / ms[1] - 1.0, "framed_GiBps": total / ms[0] / 2 ** 30 * 1e3,
                   "frame_ratio": total / sum(fr),
                   "block_ratio": total / sum(r if r > 0 else B for r in br),
                   "stored_blocks": sum(1 for r in br if r == 0), "decode_ms": dms,
                   "decode_GiBps": total / dms / 2 ** 30 * 1e3}
            if bsid == 4 and mode == 0:     # the yardstick: the existing framed call over compress_batch
                oscr = torch.empty(amd.lz4f_compress_scratch_size(nframes, n), dtype=torch.uint8,
                                   device="cuda")
                rows2d, cslot = src[:total].view(nb, B), (amd.compressBound(B) + 15) // 16 * 16
                comp = torch.empty((nb, cslot), dtype=torch.uint8, device="cuda")
                old = lambda: amd.lz4f_compress_batch(sptr, sizes, optr, caps, fres, n, 4, oscr)
                plain = lambda: amd.compress_batch(rows2d, bsz, comp, bres)
                oms = alternate(torch, [old, plain, framed], reps)
                assert fres.cpu().tolist() == fr
                row.update({"existing_framed_ms": oms[0], "compress_batch_ms": oms[1],
                            "existing_overhead": oms[0] / oms[1] - 1.0,
                            "framed_ms_beside_existing": oms[2]})
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4f_prefs.json"))
    a = ap.parse_args()
    assert a.reps >= 5 and a.mib % 4 == 0
    import torch
    import libapenetwork_amd as amd
    n = a.mib << 20
    rows = []
    for name, src in datasets(torch, amd, a.frames * n).items():
        rows += run(torch, amd, name, src, a.frames, n, a.reps)
    doc = {"tool": "tools/lz4f_prefs_bench.py", "device": torch.cuda.get_device_name(0),
           "frames": a.frames, "frame_bytes": n, "depth": DEPTH, "flags": 4, "reps": a.reps,
           "slice": amd.compress_large_slice_size(), "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
