#!/usr/bin/env python3
"""LZ4 frames with a dictionary on one MI355X (include/ape_lz4f_dict.h): what the
frame layer costs over the bare block calls.  The workload is tools/dict_bench.py's: 16384
messages of 1 KiB or 4 KiB cut from the 32 KiB that follow the first 61440 bytes of one `comp`
stream (tests/golden/inputs.py), that first part being the dictionary.  "64 dictionaries" are 64
prepared objects (and 64 table entries) with the same bytes at 64 addresses, message i naming
object i % 64: the footprint of 64 objects, not 64 kinds of content.

  compress  each mode's framed call beside its bare usingCDicts call on the same messages (the
            price of plan, layout, hash and pack; flags 7, an ID per frame), and the ratio of the
            frames beside the ratio of the blocks
  decode    the framed call (flag 4, verifying) on those frames beside
            decompress_safe_usingDict on the bare blocks, and beside itself with a table of 1,
            64 and 4096 entries whose match is the last one (the price of the lookup)

One process, the sides of a pair alternating rep by rep, medians of --reps by HIP events around
whole calls.  Prints one JSON line per case and writes --out.
usage: lz4f_dict_bench.py [--reps 7] [--out profiles/lz4f_dict.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DD, NB, DEPTH = 61440, 16384, 8


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


def run(L, ndict, reps):
    import numpy as np
    import torch
    import inputs as I
    import libapenetwork_amd as amd
    stream = I.make("comp", DD + 32768, seed=7)
    d = stream[:DD]
    distinct = [stream[DD + s:DD + s + L] for s in range(0, 32768, L)]
    total = NB * L
    dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    src = dev(b"".join(distinct) * (NB // len(distinct)))
    sptr = i64([src.data_ptr() + i * L for i in range(NB)])
    sizes = i32([L] * NB)
    slot = (amd.lz4f_compress_cdicts_bound(L, 7) + 15) // 16 * 16
    out = torch.empty(NB * slot, dtype=torch.uint8, device="cuda")
    optr, caps = i64([out.data_ptr() + i * slot for i in range(NB)]), i32([slot] * NB)
    bout = torch.empty(NB * slot, dtype=torch.uint8, device="cuda")
    bptr = i64([bout.data_ptr() + i * slot for i in range(NB)])
    fres, bres = i32([0] * NB), i32([0] * NB)
    dcopies = dev(d * ndict)
    dptr, dsz = i64([dcopies.data_ptr() + k * DD for k in range(ndict)]), i32([DD] * ndict)
    ids = i32([1 + i % ndict for i in range(NB)])
    rows = []
    for mode, name in ((0, "fast"), (1, "hc"), (2, "hc_opt")):
        osz = amd.cdict_size() if mode == 0 else amd.hc_cdict_size()
        objs = torch.empty(ndict * osz, dtype=torch.uint8, device="cuda")
        prepare = amd.cdict_prepare_batch if mode == 0 else amd.hc_cdict_prepare_batch
        prepare(dptr, dsz, L, objs, osz)
        cptr = i64([objs.data_ptr() + (i % ndict) * osz for i in range(NB)])
        fscr = torch.empty(amd.lz4f_compress_cdicts_scratch_size(NB, L, mode), dtype=torch.uint8,
                           device="cuda")
        if mode:
            bscr = torch.empty((amd.compress_hc_cdict_scratch_size if mode == 1 else
                                amd.compress_hc_opt_cdict_scratch_size)(NB, L), dtype=torch.uint8,
                               device="cuda")
        framed = lambda: amd.lz4f_compress_cdicts_batch(sptr, sizes, optr, caps, fres, cptr, ids, L,
                                                        mode, DEPTH if mode else 0, 7, fscr)
        if mode == 0:
            bare = lambda: amd.compress_cdicts_batch(sptr, sizes, bptr, caps, bres, cptr)
        else:
            f = amd.compress_hc_cdicts_batch if mode == 1 else amd.compress_hc_opt_cdicts_batch
            bare = lambda: f(sptr, sizes, bptr, caps, bres, cptr, L, DEPTH, bscr)
        ms = alternate(torch, [framed, bare], reps)
        fr, br = fres.cpu().tolist(), bres.cpu().tolist()
        assert min(fr) > 0 and min(br) > 0
        rows.append({"case": "compress_%s" % name, "msg": L, "dicts": ndict, "framed_ms": ms[0],
                     "bare_ms": ms[1], "framed_GiBps": total / ms[0] / 2 ** 30 * 1e3,
                     "bare_GiBps": total / ms[1] / 2 ** 30 * 1e3,
                     "frame_ratio": total / sum(fr), "block_ratio": total / sum(br)})
        print(json.dumps(rows[-1]), flush=True)
    # decode: the hc_opt frames and blocks of the last pass
    dst = torch.empty(NB * L, dtype=torch.uint8, device="cuda")
    tptr, room = i64([dst.data_ptr() + i * L for i in range(NB)]), i32([L] * NB)
    res = i32([0] * NB)
    mdptr, mdsz = i64([dcopies.data_ptr() + (i % ndict) * DD for i in range(NB)]), i32([DD] * NB)
    dscr = torch.empty(amd.lz4f_decompress_dicts_scratch_size(NB, 1, 4), dtype=torch.uint8,
                       device="cuda")
    calls, names = [], []
    for nt in (max(ndict, 1), 64, 4096):
        if nt < ndict or nt in names:
            continue
        # the keys the frames name are the table's last ndict entries
        keys = [1 << 20 | k for k in range(nt - ndict)] + [1 + k for k in range(ndict)]
        tid = i32(keys)
        tp = i64([dcopies.data_ptr()] * (nt - ndict) +
                 [dcopies.data_ptr() + k * DD for k in range(ndict)])
        tsz = i32([DD] * nt)
        calls.append(lambda tid=tid, tp=tp, tsz=tsz: amd.lz4f_decompress_dicts_batch(
            optr, fres, tptr, room, res, 1, tid, tp, tsz, 4, dscr))
        names.append(nt)
    calls.append(lambda: amd.decompress_dict_batch(bptr, bres, tptr, room, mdptr, mdsz, res))
    ms = alternate(torch, calls, reps)
    assert res.cpu().tolist() == [L] * NB
    calls[0]()
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [L] * NB and bytes(dst[:L].cpu().numpy()) == distinct[0]
    row = {"case": "decode", "msg": L, "dicts": ndict, "bare_usingDict_ms": ms[-1],
           "bare_GiBps": total / ms[-1] / 2 ** 30 * 1e3}
    for nt, t in zip(names, ms):
        row["framed_ntable%d_ms" % nt] = t
    row["framed_GiBps"] = total / ms[0] / 2 ** 30 * 1e3
    rows.append(row)
    print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4f_dict.json"))
    a = ap.parse_args()
    import torch
    rows = []
    for L in (1024, 4096):
        for ndict in (1, 64):
            rows += run(L, ndict, a.reps)
    doc = {"tool": "tools/lz4f_dict_bench.py", "device": torch.cuda.get_device_name(0),
           "messages": NB, "dictionary_bytes": DD, "depth": DEPTH, "reps": a.reps, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
