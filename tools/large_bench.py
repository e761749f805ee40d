#!/usr/bin/env python3
"""APE_LZ4_compress_large_batch_dev on one MI355X: 16 inputs of 16 MiB and 256 inputs of
1 MiB, on device-synthesised App. C blocks laid end to end ("appC") and on the torch/lib
slice tools/ratio_files.py uses ("sobin").  Per case:

  large        the whole call (GiB/s of input, median of --reps by HIP events) and its ratio
  stages       plan / encode / offsets / stitch of one call (APE_LZ4_compress_large_timed_dev)
  prefix       the same slices through compress_withPrefix_batch_dev alone: what the stitch
               (plan + offsets + stitch + scratch traffic) costs on top
  blocks64k    the same bytes through compress_batch_dev as independent 64 KiB blocks (not
               one LZ4 block; the ratio without history beyond the block)
  host         one input through the one-shot host codec (what a caller gets today)
  ref_ratio    the reference's compress_default ratio on one input (oracle/_ref, when built)

--decode runs the way back instead (profiles/large_indexed.json): per case and restart period
R in {128 KiB, 256 KiB, 1 MiB}, compress_large_indexed, then

  ratio_vs_R0  the block's size with R = 0 over its size with R (what the restart points cost)
  indexed      decompress_indexed_ptr_batch, one wave per segment
  plain        decompress_ptr_batch on the same blocks, one wave per block

both decoders warmed up, then timed alternately (HIP events, median of --reps each); the
output of each is compared with the source.

--range reads byte ranges instead (profiles/large_range.json): 16 x 16 MiB of App. C blocks, of
the torch/lib slice and of random bytes, compress_large_indexed at R = 256 KiB, then
decompress_range_indexed_ptr_batch for

  4KiB     4096 requests of 4 KiB at random offsets of random blocks
  1MiB     256 requests of 1 MiB
  whole    one request (0, n) per block

each sized by the documented retry (capacity 0 gives ERANGE and need), warmed up, compared with
the source, then timed by HIP events (median of 7) alternately with decompress_indexed_ptr_batch
of the same blocks -- the only other way to those bytes.

Each case runs in a child process of its own under a time limit; the first failure ends the
run.  Prints one JSON line per case and writes profiles/large_compress.json (--out).
usage: large_bench.py [--decode | --range] [--reps 5] [--out FILE] [--case NAME]"""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MB = 1 << 20
CASES = {"appC_16x16MiB": ("appC", 16, 16 * MB), "appC_256x1MiB": ("appC", 256, MB),
         "sobin_16x16MiB": ("sobin", 16, 16 * MB), "sobin_256x1MiB": ("sobin", 256, MB),
         "pysrc_16x4MiB": ("pysrc", 16, 4 * MB)}
CASE_TIMEOUT = 240   # seconds per child


def sobin(nbytes):
    import torch
    so = os.path.join(os.path.dirname(torch.__file__), "lib")
    big = sorted(glob.glob(so + "/*.so"), key=os.path.getsize)[-1]
    with open(big, "rb") as f:
        f.seek(50 << 20)
        return f.read(nbytes)


def median_ms(torch, fn, reps):
    ts = []
    for _ in range(reps + 1):   # (the first call warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = sorted(ts[1:])
    return ts[len(ts) // 2]


def run_case(name, reps):
    import numpy as np
    import torch
    import libapenetwork_amd as amd
    kind, nin, n = CASES[name]
    total = nin * n
    S = amd.compress_large_slice_size()
    flat = torch.empty(total, dtype=torch.uint8, device="cuda")
    fill(torch, np, kind, flat, n)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    bound = amd.compressBound(n)
    slot = (bound + 15) // 16 * 16
    out = torch.empty(nin * slot, dtype=torch.uint8, device="cuda")
    sptr = i64([flat.data_ptr() + i * n for i in range(nin)])
    dptr = i64([out.data_ptr() + i * slot for i in range(nin)])
    sizes, caps, res = i32([n] * nin), i32([bound] * nin), i32([0] * nin)
    scr = torch.empty(amd.compress_large_scratch_size(nin, n), dtype=torch.uint8, device="cuda")
    rec = {"case": name, "inputs": nin, "input_bytes": n, "slice": S, "scratch_bytes": scr.numel()}
    gibs = lambda ms: round(total / (ms * 1e-3) / (1 << 30), 2)

    def large():
        amd.compress_large_ptr_batch(sptr, sizes, dptr, caps, res, n, scratch=scr)
    ms = median_ms(torch, large, reps)
    rs = res.cpu().tolist()
    assert min(rs) > 0, rs
    # (ratio_input0: the input the host codec and the reference compress below)
    rec["large"] = {"ms": round(ms, 3), "GiBps": gibs(ms), "ratio": round(total / sum(rs), 4),
                    "ratio_input0": round(n / rs[0], 4)}
    # the block is valid: input 0 through the host decoder
    blk0 = out[:rs[0]].cpu().numpy().tobytes()
    src0 = flat[:n].cpu().numpy().tobytes()
    r, back = amd.decompress_safe(blk0, n)
    assert r == n and back == src0, "host decode of the large block"

    ms4 = (C.c_float * 4)()
    f = amd.lib().APE_LZ4_compress_large_timed_dev
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    best = None
    for _ in range(3):
        rc = f(sptr.data_ptr(), sizes.data_ptr(), dptr.data_ptr(), caps.data_ptr(), res.data_ptr(),
               nin, n, 1, scr.data_ptr(), scr.numel(), torch.cuda.current_stream().cuda_stream, ms4)
        assert rc == 0, amd.gpu_last_error()
        if best is None or sum(ms4) < sum(best):
            best = list(ms4)
    rec["stages_ms"] = dict(zip(("plan", "encode", "offsets", "stitch"), (round(x, 3) for x in best)))

    # the same slices through withPrefix alone (outputs to slots of their own)
    starts = [(i, st) for i in range(nin) for st in range(0, n, S)]
    lens = [min(S, n - st) for _, st in starts]
    sb = (amd.compressBound(S) + 15) // 16 * 16
    pout = torch.empty(len(starts) * sb, dtype=torch.uint8, device="cuda")
    pp = i64([flat.data_ptr() + i * n + st for i, st in starts])
    pd = i64([pout.data_ptr() + q * sb for q in range(len(starts))])
    pl, pre, pc, pr = i32(lens), i32([st for _, st in starts]), i32([sb] * len(starts)), i32([0] * len(starts))
    ms = median_ms(torch, lambda: amd.compress_prefix_batch(pp, pl, pre, pd, pc, pr), reps)
    rec["prefix"] = {"ms": round(ms, 3), "GiBps": gibs(ms), "slices": len(starts),
                     "ratio_unstitched": round(total / int(pr.sum()), 4)}
    rec["stitch_overhead_pct"] = round(100 * (rec["large"]["ms"] / ms - 1), 1)
    del pout

    # independent 64 KiB blocks
    nb = total // 65536
    bslot = (amd.compressBound(65536) + 15) // 16 * 16
    bout = torch.empty((nb, bslot), dtype=torch.uint8, device="cuda")
    bs, br = i32([65536] * nb), i32([0] * nb)
    ms = median_ms(torch, lambda: amd.compress_batch(flat.view(nb, 65536), bs, bout, br), reps)
    rec["blocks64k"] = {"ms": round(ms, 3), "GiBps": gibs(ms), "ratio": round(total / int(br.sum()), 4)}

    # one input through the one-shot host codec (routing default: every one-shot on the host)
    hin, hout = C.create_string_buffer(src0, n), C.create_string_buffer(bound)
    t0 = time.perf_counter()
    r = amd.lib().APE_LZ4_compress_default(hin, hout, n, bound)
    dt = time.perf_counter() - t0
    assert r > 0
    rec["host_oneshot"] = {"ms": round(dt * 1e3, 2), "GiBps": round(n / dt / (1 << 30), 3),
                           "ratio": round(n / r, 4)}
    rec["large_vs_host_speedup"] = round(rec["large"]["GiBps"] / rec["host_oneshot"]["GiBps"], 1)
    refp = os.path.join(ROOT, "oracle", "_ref", "libape_lz4_ref.so")
    if os.path.exists(refp):
        ref = C.CDLL(refp)
        o = C.create_string_buffer(bound)
        rec["ref_ratio"] = round(n / ref.APE_LZ4_compress_default(src0, o, n, bound), 4)
        rec["ratio_vs_ref"] = round(rec["large"]["ratio_input0"] / rec["ref_ratio"], 4)
    return rec


def fill(torch, np, kind, flat, n):
    """The case's inputs, laid end to end in flat."""
    import libapenetwork_amd as amd
    if kind == "appC":
        amd.synth_blocks(flat.view(-1, 65536), 65536, 0, 1)
    elif kind == "rand":
        g = torch.Generator(device="cuda")
        g.manual_seed(20264)
        flat[:] = torch.randint(0, 256, (flat.numel(),), dtype=torch.uint8, device="cuda", generator=g)
    elif kind == "pysrc":   # ratio_files.py's other corpus: 4 MiB of Python sources, repeated
        py = b"".join(open(f, "rb").read() for f in sorted(glob.glob("/usr/lib/python3.10/*.py")))
        assert len(py) >= n, "Python sources shorter than 4 MiB"
        flat.view(-1, n)[:] = torch.from_numpy(np.frombuffer(py[:n], dtype=np.uint8).copy()).cuda()
    else:
        one = torch.from_numpy(np.frombuffer(sobin(16 * MB), dtype=np.uint8).copy()).cuda()
        assert one.numel() == 16 * MB, "torch/lib slice shorter than 16 MiB"
        flat.view(-1, 16 * MB)[:] = one
    torch.cuda.synchronize()


DECODE_R = (128 << 10, 256 << 10, MB)


def run_decode_case(name, reps):
    import numpy as np
    import torch
    import libapenetwork_amd as amd
    kind, nin, n = CASES[name]
    total = nin * n
    flat = torch.empty(total, dtype=torch.uint8, device="cuda")
    fill(torch, np, kind, flat, n)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    bound = amd.compressBound(n)
    slot = (bound + 15) // 16 * 16
    out = torch.empty(nin * slot, dtype=torch.uint8, device="cuda")
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    sptr = i64([flat.data_ptr() + i * n for i in range(nin)])
    dptr = i64([out.data_ptr() + i * slot for i in range(nin)])
    bptr = i64([back.data_ptr() + i * n for i in range(nin)])
    sizes, caps, res, dres = i32([n] * nin), i32([bound] * nin), i32([0] * nin), i32([0] * nin)
    scr = torch.empty(amd.compress_large_scratch_size(nin, n), dtype=torch.uint8, device="cuda")
    rec = {"case": name, "inputs": nin, "input_bytes": n, "slice": amd.compress_large_slice_size(),
           "periods": []}
    gibs = lambda ms: round(total / (ms * 1e-3) / (1 << 30), 2)
    size0 = None
    for R in (0,) + DECODE_R:
        nseg = amd.large_index_segments(n, R)
        index = torch.zeros((nin, amd.large_index_size(n, R)), dtype=torch.uint8, device="cuda")
        amd.compress_large_indexed_ptr_batch(sptr, sizes, dptr, caps, res, n, R, index=index,
                                             scratch=scr)
        torch.cuda.synchronize()
        rs = res.cpu().tolist()
        assert min(rs) > 0, rs
        if R == 0:
            size0 = sum(rs)
            continue

        def check(what):
            torch.cuda.synchronize()
            assert dres.cpu().tolist() == [n] * nin, (what, dres.cpu().tolist())
            assert torch.equal(back, flat), what
            back.zero_()

        indexed = lambda: amd.decompress_indexed_ptr_batch(dptr, res, bptr, sizes, index, nseg, dres)
        plain = lambda: amd.decompress_ptr_batch(dptr, res, bptr, sizes, dres)
        for what, fn in (("indexed", indexed), ("plain", plain)):   # warm-up, checked
            fn()
            check(what)
        ts = {"indexed": [], "plain": []}
        for _ in range(reps):   # alternately
            for what, fn in (("indexed", indexed), ("plain", plain)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts[what].append(e0.elapsed_time(e1))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        rec["periods"].append({
            "R": R, "segments": nseg, "ratio": round(total / sum(rs), 4),
            "ratio_R0": round(total / size0, 4), "ratio_vs_R0": round(size0 / sum(rs), 4),
            "indexed": {"ms": round(med["indexed"], 3), "GiBps": gibs(med["indexed"]),
                        "min_ms": round(min(ts["indexed"]), 3), "max_ms": round(max(ts["indexed"]), 3)},
            "plain": {"ms": round(med["plain"], 3), "GiBps": gibs(med["plain"]),
                      "min_ms": round(min(ts["plain"]), 3), "max_ms": round(max(ts["plain"]), 3)},
            "speedup": round(med["plain"] / med["indexed"], 2)})
    return rec


RANGE_CASES = {"appC_16x16MiB": ("appC", 16, 16 * MB), "sobin_16x16MiB": ("sobin", 16, 16 * MB),
               "rand_16x16MiB": ("rand", 16, 16 * MB)}
RANGE_R = 256 << 10
RANGE_REPS = 7
# name: (requests, bytes each (0: the whole block), waves per request)
RANGE_MODES = {"4KiB": (4096, 4096, 2), "1MiB": (256, MB, 6), "whole": (0, 0, 64)}


def run_range_case(name, reps):
    import numpy as np
    import torch
    import libapenetwork_amd as amd
    kind, nin, n = RANGE_CASES[name]
    total, R = nin * n, RANGE_R
    flat = torch.empty(total, dtype=torch.uint8, device="cuda")
    fill(torch, np, kind, flat, n)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    bound = amd.compressBound(n)
    slot = (bound + 15) // 16 * 16
    out = torch.empty(nin * slot, dtype=torch.uint8, device="cuda")
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    sptr = i64([flat.data_ptr() + i * n for i in range(nin)])
    dptr = i64([out.data_ptr() + i * slot for i in range(nin)])
    bptr = i64([back.data_ptr() + i * n for i in range(nin)])
    sizes, caps, res, dres = i32([n] * nin), i32([bound] * nin), i32([0] * nin), i32([0] * nin)
    scr = torch.empty(amd.compress_large_scratch_size(nin, n), dtype=torch.uint8, device="cuda")
    nseg = amd.large_index_segments(n, R)
    index = torch.zeros((nin, amd.large_index_size(n, R)), dtype=torch.uint8, device="cuda")
    amd.compress_large_indexed_ptr_batch(sptr, sizes, dptr, caps, res, n, R, index=index, scratch=scr)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    assert min(rs) > 0, rs
    rec = {"case": name, "inputs": nin, "input_bytes": n, "R": R, "segments": nseg,
           "ratio": round(total / sum(rs), 4), "reps": reps, "modes": {}}

    def whole():
        amd.decompress_indexed_ptr_batch(dptr, res, bptr, sizes, index, nseg, dres)
    whole()
    torch.cuda.synchronize()
    assert dres.cpu().tolist() == [n] * nin and torch.equal(back, flat), "whole-block decode"
    rng = np.random.default_rng(20264)
    for mode, (nreq, size, waves) in RANGE_MODES.items():
        if nreq:
            blk = rng.integers(0, nin, nreq).tolist()
            st = rng.integers(0, n - size + 1, nreq).tolist()
        else:
            nreq, size, blk, st = nin, n, list(range(nin)), [0] * nin
        block_of, starts, lens = i32(blk), i32(st), i32([size] * nreq)
        win, rres = i32([0] * (2 * nreq)), i32([0] * nreq)
        none = i64([0] * nreq)

        def read(dst, rcaps):
            amd.decompress_range_indexed_ptr_batch(dptr, res, index, nseg, starts, lens, dst, rcaps,
                                                   win, rres, block_of=block_of,
                                                   waves_per_request=waves)
        read(none, i32([0] * nreq))   # the documented retry: ERANGE and the bytes needed
        torch.cuda.synchronize()
        assert rres.cpu().tolist() == [amd.ERANGE] * nreq
        need = win.cpu().tolist()[1::2]
        offs = np.concatenate(([0], np.cumsum([(c + 15) // 16 * 16 for c in need]))).tolist()
        buf = torch.empty(offs[-1], dtype=torch.uint8, device="cuda")
        rptr, rcaps = i64([buf.data_ptr() + o for o in offs[:-1]]), i32(need)
        read(rptr, rcaps)             # warm-up, checked
        torch.cuda.synchronize()
        assert rres.cpu().tolist() == [size] * nreq, mode
        w0 = win.cpu().tolist()[0::2]
        for q in range(nreq):
            got = buf[offs[q] + w0[q]:offs[q] + w0[q] + size]
            assert torch.equal(got, flat[blk[q] * n + st[q]:blk[q] * n + st[q] + size]), (mode, q)
        ts = {"range": [], "whole": []}
        for _ in range(reps):   # alternately
            for what, fn in (("range", lambda: read(rptr, rcaps)), ("whole", whole)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts[what].append(e0.elapsed_time(e1))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        rec["modes"][mode] = {
            "requests": nreq, "bytes_each": size, "waves_per_request": waves,
            "need_bytes": int(sum(need)), "need_max": int(max(need)),
            "range_ms": round(med["range"], 4), "range_min_ms": round(min(ts["range"]), 4),
            "range_max_ms": round(max(ts["range"]), 4),
            "whole_blocks_ms": round(med["whole"], 4), "whole_min_ms": round(min(ts["whole"]), 4),
            "whole_max_ms": round(max(ts["whole"]), 4),
            "range_vs_whole": round(med["range"] / med["whole"], 4)}
        del buf
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--decode", action="store_true", help="the decode leg (see above)")
    ap.add_argument("--range", action="store_true", dest="ranges", help="the range leg (see above)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    a = ap.parse_args()
    leg = "--range" if a.ranges else "--decode" if a.decode else ""
    if a.ranges:
        a.reps = RANGE_REPS
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", {"--range": "large_range.json", "--decode": "large_indexed.json",
                                                "": "large_compress.json"}[leg])
    if a.case:
        run = {"--range": run_range_case, "--decode": run_decode_case, "": run_case}[leg]
        print(json.dumps(run(a.case, a.reps)), flush=True)
        return 0
    recs = []
    for name in (RANGE_CASES if a.ranges else CASES):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                                "--reps", str(a.reps)] + ([leg] if leg else []),
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
        json.dump({"tool": ("tools/large_bench.py " + leg).strip(),
                   "reps": a.reps, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
