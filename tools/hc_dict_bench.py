#!/usr/bin/env python3
"""The high-ratio mode against a prepared dictionary on one MI355X: 16384 independent 1 KiB and
4 KiB messages, one 61440-byte dictionary, depths 8 and 64.  Dictionary and messages are cut
from one stream of the `comp` generator as tools/dict_bench.py cuts them: the dictionary is the
stream's first 61440 bytes, the messages are the 32 KiB that follow, cut every L bytes and
repeated across the batch (each copy at its own address; blocks are independent, so repetition
changes no block's work).  Per case, in one process, ms per call (median of --reps by HIP
events, with min and max), GiB/s of MESSAGE bytes and the ratio of:

  hc_cdict  (a) compress_hc_usingCDict_batch_dev on a prepared high-ratio dictionary, per depth,
            and the one-off hc_cdict_prepare time
  staged    (b) the only way before: a staging copy [dictionary | message] per message (two
            torch copies, timed), then compress_hc_withPrefix_batch_dev in its passes of 1024
            blocks, per depth
  cdict     (c) the fast compress_usingCDict_batch_dev

Every output is decoded on the GPU with decompress_safe_usingDict and the original dictionary
and compared with the messages; (a)'s bytes are compared with (b)'s.  Each case runs in a child
process of its own under a time limit; the first failure ends the run.  Prints one JSON line
per case and writes profiles/hc_dict_compress.json (--out).
usage: hc_dict_bench.py [--reps 5] [--messages 16384] [--out FILE] [--case NAME]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DD = 61440
CASES = {"msg1KiB": 1024, "msg4KiB": 4096}
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


def run_case(name, reps, nb):
    import numpy as np
    import torch
    import inputs as I
    import libapenetwork_amd as amd
    L = CASES[name]
    stream = I.make("comp", DD + 32768, seed=7)
    d = stream[:DD]
    distinct = [stream[DD + s:DD + s + L] for s in range(0, 32768, L)]
    k = len(distinct)
    assert nb % k == 0, (nb, k)
    total = nb * L
    dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device="cuda")
    ddict = dev(d)
    msgs = dev(b"".join(distinct)).view(k, L).repeat(nb // k, 1).contiguous()
    bound = amd.compressBound(L)
    slot = (bound + 15) // 16 * 16
    out = torch.empty((nb, slot), dtype=torch.uint8, device="cuda")
    back = torch.empty((nb, L), dtype=torch.uint8, device="cuda")
    sizes, caps, res, dres = i32([L] * nb), i32([bound] * nb), i32([0] * nb), i32([0] * nb)
    sptr = i64([msgs.data_ptr() + i * L for i in range(nb)])
    dptr = i64([out.data_ptr() + i * slot for i in range(nb)])
    bptr = i64([back.data_ptr() + i * L for i in range(nb)])
    dictp, dicts = i64([ddict.data_ptr()] * nb), i32([DD] * nb)
    D = amd.hc_cdict_window(DD, L)
    rec = {"case": name, "messages": nb, "message_bytes": L, "distinct_messages": k,
           "dict_bytes": DD, "window": D}

    def entry(ts):
        """The call's figures, after its output went through the GPU's usingDict decoder."""
        rs = res.cpu().tolist()
        assert min(rs) > 0, min(rs)
        back.zero_()
        amd.decompress_dict_batch(dptr, res, bptr, sizes, dictp, dicts, dres)
        torch.cuda.synchronize()
        assert bool((dres == L).all()) and bool(torch.equal(back, msgs)), "usingDict round trip"
        med = ts[len(ts) // 2]
        e = {"ms": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
             "GiBps": round(total / (med * 1e-3) / (1 << 30), 3), "ratio": round(total / sum(rs), 4)}
        return e

    # (a) the prepared high-ratio dictionary
    obj = torch.empty(amd.hc_cdict_size(), dtype=torch.uint8, device="cuda")
    tp = times_ms(torch, lambda: amd.hc_cdict_prepare(ddict, L, obj), reps)
    scratch = torch.empty(amd.compress_hc_cdict_scratch_size(nb, L), dtype=torch.uint8, device="cuda")
    rec["hc_cdict"] = {"prepare_ms": round(tp[len(tp) // 2], 4), "object_bytes": obj.numel(),
                       "scratch_bytes": scratch.numel()}
    blocks = {}
    for depth in DEPTHS:
        ts = times_ms(torch, lambda: amd.compress_hc_cdict_batch(sptr, sizes, dptr, caps, res, obj, L,
                                                                 depth, scratch), reps)
        rec["hc_cdict"]["depth%d" % depth] = entry(ts)
        blocks[depth] = (res.clone(), out.clone())   # for the comparison with (b)'s
    del scratch

    # (b) staged [dictionary tail | message] + compress_hc_withPrefix
    stage = torch.empty((nb, D + L), dtype=torch.uint8, device="cuda")
    tail = ddict[DD - D:]

    def copy():
        stage[:, :D] = tail
        stage[:, D:] = msgs
    tc = times_ms(torch, copy, reps)
    pp = i64([stage.data_ptr() + i * (D + L) + D for i in range(nb)])
    pre = i32([D] * nb)
    hscr = torch.empty(amd.compress_hc_scratch_size(nb), dtype=torch.uint8, device="cuda")
    med = lambda ts: ts[len(ts) // 2]
    rec["staged"] = {"copy": {"ms": round(med(tc), 4), "ms_min": round(tc[0], 4),
                              "ms_max": round(tc[-1], 4)},
                     "staging_bytes": stage.numel(), "scratch_bytes": hscr.numel()}
    for depth in DEPTHS:
        ts = times_ms(torch, lambda: amd.compress_hc_prefix_ptr_batch(pp, sizes, pre, dptr, caps, res,
                                                                      depth, hscr), reps)
        e = entry(ts)
        e["ms_copy_plus_encode"] = round(med(tc) + e["ms"], 4)
        rec["staged"]["depth%d" % depth] = e
        ares, aout = blocks.pop(depth)
        assert bool(torch.equal(ares, res)), "sizes of (a) and (b)"
        width = torch.arange(slot, device="cuda")[None, :] < res[:, None]
        assert bool(torch.equal(aout * width, out * width)), "bytes of (a) and (b)"
        a = rec["hc_cdict"]["depth%d" % depth]
        rec["hc_cdict_vs_staged_depth%d" % depth] = {
            "encode": round(e["ms"] / a["ms"], 2),
            "copy_plus_encode": round(e["ms_copy_plus_encode"] / a["ms"], 2)}
    del stage, hscr

    # (c) the fast prepared dictionary
    fobj = torch.empty(amd.cdict_size(), dtype=torch.uint8, device="cuda")
    amd.cdict_prepare(ddict, L, fobj)
    ts = times_ms(torch, lambda: amd.compress_cdict_batch(sptr, sizes, dptr, caps, res, fobj), reps)
    rec["cdict"] = entry(ts)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--messages", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hc_dict_compress.json"))
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, a.reps, a.messages)), flush=True)
        return 0
    recs = []
    for name in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                                "--reps", str(a.reps), "--messages", str(a.messages)],
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
        json.dump({"tool": "tools/hc_dict_bench.py", "reps": a.reps, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
