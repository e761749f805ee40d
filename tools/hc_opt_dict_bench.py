#!/usr/bin/env python3
"""The cost-minimising parse against a prepared dictionary on one MI355X: 16384 independent 1 KiB
and 4 KiB messages, one 61440-byte dictionary, depths 8 and 64, cut as tools/hc_dict_bench.py
cuts them (the dictionary is the `comp` stream's first 61440 bytes, the messages the 32 KiB that
follow, cut every L bytes and repeated across the batch, each copy at its own address).  Per
case and depth, three calls interleaved in one process, repetition by repetition, ms per call
(median of --reps by HIP events, with min and max), GiB/s of MESSAGE bytes, the ratio and the
scratch of:

  opt_cdict  (a) compress_hc_opt_usingCDict_batch_dev on a prepared high-ratio dictionary
  lazy_cdict (b) compress_hc_usingCDict_batch_dev, the lazy parse, on the same object
  staged     (c) the only way to (a)'s bytes before: a staging copy [dictionary | message] per
             message (two torch copies, timed with the call), then
             compress_hc_opt_withPrefix_batch_dev in its passes of 1024 blocks

Every output is decoded on the GPU with decompress_safe_usingDict and the original dictionary
and compared with the messages; (a)'s bytes are compared with (c)'s.  Each case runs in a child
process of its own under a time limit; the first failure ends the run.  Prints one JSON line
per case and writes profiles/hc_opt_dict.json (--out).  --only-opt runs (a) alone, twice per
depth, for a kernel trace of its own.
usage: hc_opt_dict_bench.py [--reps 5] [--messages 16384] [--out FILE] [--case NAME] [--only-opt]"""
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


def interleaved_ms(torch, fns, reps):
    """Sorted times of every function, the functions taking turns within each repetition (the
    first turn of each warms up)."""
    ts = [[] for _ in fns]
    for _ in range(reps + 1):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [sorted(t[1:]) for t in ts]


def run_case(name, reps, nb, only_opt):
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
    sizes, caps, dres = i32([L] * nb), i32([bound] * nb), i32([0] * nb)
    sptr = i64([msgs.data_ptr() + i * L for i in range(nb)])
    back = torch.empty((nb, L), dtype=torch.uint8, device="cuda")
    bptr = i64([back.data_ptr() + i * L for i in range(nb)])
    dictp, dicts = i64([ddict.data_ptr()] * nb), i32([DD] * nb)
    D = amd.hc_cdict_window(DD, L)
    # one output and one result array per call: the three take turns
    outs = [torch.empty((nb, slot), dtype=torch.uint8, device="cuda") for _ in range(3)]
    ress = [i32([0] * nb) for _ in range(3)]
    dptrs = [i64([o.data_ptr() + i * slot for i in range(nb)]) for o in outs]

    obj = torch.empty(amd.hc_cdict_size(), dtype=torch.uint8, device="cuda")
    amd.hc_cdict_prepare(ddict, L, obj)
    oscr = torch.empty(amd.compress_hc_opt_cdict_scratch_size(nb, L), dtype=torch.uint8, device="cuda")
    opt = lambda depth: amd.compress_hc_opt_cdict_batch(sptr, sizes, dptrs[0], caps, ress[0], obj, L,
                                                        depth, oscr)
    if only_opt:
        for depth in DEPTHS:
            for _ in range(2):
                opt(depth)
        torch.cuda.synchronize()
        assert int(ress[0].min()) > 0
        return {"case": name, "only_opt": True}

    lscr = torch.empty(amd.compress_hc_cdict_scratch_size(nb, L), dtype=torch.uint8, device="cuda")
    stage = torch.empty((nb, D + L), dtype=torch.uint8, device="cuda")
    tail = ddict[DD - D:]
    pp = i64([stage.data_ptr() + i * (D + L) + D for i in range(nb)])
    pre = i32([D] * nb)
    hscr = torch.empty(amd.compress_hc_opt_scratch_size(nb), dtype=torch.uint8, device="cuda")
    lazy = lambda depth: amd.compress_hc_cdict_batch(sptr, sizes, dptrs[1], caps, ress[1], obj, L,
                                                     depth, lscr)

    def staged(depth):
        stage[:, :D] = tail
        stage[:, D:] = msgs
        amd.compress_hc_opt_prefix_ptr_batch(pp, sizes, pre, dptrs[2], caps, ress[2], depth, hscr)

    def entry(ts, which, scratch_bytes):
        """The call's figures, after its output went through the GPU's usingDict decoder."""
        rs = ress[which].cpu().tolist()
        assert min(rs) > 0, min(rs)
        back.zero_()
        amd.decompress_dict_batch(dptrs[which], ress[which], bptr, sizes, dictp, dicts, dres)
        torch.cuda.synchronize()
        assert bool((dres == L).all()) and bool(torch.equal(back, msgs)), "usingDict round trip"
        med = ts[len(ts) // 2]
        return {"ms": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                "GiBps": round(total / (med * 1e-3) / (1 << 30), 3),
                "ratio": round(total / sum(rs), 4), "scratch_bytes": scratch_bytes}

    rec = {"case": name, "messages": nb, "message_bytes": L, "distinct_messages": k,
           "dict_bytes": DD, "window": D, "staging_bytes": stage.numel()}
    for depth in DEPTHS:
        ta, tb, tc = interleaved_ms(torch, [lambda: opt(depth), lambda: lazy(depth),
                                            lambda: staged(depth)], reps)
        a = entry(ta, 0, oscr.numel())
        b = entry(tb, 1, lscr.numel())
        c = entry(tc, 2, hscr.numel())
        assert bool(torch.equal(ress[0], ress[2])), "sizes of (a) and (c)"
        width = torch.arange(slot, device="cuda")[None, :] < ress[0][:, None]
        assert bool(torch.equal(outs[0] * width, outs[2] * width)), "bytes of (a) and (c)"
        rec["depth%d" % depth] = {
            "opt_cdict": a, "lazy_cdict": b, "staged": c,
            "staged_over_opt_cdict": round(c["ms"] / a["ms"], 2),
            "opt_cdict_over_lazy_cdict": round(a["ms"] / b["ms"], 2),
            "opt_cdict_faster_than_staged": a["ms"] < c["ms"]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--messages", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hc_opt_dict.json"))
    ap.add_argument("--case", help="run one case in this process (used by the parent)")
    ap.add_argument("--only-opt", action="store_true")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, a.reps, a.messages, a.only_opt)), flush=True)
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
        json.dump({"tool": "tools/hc_opt_dict_bench.py", "reps": a.reps, "cases": recs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
