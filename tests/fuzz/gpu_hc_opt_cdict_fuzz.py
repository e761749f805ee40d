#!/usr/bin/env python3
"""Time-bounded GPU fuzz of the cost-minimising parse against a prepared dictionary (run by hand
on a GPU box; the pytest suite runs bounded forms in tests/test_gpu_hc_opt_cdict.py).

The batches are tests/fuzz/gpu_hc_cdict_fuzz.py's: one dictionary of 0 B .. 70 KiB, prepared for
a random maxSrcSize, a random depth, and 200 messages of 0 .. maxSrcSize + 1 bytes spliced from
pieces of the dictionary (its last bytes among them), of the message so far and of fresh
content, at capacities around the bound, 0 and random values, through
APE_LZ4_compress_hc_opt_usingCDict_batch_dev with a scratch of a random number of slots and
random content: a size above maxSrcSize gives APE_LZ4_GPU_ERANGE; EVERY other block has the
result and the bytes of APE_LZ4_compress_hc_opt_withPrefix_batch_dev on the staged window
[dictionary tail | message] at the same capacity; every K-th is tests/hcoptdictmodel.py's; a
nonzero block decodes with the oracle's decompress_safe_usingDict and the ORIGINAL dictionary
to the message; a block with result 0 has left its destination untouched, and a capacity >=
compressBound never fails.  Canaries around every dst slot are checked per batch.

  python3 tests/fuzz/gpu_hc_opt_cdict_fuzz.py SECONDS [SEED] [K]
prints a JSON summary; exit 1 on the first mismatch."""
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.join(TESTS, "golden"), os.path.dirname(TESTS), HERE]

import hcoptdictmodel  # noqa: E402
from gpu_cdict_fuzz import message, spliced  # noqa: E402
from gpuutil import CANARY, alloc_out, check_canaries, ints, pack  # noqa: E402

ERANGE = -2147483648


def fail(what, **kw):
    print(json.dumps(dict(mismatch=what, **kw)), flush=True)
    sys.exit(1)


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20262
    every = int(sys.argv[3]) if len(sys.argv) > 3 else 25
    import torch
    import libapenetwork_amd as amd
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    orc = ctypes.CDLL(os.path.join(os.path.dirname(TESTS), "oracle", "liblz4_oracle.so"))
    rng = random.Random(seed)
    t0, nb, checked, erange, modelled, zero = time.time(), 0, 0, 0, 0, 0
    while time.time() - t0 < seconds:
        dsz = rng.choice([0, 1, 3, 4, 63, 100, 4095, 32768, 61440, 65535, 70000, rng.randrange(70001)])
        max_src = rng.choice([1, 13, 64, 255, 256, 257, 1000, 1024, 4096, 8192, 65536,
                              rng.randrange(1, 65537)])
        depth = rng.choice([0, 1, 2, 8, 8, 8, 64, 256, rng.randrange(1, 257)])
        d = spliced(rng, dsz)
        lens = [rng.choice([0, 1, 12, 13, 64, 127, 128, max_src, max_src + 1,
                            rng.randrange(max_src + 1), rng.randrange(min(max_src, 2048) + 1)])
                for _ in range(199)] + [max_src]   # (at least one message is in range)
        msgs = [message(rng, d, n) for n in lens]
        caps = []
        for m in msgs:
            bound = amd.compressBound(len(m))
            caps.append(rng.choice([bound, bound, bound, bound - 1, 0, rng.randrange(bound + 1)]))
        n = len(msgs)
        hd = np.zeros(dsz + 67, np.uint8)
        hd[3:3 + dsz] = np.frombuffer(d, np.uint8)
        ddev = torch.from_numpy(hd).cuda()
        obj = torch.full((amd.hc_cdict_size(),), rng.randrange(256), dtype=torch.uint8, device="cuda")
        amd.hc_cdict_prepare(ddev[3:3 + dsz], max_src, obj)
        src, sptr, _ = pack(torch, msgs, misalign=[rng.randrange(16) for _ in msgs])
        dst, dptr, doffs = alloc_out(torch, caps, misalign=[rng.randrange(16) for _ in msgs])
        res = ints(torch, [-7] * n)
        slots = rng.choice([1, n, rng.randrange(1, n + 1)])
        scratch = torch.full((amd.compress_hc_opt_cdict_scratch_size(slots, max_src),),
                             rng.randrange(256), dtype=torch.uint8, device="cuda")
        amd.compress_hc_opt_cdict_batch(sptr, ints(torch, lens), dptr, ints(torch, caps), res, obj,
                                        max_src, depth, scratch)
        # the staged call on the messages that are in range
        D = amd.hc_cdict_window(dsz, max_src)
        tail = d[dsz - D:]
        inr = [i for i in range(n) if lens[i] <= max_src]
        wsrc, wptr, _ = pack(torch, [tail + msgs[i] for i in inr],
                             misalign=[rng.randrange(16) for _ in inr])
        scaps = [caps[i] for i in inr]
        sdst, sdptr, sdoffs = alloc_out(torch, scaps, misalign=[rng.randrange(16) for _ in inr])
        sres = ints(torch, [-7] * len(inr))
        hscr = torch.empty(amd.compress_hc_opt_scratch_size(min(len(inr), 64)), dtype=torch.uint8,
                           device="cuda")
        amd.compress_hc_opt_prefix_ptr_batch(wptr + D, ints(torch, [lens[i] for i in inr]),
                                             ints(torch, [D] * len(inr)), sdptr, ints(torch, scaps),
                                             sres, depth, hscr)
        torch.cuda.synchronize()
        rs, srs = res.cpu().tolist(), dict(zip(inr, sres.cpu().tolist()))
        host, shost = dst.cpu().numpy(), sdst.cpu().numpy()
        soff = dict(zip(inr, sdoffs))
        db = ctypes.create_string_buffer(d + bytes(64), dsz + 64)
        for i, (m, cap, r) in enumerate(zip(msgs, caps, rs)):
            info = dict(batch=nb, block=i, n=len(m), cap=cap, dict=dsz, max_src=max_src,
                        depth=depth, slots=slots, gpu=r)
            if r <= 0 and bool((host[doffs[i]:doffs[i] + max(cap, 1)] != CANARY).any()):
                fail("a block without a result wrote to its destination", **info)
            if len(m) > max_src:
                if r != ERANGE:
                    fail("erange", **info)
                erange += 1
                continue
            if r != srs[i]:
                fail("result differs from the staged call's", staged=srs[i], **info)
            if r < 0 or r > cap:
                fail("range", **info)
            if r == 0:
                if cap >= amd.compressBound(len(m)):
                    fail("failed at the bound", **info)
                zero += 1
                continue
            out = host[doffs[i]:doffs[i] + r].tobytes()
            if out != shost[soff[i]:soff[i] + r].tobytes():
                fail("bytes differ from the staged call's", **info)
            if (checked + i) % every == 0:
                if out != hcoptdictmodel.compress(d, m, max_src, depth or 64):
                    fail("bytes differ from the model's", **info)
                modelled += 1
            o = ctypes.create_string_buffer(len(m) + 64)
            dr = orc.orc_decompress_safe_usingDict(
                ctypes.create_string_buffer(out + bytes(64), r + 64), o, r, len(m), db, dsz)
            if dr != len(m) or o.raw[:len(m)] != m:
                fail("roundtrip", decoded=dr, **info)
        check_canaries()
        checked += n
        nb += 1
    print(json.dumps({"seconds": round(time.time() - t0, 1), "seed": seed, "batches": nb,
                      "blocks_checked": checked, "against_the_model": modelled,
                      "erange_blocks": erange, "too_small_capacity": zero, "mismatches": 0,
                      "canaries": "intact"}))


if __name__ == "__main__":
    main()
