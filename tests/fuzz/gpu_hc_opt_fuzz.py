#!/usr/bin/env python3
"""Time-bounded GPU fuzz of the high-ratio mode's cost-minimising parse (run by hand on a GPU
box; the pytest suite runs bounded forms in tests/test_gpu_hc_opt.py).

Per batch 48 windows of history + block (the block 0 .. 65537 bytes, the history 0 .. what a
window of 65536 bytes holds beside it, sometimes more offered than fits), each spliced from
App. C / text / random / periodic / zero content and from copies of the window so far (so that
chains are long, matches reach the search cap and run from the history into the block), at one
random depth of 1 .. 256, at capacities around the output size, 0 and random values, at random
alignments and with a scratch of a random number of blocks and a random fill, through
APE_LZ4_compress_hc_opt_withPrefix_batch_dev (every fourth batch without history through
APE_LZ4_compress_hc_opt_batch_dev).  A size above 65536 gives APE_LZ4_GPU_ERANGE.  EVERY block
that got room for any output goes back through the GPU's usingDict decoder and must be its
input; every K-th block is also compared with tests/hcoptmodel.py: its size and bytes when they
fit the capacity, 0 when they do not.  Canaries around every dst slot are checked per batch.

  python3 tests/fuzz/gpu_hc_opt_fuzz.py SECONDS [SEED] [K]
prints a JSON summary; exit 1 on the first mismatch."""
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.join(TESTS, "golden"), os.path.dirname(TESTS)]

import hcoptmodel  # noqa: E402
import inputs as I  # noqa: E402
from gpuutil import alloc_out, check_canaries, fetch, ints, pack  # noqa: E402

KINDS = ["comp", "text", "rand", "period3", "period7", "zeros", "byte"]
ERANGE = -2147483648
BLOCKS = 48


def window(rng, n):
    out = bytearray()
    while len(out) < n:
        ln = rng.choice([1, 3, 4, 5, 12, 40, 271, 272, 273, 300, rng.randrange(1, 20000)])
        if out and rng.randrange(3) == 0:   # the window so far
            st = rng.randrange(len(out))
            out += out[st:st + ln]
        else:
            out += I.make(rng.choice(KINDS), ln, seed=rng.randrange(1 << 30))
    return bytes(out[:n])


def fail(what, **kw):
    print(json.dumps(dict(mismatch=what, **kw)), flush=True)
    sys.exit(1)


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20263
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    import torch
    import libapenetwork_amd as amd
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    rng = random.Random(seed)
    t0, nb, modelled, tripped, erange, short = time.time(), 0, 0, 0, 0, 0
    while time.time() - t0 < seconds:
        plain = nb % 4 == 3
        depth = rng.choice([1, 2, 8, 64, 256, rng.randrange(1, 257)])
        lens = [rng.choice([0, 1, 12, 13, 64, 272 + 5, 4096, 65535, 65536, 65537,
                            rng.randrange(65537), rng.randrange(2049)]) for _ in range(BLOCKS)]
        hists = [0 if plain or n > 65536 else
                 min(rng.choice([0, 1, 63, 64, 65536 - n, rng.randrange(65536 - n + 1)]), 65536 - n)
                 for n in lens]
        wins = [window(rng, h + n) for h, n in zip(hists, lens)]
        # offered: the used history, or more of it than the window holds (only where the block
        # then still uses exactly `h`: the bytes before the window are not the test's)
        offered = [h if h < 65536 - n else h + rng.choice([0, 9]) for h, n in zip(hists, lens)]
        src, wptr, _ = pack(torch, wins, misalign=[rng.randrange(16) for _ in wins], extra=80)
        sptr = wptr + torch.tensor(hists, dtype=torch.int64, device="cuda")
        bound = [amd.compressBound(min(n, 65536)) for n in lens]
        want = [hcoptmodel.compress_prefix(w, h, depth) if i % K == 0 and n <= 65536 else None
                for i, (w, h, n) in enumerate(zip(wins, hists, lens))]
        caps = [rng.choice([len(w), len(w), b, len(w) - 1, 0, rng.randrange(len(w) + 1)])
                if w is not None else rng.choice([b, b, b, 0, rng.randrange(b + 1)])
                for w, b in zip(want, bound)]
        dst, dptr, doffs = alloc_out(torch, caps, misalign=[rng.randrange(16) for _ in wins])
        res = ints(torch, [-7] * BLOCKS)
        scratch = torch.full((amd.compress_hc_opt_scratch_size(rng.randrange(1, BLOCKS + 1)),),
                             rng.randrange(256), dtype=torch.uint8, device="cuda")
        if plain:
            amd.compress_hc_opt_ptr_batch(sptr, ints(torch, lens), dptr, ints(torch, caps), res,
                                          depth, scratch)
        else:
            amd.compress_hc_opt_prefix_ptr_batch(sptr, ints(torch, lens), ints(torch, offered), dptr,
                                                 ints(torch, caps), res, depth, scratch)
        torch.cuda.synchronize()
        rs = res.cpu().tolist()
        # every block back through the GPU's decoder, its history as the dictionary
        back, bptr, boffs = alloc_out(torch, [min(n, 65536) for n in lens])
        bres = ints(torch, [-7] * BLOCKS)
        amd.decompress_dict_batch(dptr, ints(torch, [max(r, 0) for r in rs]), bptr,
                                  ints(torch, [min(n, 65536) for n in lens]), wptr,
                                  ints(torch, hists), bres)
        torch.cuda.synchronize()
        brs = bres.cpu().tolist()
        for i, (w, h, n, cap, r) in enumerate(zip(wins, hists, lens, caps, rs)):
            info = dict(batch=nb, block=i, n=n, history=h, cap=cap, depth=depth, gpu=r)
            if n > 65536:
                if r != ERANGE:
                    fail("erange", **info)
                erange += 1
                continue
            if r < 0 or r > cap or r > bound[i]:
                fail("result out of range", **info)
            if r > 0:
                if brs[i] != n or fetch(back, boffs[i], n) != w[h:]:
                    fail("round trip", decoded=brs[i], **info)
                tripped += 1
            else:
                short += 1
            if want[i] is not None:
                m = want[i]
                if len(m) > cap:
                    if r != 0:
                        fail("does not fit, yet not 0", model=len(m), **info)
                elif r != len(m) or fetch(dst, doffs[i], r) != m:
                    fail("bytes", model=len(m), **info)
                modelled += 1
            elif r == 0 and cap >= bound[i]:
                fail("0 with room for compressBound", **info)
        check_canaries()
        nb += 1
    print(json.dumps({"seconds": round(time.time() - t0, 1), "seed": seed, "batches": nb,
                      "blocks": nb * BLOCKS, "round_trips": tripped, "blocks_modelled": modelled,
                      "every": K, "erange_blocks": erange, "blocks_without_output": short,
                      "mismatches": 0, "canaries": "intact"}))


if __name__ == "__main__":
    main()
