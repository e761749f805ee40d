#!/usr/bin/env python3
"""Time-bounded GPU fuzz of the high-ratio encoder against its model (run by hand on a GPU box;
the pytest suite runs bounded forms in tests/test_gpu_hc.py).

Per batch 48 blocks of 0 .. 65537 bytes, each spliced from App. C / text / random / periodic /
zero content and from copies of the block so far (so that chains are long and matches reach the
search cap), at one random depth of 1 .. 256, at capacities around the output size, 0 and random
values, at random alignments and with a scratch of a random number of blocks, through
APE_LZ4_compress_hc_batch_dev: a size above 65536 gives APE_LZ4_GPU_ERANGE; otherwise the result
and the bytes are tests/hcmodel.py's when they fit the capacity, and 0 when they do not.
Canaries around every dst slot are checked per batch.

  python3 tests/fuzz/gpu_hc_fuzz.py SECONDS [SEED]
prints a JSON summary; exit 1 on the first mismatch."""
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.join(TESTS, "golden"), os.path.dirname(TESTS)]

import hcmodel  # noqa: E402
import inputs as I  # noqa: E402
from gpuutil import alloc_out, check_canaries, fetch, ints, pack  # noqa: E402

KINDS = ["comp", "text", "rand", "period3", "period7", "zeros", "byte"]
ERANGE = -2147483648
BLOCKS = 48


def block(rng, n):
    out = bytearray()
    while len(out) < n:
        ln = rng.choice([1, 3, 4, 5, 12, 40, 271, 272, 273, 300, rng.randrange(1, 20000)])
        if out and rng.randrange(3) == 0:   # the block so far
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
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20262
    import torch
    import libapenetwork_amd as amd
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    rng = random.Random(seed)
    t0, nb, checked, erange, short = time.time(), 0, 0, 0, 0
    while time.time() - t0 < seconds:
        depth = rng.choice([1, 2, 8, 64, 256, rng.randrange(1, 257)])
        lens = [rng.choice([0, 1, 12, 13, 64, 272 + 5, 4096, 65535, 65536, 65537,
                            rng.randrange(65537), rng.randrange(2049)]) for _ in range(BLOCKS)]
        blobs = [block(rng, n) for n in lens]
        want = [hcmodel.compress(b, depth) if len(b) <= 65536 else b"" for b in blobs]
        caps = [rng.choice([len(w), len(w), amd.compressBound(len(b)), len(w) - 1, 0,
                            rng.randrange(len(w) + 1)]) for b, w in zip(blobs, want)]
        src, sptr, _ = pack(torch, blobs, misalign=[rng.randrange(16) for _ in blobs])
        dst, dptr, doffs = alloc_out(torch, caps, misalign=[rng.randrange(16) for _ in blobs])
        res = ints(torch, [-7] * BLOCKS)
        scratch = torch.full((amd.compress_hc_scratch_size(rng.randrange(1, BLOCKS + 1)),),
                             rng.randrange(256), dtype=torch.uint8, device="cuda")
        amd.compress_hc_ptr_batch(sptr, ints(torch, lens), dptr, ints(torch, caps), res, depth,
                                  scratch)
        torch.cuda.synchronize()
        rs = res.cpu().tolist()
        for i, (b, w, cap, r) in enumerate(zip(blobs, want, caps, rs)):
            info = dict(batch=nb, block=i, n=len(b), cap=cap, depth=depth, gpu=r, model=len(w))
            if len(b) > 65536:
                if r != ERANGE:
                    fail("erange", **info)
                erange += 1
            elif len(w) > cap:
                if r != 0:
                    fail("does not fit, yet not 0", **info)
                short += 1
            elif r != len(w) or fetch(dst, doffs[i], r) != w:
                fail("bytes", **info)
        check_canaries()
        checked += BLOCKS
        nb += 1
    print(json.dumps({"seconds": round(time.time() - t0, 1), "seed": seed, "batches": nb,
                      "blocks_checked": checked, "erange_blocks": erange,
                      "blocks_over_capacity": short, "mismatches": 0, "canaries": "intact"}))


if __name__ == "__main__":
    main()
