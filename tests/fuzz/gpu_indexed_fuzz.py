#!/usr/bin/env python3
"""Time-bounded GPU fuzz of indexed large blocks against the oracle (TEST INFRASTRUCTURE, run by
hand on a GPU box; the pytest suite runs the bounded form, tests/test_gpu_indexed.py).

Inputs of mixed content and random size go through APE_LZ4_compress_large_indexed_batch_dev
with a random restart period; every block must decode on the oracle to its source, and
through APE_LZ4_decompress_safe_indexed_batch_dev to n and the source.  Then most blocks are
mutated -- bytes of the stream flipped, or a word of the index changed, swapped or replaced --
and decoded again: every result must be negative or equal the oracle's decompress_safe of
that stream in value and bytes (a stream with a zero offset: in value), and no byte outside
any dst[0, cap) may change.  Capacities are n, or n plus slack.

  python3 tests/fuzz/gpu_indexed_fuzz.py SECONDS [SEED]"""
import ctypes as C
import json
import os
import random
import struct
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.join(TESTS, "golden"), os.path.dirname(TESTS)]

import gen_golden  # noqa: E402
import gpuutil  # noqa: E402
import inputs as I  # noqa: E402
from lz4util import orc_decompress  # noqa: E402
from test_gpu_indexed import Packed, run_decode, words_of  # noqa: E402

KINDS = ["comp", "comp", "text", "rand", "period3", "zeros"]


def fail(**kw):
    print(json.dumps(kw), flush=True)
    sys.exit(1)


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20263
    import torch
    import libapenetwork_amd as amd
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    orc = C.CDLL(os.path.join(os.path.dirname(TESTS), "oracle", "liblz4_oracle.so"))
    S = amd.compress_large_slice_size()
    rng = random.Random(seed)
    t0, nb, checked, rejected = time.time(), 0, 0, 0
    while time.time() - t0 < seconds:
        R = S * rng.choice([1, 1, 2, 3, 4, 8])
        srcs = []
        for _ in range(24):
            n = rng.choice([rng.randrange(65537, 4 * R), rng.randrange(1, 65537), rng.randrange(65537, 600000)])
            plain = bytearray()
            while len(plain) < n:
                plain += I.make(rng.choice(KINDS), rng.randrange(1000, 120000), seed=rng.randrange(1 << 30))
            srcs.append(bytes(plain[:n]))
        good = Packed(torch, amd, srcs, R)
        nw = 4 + 2 * (good.max_seg + 1)
        blocks, idx, caps = [], [], []
        for i, (s, c, r) in enumerate(zip(srcs, good.outs, good.rs)):
            if r <= 0 or orc_decompress(orc, c, len(s)) != (len(s), s):
                fail(mismatch="compress", batch=nb, block=i, n=len(s), R=R, result=r)
            w = words_of(good.index, i, nw)
            w = w[:4 + 2 * (w[1] + 1)]
            blocks.append(c)
            idx.append(w)
            caps.append(len(s))
            for _ in range(6):
                m, stream = list(w), c
                how = rng.randrange(4)
                if how == 0:
                    b = bytearray(c)
                    for _ in range(rng.choice([1, 1, 2, 8])):
                        b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
                    stream = bytes(b)
                elif how == 1:
                    k = rng.randrange(len(m))
                    m[k] = (m[k] + rng.choice([1, -1, 2, -3, 17, 1 << 16])) & 0xFFFFFFFF
                elif how == 2 and w[1] > 1:
                    a, b2 = rng.randrange(w[1] + 1), rng.randrange(w[1] + 1)
                    m[4 + 2 * a:6 + 2 * a], m[4 + 2 * b2:6 + 2 * b2] = w[4 + 2 * b2:6 + 2 * b2], w[4 + 2 * a:6 + 2 * a]
                else:
                    m[rng.randrange(len(m))] = rng.choice([0, 1, rng.randrange(1 << 32), len(c), len(s)])
                blocks.append(stream)
                idx.append(m)
                caps.append(len(s) + rng.choice([0, 0, 1, 100]))
        rs, outs = run_decode(torch, amd, blocks, caps, idx, good.max_seg)
        for k, (b, w, cap, r, out) in enumerate(zip(blocks, idx, caps, rs, outs)):
            first = k % 7 == 0
            if first and (r != cap or out != srcs[k // 7]):
                fail(mismatch="round trip", batch=nb, block=k, n=cap, R=R, gpu=r)
            if r < 0:
                rejected += 1
                continue
            er, eout = orc_decompress(orc, b, cap)
            if r != er or (out != eout and not gen_golden.has_offset0(b)):
                fail(mismatch="indexed decode", batch=nb, block=k, csize=len(b), cap=cap, R=R,
                     gpu=r, oracle=er, index=struct.pack("<%dI" % len(w), *w).hex())
        gpuutil.check_canaries()   # nothing written outside any dst[0, cap)
        nb += 1
        checked += len(blocks)
        print("batch %d: %d blocks, %d rejected, %.0f s" % (nb, checked, rejected, time.time() - t0), flush=True)
    print(json.dumps({"seconds": round(time.time() - t0, 1), "seed": seed, "batches": nb,
                      "blocks_checked": checked, "rejected": rejected, "mismatches": 0,
                      "canaries": "intact"}), flush=True)


if __name__ == "__main__":
    main()
