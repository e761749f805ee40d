#!/usr/bin/env python3
"""Time-bounded GPU fuzz of byte-range reads from indexed blocks against the Python model
(TEST INFRASTRUCTURE, run by hand on a GPU box; the pytest suite runs the bounded form,
tests/test_gpu_range.py).

Inputs of mixed content and random size go through APE_LZ4_compress_large_indexed_batch_dev
with a random restart period.  Each block, and several mutations of it -- bytes of the stream
flipped, or a word of the index changed, swapped or replaced -- gets random requests (around
segment boundaries, near the end, past it, of any length) through
APE_LZ4_decompress_range_indexed_batch_dev with a random number of waves per request.  The
judge is tests/rangeutil.py: the window always equals the model's; a result is negative if and
only if the model's is; a positive one equals it in value and bytes (a stream with a zero
offset: in value); on the unmutated block the bytes are the source's; no byte of a dst past
need, or outside it, may change.  Capacities are need, need plus slack, or need - 1.

  python3 tests/fuzz/gpu_range_fuzz.py SECONDS [SEED]"""
import json
import os
import random
import struct
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.join(TESTS, "golden"), os.path.dirname(TESTS)]

import gpuutil  # noqa: E402
import inputs as I  # noqa: E402
import rangeutil as RU  # noqa: E402
from test_gpu_range import compressed, index_stride, read_ranges, uploaded  # noqa: E402

KINDS = ["comp", "comp", "text", "rand", "period3", "zeros"]
CANARY = bytes([gpuutil.CANARY])


def fail(**kw):
    print(json.dumps(kw), flush=True)
    sys.exit(1)


def mutate(rng, w, c, n):
    m, stream = list(w), c
    used = 4 + 2 * (w[1] + 1)
    how = rng.randrange(4)
    if how == 0:
        b = bytearray(c)
        for _ in range(rng.choice([1, 1, 2, 8])):
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        stream = bytes(b)
    elif how == 1:
        k = rng.randrange(used)
        m[k] = (m[k] + rng.choice([1, -1, 2, -3, 17, 1 << 16])) & 0xFFFFFFFF
    elif how == 2 and w[1] > 1:
        a, b2 = rng.randrange(w[1] + 1), rng.randrange(w[1] + 1)
        m[4 + 2 * a:6 + 2 * a], m[4 + 2 * b2:6 + 2 * b2] = w[4 + 2 * b2:6 + 2 * b2], w[4 + 2 * a:6 + 2 * a]
    else:
        m[rng.randrange(used)] = rng.choice([0, 1, rng.randrange(1 << 32), len(c), n])
    return m, stream


def request(rng, w, n):
    edges = [w[5 + 2 * j] for j in range(w[1] + 1)]
    a = rng.choice([rng.choice(edges) + rng.randrange(-2, 3), rng.randrange(n + 1),
                    n - rng.randrange(40), rng.randrange(-2, n + 3)])
    ln = rng.choice([0, 1, rng.randrange(64), rng.randrange(5000), rng.randrange(n + 2), n, -1])
    return max(min(a, 0x7FFFFFFF), -0x80000000), ln


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20264
    import torch
    import libapenetwork_amd as amd
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    S = amd.compress_large_slice_size()
    rng = random.Random(seed)
    t0, nb, checked, rejected, refused = time.time(), 0, 0, 0, 0
    while time.time() - t0 < seconds:
        R = S * rng.choice([1, 1, 2, 3, 4])
        srcs = []
        for _ in range(8):
            n = rng.choice([rng.randrange(65537, 4 * R), rng.randrange(1, 65537), rng.randrange(65537, 300000)])
            plain = bytearray()
            while len(plain) < n:
                plain += I.make(rng.choice(KINDS), rng.randrange(1000, 120000), seed=rng.randrange(1 << 30))
            srcs.append(bytes(plain[:n]))
        good = compressed(torch, amd, srcs, R)
        blocks, words, owner = [], [], []
        full = index_stride(good.max_seg) // 4   # (the model sees the zeros the device sees)
        good.words = [w + [0] * (full - len(w)) for w in good.words]
        for i, (s, c, w) in enumerate(zip(srcs, good.blocks, good.words)):
            blocks.append(c)
            words.append(w)
            owner.append(i)
            for _ in range(4):
                m, stream = mutate(rng, w, c, len(s))
                blocks.append(stream)
                words.append(m)
                owner.append(i)
        d = uploaded(torch, blocks, words, good.max_seg)
        reqs, want, caps, memos = [], [], [], {}
        for k in range(len(blocks)):
            w0, n = good.words[owner[k]], len(srcs[owner[k]])
            for _ in range(5):
                a, ln = request(rng, w0, n)
                x = RU.decode_range(blocks[k], words[k], a, ln, 1 << 30, good.max_seg,
                                    memo=memos.setdefault(owner[k], {}))
                cap = max(x[1][1] + rng.choice([0, 0, 1, 64, -1]), 0)
                if cap < x[1][1]:
                    x = (RU.ERANGE, x[1], b"")
                reqs.append((k, a, ln))
                want.append(x)
                caps.append(cap)
        rs, wins, bufs = read_ranges(torch, amd, d, reqs, caps, rng.choice([1, 2, 3, 4, 9]))
        for q, ((k, a, ln), (er, ewin, edata)) in enumerate(zip(reqs, want)):
            ctx = dict(batch=nb, request=q, block=k, a=a, length=ln, cap=caps[q], R=R, gpu=rs[q],
                       model=er, window=wins[q], model_window=ewin, csize=len(blocks[k]),
                       index=struct.pack("<%dI" % len(words[k]), *words[k]).hex())
            if wins[q] != ewin or (rs[q] < 0) != (er < 0):
                fail(mismatch="window or sign", **ctx)
            if (er == RU.ERANGE or (er == -1 and ewin == (0, 0))) and rs[q] != er:
                fail(mismatch="plan code", **ctx)
            written = 0 if er == RU.ERANGE else min(ewin[1], caps[q])
            if bufs[q][written:] != CANARY * (caps[q] - written):
                fail(mismatch="write past need", **ctx)
            if er == RU.ERANGE:
                refused += 1
            if er < 0:
                rejected += 1
                continue
            if rs[q] != er or (bufs[q][ewin[0]:ewin[0] + er] != edata and not RU.has_offset0(blocks[k])):
                fail(mismatch="range decode", **ctx)
            if blocks[k] is good.blocks[owner[k]] and words[k] is good.words[owner[k]] and \
                    edata != srcs[owner[k]][a:a + er]:
                fail(mismatch="round trip", **ctx)
        gpuutil.check_canaries()   # nothing written outside any dst[0, cap)
        nb += 1
        checked += len(reqs)
        print("batch %d: %d requests, %d negative (%d for capacity), %.0f s" %
              (nb, checked, rejected, refused, time.time() - t0), flush=True)
    print(json.dumps({"seconds": round(time.time() - t0, 1), "seed": seed, "batches": nb,
                      "requests_checked": checked, "negative": rejected, "mismatches": 0,
                      "canaries": "intact"}), flush=True)


if __name__ == "__main__":
    main()
