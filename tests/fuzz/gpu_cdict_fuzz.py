#!/usr/bin/env python3
"""Time-bounded GPU fuzz of the prepared-dictionary encoder against the oracle (run by hand on a
GPU box; the pytest suite runs bounded forms in tests/test_gpu_cdict.py).

Per batch one dictionary of 0 B .. 70 KiB spliced from App. C / text / random / periodic / zero
content, prepared for a random maxSrcSize, and 400 messages of 0 .. maxSrcSize + 1 bytes, each
spliced from pieces of the dictionary (its last bytes among them, so that matches reach the
dictionary's end), of the message so far and of fresh content, at capacities around the bound,
0 and random values, through APE_LZ4_compress_usingCDict_batch_dev: a size above maxSrcSize gives
APE_LZ4_GPU_ERANGE; otherwise 0 <= ret <= cap, a capacity >= compressBound never fails, and a
nonzero block decodes with the oracle's decompress_safe_usingDict and the ORIGINAL dictionary
to the message.  Canaries around every dst slot are checked per batch.

With --model K the bytes of every K-th block are also compared with tests/encmodel.py's
encode_cdict (the definition of this encoder's output; the pytest suite holds the kernel to it in
tests/test_gpu_cdict_model.py).

  python3 tests/fuzz/gpu_cdict_fuzz.py SECONDS [SEED] [--model K]
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
sys.path[:0] = [TESTS, os.path.join(TESTS, "golden"), os.path.dirname(TESTS)]

import inputs as I  # noqa: E402
from gpuutil import alloc_out, check_canaries, fetch, ints, pack  # noqa: E402

KINDS = ["comp", "text", "rand", "period3", "zeros", "byte"]
ERANGE = -2147483648


def spliced(rng, n):
    out = bytearray()
    while len(out) < n:
        out += I.make(rng.choice(KINDS), rng.randrange(1, min(n, 8192) + 1), seed=rng.randrange(1 << 30))
    return bytes(out[:n])


def message(rng, d, n):
    out = bytearray()
    while len(out) < n:
        k = rng.randrange(4)
        ln = rng.choice([1, 3, 4, 5, 12, 40, 300, rng.randrange(1, 2000)])
        if k == 0 and d:       # the dictionary's end
            out += d[-min(ln, len(d)):]
        elif k == 1 and d:     # anywhere in the dictionary
            st = rng.randrange(len(d))
            out += d[st:st + ln]
        elif k == 2 and out:   # the message so far
            st = rng.randrange(len(out))
            out += out[st:st + ln]
        else:
            out += I.make(rng.choice(KINDS), ln, seed=rng.randrange(1 << 30))
    return bytes(out[:n])


def fail(what, **kw):
    print(json.dumps(dict(mismatch=what, **kw)), flush=True)
    sys.exit(1)


def main():
    argv = sys.argv[1:]
    model_every = 0
    if "--model" in argv:
        at = argv.index("--model")
        model_every = int(argv[at + 1])
        del argv[at:at + 2]
        import encmodel
    seconds = float(argv[0]) if len(argv) > 0 else 60.0
    seed = int(argv[1]) if len(argv) > 1 else 20261
    import torch
    import libapenetwork_amd as amd
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    orc = ctypes.CDLL(os.path.join(os.path.dirname(TESTS), "oracle", "liblz4_oracle.so"))
    rng = random.Random(seed)
    t0, nb, checked, erange, modelled = time.time(), 0, 0, 0, 0
    while time.time() - t0 < seconds:
        dsz = rng.choice([0, 1, 63, 64, 100, 4096, 32768, 61440, 65536, 70000, rng.randrange(70001)])
        max_src = rng.choice([1, 64, 128, 1024, 4096, 8192, 65536, rng.randrange(1, 65537)])
        d = spliced(rng, dsz)
        lens = [rng.choice([0, 1, 12, 13, 64, 127, 128, max_src, max_src + 1,
                            rng.randrange(max_src + 1), rng.randrange(min(max_src, 2048) + 1)])
                for _ in range(400)]
        msgs = [message(rng, d, n) for n in lens]
        caps = []
        for m in msgs:
            bound = amd.compressBound(len(m))
            caps.append(rng.choice([bound, bound, bound, bound - 1, 0, rng.randrange(bound + 1)]))
        hd = np.zeros(dsz + 67, np.uint8)
        hd[3:3 + dsz] = np.frombuffer(d, np.uint8)
        ddev = torch.from_numpy(hd).cuda()
        obj = torch.full((amd.cdict_size(),), rng.randrange(256), dtype=torch.uint8, device="cuda")
        amd.cdict_prepare(ddev[3:3 + dsz], max_src, obj)
        src, sptr, _ = pack(torch, msgs, misalign=[rng.randrange(16) for _ in msgs])
        dst, dptr, doffs = alloc_out(torch, caps, misalign=[rng.randrange(16) for _ in msgs])
        res = ints(torch, [-7] * len(msgs))
        amd.compress_cdict_batch(sptr, ints(torch, lens), dptr, ints(torch, caps), res, obj)
        torch.cuda.synchronize()
        rs = res.cpu().tolist()
        db = ctypes.create_string_buffer(d + bytes(64), dsz + 64)
        for i, (m, cap, r) in enumerate(zip(msgs, caps, rs)):
            info = dict(batch=nb, block=i, n=len(m), cap=cap, dict=dsz, max_src=max_src, gpu=r)
            if len(m) > max_src:
                if r != ERANGE:
                    fail("erange", **info)
                erange += 1
                continue
            if r < 0 or r > cap:
                fail("range", **info)
            if model_every and i % model_every == 0:
                want = encmodel.encode_cdict(m, d, max_src)
                out = fetch(dst, doffs[i], r)
                if (r, out) != ((len(want), want) if len(want) <= cap else (0, b"")):
                    fail("model", model=len(want), **info)
                modelled += 1
            if r == 0:
                if cap >= amd.compressBound(len(m)):
                    fail("failed at the bound", **info)
                continue
            out = fetch(dst, doffs[i], r)
            o = ctypes.create_string_buffer(len(m) + 64)
            dr = orc.orc_decompress_safe_usingDict(
                ctypes.create_string_buffer(out + bytes(64), r + 64), o, r, len(m), db, dsz)
            if dr != len(m) or o.raw[:len(m)] != m:
                fail("roundtrip", decoded=dr, **info)
        check_canaries()
        checked += len(msgs)
        nb += 1
    print(json.dumps({"seconds": round(time.time() - t0, 1), "seed": seed, "batches": nb,
                      "blocks_checked": checked, "erange_blocks": erange, "model_blocks": modelled,
                      "mismatches": 0,
                      "canaries": "intact"}))


if __name__ == "__main__":
    main()
