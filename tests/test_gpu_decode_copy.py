"""The decoder's copy scheduler against the plain decoder, class by class.

Every part of the corpus of tests/decseq.py (offset x length grid, segment edges, slid windows,
dependent chains, dictionary ends, multi-batch and restaged variants, flush edges) goes through
decompress_ptr_batch, decompress_partial_batch (target at or past the end, inside a probe's
match, inside its literals), decompress_fast and decompress_dict_batch.  For each block the
return value equals the oracle's, dst[0:ret] equals the plain byte-at-a-time decoder's output,
and the canaries around every output are intact (conftest).  A failure names the block's probes
(off, n, position) and the class tests/deccopyclass.py gives them, so it points at a branch of
copy_segment.  tests/test_dec_copy_classes.py proves on the CPU what the corpus reaches.
"""
import ctypes as C
import random

import numpy as np
import pytest

import decseq as S
from gpuutil import alloc_out, ints, pack
from lz4util import buf, orc_decompress

pytestmark = pytest.mark.gpu

PARTS = {
    "grid": lambda: [(b, 0) for b in S.grid()],
    "edge1": lambda: [(b, 0) for b in S.edges(1)],
    "edge2": lambda: [(b, 0) for b in S.edges(2)],
    "slide": lambda: [(b, 0) for b in S.slides()],
    "chain": lambda: [(b, 0) for b in S.chains()],
    "multi-short": lambda: [(b, 0) for b in S.multibatch("short")],
    "multi-restage": lambda: [(b, 0) for b in S.multibatch("restage")],
    "flush": S.flush_edges,
}


def _report(bad, dict_mode=False):
    return "%d blocks differ; first: %s" % (
        len(bad), " | ".join("%s -> %s" % (b.describe(dict_mode, da), why) for b, da, why in bad[:4]))


def _check(blocks, rets, host, doffs, exp_rets, dict_mode=False, prefix=False):
    """ret == the oracle's, dst[0:ret] == the plain decoder's (its prefix for a partial decode)."""
    bad = []
    for (b, da), r, o, er in zip(blocks, rets, doffs, exp_rets):
        if r != er:
            bad.append((b, da, "ret %d, oracle %d" % (r, er)))
        elif r > 0:
            got = host[o:o + r].tobytes()
            want = b.out[:r] if prefix else b.out
            if got != want:
                at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]),
                          min(len(got), len(want)))
                bad.append((b, da, "first wrong byte at %d of %d" % (at, r)))
    assert not bad, _report(bad, dict_mode)


def _inputs(torch, blocks):
    comps = [b.comp for b, _ in blocks]
    src, sptr, _ = pack(torch, comps)
    return src, sptr, ints(torch, map(len, comps))


@pytest.mark.parametrize("part", sorted(PARTS))
def test_decompress_safe(cuda, product, oracle, part):
    torch = cuda
    blocks = PARTS[part]()
    caps = [b.size for b, _ in blocks]
    src, sptr, sizes = _inputs(torch, blocks)
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[da for _, da in blocks])
    res = ints(torch, [0] * len(blocks))
    product.decompress_ptr_batch(sptr, sizes, dptr, ints(torch, caps), res)
    torch.cuda.synchronize()
    exp = [orc_decompress(oracle, b.comp, b.size)[0] for b, _ in blocks]
    assert exp == caps
    _check(blocks, res.cpu().tolist(), dst.cpu().numpy(), doffs, exp)


def _targets(blocks, kind, rng):
    """kind 0: at or past the output size; 1: inside a probe's match; 2: inside its literals."""
    out = []
    for b, _ in blocks:
        if kind == 0:
            out.append(b.size + rng.choice((0, 0, 1, 7)))
        elif not b.probes:
            out.append(rng.randrange(0, b.size + 1))
        else:
            i = rng.choice(b.probes)
            o, m, me = S.layout(b.seqs, b.tail)[i]
            out.append(rng.randrange(m, me) if kind == 1 else rng.randrange(o, m + 1))
    return out


@pytest.mark.parametrize("kind", ["past-end", "in-match", "in-literals"])
@pytest.mark.parametrize("part", sorted(PARTS))
def test_decompress_partial(cuda, product, oracle, part, kind):
    torch = cuda
    blocks = PARTS[part]()
    k = ["past-end", "in-match", "in-literals"].index(kind)
    tg = _targets(blocks, k, random.Random(31 + k))
    caps = [b.size for b, _ in blocks]
    src, sptr, sizes = _inputs(torch, blocks)
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[da for _, da in blocks])
    res = ints(torch, [0] * len(blocks))
    product.decompress_partial_batch(sptr, sizes, dptr, ints(torch, tg), ints(torch, caps), res)
    torch.cuda.synchronize()
    exp = []
    for (b, _), t in zip(blocks, tg):
        er, eo = orc_decompress(oracle, b.comp, b.size, t)
        assert 0 <= er <= b.size and (eo == b.out[:er] or any(s[1] == 0 for s in b.seqs)), b.describe()
        assert k or er == b.size, b.describe()     # a target at or past the end: the full decode
        exp.append(er)
    _check(blocks, res.cpu().tolist(), dst.cpu().numpy(), doffs, exp, prefix=True)


@pytest.mark.parametrize("part", sorted(PARTS))
def test_decompress_fast(cuda, product, oracle, part):
    """decompress_fast on the (valid) blocks: consumed bytes as the oracle's, bytes as the plain
    decoder's."""
    torch = cuda
    blocks = PARTS[part]()
    osz = [b.size for b, _ in blocks]
    src, sptr, sizes = _inputs(torch, blocks)
    dst, dptr, doffs = alloc_out(torch, osz, misalign=[da for _, da in blocks])
    res = ints(torch, [0] * len(blocks))
    product.decompress_fast_ptr_batch(sptr, sizes, dptr, ints(torch, osz), res)
    torch.cuda.synchronize()
    rets = res.cpu().tolist()
    exp = [oracle.orc_decompress_fast(buf(b.comp), C.create_string_buffer(b.size + 64), b.size)
           for b, _ in blocks]
    assert exp == [len(b.comp) for b, _ in blocks]
    bad = [(b, da, "consumed %d, oracle %d" % (r, e)) for (b, da), r, e in zip(blocks, rets, exp) if r != e]
    assert not bad, _report(bad)
    _check(blocks, osz, dst.cpu().numpy(), doffs, osz)


# ------------------------------------------------------------------ dictionary
def _orc_dict(oracle, b, d):
    o = C.create_string_buffer(b.size + 64)
    return oracle.orc_decompress_safe_usingDict(buf(b.comp), o, len(b.comp), b.size, buf(d), len(d))


def _dict_decode(torch, amd, blocks, dicts, adjacent):
    """decompress_dict_batch with dicts[i] right before its output slot (adjacent: one
    alloc_out slot holds dictionary + output, and the dictionary is checked to be untouched)
    or detached (one device copy per distinct dictionary, at an odd address).
    Returns (results, host copy of the outputs, output offsets)."""
    n = len(blocks)
    src, sptr, sizes = _inputs(torch, blocks)
    caps = [b.size for b, _ in blocks]
    if adjacent:
        dst, _, offs = alloc_out(torch, [len(d) + c for d, c in zip(dicts, caps)])
        host = dst.cpu().numpy()
        for o, d in zip(offs, dicts):
            host[o:o + len(d)] = np.frombuffer(d, np.uint8)
        dst.copy_(torch.from_numpy(host))
        dictp = [dst.data_ptr() + o for o in offs]
        doffs = [o + len(d) for o, d in zip(offs, dicts)]
    else:
        dst, _, doffs = alloc_out(torch, caps)
        uniq = {}
        for d in dicts:
            uniq.setdefault(id(d), d)
        ddev, _, dpos = pack(torch, [b"\0\0\0" + d for d in uniq.values()], min_len=4)
        at = {k: dpos[i] + 3 for i, k in enumerate(uniq)}
        dictp = [ddev.data_ptr() + at[id(d)] for d in dicts]
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    res = ints(torch, [0] * n)
    amd.decompress_dict_batch(sptr, sizes, t64([dst.data_ptr() + o for o in doffs]), ints(torch, caps),
                              t64(dictp), ints(torch, [len(d) for d in dicts]), res)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    if adjacent:
        for o, d, (b, _) in zip(offs, dicts, blocks):
            assert host[o:o + len(d)].tobytes() == d, "dictionary overwritten: " + b.describe(True)
    return res.cpu().tolist(), host, doffs


@pytest.mark.parametrize("adjacent", [False, True], ids=["detached", "adjacent"])
def test_dictionary_ends(cuda, product, oracle, adjacent):
    """(d): sources inside, at the end of, straddling and at the first byte of the dictionary,
    sizes 1..70000; and an offset one past what dictionary + output allow fails as the oracle."""
    good, bad = S.dictionary()
    if adjacent:   # every block of a small dictionary; of the 64 KiB ones (a copy each) every 16th
        good = [b for i, b in enumerate(good) if len(b.hist) <= 100 or i % 16 == 0]
        bad = [b for b in bad if len(b.hist) <= 100]
    blocks = [(b, len(b.hist) & 15 if adjacent else 0) for b in good + bad]
    rets, host, doffs = _dict_decode(cuda, product, blocks, [b.hist for b, _ in blocks], adjacent)
    exp = [_orc_dict(oracle, b, b.hist) for b, _ in blocks]
    assert exp[:len(good)] == [b.size for b in good] and all(e < 0 for e in exp[len(good):])
    ng = len(good)
    _check(blocks[:ng], rets[:ng], host, doffs[:ng], exp[:ng], dict_mode=True)
    wrong = [(b, da, "ret %d, oracle %d" % (r, e))
             for (b, da), r, e in zip(blocks[ng:], rets[ng:], exp[ng:]) if r != e]
    assert not wrong, _report(wrong, True)


@pytest.mark.parametrize("dsize", [0, 100])
def test_grid_with_an_unused_dictionary(cuda, product, oracle, dsize):
    """(a) through the dictionary instantiation with no dictionary and with 100 bytes no match
    reaches: the same bytes."""
    blocks = [(b, 0) for b in S.grid()]
    d = random.Random(8).randbytes(dsize)
    rets, host, doffs = _dict_decode(cuda, product, blocks, [d] * len(blocks), False)
    exp = [_orc_dict(oracle, b, d) for b, _ in blocks]
    assert exp == [b.size for b, _ in blocks]
    _check(blocks, rets, host, doffs, exp)
