"""APE_LZ4_decompress_safe_size_batch_dev (include/ape_lz4f_placed.h) against the oracle: the
value decompress_safe returns -- the decoded size or -(ip)-1 -- for every block of the corpus at
every capacity, result for result and with no block left out, without a destination.  With
dictionary sizes, against the oracle's decompress_safe_usingDict."""
import base64
import ctypes as C
import random

import pytest

import decseq as S
import inputs as I
from gpuutil import ints, pack
from lz4util import buf, orc_compress, orc_decompress, walk_ok

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def _valid_blocks(oracle, golden):
    """[(name, block, decoded size)]: every block decodes at that capacity."""
    out = []
    for d in golden["decode"]:
        out.append(("golden " + d["name"], base64.b64decode(d["comp_b64"]), d["cap"]))
    for part, blocks in (("grid", S.grid()), ("edge1", S.edges(1)), ("edge2", S.edges(2)),
                         ("slide", S.slides()), ("chain", S.chains()),
                         ("multi-short", S.multibatch("short")),
                         ("multi-restage", S.multibatch("restage")),
                         ("flush", [b for b, _ in S.flush_edges()])):
        out += [("%s %d" % (part, k), b.comp, b.size) for k, b in enumerate(blocks)]
    rng = random.Random(77)
    # more than 2304 compressed bytes and more than 64 sequences: restaged, several batches
    for k in range(3):
        src = I.synth_comp(65536, 500 + k)
        r, comp = orc_compress(oracle, src)
        assert r > 2304 * 2
        out.append(("synth %d" % k, comp, len(src)))
    seqs = [(rng.randbytes(20), 1 + rng.randrange(20), 4 + rng.randrange(30)) for _ in range(200)]
    comp, plain = S.build(seqs, rng.randbytes(S.TAIL))
    assert len(comp) > 2304 and len(seqs) > 64
    out.append(("200 sequences", comp, len(plain)))
    # tokens with 255 extension bytes: literal runs and matches of 15 + 255 k + r
    for lits, ml in ((15 + 255, 4 + 15 + 255), (15 + 510 + 3, 4 + 15 + 510 + 7), (15 + 254, 4 + 15 + 254),
                     (15 + 255 * 9, 40), (3, 4 + 15 + 255 * 10), (2400, 2400)):
        comp, plain = S.build([(rng.randbytes(100), 7, 9), (rng.randbytes(lits), 50, ml),
                               (rng.randbytes(5), 3, 4)], rng.randbytes(S.TAIL))
        out.append(("extensions %d %d" % (lits, ml), comp, len(plain)))
    # a single literal run: 32 bytes of input and more, with one, two and many length bytes
    for n in (31, 32, 100, 15 + 255 - 1, 15 + 255, 15 + 255 + 1, 3000, 65536):
        comp, plain = S.build([], rng.randbytes(n))
        out.append(("one run %d" % n, comp, n))
    out.append(("one byte 00", b"\x00", 0))
    for name, comp, n in out:
        if not name.startswith("golden"):
            assert orc_decompress(oracle, comp, n)[0] == n, name
    return out


def _mutations(valid):
    """Truncations and byte flips (two of each, seeded) of every block -- of the copy-class
    corpus, whose thousands of blocks differ in one sequence, every fourth."""
    rng = random.Random(78)
    out = []
    for k, (name, comp, n) in enumerate(valid):
        if len(comp) < 2 or (name.split()[0] in ("grid", "edge1", "edge2", "slide", "chain") and k % 4):
            continue
        for cut in {rng.randrange(1, len(comp)), len(comp) - 1}:
            out.append(("%s cut %d" % (name, cut), comp[:cut], n))
        for _ in range(2):
            at = rng.randrange(len(comp))
            bad = bytearray(comp)
            bad[at] ^= 1 << rng.randrange(8)
            out.append(("%s flip %d" % (name, at), bytes(bad), n))
    return out


@pytest.fixture(scope="module")
def corpus(oracle, golden):
    valid = _valid_blocks(oracle, golden)
    return valid + _mutations(valid)


def _size(cuda, product, blocks, entries, dict_sizes=None):
    """entries: (block index, csize, cap).  The results, after checking that nothing but them
    was written: the words on either side of the results and the sources' buffer."""
    src, sptr, _ = pack(cuda, blocks)
    before = src.clone()
    idx = cuda.tensor([e[0] for e in entries], dtype=cuda.int64, device="cuda")
    n = len(entries)
    res = ints(cuda, [POISON] * (n + 2))
    product.decompress_size_ptr_batch(
        sptr[idx].contiguous(), ints(cuda, [e[1] for e in entries]),
        ints(cuda, [e[2] for e in entries]), res[1:n + 1],
        dict_sizes=None if dict_sizes is None else ints(cuda, dict_sizes))
    cuda.cuda.synchronize()
    host = res.cpu().tolist()
    assert host[0] == POISON and host[-1] == POISON
    assert cuda.equal(src, before)
    return host[1:-1]


def test_every_block_at_every_capacity_gives_the_oracles_return(cuda, product, oracle, corpus):
    blocks = [c for _, c, _ in corpus]
    entries = []
    for k, (_, comp, n) in enumerate(corpus):
        entries += [(k, len(comp), cap) for cap in (n, n - 1, n + 1, n + 12, 0, -1)]
        entries.append((k, 0, n))
    got = _size(cuda, product, blocks, entries)
    want = []
    for k, csize, cap in entries:
        o = C.create_string_buffer(max(cap, 0) + 64)
        want.append(oracle.orc_decompress_safe(buf(blocks[k]), o, csize, cap))
    bad = [(corpus[e[0]][0], e[1], e[2], g, w) for e, g, w in zip(entries, got, want) if g != w]
    assert not bad, "%d of %d differ; first (block, csize, cap, got, oracle): %s" % (
        len(bad), len(entries), bad[:5])
    # the corpus reaches what it is meant to: sizes, errors, and the special cases
    assert sum(w > 0 for w in want) > len(corpus) and sum(w < -1 for w in want) > len(corpus)
    assert {-1, -2, -3, 0} <= set(want)


DICT_SIZES = (0, 1, 65535, 65536, 70000)


def test_with_dictionary_sizes_against_using_dict(cuda, product, oracle):
    """Blocks written by compress_prefix_batch whose first match reaches into the history."""
    text = I.make("text", 3000, 11)
    chunks = []
    for hist_len, n, period in ((3000, 3000, 3000), (65536, 4000, 3000), (128, 200, 37),
                                (70000, 30000, 3000), (100, 64, 37)):
        whole = (text[:period] * (100000 // period + 1))[:hist_len + n]
        chunks.append((whole, hist_len, n))
    src, sptr, offs = pack(cuda, [w for w, _, _ in chunks])
    at = cuda.tensor([h for _, h, _ in chunks], dtype=cuda.int64, device="cuda")
    caps = [n + n // 255 + 16 for _, _, n in chunks]
    dst = cuda.zeros((len(chunks), max(caps)), dtype=cuda.uint8, device="cuda")
    dptr = cuda.tensor([dst.data_ptr() + k * dst.stride(0) for k in range(len(chunks))],
                       dtype=cuda.int64, device="cuda")
    res = ints(cuda, [0] * len(chunks))
    product.compress_prefix_batch(sptr + at, ints(cuda, [n for _, _, n in chunks]),
                                  ints(cuda, [h for _, h, _ in chunks]), dptr, ints(cuda, caps), res)
    cuda.cuda.synchronize()
    sizes = res.cpu().tolist()
    assert all(s > 0 for s in sizes)
    host = dst.cpu().numpy()
    blocks = [host[k, :s].tobytes() for k, s in enumerate(sizes)]
    for b in blocks:   # the first match starts before the block
        lit, off, _ = walk_ok(b)[0]
        assert off > lit
    entries, dsz, want = [], [], []
    for k, (whole, hist_len, n) in enumerate(chunks):
        history = whole[:hist_len]
        for d in DICT_SIZES:
            dictionary = (bytes(max(d - hist_len, 0)) + history)[-d:] if d else b""
            for cap in (n, n - 1, n + 12, 0):
                entries.append((k, sizes[k], cap))
                dsz.append(d)
                o = C.create_string_buffer(max(cap, 0) + 64)
                want.append(oracle.orc_decompress_safe_usingDict(
                    buf(blocks[k]), o, sizes[k], cap, buf(dictionary), d))
    got = _size(cuda, product, blocks, entries, dict_sizes=dsz)
    bad = [(e, d, g, w) for e, d, g, w in zip(entries, dsz, got, want) if g != w]
    assert not bad, "%d differ; first ((block, csize, cap), dict, got, oracle): %s" % (
        len(bad), bad[:5])
    # the history matters: the blocks decode with enough of it, and fail at the offset without
    for k, (_, hist_len, n) in enumerate(chunks):
        by = {(d, e[2]): w for e, d, w in zip(entries, dsz, want) if e[0] == k}
        assert by[(70000, n)] == n and by[(0, n)] < 0, k
    # a null array is no dictionary
    assert _size(cuda, product, blocks, entries[:8]) == \
        _size(cuda, product, blocks, entries[:8], dict_sizes=[0] * 8)


def test_an_empty_batch(cuda, product):
    assert product.lib().APE_LZ4_decompress_safe_size_batch_dev(None, None, None, None, None, 0,
                                                                None) == 0
