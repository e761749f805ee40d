"""The index format of indexed blocks, pinned without a GPU: tests/indexutil.py is a Python
model of the stitch, the index and the segment-by-segment decode (include/ape_lz4_gpu.h).
Independent oracle-compressed chunks are stitched into one block; the model must give back
the source, and must never give other bytes when a word of the index is wrong."""
import pytest

import indexutil as X
from lz4util import I, orc_compress, orc_decompress

SIZES = (70000, 13, 65536, 100000, 1)


_CACHE = {}


def case(oracle):
    """(source, block, index words, chunk starts): built once."""
    if "v" not in _CACHE:
        text = I.make("text", sum(SIZES))
        chunks, pos = [], 0
        for n in SIZES:
            chunks.append(text[pos:pos + n])
            pos += n
        streams = [orc_compress(oracle, c)[1] for c in chunks]
        block = X.stitch(streams)
        starts = [sum(SIZES[:k]) for k in range(len(SIZES))]
        _CACHE["v"] = (text, block, X.build_index(block, starts), starts)
    return _CACHE["v"]


def test_stitched_block_is_one_lz4_block(oracle):
    src, block, words, _ = case(oracle)
    assert orc_decompress(oracle, block, len(src)) == (len(src), src)
    assert X.stitch([block]) == block   # (parse and emit are inverses on it)


def test_index_invariants(oracle):
    src, block, words, starts = case(oracle)
    nseg = len(SIZES)
    assert words[:4] == [X.MAGIC, nseg, len(src), len(block)]
    pairs = [(words[4 + 2 * j], words[5 + 2 * j]) for j in range(nseg + 1)]
    assert pairs[0] == (0, 0) and pairs[-1] == (len(block), len(src))
    assert pairs == sorted(pairs)
    seqs = {s[0]: s for s in X.walk(block)}
    for j, (ip, op) in enumerate(pairs[:-1]):
        assert ip in seqs and seqs[ip][1] == op and op <= starts[j]
    for ip, op, lit, off, ml in seqs.values():
        if ml:
            j = max(k for k in range(nseg) if pairs[k][0] <= ip)
            assert op + lit - off >= pairs[j][1]
    # the chunk of 13 bytes has no match: its segment is empty; the last chunk (1 byte) has
    # none either, and its segment is the final run
    assert pairs[1] == pairs[2]
    assert seqs[pairs[4][0]][4] == 0 and pairs[4][0] < pairs[5][0]


def test_model_decodes_to_the_source(oracle):
    src, block, words, _ = case(oracle)
    assert X.decode_indexed(block, words, len(src)) == (len(src), src)
    assert X.decode_indexed(block, words, len(src) + 17) == (len(src), src)
    assert X.decode_indexed(block, X.trivial_index(len(block), len(src)), len(src)) == (len(src), src)
    assert X.decode_indexed(block, words, len(src), max_segments=len(SIZES) - 1)[0] == X.ERANGE
    assert X.decode_indexed(block, words, len(src) - 1)[0] == -1


def test_a_wrong_index_word_never_gives_other_bytes(oracle):
    src, block, words, _ = case(oracle)
    changed = 0
    for k in range(len(words)):
        for d in (1, -1, 1 << 31):
            w = list(words)
            w[k] = (w[k] + d) & 0xFFFFFFFF
            r, out = X.decode_indexed(block, w, len(src))
            assert r < 0 or (r, out) == (len(src), src), (k, d)
            changed += r < 0
    assert changed   # (the model does reject)


@pytest.mark.parametrize("cut", [1, 2, 3])
def test_a_stop_inside_a_sequence_is_rejected(oracle, cut):
    """An entry that is no token position: the chain steps over it, or the parse from it
    ends elsewhere."""
    src, block, words, _ = case(oracle)
    w = list(words)
    w[4 + 2 * 3] += cut
    r, out = X.decode_indexed(block, w, len(src))
    assert r < 0 or (r, out) == (len(src), src)
