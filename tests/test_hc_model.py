"""The high-ratio encoder's policy on the CPU: tests/hcmodel.py (the definition of what
APE_LZ4_compress_hc_batch_dev writes) against the oracle -- every block decodes with the
reference's decoder, stays within compressBound, and beats compress_default where a deep search
should."""
import pytest

import hcmodel
from hcmodel import CAP
from lz4util import I, orc_compress, orc_decompress

SIZES = [0, 1, 4, 5, 11, 12, 13, 14, 15, 16, 17, 63, 64, 65, 100, 255, 256, CAP - 1, CAP,
         CAP + 1, CAP + 4, CAP + 5, CAP + 6, 4095, 4096]


def check(oracle, src, depth):
    out = hcmodel.compress(src, depth)
    n = len(src)
    assert len(out) <= oracle.orc_compressBound(n), (n, depth)
    assert orc_decompress(oracle, out, n) == (n, src), (n, depth)
    return out


@pytest.mark.parametrize("content", I.ENC_CONTENTS)
def test_edge_sizes_decode_and_stay_within_the_bound(oracle, content):
    for n in SIZES:
        src = I.make(content, n, seed=n)
        for depth in (1, 64):
            check(oracle, src, depth)


@pytest.mark.parametrize("content", ["zeros", "period3", "rand"])
def test_full_blocks_of_degenerate_content(oracle, content):
    src = I.make(content, 65536)
    for depth in (1, 64):
        check(oracle, src, depth)


@pytest.mark.parametrize("content,seed", [("text", 1), ("comp", 3)])
def test_deep_search_beats_compress_default(oracle, content, seed):
    src = I.make(content, 65536, seed=seed)
    ref, _ = orc_compress(oracle, src)
    d8, d64 = len(check(oracle, src, 8)), len(check(oracle, src, 64))
    print("%s: compress_default %d, depth 8 %d, depth 64 %d" % (content, ref, d8, d64))
    assert d8 < ref and d64 < ref
    assert d64 <= d8


@pytest.mark.parametrize("content", I.ENC_CONTENTS)
def test_the_vectorised_search_is_the_plain_one(content):
    """search() (numpy, all positions at once) restates search_plain() (one position at a
    time): the same block on sizes around every rule's edge."""
    for n in (0, 12, 13, 17, 100, CAP + 5, CAP + 6, 1500):
        src = I.make(content, n, seed=n + 1)
        for depth in (1, 3, 64):
            assert hcmodel.compress(src, depth) == hcmodel.compress(src, depth, plain=True), \
                (n, depth)


def test_ties_go_to_the_nearest_and_collisions_spend_depth():
    # "abcdX" three times: the position of the last one sees two candidates of length 4
    src = b"abcd1abcd2abcd3" + bytes(range(100, 120))
    M = hcmodel.search_plain(src, 64)
    assert M[10] == (4, 5) and M[5] == (4, 0)
    # depth 1 sees only the nearest chain member
    src = b"abcdefgh--abcdxxxx--abcdefgh" + bytes(range(100, 120))
    assert hcmodel.search_plain(src, 1)[20] == (4, 10)
    assert hcmodel.search_plain(src, 2)[20] == (8, 0)
