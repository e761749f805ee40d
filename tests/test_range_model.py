"""Byte ranges of indexed blocks, pinned without a GPU: tests/rangeutil.py is a Python model
of the range read (include/ape_lz4_gpu.h, "byte ranges of indexed blocks").  On reference-made
and handcrafted multi-segment blocks a read around every segment boundary must give the
oracle's decompress_safe slice at the place the window says, with exactly the documented
need; and the test for a final literal run must take runs and nothing else."""
import pytest

import indexutil as X
import rangeutil as RU
from lz4util import I, orc_compress, orc_decompress
from rangeutil import stop_edge_block

SIZES = (70000, 13, 65536, 100000, 1)

_CACHE = {}


def cases(oracle):
    """[(block, words, the oracle's decode)]: chunks compressed by the oracle and stitched
    (an empty segment, a last segment that is the final run), and two handcrafted blocks
    (many short segments, empty ones, a 40-byte final run)."""
    if "v" not in _CACHE:
        text = I.make("text", sum(SIZES))
        starts = [sum(SIZES[:k]) for k in range(len(SIZES))]
        streams = [orc_compress(oracle, text[a:a + n])[1] for a, n in zip(starts, SIZES)]
        block = X.stitch(streams)
        r, plain = orc_decompress(oracle, block, len(text))
        assert r == len(text) and plain == text
        out = [(block, X.build_index(block, starts), plain)]
        for seed, sized in ((0, None), (5, 2304)):
            b, w, n = stop_edge_block(seed, sized)
            r, plain = orc_decompress(oracle, b, n)
            assert r == n
            out.append((b, w, plain))
        _CACHE["v"] = out
    return _CACHE["v"]


def expected_window(block, words, a, m):
    """The documented formula, written out once more: (a - lo, hi - lo)."""
    nseg, n = words[1], words[2]
    ip = [words[4 + 2 * j] for j in range(nseg + 1)]
    op = [words[5 + 2 * j] for j in range(nseg + 1)]
    j0 = max(j for j in range(nseg) if op[j] <= a < op[j + 1])
    j1 = max(j for j in range(nseg) if op[j] <= a + m - 1 < op[j + 1])
    run = j1 == nseg - 1 and RU.final_run(block, n, ip[j1], op[j1]) is not None
    lo = a if run and j0 == nseg - 1 else op[j0]
    E = a + m if run else op[j1 + 1]
    hi = E if run and j0 == nseg - 1 else min(E + 16, n)
    return a - lo, hi - lo


@pytest.mark.parametrize("which", [0, 1, 2])
def test_reads_around_every_segment_boundary(oracle, which):
    block, words, plain = cases(oracle)[which]
    nseg, n = words[1], words[2]
    assert len(plain) == n
    memo = {}
    bounds = sorted({words[5 + 2 * j] for j in range(nseg + 1)})
    seen = 0
    for b in bounds:
        for a in (b - 1, b, b + 1):
            for length in (1, 2, 300, n):
                if not 0 <= a < n:
                    continue
                m = min(length, n - a)
                r, win, data = RU.decode_range(block, words, a, length, n, memo=memo)
                assert r == m and data == plain[a:a + m], (a, length, r)
                assert win == expected_window(block, words, a, m), (a, length)
                assert 0 <= win[0] and win[0] + m <= win[1] <= n
                # exactly need bytes of room suffice; one less is ERANGE with the same window
                assert RU.decode_range(block, words, a, length, win[1], memo=memo) == (r, win, data)
                assert RU.decode_range(block, words, a, length, win[1] - 1, memo=memo) == \
                    (RU.ERANGE, win, b"")
                seen += 1
    assert seen > 4 * len(bounds)
    # the ends of the block and the empty range
    assert RU.decode_range(block, words, 0, n, n) == (n, (0, n), plain)
    assert RU.decode_range(block, words, n, 0, 0) == (0, (0, 0), b"")
    assert RU.decode_range(block, words, n, 5, 0) == (0, (0, 0), b"")
    assert RU.decode_range(block, words, 7, 0, 0) == (0, (0, 0), b"")
    for a, length in ((n + 1, 1), (-1, 1), (0, -1)):
        assert RU.decode_range(block, words, a, length, n) == (-1, (0, 0), b"")
    assert RU.decode_range(block, words, 0, 1, n, max_segments=nseg - 1)[0] == RU.ERANGE


def test_binary_search_is_the_documented_one():
    op = [0, 0, 10, 10, 10, 25, 40]   # empty segments: equal neighbours
    nseg = len(op) - 1
    for x in range(40):
        j = RU.find_segment(op, nseg, x)
        assert op[j] <= x < op[j + 1]
    assert RU.find_segment([0, 7], 1, 3) == 0
    # a column that is not sorted: the search still ends, the plan's checks reject the request
    words = [X.MAGIC, 3, 30, 9, 0, 0, 3, 20, 6, 10, 9, 30]
    assert RU.decode_range(bytes(9), words, 15, 1, 64)[0] == -1


def run_block(L, lead=True):
    """Two segments: one sequence with a match (or nothing), then a final run of L bytes."""
    tail = bytes((7 * k + 1) & 255 for k in range(L))
    first = [(b"abcdefgh", 8, 12)] if lead else []
    block = X.emit(first + [(tail, 0, 0)])
    ip1 = len(X.emit(first)) if lead else 0
    op1 = 20 if lead else 0
    n = op1 + L
    if lead:
        words = [X.MAGIC, 2, n, len(block), 0, 0, ip1, op1, len(block), n]
    else:
        words = X.trivial_index(len(block), n)
    return block, words, tail, op1


def test_an_empty_final_run():
    block, words, _, _ = run_block(0, lead=False)   # (no match may end a block: the run alone)
    assert block == b"\x00" and RU.final_run(block, 0, 0, 0) == 1
    assert RU.decode_range(block, words, 0, 5, 0) == (0, (0, 0), b"")
    assert RU.decode_range(block, words, 1, 5, 0) == (-1, (0, 0), b"")


@pytest.mark.parametrize("L", [14, 15, 16, 269, 270, 271, 15 + 2 * 255])
def test_final_runs_are_recognised(oracle, L):
    block, words, tail, op1 = run_block(L)
    n = words[2]
    r, plain = orc_decompress(oracle, block, n)
    assert r == n and plain[op1:] == tail
    lit0 = RU.final_run(block, n, words[6], op1)
    assert lit0 is not None and block[lit0:] == tail
    for a, m in ((op1, L), (op1 + L // 2, L - L // 2), (op1 + 1, 3), (n - 1, 1)):
        if m < 1 or a + m > n or a < op1:
            continue
        # inside the run: the window is the range itself
        assert RU.decode_range(block, words, a, m, m) == (m, (0, m), tail[a - op1:a - op1 + m])
    if L:
        # straddling op_last: from the first segment's start to the range's end, no tail of 16
        r, win, data = RU.decode_range(block, words, op1 - 3, 4, 64)
        assert (r, win) == (4, (op1 - 3, min(op1 + 1 + 16, n))) and data == plain[op1 - 3:op1 + 1]
    # a wrong byte anywhere in the token or the length bytes: no run
    for k in range(words[6], lit0):
        for bit in (0x10, 0x01) if k == words[6] else (0x01, 0x80):
            broken = bytearray(block)
            broken[k] ^= bit
            took = RU.final_run(bytes(broken), n, words[6], op1) is not None
            assert took == (k == words[6] and bit == 0x01)   # (the token's match nibble is unused)


def test_a_block_that_is_one_run():
    block, words, tail, _ = run_block(70000, lead=False)
    assert words[1] == 1
    assert RU.decode_range(block, words, 12345, 4096, 4096) == (4096, (0, 4096), tail[12345:12345 + 4096])
    assert RU.decode_range(block, words, 0, 70000, 70000) == (70000, (0, 70000), tail)
    assert RU.decode_range(block, words, 69999, 9, 1) == (1, (0, 1), tail[-1:])
    assert RU.decode_range(block, words, 100, 10, 9) == (RU.ERANGE, (0, 10), b"")


def closed_form_counter_example(k=3):
    """A last segment of k sequences of 15 literals and a 4-byte match, then a final run: such
    a sequence costs 19 bytes (token, one length byte, 15 literals, the offset) and produces
    19, so the segment meets the closed form 1 + lenbytes(L) + L of one run of L bytes
    whenever its final run has as many length bytes as a run of L would."""
    seqs = [(bytes(range(q, q + 15)), 15, 4) for q in range(k)]
    for final in range(12, 400):
        tail = bytes((3 * q) & 255 for q in range(final))
        seg = X.emit(seqs + [(tail, 0, 0)])
        L = 19 * k + final
        if len(seg) == 1 + RU.lenbytes(L) + L:
            return seqs, tail
    raise AssertionError("no counter-example")


def counter_example_block():
    seqs, tail = closed_form_counter_example()
    first = [(b"abcdefgh", 8, 12)]
    block = X.emit(first + seqs + [(tail, 0, 0)])
    ip1 = len(X.emit(first))
    n = 20 + sum(len(s[0]) + s[2] for s in seqs) + len(tail)
    return block, [X.MAGIC, 2, n, len(block), 0, 0, ip1, 20, len(block), n]


def test_the_closed_form_alone_is_not_a_run(oracle):
    block, words = counter_example_block()
    n, c = words[2], words[3]
    L = n - 20
    assert c - words[6] == 1 + RU.lenbytes(L) + L          # the closed form holds ...
    assert RU.final_run(block, n, words[6], 20) is None     # ... and the bytes deny it
    r, plain = orc_decompress(oracle, block, n)
    assert r == n
    for a, m in ((25, 10), (19, 5), (n - 3, 3), (20, L)):
        r, win, data = RU.decode_range(block, words, a, m, n)
        assert (r, data) == (m, plain[a:a + m])
        assert win == (a - (20 if a >= 20 else 0), n - (20 if a >= 20 else 0))   # a decode to n
