"""The high-ratio mode's cost-minimising parse on the CPU: tests/hcoptmodel.py (the definition of
what APE_LZ4_compress_hc_opt_batch_dev, its withPrefix form and
APE_LZ4_compress_large_hc_opt_batch_dev write) against the oracle's decoders, against the lazy
parse it replaces (tests/hcmodel.py, tests/hclargemodel.py) -- and against its own wrong
neighbours on the inputs that tests/test_gpu_hc_opt.py runs on the GPU."""
import functools

import pytest

import hclargemodel
import hcmodel
import hcoptmodel as M
from lz4util import I, orc_decompress
from test_gpu_hc import DEPTHS, blocks
from test_hc_large_model import check_large, data, dict_decode

# Blocks of the grid that the cost-minimising parse makes LARGER than the lazy one, per depth (at
# most 2 each; DESIGN.md 3.16 names them).  None: on this grid the new parse never loses.
LARGER = {1: [], 8: [], 64: [], 256: []}


@functools.lru_cache(maxsize=None)
def lazy(depth):
    return [hcmodel.compress(b, depth) for b in blocks()]


@functools.lru_cache(maxsize=None)
def opt(depth):
    return [M.compress(b, depth) for b in blocks()]


def name(i):
    """Block i of the grid as "content size"."""
    sizes = len(blocks()) - 6
    per = sizes // len(I.ENC_CONTENTS)
    if i < sizes:
        return "%s %d" % (I.ENC_CONTENTS[i // per], len(blocks()[i]))
    return ("text 65536", "comp 65536", "zeros 65536", "period3 65536", "rand 65536",
            "comp 65535")[i - sizes]


@pytest.mark.parametrize("depth", DEPTHS)
def test_grid_decodes_costs_what_it_says_and_is_no_larger_than_lazy(oracle, depth):
    total_lazy = total_opt = 0
    for i, (src, out, was) in enumerate(zip(blocks(), opt(depth), lazy(depth))):
        n = len(src)
        assert len(out) <= oracle.orc_compressBound(n), (name(i), depth)
        assert orc_decompress(oracle, out, n) == (n, src), (name(i), depth)
        ML, MQ = hclargemodel.search(src, 0, depth)
        A, _ = M.price(src, 0, ML.tolist(), MQ.tolist())
        assert int(A[0]) == len(out), (name(i), depth)
        if name(i) not in LARGER[depth]:
            assert len(out) <= len(was), (name(i), depth, len(out), len(was))
        total_lazy += len(was)
        total_opt += len(out)
    assert len(LARGER[depth]) <= 2
    print("depth %d: %d blocks, lazy %d bytes, cost-minimising %d" % (
        depth, len(blocks()), total_lazy, total_opt))


def test_size_table():
    """The table of DESIGN.md 3.16 (pytest -s prints it)."""
    pick = [(nm, i) for i, nm in enumerate(map(name, range(len(blocks())))) if "655" in nm]
    for nm, i in pick:
        print("%-14s %s" % (nm, "  ".join("depth %d: %d -> %d" % (d, len(lazy(d)[i]), len(opt(d)[i]))
                                          for d in DEPTHS)))
    for nm, i in pick[:2]:   # text and comp: the parse pays at every depth
        for d in DEPTHS:
            assert len(opt(d)[i]) < len(lazy(d)[i])


def test_the_shortcut_for_the_full_length_is_the_plain_one():
    half = I.make("comp", 8192, seed=2)
    cases = [I.make(c, 4096) for c in ("zeros", "byte", "period2", "period3", "period7")]
    cases.append(half + half)
    for src in cases:
        for depth in (1, 8):
            ML, MQ = hclargemodel.search(src, 0, depth)
            ML, MQ = ML.tolist(), MQ.tolist()
            E = M.full_length(src, 0, ML, MQ)
            assert E == M.full_length_plain(src, 0, ML, MQ)
            assert max(E) > M.CAP
    # with history: the window's positions, the block's matches
    w = cases[-1]
    ML, MQ = hclargemodel.search(w, 8192, 8)
    assert M.full_length(w, 8192, ML.tolist(), MQ.tolist()) == \
        M.full_length_plain(w, 8192, ML.tolist(), MQ.tolist())


@pytest.mark.parametrize("content", I.ENC_CONTENTS)
def test_the_window_form(oracle, content):
    whole = I.make(content, 65536 + 4096, seed=5)
    for n in (0, 12, 13, 100, 4096):
        src = whole[65536:65536 + n]
        assert M.compress_prefix(src, 0, 8) == M.compress(src, 8)
        for pre in (1, 63, 64, 1000, 65536 - n):
            window = whole[65536 - pre:65536 + n]
            out = M.compress_prefix(window, pre, 8)
            assert len(out) <= oracle.orc_compressBound(n)
            assert dict_decode(oracle, out, n, window[:pre]) == (n, src), (n, pre)
            if pre <= 1000:   # (the full window once: the lazy model is slow)
                assert len(out) <= len(hclargemodel.compress_prefix(window, pre, 8)), (n, pre)


@pytest.mark.parametrize("content", ["comp", "text"])
def test_large_inputs(oracle, content):
    src = data(content, 200000)
    for restart in (0, 65536):
        out = M.compress_large(src, 8, restart)
        check_large(oracle, src, out, restart)
        was = hclargemodel.compress_large(src, 8, restart)
        print("%s 200000 depth 8 restart %d: lazy %d, cost-minimising %d" % (
            content, restart, len(was), len(out)))
        assert len(out) <= len(was)
    small = data(content, 4096)
    assert M.compress_large(small, 8) == M.compress(small, 8)


# The rule, moved to its neighbours.
WRONG = {
    "shortest length on ties": M.RULE._replace(longest=False),
    "literal wins ties": M.RULE._replace(match_wins_ties=False),
    "no full-length candidate": M.RULE._replace(full_length=False),
    "no literal-length term": M.RULE._replace(literal_term=False),
}


@pytest.mark.parametrize("which", sorted(WRONG))
def test_the_gpu_inputs_tell_the_rule_from_its_neighbour(which):
    """A kernel that followed the wrong rule would write different bytes for at least one block
    of the GPU tests' grid (and so fail there)."""
    told = [name(i) for i, (b, want) in enumerate(zip(blocks(), opt(8)))
            if M.compress(b, 8, WRONG[which]) != want]
    print("%s: told apart by %s" % (which, told))
    assert told


def test_the_gpu_inputs_tell_the_parse_from_the_lazy_one():
    told = [name(i) for i in range(len(blocks())) if opt(8)[i] != lazy(8)[i]]
    print("the lazy parse: told apart by %d blocks" % len(told))
    assert told
