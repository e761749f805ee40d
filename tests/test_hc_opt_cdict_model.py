"""The cost-minimising parse against a prepared dictionary, on the CPU: tests/hcoptdictmodel.py
(the definition of what APE_LZ4_compress_hc_opt_usingCDict_batch_dev writes) against the
oracle's usingDict decoder, against tests/hcoptmodel.py and tests/hcdictmodel.py, and against its
wrong neighbours on the inputs that tests/test_gpu_hc_opt_cdict.py runs on the GPU (which
imports the two new families from here)."""
import functools

import pytest

import hcdictmodel
import hclargemodel
import hcoptdictmodel as M
import hcoptmodel
from hcmodel import CAP
from lz4util import I, walk_ok
from test_gpu_cdict import dict_of
from test_gpu_stream import orc_dict_decode
from test_hc_cdict_model import (DICT_SIZES, FAMILY_DICT_SIZES, FAMILY_MAX_SRC, LENGTHS, MAX_SRC,
                                 boundary_family, grid_messages, tail_family)

LONG_J = (1, 2, 3, 4, 5, 64, 100, 300)
RUN_J = (1, 2, 3, 4, 7, 64, 100)


def long_boundary(d, j):
    """A message whose later part repeats [the dictionary's last j bytes | its own first 300]:
    that part's match starts j bytes before the message and is j + 300 bytes long, so the search
    reports 272 of them and the parse's extension reads on, in the dictionary (j = 300), across
    the boundary or in the message."""
    head = I.make("rand", 300, seed=5000 + j)
    return head + I.make("rand", 30, seed=6000 + j) + d[-j:] + head + I.make("rand", 40, seed=7000 + j)


def run_message(d, j):
    """700 bytes that continue the dictionary's last j bytes with period j: every position of
    the run has a capped match at offset j, the first j of them from the dictionary."""
    return (d[-j:] * (700 // j + 1))[:700] + I.make("rand", 100, seed=8000 + j)


def long_family(d):
    return [long_boundary(d, j) for j in LONG_J if j <= len(d)]


def run_family(d):
    return [run_message(d, j) for j in RUN_J if j <= len(d)]


@functools.lru_cache(maxsize=None)
def block(dict_size, message, max_src, depth):
    return M.compress(dict_of(dict_size), message, max_src, depth)


@functools.lru_cache(maxsize=None)
def lazy_block(dict_size, message, max_src, depth):
    return hcdictmodel.compress(dict_of(dict_size), message, max_src, depth)


def families(d):
    return boundary_family(d) + tail_family(d)


@pytest.mark.parametrize("dict_size", [70000, 100])
def test_blocks_decode_and_the_cost_is_the_size(oracle, dict_size):
    """The original dictionary is larger than D (70000) or smaller than 64 KiB (100)."""
    d = dict_of(dict_size)
    cases = [(m, MAX_SRC, 8) for L in LENGTHS for m in grid_messages(L, 2)]
    cases += [(m, FAMILY_MAX_SRC, 8)
              for m in boundary_family(d) + tail_family(d)[::7] + long_family(d) + run_family(d)]
    cases += [(grid_messages(1000, 1)[0], MAX_SRC, depth) for depth in (1, 64, 256)]
    for m, max_src, depth in cases:
        c = block(dict_size, m, max_src, depth)
        assert orc_dict_decode(oracle, c, len(m), d) == (len(m), m), (len(m), max_src, depth)
        win, D, ML, MQ = M.searched(d, m, max_src, depth)
        assert D == hcdictmodel.window(dict_size, max_src) and win[D:] == m
        A, _ = hcoptmodel.price(win, D, ML, MQ)
        assert int(A[D]) == len(c), (len(m), max_src, depth)


def test_without_a_window_it_is_the_block_model():
    for m in grid_messages(1000, 2) + grid_messages(13, 1) + grid_messages(5, 1):
        assert M.compress(b"", m, MAX_SRC, 8) == hcoptmodel.compress(m, 8)
        assert M.compress(dict_of(4096), m, 65536, 8) == hcoptmodel.compress(m, 8)


def test_it_is_the_prefix_model_on_the_window():
    d = dict_of(4095)
    for m in grid_messages(1000, 2) + long_family(d)[:2]:
        assert M.compress(d, m, FAMILY_MAX_SRC, 8) == hcoptmodel.compress_prefix(d + m, len(d), 8)


@pytest.mark.parametrize("dict_size", DICT_SIZES)
def test_no_block_grows_on_the_grid(dict_size):
    for L in LENGTHS:
        for m in grid_messages(L):
            assert len(block(dict_size, m, MAX_SRC, 8)) <= len(lazy_block(dict_size, m, MAX_SRC, 8)), L


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_no_block_grows_on_the_families(dict_size, depth):
    for k, m in enumerate(families(dict_of(dict_size))):
        assert len(block(dict_size, m, FAMILY_MAX_SRC, depth)) <= \
            len(lazy_block(dict_size, m, FAMILY_MAX_SRC, depth)), k


def _crossing(c):
    """The matches of block c longer than the cap whose source starts in the dictionary and
    runs into the message."""
    pos, out = 0, []
    for lit, off, ml in walk_ok(c):
        pos += lit
        if ml > CAP and 0 < off - pos < ml:
            out.append((pos, off, ml))
        pos += ml
    return out


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_the_new_families_extend_across_the_boundary(dict_size):
    d = dict_of(dict_size)
    msgs = long_family(d) + run_family(d)
    assert len(msgs) == (15 if dict_size >= 300 else 14) and max(map(len, msgs)) <= FAMILY_MAX_SRC
    for k, m in enumerate(msgs):
        assert _crossing(block(dict_size, m, FAMILY_MAX_SRC, 8)), k


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_the_run_shortcut_crosses_the_boundary(dict_size):
    """run_message: the capped matches at offset j are one run; its upper members have their
    source in the message, its first j in the dictionary, and E comes down the run unbroken."""
    d = dict_of(dict_size)
    for j in RUN_J:
        win, D, ML, MQ = M.searched(d, run_message(d, j), FAMILY_MAX_SRC, 8)
        run = [p for p in range(D, D + 700 - CAP) if ML[p] == CAP and p - MQ[p] == j]
        assert run == list(range(D, D + 700 - CAP)), j
        assert all(MQ[p] < D for p in run[:j]) and all(MQ[p] >= D for p in run[j:])
        E = hcoptmodel.full_length(win, D, ML, MQ)
        assert E == hcoptmodel.full_length_plain(win, D, ML, MQ)
        assert all(p + E[p] == run[-1] + E[run[-1]] for p in run) and E[D] >= 700


def _differs(d, msgs, depth=8, **how):
    return [M.compress(d, m, FAMILY_MAX_SRC, depth) != M.compress(d, m, FAMILY_MAX_SRC, depth, **how)
            for m in msgs]


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_neighbours_of_the_full_length(dict_size):
    """Every message of both families tells the rule from the one without the full-length
    candidate and from the one whose extension stops at the dictionary's end."""
    d = dict_of(dict_size)
    msgs = long_family(d) + run_family(d)
    assert all(_differs(d, msgs, rule=hcoptmodel.RULE._replace(full_length=False)))
    assert all(_differs(d, msgs, stop_at_dict=True))
    # the neighbour is this kernel's alone: without a dictionary it is the rule
    assert not any(_differs(b"", msgs, stop_at_dict=True))


GRID_DICT_SIZES = (0, 3, 100, 4095, 61440, 70000)


def _grid_differs(dict_size, depth, rule):
    d = dict_of(dict_size)
    return [M.compress(d, m, MAX_SRC, depth) != M.compress(d, m, MAX_SRC, depth, rule)
            for m in grid_messages(1000)]


@pytest.mark.parametrize("depth", [1, 8, 64])
@pytest.mark.parametrize("dict_size", GRID_DICT_SIZES)
def test_other_neighbours_on_the_grid(dict_size, depth):
    """The families above do not tell the rule from these; grid_messages(1000) does, at every
    dictionary size and depth of this grid: all four messages for shortest-on-ties, some for
    literal-wins-ties and for the lazy parse."""
    R = hcoptmodel.RULE
    assert all(_grid_differs(dict_size, depth, R._replace(longest=False)))
    assert any(_grid_differs(dict_size, depth, R._replace(match_wins_ties=False)))
    assert any(block(dict_size, m, MAX_SRC, depth) != lazy_block(dict_size, m, MAX_SRC, depth)
               for m in grid_messages(1000))
    assert all(len(block(dict_size, m, MAX_SRC, depth)) <= len(lazy_block(dict_size, m, MAX_SRC, depth))
               for m in grid_messages(1000))


@pytest.mark.parametrize("depth", [1, 8, 64])
@pytest.mark.parametrize("dict_size", [0, 3, 100])
def test_neighbour_without_the_literal_term(dict_size, depth):
    """Dictionary sizes 0, 3 and 100 show it at every depth.  (Behind 61440 or 70000 bytes and
    above depth 1 literal runs of 15 are too rare on these messages: nothing differs there.)"""
    assert any(_grid_differs(dict_size, depth, hcoptmodel.RULE._replace(literal_term=False)))
