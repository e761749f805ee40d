"""The high-ratio mode against a prepared dictionary, on the CPU: tests/hcdictmodel.py (the
definition of what APE_LZ4_compress_hc_usingCDict_batch_dev writes) against the oracle's
usingDict decoder, against tests/hclargemodel.py, and against its own wrong neighbours on the
inputs that tests/test_gpu_hc_cdict.py runs on the GPU (which imports them from here)."""
import pytest

import hcdictmodel as M
import hclargemodel
from lz4util import I, walk_ok
from test_gpu_cdict import dict_of, plain
from test_gpu_stream import orc_dict_decode

BASE = 70000
MAX_SRC = 1000
DICT_SIZES = (0, 1, 3, 4, 63, 100, 4095, 65535, 70000)
LENGTHS = (0, 1, 5, 12, 13, 64, 65, 1000)
BOUNDARY_J = (1, 2, 3, 4, 5, 8, 20, 64, 300)
FAMILY_MAX_SRC = 1024
FAMILY_DICT_SIZES = (100, 61440)


def grid_messages(L, count=4):
    """`count` messages of L bytes, MAX_SRC bytes apart behind the dictionary's end."""
    return [plain()[BASE + MAX_SRC * k:BASE + MAX_SRC * k + L] for k in range(count)]


def boundary_message(d, j):
    """A message whose later part repeats [the dictionary's last j bytes | its own first 24]:
    the longest match of that part starts j bytes before the message, at a position whose 4
    bytes straddle the boundary (j <= 3) or inside the dictionary, running on into the message
    (j >= 4; 300 + 24 bytes pass the search's cap of 272, so the parse extends it across)."""
    head = I.make("rand", 24, seed=1000 + j)
    return head + I.make("rand", 30, seed=2000 + j) + d[-j:] + head + I.make("rand", 40, seed=3000 + j)


def boundary_family(d):
    return [boundary_message(d, j) for j in BOUNDARY_J]


def tail_family(d):
    """The messages of test_gpu_cdict.test_matches_stop_at_the_dictionary_end: they continue the
    dictionary's last j bytes."""
    msgs = []
    for j in (1, 2, 3, 4, 7, 8, 9, 20, 63, 64, 200):
        for fill in (0x00, 0xFF, 0xCD):
            first = d[-j:] + bytes([fill]) * 48 + I.make("rand", 100, seed=j)
            msgs += [first, d[-j:] + d[-j:] + first]
    assert max(map(len, msgs)) <= FAMILY_MAX_SRC
    return msgs


def test_window():
    assert [M.window(s, 1000) for s in DICT_SIZES] == [0, 1, 3, 4, 63, 100, 4095, 64536, 64536]
    assert M.window(70000, 65536) == 0 and M.window(70000, 1) == 65535
    assert M.window(61440, 1024) == 61440 and M.window(100, 1024, M.RULE._replace(round64=True)) == 64


@pytest.mark.parametrize("dict_size", [70000, 100])
def test_blocks_decode_with_the_original_dictionary(oracle, dict_size):
    """The original is larger than D (70000) or smaller than 64 KiB (100)."""
    d = dict_of(dict_size)
    cases = [(m, MAX_SRC, 8) for L in LENGTHS for m in grid_messages(L, 2)]
    cases += [(m, FAMILY_MAX_SRC, 8) for m in boundary_family(d) + tail_family(d)[::7]]
    cases += [(grid_messages(1000, 1)[0], MAX_SRC, depth) for depth in (1, 64, 256)]
    for m, max_src, depth in cases:
        c = M.compress(d, m, max_src, depth)
        assert orc_dict_decode(oracle, c, len(m), d) == (len(m), m), (len(m), max_src, depth)


def test_without_a_dictionary_it_is_the_block_model():
    for m in grid_messages(1000, 2) + grid_messages(13, 1):
        assert M.compress(b"", m, MAX_SRC, 8) == hclargemodel.compress_prefix(m, 0, 8)
        assert M.compress(dict_of(4096), m, 65536, 8) == hclargemodel.compress_prefix(m, 0, 8)


@pytest.mark.parametrize("dict_size", [3, 100, 4095])
def test_the_plain_search_is_the_windowed_one(dict_size):
    """search_plain carries the neighbours; with the rule itself it is hclargemodel.search."""
    d = dict_of(dict_size)
    for m in grid_messages(1000, 2) + grid_messages(13, 1) + boundary_family(d):
        D = M.window(len(d), FAMILY_MAX_SRC)
        win = d[len(d) - D:] + m
        for depth in (1, 8):
            ML, MQ = hclargemodel.search(win, D, depth)
            assert M.search_plain(win, D, depth) == (ML.tolist(), MQ.tolist()), (len(m), depth)


def _differs(d, msgs, max_src, rule, depth=8):
    return [M.compress(d, m, max_src, depth) != M.compress(d, m, max_src, depth, rule) for m in msgs]


@pytest.mark.parametrize("dict_size", [100, 4095])
def test_neighbour_window_rounded_to_64(dict_size):
    """(At 61440 and 70000 with maxSrcSize 1000 it changes nothing: sizes that are no multiple
    of 64 are what tells the two apart.)"""
    assert any(_differs(dict_of(dict_size), grid_messages(1000), MAX_SRC,
                        M.RULE._replace(round64=True)))


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_neighbour_match_ends_at_the_dictionary_end(dict_size):
    d = dict_of(dict_size)
    msgs = [boundary_message(d, j) for j in BOUNDARY_J if 4 <= j <= 64]
    assert all(_differs(d, msgs, FAMILY_MAX_SRC, M.RULE._replace(stop_at_dict=True)))


def test_a_capped_match_is_extended_across_the_boundary():
    """j = 300: the match starts 300 bytes before the message, the search reports 272 of its 324
    bytes, and the parse's extension is what crosses into the message."""
    d = dict_of(61440)
    pos = 0
    crossing = []
    for lit, off, ml in walk_ok(M.compress(d, boundary_message(d, 300), FAMILY_MAX_SRC, 8)):
        pos += lit
        crossing.append(ml > hclargemodel.CAP and 0 < off - pos < ml)
        pos += ml
    assert any(crossing)


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_neighbour_straddling_positions_left_out_of_the_chains(dict_size):
    d = dict_of(dict_size)
    msgs = [boundary_message(d, j) for j in (1, 2, 3)]
    assert all(_differs(d, msgs, FAMILY_MAX_SRC, M.RULE._replace(straddle=False)))


@pytest.mark.parametrize("dict_size", [100, 61440])
def test_neighbour_no_history(dict_size):
    d = dict_of(dict_size)
    assert any(_differs(d, grid_messages(1000), MAX_SRC, M.RULE._replace(history=False)))
    assert any(_differs(d, tail_family(d)[-6:], FAMILY_MAX_SRC, M.RULE._replace(history=False)))
