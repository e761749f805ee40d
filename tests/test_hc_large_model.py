"""The high-ratio mode with history and on large inputs, on the CPU: tests/hclargemodel.py (the
definition of what APE_LZ4_compress_hc_withPrefix_batch_dev and
APE_LZ4_compress_large_hc_batch_dev write) against tests/hcmodel.py, the oracle's decoders and
tests/indexutil.py -- and against its own wrong neighbours on the inputs that
tests/test_gpu_hc_large.py runs on the GPU."""
import ctypes as C
import functools

import pytest

import hclargemodel as M
import hcmodel
import indexutil
from lz4util import I, buf, orc_compress, orc_decompress
from test_hc_model import SIZES

S = M.SLICE
PREFIXES = [1, 3, 4, 11, 12, 63, 64, 65, 4096]
CONTENTS = ("comp", "text", "rand", "zeros", "period7")


@functools.lru_cache(maxsize=None)
def _master(content):
    # every generator of inputs.py builds its output front to back: make(c, n) is a prefix
    return I.make(content, 200000)


def data(content, n):
    return _master(content)[:n]


def large_sizes(s):
    return [65537, 65549, 2 * s, 2 * s + 1, 3 * s - 1, 3 * s + 5, 3 * s + 12, 3 * s + 13, 200000]


def mixed():
    """Match-less slices before, between and after compressible ones: carries across several."""
    return I.synth_rand(100000, 7) + data("comp", 150000) + I.synth_rand(40000, 8) + bytes(70000)


def gpu_large_inputs(s):
    """The depth-8 grid of tests/test_gpu_hc_large.py: [(name, bytes)]."""
    out = [("comp %d" % n, data("comp", n)) for n in large_sizes(s)]
    out += [("%s %d" % (c, n), data(c, n)) for c in CONTENTS[1:] for n in (65537, 3 * s + 13, 200000)]
    return out + [("mixed", mixed())]


def dict_decode(oracle, comp, n, history):
    out = C.create_string_buffer(max(n, 1) + 64)
    r = oracle.orc_decompress_safe_usingDict(buf(comp), out, len(comp), n, buf(history),
                                             len(history))
    return r, out.raw[:max(r, 0)]


@pytest.mark.parametrize("content", I.ENC_CONTENTS)
def test_without_history_it_is_the_block_model(content):
    for n in SIZES:
        src = I.make(content, n, seed=n)
        for depth in (1, 64):
            assert M.compress_prefix(src, 0, depth) == hcmodel.compress(src, depth), (n, depth)


def test_used_history():
    assert [M.used_history(p, 100) for p in (-5, 0, 1, 63, 64, 65, 65436, 65437, 70000)] == \
        [0, 0, 1, 63, 64, 65, 65436, 65436, 65436]
    assert [M.used_history(1 << 30, n) for n in (0, 1, 65535, 65536)] == [65536, 65535, 1, 0]
    assert M.slices(200000, 32768)[-1] == (196608, 3392, 62144)
    assert M.slices(200000, 32768, restart=65536)[3:5] == [(98304, 32768, 32768), (131072, 32768, 0)]


@pytest.mark.parametrize("content", I.ENC_CONTENTS)
def test_blocks_with_history_decode_with_the_dictionary(oracle, content):
    """Every size x every prefix, and the prefix that clamps to exactly 65536 - size."""
    whole = I.make(content, 65536 + 4096, seed=5)
    for n in SIZES:
        for pre in PREFIXES + [65536 - n + 7]:
            h = M.used_history(pre, n)
            assert h == min(pre, 65536 - n)
            window = whole[65536 - h:65536 + n]
            for depth in (8,) if pre > 4096 else (1, 64):   # (the full window once: it is slow)
                out = M.compress_prefix(window, h, depth)
                assert len(out) <= oracle.orc_compressBound(n)
                assert dict_decode(oracle, out, n, window[:h]) == (n, window[h:]), (n, pre, depth)


def test_history_is_searched():
    """A block that repeats its history is one match into it; without it, literals."""
    hist = I.synth_rand(300, 1)
    out = M.compress_prefix(hist + hist[:100], 300, 8)
    assert indexutil.parse(out) == [(b"", 300, 95), (hist[95:100], 0, 0)]
    assert len(M.compress_prefix(hist[:100], 0, 8)) == 102
    # fewer than 13 bytes: one literal run, whatever the history
    assert M.compress_prefix(hist + hist[:12], 300, 8) == b"\xc0" + hist[:12]


def check_large(oracle, src, block, restart=0):
    n = len(src)
    assert len(block) <= oracle.orc_compressBound(n)
    assert orc_decompress(oracle, block, n) == (n, src)
    seqs = indexutil.walk(block)
    assert seqs[-1][1] + seqs[-1][2] == n
    if restart:
        for _, op, lits, off, ml in seqs:
            if ml:
                at = op + lits
                assert at - off >= at // restart * restart, (at, off)
        words = indexutil.build_index(block, range(0, n, restart))
        assert indexutil.decode_indexed(block, words, n) == (n, src)


@pytest.mark.parametrize("content", CONTENTS)
def test_large_blocks_decode_and_cover_their_input(oracle, content):
    for n in large_sizes(S):
        src = data(content, n)
        check_large(oracle, src, M.compress_large(src, 8, S=S))


@pytest.mark.parametrize("restart", [S, 2 * S])
@pytest.mark.parametrize("content", CONTENTS)
def test_no_match_crosses_a_restart_point(oracle, content, restart):
    for n in (65537, 2 * S + 1, 3 * S + 13, 200000):
        src = data(content, n)
        check_large(oracle, src, M.compress_large(src, 8, restart, S=S), restart)


def test_the_mixed_input_carries_runs_across_slices(oracle):
    src = mixed()
    block = M.compress_large(src, 8, S=S)
    check_large(oracle, src, block)
    assert max(s[2] for s in indexutil.walk(block)) > S   # a run longer than any one slice
    for restart in (S, 2 * S):
        check_large(oracle, src, M.compress_large(src, 8, restart, S=S), restart)


def test_small_inputs_are_the_block_model():
    for n in (0, 1, 12, 13, 4096, 65536):
        src = data("comp", n)
        assert M.compress_large(src, 8, S=S) == hcmodel.compress(src, 8)


@pytest.mark.parametrize("content", ["text", "comp"])
def test_orders(oracle, content):
    """History pays: large < independent 64 KiB blocks < compress_default; depth pays."""
    src = data(content, 200000)
    ref, _ = orc_compress(oracle, src)
    size = {}
    for depth in (8, 64):
        large = len(M.compress_large(src, depth, S=S))
        alone = sum(len(hcmodel.compress(src[i:i + 65536], depth)) for i in range(0, len(src), 65536))
        restarts = len(M.compress_large(src, depth, 65536, S=S))
        print("%s 200000 depth %d: compress_default %d, independent 64 KiB blocks %d, large %d, "
              "large with restart points every 64 KiB %d" % (content, depth, ref, alone, large, restarts))
        assert large < alone < ref
        size[depth] = large
    assert size[64] <= size[8]


# The rule, moved to its neighbours.
WRONG = {
    "history ignored": M.RULE._replace(history=False),
    "a fixed 32 KiB of history": M.RULE._replace(fixed=32768),
    "matches capped at the input's end": M.RULE._replace(mx_slice=False),
}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_the_gpu_inputs_tell_the_rule_from_its_neighbour(name):
    """A kernel that followed the wrong rule would write different bytes for at least one input
    of the GPU tests (and so fail there)."""
    told = [nm for nm, src in gpu_large_inputs(S)
            if M.compress_large(src, 8, S=S, rule=WRONG[name]) != M.compress_large(src, 8, S=S)]
    print("%s: told apart by %s" % (name, told))
    assert told
    if name == "a fixed 32 KiB of history":   # only a short last slice has room for more
        sizes = dict((nm, len(src)) for nm, src in gpu_large_inputs(S))
        assert "comp 200000" in told and "text 200000" in told
        assert all(M.slices(sizes[nm], S)[-1][2] > 32768 for nm in told)
