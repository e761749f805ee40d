"""The dictionary trainer's rule, tests/dicttrainmodel.py, on the CPU: hand-checked cases, the
rule against its wrong neighbours on the inputs of tests/test_gpu_dict_train.py (a kernel that
followed a neighbour would write other bytes for at least one of them), and the quality
condition: a trained dictionary beats what a caller without a trainer does, judged by the
product's host codec (loadDict + compress_fast_continue, byte-identical to the reference)."""
import ctypes as C
import functools

import pytest

import dicttrainmodel as M
from lz4util import I

Case = functools.partial(dict, sizes=None)


def rand(n, seed):
    return I.make("rand", n, seed=seed)


@functools.lru_cache(maxsize=None)
def collision_pair():
    """Two 8-byte strings with the same table index, by a seeded search (about 2^11 random
    strings suffice for a table of 2^20 entries)."""
    seen = {}
    stream = rand(8 * 8192, 77)
    for o in range(0, len(stream), 8):
        s = stream[o:o + 8]
        other = seen.setdefault(M.index_of(s), s)
        if other != s:
            return other, s
    raise AssertionError("no collision in 8192 strings")


def edge_sizes(k, max_sample):
    """The sizes at which a slot appears, fills up or is cut: 0, 7, 8, 9, k - 1, k, k + 1, j * st
    + 7, j * st + 8 and max_sample, one negative size and one above max_sample."""
    st = k // 4
    return [0, 7, 8, 9, k - 1, k, k + 1, 5 * st + 7, 5 * st + 8, max_sample, -3, max_sample + 1,
            max_sample, 3 * st + 7, 3 * st + 8]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(samples, sizes, capacity, segment, max_sample): the smallest shapes at which
    each part of the kernels can go wrong."""
    out = {}
    n, L, cap, k = M.QUALITY[2]
    out["quality 64 x 256 B"] = Case(samples=M.corpus(n, L, 1), capacity=cap, segment=k,
                                     max_sample=L)
    # every buffer holds max_sample + 1 bytes of the same phrase stream, so that a kernel which
    # counted an ignored sample, or read past a stated size, would see repeats of the others
    k, ms = 32, 100
    stream = b"".join(M.corpus(4, 256, 3))
    sizes = edge_sizes(k, ms)
    out["edge sizes"] = Case(samples=[stream[7 * i:7 * i + ms + 1] for i in range(len(sizes))],
                             sizes=sizes, capacity=256, segment=k, max_sample=ms)
    out["one sample, fewer slots than rounds"] = Case(samples=[M.corpus(1, 64, 4)[0]],
                                                      capacity=1024, segment=16, max_sample=64)
    few = M.corpus(12, 200, 5)
    out["capacity no multiple of the segment"] = Case(samples=few, capacity=1000, segment=48,
                                                      max_sample=200)
    out["capacity of one segment"] = Case(samples=few, capacity=64, segment=64, max_sample=200)
    three = M.corpus(3, 2048, 6)
    out["segment 16"] = Case(samples=three, capacity=256, segment=16, max_sample=2048)
    out["segment 1024"] = Case(samples=three, capacity=4096, segment=1024, max_sample=2048)
    out["identical samples"] = Case(samples=[M.corpus(1, 200, 8)[0]] * 8, capacity=512,
                                    segment=32, max_sample=200)
    out["one repeated string"] = Case(samples=[b"abcdefgh" * 32, rand(256, 5)], capacity=128,
                                      segment=32, max_sample=256)
    a, b = collision_pair()
    # sample 0's first segment holds both strings of the pair, sample 1's the first of them and
    # one more string that is as frequent: equal by distinct strings, not by distinct indices
    c = rand(8, 91)
    tail = b"".join(rand(8, 100 + t) for t in range(2))
    out["collision pair"] = Case(samples=[a + b + tail, a + c + tail[::-1], a, b, c, c],
                                 capacity=32, segment=32, max_sample=32)
    out["random bytes"] = Case(samples=[rand(100, 200 + i) for i in range(256)], capacity=1024,
                               segment=32, max_sample=100)
    # more samples than the count pass has waves (16384) and more slots in a round than the
    # score pass has (4096): both loop
    stream = b"".join(M.corpus(64, 1024, 10))
    out["more samples and slots than waves"] = Case(
        samples=[stream[3 * i:3 * i + 16] for i in range(17000)], capacity=32, segment=16,
        max_sample=16)
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    """(dictionary, info) of a case -- computed once, shared by the CPU and the GPU tests."""
    return M.train(**cases()[name])


# ---- hand-checked ----
P = bytes(range(50, 66))                                     # the phrase that occurs twice
ONE = bytes(range(0, 8)) + P + bytes(range(100, 108)) + P    # 48 bytes, P at 8 and at 32


def test_one_sample_whose_best_segment_is_known():
    """k 16, st 4: slot 2 is P exactly, 9 substrings counted twice each (18); slot 8 is P again
    and ties, every other slot holds fewer of P's substrings."""
    d, info = M.train([ONE], 16, 16, 48)
    assert d == P and info == [16, 1, 0, 0]


def test_layout_and_zero_fill():
    """Capacity 40: two rounds over slots [0, 6) and [6, 12).  Round 0 takes P (slot 2) and zeroes
    its nine counts; in round 1 slot 8 (P again) and slots 9, 10 are worth 0, slot 7 keeps 4
    substrings that are not P's, slot 6 = [24, 40) keeps 8 and wins.  Pick 0 lies last."""
    d, info = M.train([ONE], 40, 16, 48)
    assert d == bytes(8) + ONE[24:40] + P
    assert info == [32, 2, 0, 0]


def test_info_counts_ignored_samples_and_negative_sizes_are_empty():
    d, info = M.train([ONE, ONE + b"x", ONE, ONE], 16, 16, 48, sizes=[48, 49, -5, 7])
    assert (d, info) == (P, [16, 1, 1, 0])
    d, info = M.train([], 64, 16, 48)
    assert (d, info) == (bytes(64), [0, 0, 0, 0])
    d, info = M.train([ONE + b"x"], 64, 16, 48)              # nothing but an ignored sample
    assert (d, info) == (bytes(64), [0, 0, 1, 0])


def test_the_dictionary_always_has_capacity_bytes():
    for name, case in cases().items():
        d, info = model(name)
        assert len(d) == case["capacity"], name
        u = info[0]
        assert d[:len(d) - u] == bytes(len(d) - u) and 0 < u <= len(d), name
        assert info[1] <= case["capacity"] // case["segment"]
    assert model("one sample, fewer slots than rounds")[1][0] < 1024
    assert model("edge sizes")[1][2] == 1


def test_the_collision_pair_collides():
    a, b = collision_pair()
    assert a != b and M.index_of(a) == M.index_of(b)


# ---- the rule against its wrong neighbours ----
WRONG = {
    "every occurrence counted, not distinct indices": M.RULE._replace(distinct="none"),
    "distinct strings, not distinct indices": M.RULE._replace(distinct="string"),
    "no zeroing after a pick": M.RULE._replace(zeroing=False),
    "the highest slot wins a tie": M.RULE._replace(low_tie=False),
    "picks laid front to back": M.RULE._replace(back_to_front=False),
    "substrings counted across the sample boundary": M.RULE._replace(within_sample=False),
    "n not cut at the sample's end": M.RULE._replace(cut_n=False),
}


@pytest.mark.parametrize("name", list(WRONG))
def test_the_gpu_inputs_tell_the_rule_from_its_neighbour(name):
    hits = [c for c, case in cases().items() if M.train(rule=WRONG[name], **case) != model(c)]
    print(name, "->", hits)
    assert hits, name


# ---- the quality condition ----
def compressed_total(amd, messages, dictionary):
    """loadDict + compress_fast_continue at acceleration 1, a fresh stream per message."""
    L = C.CDLL(amd.LIB_PATH)   # a handle of its own: the signatures set here are not amd.lib()'s
    L.APE_LZ4_createStream.restype = C.c_void_p
    L.APE_LZ4_freeStream.argtypes = [C.c_void_p]
    L.APE_LZ4_resetStream.argtypes = [C.c_void_p]
    L.APE_LZ4_loadDict.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.APE_LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int,
                                                 C.c_int, C.c_int]
    st = C.c_void_p(L.APE_LZ4_createStream())
    total = 0
    try:
        for m in messages:
            L.APE_LZ4_resetStream(st)
            if dictionary:
                assert L.APE_LZ4_loadDict(st, dictionary, len(dictionary)) == min(len(dictionary), 65536)
            cap = amd.compressBound(len(m))
            out = C.create_string_buffer(cap)
            r = L.APE_LZ4_compress_fast_continue(st, m, out, len(m), cap, 1)
            assert r > 0
            total += r
    finally:
        L.APE_LZ4_freeStream(st)
    return total


@pytest.mark.parametrize("row", range(3))
def test_a_trained_dictionary_beats_the_naive_ones(product, row):
    """The issue's prototype: 54613 / 33014 / 23254 bytes trained against 67908 / 39299 / 24744
    for the better naive dictionary (ratios 0.804, 0.840, 0.940)."""
    n, L, cap, k = M.QUALITY[row]
    train, held_out = M.corpus(n, L, 1), M.corpus(128, L, 2)
    d, info = M.train(train, cap, k, L)
    none = compressed_total(product, held_out, b"")
    head = compressed_total(product, held_out, M.naive(train, cap))
    tail = compressed_total(product, held_out, M.naive(train, cap, tail=True))
    trained = compressed_total(product, held_out, d)
    print("%d x %d B -> %d B, k %d: none %d head %d tail %d trained %d (%.3f of the better naive), "
          "info %s" % (n, L, cap, k, none, head, tail, trained, trained / min(head, tail), info))
    assert trained < head and trained < tail
    if row < 2:
        assert trained <= 0.90 * min(head, tail)
