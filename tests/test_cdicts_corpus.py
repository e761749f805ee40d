"""tests/cdictscorpus.py can fail a wrong kernel: for every ordered pair (k, other) of distinct
dictionaries of a set, at least one message assigned to k has different bytes when it is
compressed against `other` -- under the fast encoder's model for both sets, and under the
high-ratio model at depth 8 for the content set.  Messages are assigned round-robin, so a kernel
that used object 0 for every message, or d_cdict[i - 1] or d_cdict[i + 1] for message i, would
write other bytes than the single-dictionary call for some message of every dictionary
(tests/test_gpu_cdicts.py compares exactly those).  The model runs only on messages of at most
1000 bytes."""
import functools

import pytest

import cdictscorpus as K
import encmodel
import hcdictmodel


@functools.lru_cache(maxsize=None)
def fast(name, j, k):
    s = {x.name: x for x in K.sets()}[name]
    return encmodel.encode_cdict(s.messages[j], s.dicts[k], K.MAX_SRC)


@functools.lru_cache(maxsize=None)
def deep(name, j, k):
    s = {x.name: x for x in K.sets()}[name]
    return hcdictmodel.compress(s.dicts[k], s.messages[j], K.MAX_SRC, 8)


def telling(s, model, k, other):
    """the messages of dictionary k, largest first, until one tells `other` from k"""
    mine = sorted((j for j in s.of(k) if j in set(s.small())), key=lambda j: -len(s.messages[j]))
    return next((j for j in mine if model(s.name, j, k) != model(s.name, j, other)), None)


def test_the_shape_of_the_corpus():
    for s in K.sets():
        assert len(s.dicts) == 4 and len(s.messages) == 64
        assert s.owner == [j % 4 for j in range(64)]
        assert sorted({len(m) for m in s.messages}) == list(K.LENGTHS)
        for k in range(4):
            assert sorted(len(s.messages[j]) for j in s.of(k)) == sorted(K.LENGTHS * K.ROUNDS)
    c = K.content_set()
    assert [len(d) for d in c.dicts] == [K.DICT_BYTES] * 4 and len(set(c.dicts)) == 4
    assert [len(d) for d in K.size_set().dicts] == list(K.SIZES)


@pytest.mark.parametrize("name", ["content", "size"])
def test_every_pair_of_dictionaries_is_told_apart_by_the_fast_model(name):
    s = {x.name: x for x in K.sets()}[name]
    for k in range(4):
        for other in range(4):
            if other != k:
                assert telling(s, fast, k, other) is not None, (name, k, other)


def test_every_pair_of_content_dictionaries_is_told_apart_by_the_high_ratio_model():
    s = K.content_set()
    for k in range(4):
        for other in range(4):
            if other != k:
                assert telling(s, deep, k, other) is not None, (k, other)
