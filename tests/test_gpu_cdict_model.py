"""GPU prepared-dictionary encoder (APE_LZ4_cdict_prepare_dev +
APE_LZ4_compress_usingCDict_batch_dev) against tests/encmodel.py, byte for byte.

encmodel.encode_cdict states the block of (message, dictionary, maxSrcSize).  Every assertion
here is byte equality with it: at the message sizes where the kernel changes path, at every
window size D the object can have, and on messages built for the rules a detached dictionary
adds: the hashed positions end 8 bytes before D, a candidate within 3 bytes of
D is none, a match out of the dictionary ends at D.  The dictionary lies at an odd address and
sources and destinations are misaligned (test_gpu_cdict's helpers).

The case lists are plain functions, so that tests/test_cdict_destsize_model.py (CPU) can show
that these inputs tell the model from its wrong neighbours."""
import functools
import random

import pytest

import encmodel
from lz4util import I
from test_gpu_cdict import encode, prepare
from test_gpu_encode_model import SMALL_SIZES

pytestmark = pytest.mark.gpu

BASE = 70000
EDGES = (75, 76, 77, 76 + 1023, 76 + 1024, 76 + 1025)   # C1, stage 2, extend_match


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


@functools.lru_cache(maxsize=None)
def _natural():
    return I.make("comp", 400000, seed=7)


@functools.lru_cache(maxsize=None)
def dictionary(key):
    """("nat", size): the bytes before the natural messages; ("rand", size): random bytes, so
    that a crafted message matches where it was built to and nowhere else."""
    kind, size = key
    return _natural()[BASE - size:BASE] if kind == "nat" else _rand(900, 70000)[70000 - size:]


@functools.lru_cache(maxsize=None)
def model(msg, key, max_src):
    """The model's block of one case, computed once for the whole session."""
    return encmodel.encode_cdict(msg, dictionary(key), max_src)


def window_of(key, max_src):
    return encmodel.cdict_window(key[1], max_src)


# ---------------- the inputs (no GPU needed to build them) ----------------
# A case is (name, message, dictionary key, maxSrcSize).
def _message(n):
    """The natural message of n bytes: the same under every dictionary and maxSrcSize."""
    at = BASE + 37 * n % 30011
    return _natural()[at:at + n]


# (dictionary size, maxSrcSize) -> D: 0 (an empty dictionary, one below 64 bytes, no room),
# 64, 128, 4096, 61440 and, for messages of up to 64 bytes, 65472
OBJECTS = [(0, 4096), (63, 4096), (64, 4096), (65, 4096), (100, 4096), (130, 4096), (70000, 4096),
           (70000, 61440), (70000, 65536), (70000, 64), (70000, 1), (61440, 1024)]


def size_cases():
    """The sizes where the kernel changes path, under every window size; n == maxSrcSize at
    4096, 1024, 64 and 1."""
    cs = []
    for size, max_src in OBJECTS:
        for n in SMALL_SIZES:
            if n <= max_src:
                cs.append(("nat %d/%d n %d" % (size, max_src, n), _message(n), ("nat", size), max_src))
    return cs


def two_window_cases():
    """The same messages against the same dictionary prepared for two maxSrcSize: D = 61440 and
    D = 4096 (size_cases has both; D comes from the object, not from the message)."""
    return [c for c in size_cases() if c[2] == ("nat", 70000) and c[3] in (4096, 61440)]


START = _rand(901, 12)     # every crafted message begins with these bytes


def _hashed_at(head, lo, want=lambda v: True):
    """The first dictionary position from lo on that is in the table under its own slot."""
    tab = encmodel.dict_table(head, len(head))
    return next(v for v in range(lo + (-lo) % 3, len(head) - 8, 3)
                if tab[encmodel.hashk(head, v)] == v and want(v))


def pieces(head):
    """(name, bytes) of strings that, inside a message, meet one rule's edge each; head is the
    window's dictionary part (D bytes)."""
    D = len(head)
    ps = []
    # The dictionary's last j bytes, then what lies at D in the window (the message's first
    # bytes: a match that is not cut runs on into them) or zeros (what lies after D in the
    # object: a match measured into the pad runs on into them).  j through the zone, through
    # the 8 bytes a hashed position needs (the last hashed position is D - 8, D - 9 or D - 10
    # as D % 3 is 2, 0 or 1), and beyond; from 64 on a whole chunk's lanes lie in the copy.
    for j in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 20, 63, 64, 65, 100, 200):
        if j <= D:
            ps.append(("last %d + start" % j, head[D - j:] + START))
            if j in (4, 8, 9, 10, 11, 12, 20, 64):
                ps.append(("last %d + zeros" % j, head[D - j:] + bytes(24)))
    # matches that end at D exactly, D - c on the producer's measurement edges (c hashed: a
    # multiple of 3; the three D of crafted_cases have the three residues)
    for L in EDGES:
        if L + 64 <= D and (D - L) % 3 == 0:
            stop = bytes([head[D - L - 1] ^ 0x3C])       # (no backward extension)
            ps.append(("%d to D + start" % L, stop + head[D - L:] + START))
            ps.append(("%d to D + zeros" % L, stop + head[D - L:] + bytes(24)))
    if D >= 4096:
        # inside the dictionary: the copy starts at a hashed position, one and two before it
        # (backward extension into the dictionary: its positions are hashed three apart, so
        # two bytes is as far as it goes without a collision)
        v = _hashed_at(head, D // 2)
        for b in (0, 1, 2):
            ps.append(("interior, %d back" % b, bytes([head[v - b - 1] ^ 0x3C]) + head[v - b:v + 40]))
        # Backward extension stopped by the candidate's position c cannot be built: the first
        # candidate the table can hold is window position 6 (0 reads as empty, 3 is below
        # min_cand = 4), and at most 4 bytes are taken, so min(4, c, pending) is never c.
        # "window start" below is the nearest there is: candidate 6, 4 bytes back, to 2.
        # ... and stopped by the pending literals: a match that ends where the copy starts
        # (one that runs one byte on into the copy: of the 2 bytes, 1 is left to take)
        a = _hashed_at(head, 300, lambda a: head[a + 20] == head[v - 2] and head[a + 21] != head[v - 1])
        ps.append(("interior, back stopped by the previous match", head[a:a + 20] + head[v - 2:v + 40]))
        # the window's first bytes: position 0 reads as an empty slot, position 3 is no
        # candidate, position 6 is one and extends back to 2
        ps.append(("window start", head[:30]))
        ps.append(("window position 3", head[3:30]))
    return ps


def placed(name, piece):
    """The piece three times: in the message's first chunk, in a chunk the steps without edge
    code take, and in the last two chunks."""
    return [(name + ", first chunk", START + piece + _rand(902, 20)),
            (name + ", inner chunk", START + _rand(903, 188) + piece + _rand(904, 160)),
            (name + ", last chunks", START + _rand(905, 120) + piece + _rand(906, 13))]


def _own_start(at, L, where):
    """A message whose bytes at `where` repeat its own bytes at `at` (window position D + at,
    inside the zone for at <= 3), L of them."""
    b = bytearray(_rand(907 + at, where + 200))
    b[where:where + L] = b[at:at + L]
    b[where + L] = b[at + L] ^ 0x55
    return bytes(b)


# (dictionary, maxSrcSize) of the crafted messages: D = 61440, 4096 and 8192 (D % 3 = 0, 1, 2),
# and the two smallest windows
CRAFTED_OBJECTS = [(("rand", 70000), 4096), (("rand", 70000), 61440), (("rand", 70000), 57344),
                   (("rand", 64), 4096), (("rand", 130), 4096)]


def crafted_cases():
    cs = []
    for key, max_src in CRAFTED_OBJECTS:
        D = window_of(key, max_src)
        head = dictionary(key)[key[1] - D:]
        tag = "D %d: " % D
        for name, piece in pieces(head):
            cs += [(tag + nm, msg, key, max_src) for nm, msg in placed(name, piece)]
        # candidates at the message's own positions 0, 3 (inside the zone) and 4 (outside)
        for at in (0, 3, 4):
            for L in (7, 12):
                for where in (100, 230):
                    cs.append((tag + "own position %d, %d bytes at %d" % (at, L, where),
                               _own_start(at, L, where), key, max_src))
    return cs


def all_cases():
    return size_cases() + crafted_cases()


# ---------------- running the kernel ----------------
def by_object(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c[2], c[3]), []).append(c)
    return groups


def run(torch, amd, cases):
    """[(case, result, bytes)], one prepare and one launch per (dictionary, maxSrcSize)."""
    out = []
    for (key, max_src), cs in by_object(cases).items():
        obj = prepare(torch, amd, dictionary(key), max_src)
        rs, outs = encode(torch, amd, obj, [c[1] for c in cs])
        out += zip(cs, rs, outs)
    return out


def assert_model(got):
    for c, r, comp in got:
        want = model(c[1], c[2], c[3])
        assert r == len(want), (c[0], r, len(want))
        assert comp == want, (c[0], next(i for i in range(r) if comp[i] != want[i]))


# ---------------- the tests ----------------
def test_sizes_and_windows(cuda, product):
    for size, max_src in OBJECTS:
        assert product.cdict_window(size, max_src) == (window_of(("nat", size), max_src))
    assert_model(run(cuda, product, size_cases()))


def test_one_message_under_two_windows(cuda, product):
    """D is the object's: the same message and dictionary give other bytes when the object
    was prepared for another maxSrcSize, the bytes the model gives."""
    cases = two_window_cases()
    got = run(cuda, product, cases)
    assert_model(got)
    by = {}
    for c, r, comp in got:
        by.setdefault(c[1], {})[c[3]] = comp
    differ = [m for m, v in by.items() if v[4096] != v[61440]]
    assert differ and sorted(differ) == sorted(
        m for m in by if model(m, ("nat", 70000), 4096) != model(m, ("nat", 70000), 61440))


def test_crafted_messages(cuda, product):
    assert_model(run(cuda, product, crafted_cases()))


def test_in_one_mixed_batch(cuda, product):
    """The crafted messages of one object shuffled among natural ones: a block's bytes do not
    depend on its neighbours in the batch."""
    key, max_src = CRAFTED_OBJECTS[0]
    cs = [c for c in crafted_cases() if (c[2], c[3]) == (key, max_src)]
    cs += [("nat n %d" % n, _message(n), key, max_src) for n in SMALL_SIZES]
    random.Random(11).shuffle(cs)
    assert_model(run(cuda, product, cs))
