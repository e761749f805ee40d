"""What the decoder's copy-phase corpus reaches, proved on the CPU (no GPU here).

tests/decseq.py writes blocks from sequence lists and defines their bytes by the plain
byte-at-a-time decoder; tests/deccopyclass.py restates which path of copy_segment a sequence
takes.  Here: build() and the plain decoder on hand-written cases and against the oracle; the
restated scheduler, run on poisoned memory, reproduces the plain decoder's bytes on every
single-batch block (so its order of rounds and passes is a possible one); the corpus reaches
every class in at least MIN_BLOCKS blocks; and eight deliberately faulty decoders, each one
class slipping, are told from the true one by the corpus -- and hardly or not at all by what
tests/test_gpu_decode.py decoded before (test_what_the_dense_blocks_catch).
"""
import collections
import ctypes as C
import functools
import random

import pytest

import deccopyclass as K
import decseq as S
from lz4util import buf, orc_decompress

MIN_BLOCKS = 8


# ------------------------------------------------------------------ build and the plain decoder
def test_build_hand_cases():
    # one literal run
    assert S.build([], b"abc") == (b"\x30abc", b"abc")
    # "abcd" + match(off 4, n 8) + 12 tail bytes: token 0x44, offset 04 00
    t = b"0123456789AB"
    assert S.build([(b"abcd", 4, 8)], t) == (b"\x44abcd\x04\x00\xc0" + t, b"abcdabcdabcd" + t)
    # offset 1 repeats the last byte; match length 19 takes the extension byte 0, 20 the byte 1
    assert S.build([(b"x", 1, 19)], t) == (b"\x1fx\x01\x00\x00\xc0" + t, b"x" * 20 + t)
    assert S.build([(b"x", 1, 20)], t)[0] == b"\x1fx\x01\x00\x01\xc0" + t
    # 273 = 4 + 15 + 254, 274 = 4 + 15 + 255: the second extension byte appears
    assert S.build([(b"x", 1, 273)], t)[0] == b"\x1fx\x01\x00\xfe\xc0" + t
    assert S.build([(b"x", 1, 274)], t)[0] == b"\x1fx\x01\x00\xff\x00\xc0" + t
    # literal length 15 takes an extension byte; a 16-byte tail too
    assert S.build([(b"q" * 15, 15, 4)], b"T" * 16)[0] == b"\xf0\x00" + b"q" * 15 + b"\x0f\x00\xf0\x01" + b"T" * 16
    # overlap: off 3, n 7 over "abc" -> abcabcabca
    assert S.build([(b"abc", 3, 7)], t)[1] == b"abcabcabca" + t
    # offset 0 decodes as zero bytes
    assert S.build([(b"abc", 0, 5)], t)[1] == b"abc" + bytes(5) + t
    # history in front: offset 5 at output position 2 reads the history's last 3 bytes first
    assert S.build([(b"ab", 5, 6)], t, history=b"..XYZ")[1] == b"abXYZabX" + t
    # one past the history is refused (strict) or yields no expected output
    with pytest.raises(AssertionError):
        S.build([(b"ab", 8, 4)], t, history=b"..XYZ")
    assert S.build([(b"ab", 8, 4)], t, history=b"..XYZ", strict=False)[1] is None
    assert S.layout([(b"abcd", 4, 8), (b"", 1, 4)], t) == [(0, 4, 12), (12, 12, 16), (16, 28, 28)]


def _orc_dict(oracle, comp, cap, d):
    o = C.create_string_buffer(max(cap, 1) + 64)
    r = oracle.orc_decompress_safe_usingDict(buf(comp), o, len(comp), cap, buf(d), len(d))
    return r, o.raw[:max(r, 0)]


def _has_off0(b):
    return any(s[1] == 0 for s in b.seqs)


def test_plain_decoder_agrees_with_the_oracle(oracle):
    """200 random blocks of the corpus: value and bytes (offset 0 excepted: the reference copies
    what dst held there), and the offsets one past the dictionary fail."""
    good, bad = S.dictionary()
    pool = S.grid() + S.edges(1) + S.edges(2) + S.slides() + S.chains() + good + \
        S.multibatch("short") + S.multibatch("restage") + [b for b, _ in S.flush_edges()]
    for b in random.Random(9).sample(pool, 200):
        r, o = _orc_dict(oracle, b.comp, b.size, b.hist) if b.hist else orc_decompress(oracle, b.comp, b.size)
        assert r == b.size == len(b.out), b.describe()
        assert o == b.out or _has_off0(b), b.describe()
    for b in bad:
        assert _orc_dict(oracle, b.comp, b.size, b.hist)[0] < 0, b.describe()


def test_constants_come_from_the_kernel():
    assert set(K.CONST) == {"kWinB", "kKeep", "kStage", "kWinNeed", "kBatch", "kLaneMax"}
    assert all(v > 0 for v in K.CONST.values())
    # the geometry the corpus is placed by, for the constants as they are today
    if (K.CONST["kWinB"], K.CONST["kKeep"]) == (2048, 512):
        assert K.segments(6000) == [(0, 2048, 0, 0), (2048, 3584, 1536, 2048),
                                    (3584, 5120, 3072, 3584), (5120, 6000, 4608, 5120)]
        assert K.segments(6000, da=5)[1] == (2048, 3584, 1536, 2043)
        assert K.segments(2048) == [(0, 2048, 0, 0)]


# ------------------------------------------------------------------ the classified corpus
@functools.lru_cache(None)
def classified():
    """[(block, dictionary instantiation?, pieces)] of parts (a)-(d): all single-batch."""
    good, _ = S.dictionary()
    out = []
    for b in S.grid() + S.edges(1) + S.edges(2) + S.slides() + S.chains() + good:
        assert b.single_batch(), b.describe()
        dm = b.part == "dict"
        pieces, got = K.simulate(b.seqs, b.tail, len(b.hist) if dm else None, 0, None, b.hist)
        assert bytes(got) == b.out, b.describe(dm)
        out.append((b, dm, pieces))
    return out


def test_scheduler_restatement_reproduces_the_plain_decoder():
    """On poisoned memory, so a pass that ran before its sources were written would show; the
    dictionary blocks also with dst misaligned as the adjacent placement makes it."""
    for b, dm, _ in classified():
        if dm and len(b.hist) & 15:
            _, got = K.simulate(b.seqs, b.tail, len(b.hist), len(b.hist) & 15, None, b.hist)
            assert bytes(got) == b.out, b.describe(True, len(b.hist) & 15)


# why a (class, round 1?, cut?) combination cannot occur in a valid single-batch block
def unreachable(cls, r1, cut):
    if cls == "wave.straddle-base":
        return ("a lane-sized match whose source starts below the window base ends below gdone "
                ">= base + kKeep - 15 > base + kLaneMax: it is lane.hist; only long matches straddle")
    if cls == "wave.hist-cap":
        return "a history source lies below base, more than 16 bytes below the capacity"
    if cls == "wave.overlap-below-base":
        return "off < n <= kLaneMax puts the source within 64 bytes of the match, above base (base <= S0 - kKeep)"
    if r1 and (cls.startswith("wave.") or cls == "zero.wave"):
        return "round 1 takes lane-path matches only (r1m is a subset of lpm)"
    if not r1 and cls in ("zero.lane", "lane.hist", "lane.dict"):
        return "no source inside the segment (pe <= gdone <= S0, <= 0, or none at all)"
    if not cut and cls == "wave.cut":
        return "a whole match has at least 4 bytes"
    if cut and cls in ("wave.long.per-dict", "wave.dict-overlap"):
        return "off < 64 reaching into the dictionary puts the match in the first 64 output bytes"
    return None


def test_every_class_is_reached():
    """Parts (b), (c), (d) reach every (class, round 1 / dependent pass, whole / cut by a
    segment edge) that can occur, each in at least MIN_BLOCKS blocks; the others are listed by
    unreachable() with the reason, and none of those occurs."""
    seen = collections.Counter()
    for b, dm, pieces in classified():
        if b.part != "grid":
            for c in {(p.cls, p.rnd == 0, p.cut) for p in pieces}:
                seen[c] += 1
    report = []
    for cls in K.CLASSES:
        for r1 in (True, False):
            for cut in (False, True):
                why, n = unreachable(cls, r1, cut), seen[(cls, r1, cut)]
                if why:
                    assert n == 0, (cls, r1, cut, n, why)
                else:
                    report.append((n, cls, "round 1" if r1 else "dependent", "cut" if cut else "whole"))
    assert not set(c for c, _, _ in seen) - set(K.CLASSES)
    short = [r for r in report if r[0] < MIN_BLOCKS]
    assert not short, short
    assert len(report) == COVERAGE_ROWS, sorted(report)


COVERAGE_ROWS = 35   # reachable combinations today (DESIGN.md 3.21 carries the counts)


def test_chains_reach_every_depth():
    """(c): chains 1..20 deep behind a first match that is itself dependent (its source is its
    own literal run), so the last pass is 2..21; in the chains with a whole-wave item in the
    middle it runs between two lane passes (the pass loop's else branch, then lanes again); and
    the span chains hold a match that waits for three or more sequences."""
    deepest = collections.Counter()
    for b, dm, pieces in classified():
        if b.part != "chain":
            continue
        deepest[max(p.rnd for p in pieces)] += 1
        variant, depth = b.note.split()[0], int(b.note.split()[1][6:])
        if variant.startswith("wave-") and depth >= 3 and b.note.endswith("front=100"):
            lanes = [p.rnd for p in pieces if p.cls.startswith("lane.") and p.rnd]
            assert any(p.cls.startswith("wave.") and min(lanes) < p.rnd < max(lanes) for p in pieces), b.describe()
        if variant == "span3" and b.note.endswith("front=100"):
            assert any(p.cls.startswith("lane.") and p.need >= 3 for p in pieces), b.describe()
    assert all(deepest[d] >= 4 for d in range(2, 22)), sorted(deepest.items())


# ------------------------------------------------------------------ wrong neighbours
def _in_class(fault, pieces):
    names = K.FAULT_CLASSES[fault]
    if fault == "cut-restart":
        return any(p.cut and p.seg > 0 and p.ma > 0 and _second(p, pieces) for p in pieces)
    if fault == "early":
        return any(p.cls.startswith("lane.") and p.rnd >= 2 for p in pieces)
    return any(p.cls in names for p in pieces)


def _second(p, pieces):
    return any(q.seq == p.seq and q.seg < p.seg for q in pieces)


@pytest.mark.parametrize("fault", sorted(K.FAULTS))
def test_wrong_neighbours_are_caught_by_the_corpus(fault):
    """Each faulty decoder (deccopyclass.FAULTS: one class slipping) differs from the true
    output on at least 3 corpus blocks, all of them blocks with a piece of the class it names:
    every block without such a piece decodes as before."""
    caught = 0
    for b, dm, pieces in classified():
        inside = _in_class(fault, pieces)
        _, got = K.simulate(b.seqs, b.tail, len(b.hist) if dm else None, 0, fault, b.hist)
        differs = got != list(b.out)
        assert inside or not differs, (fault, b.describe(dm))
        caught += differs
    print(fault, "caught on", caught, "blocks")
    assert caught >= 3, (fault, caught)


# sequence-level forms of three neighbours, for blocks of any size (segment cuts ignored)
def _plain_fault(b, fault):
    out = bytearray()
    bad = False
    for lits, off, n in b.seqs:
        out += lits
        ma = len(out)
        for t in range(n):
            out.append(out[-off] if off else 0)
        if fault == "overlap-read-all":
            bad |= 16 <= off < n <= 64
        elif fault == "lpo8":
            bad |= 8 <= off < 16 and off < n <= 64
        elif fault == "per32":
            bad |= 32 <= off < 64 and n > 64
    return bad


DENSE_BEFORE = {"overlap-read-all": 9, "lpo8": 48, "per32": 21}


def test_what_the_dense_blocks_catch():
    """The "before" numbers: the neighbours over a replay of test_gpu_decode.py's _dense_block
    (seed 77, its mix, its draws between blocks): 240 blocks, 109,886 sequences, 20 of them in
    the lane self-overlap class 16 <= off < n <= 64; 120 blocks are decoded whole (the others
    are mutated or cut short and compared up to their error only).

    Sequence-level neighbours (has the block a sequence that would decode differently; segment
    cuts ignored), blocks of the 120: overlap-read-all 9, lpo8 48, per32 21 -- the small
    offsets sit in a block's first few hundred bytes, at window base 0.
    The restated scheduler on the 62 of the 120 that are single-batch blocks (3 or 40 sequences,
    up to 4198 output bytes): round-up 56, early 28, lpo8 11, cut-restart 8, base-from-window 5,
    per32 5, overlap-read-all 2, dict-one-side 0 (no dictionary there).  So the dense blocks
    do tell most neighbours apart, by a handful of blocks each and at positions nobody chose;
    the corpus here does so at every offset, length and window relation (the counts printed by
    test_wrong_neighbours_are_caught_by_the_corpus)."""
    blocks = S.dense_replay()
    assert len(blocks) == 240 and sum(len(b.seqs) for b, _ in blocks) == 109886
    whole = [b for b, w in blocks if w]
    assert len(whole) == 120
    assert sum(16 <= s[1] < s[2] <= 64 for b, _ in blocks for s in b.seqs) == 20
    for fault, n in DENSE_BEFORE.items():
        assert sum(_plain_fault(b, fault) for b in whole) == n, fault
    single = [b for b in whole if b.single_batch()]
    got = {}
    for fault in sorted(K.FAULTS):
        got[fault] = sum(K.simulate(b.seqs, b.tail, None, 0, fault)[1] != list(b.out) for b in single)
    print(len(single), got)
    assert (len(single), got) == DENSE_SINGLE


DENSE_SINGLE = (62, {"base-from-window": 5, "cut-restart": 8, "dict-one-side": 0, "early": 28, "lpo8": 11,
                    "overlap-read-all": 2, "per32": 5, "round-up": 56})
