"""The fast encoder's rule on the CPU: tests/encmodel.py (the definition of what
APE_LZ4_compress_batch_dev, _fast_batch_dev and _withPrefix_batch_dev write) against the oracle
-- every block decodes with the reference's decoder and stays within compressBound -- and
against its own wrong neighbours: every constant of the rule, changed, changes the block of at
least one input that tests/test_gpu_encode_model.py runs on the GPU."""
import ctypes as C

import pytest

import encmodel
from encmodel import RULE
from lz4util import I, orc_decompress
from test_gpu_encode import check_valid
from test_gpu_encode_model import (SIZES, accel_cases, all_cases, bench_cases, crafted_cases, model,
                                   prefix_cases, size_cases)


def decode_with_prefix(oracle, comp, n, prefix):
    d = C.create_string_buffer(prefix + b"\0", len(prefix) + 1)
    o = C.create_string_buffer(n + 64)
    r = oracle.orc_decompress_safe_usingDict(C.c_char_p(comp + bytes(16)), o, len(comp), n, d,
                                             len(prefix))
    return r, o.raw[:max(r, 0)]


def check(oracle, case):
    name, src, prefix, accel = case
    out = model(src, prefix, accel)
    n = len(src)
    assert len(out) <= oracle.orc_compressBound(n), name
    if prefix:
        assert decode_with_prefix(oracle, out, n, prefix) == (n, src), name
        if n:
            assert decode_with_prefix(oracle, out, n - 1, prefix)[0] < 0, name
    else:
        # decodes to the input; cap = n - 1 is an error, the reference's own where it is built
        check_valid(oracle, src, out)
        if n:
            assert orc_decompress(oracle, out, n - 1)[0] < 0, name


@pytest.mark.parametrize("cases", [size_cases, crafted_cases, accel_cases, prefix_cases, bench_cases],
                         ids=lambda f: f.__name__)
def test_model_blocks_decode_and_stay_within_the_bound(oracle, cases):
    for case in cases():
        check(oracle, case)


@pytest.mark.parametrize("content", I.ENC_CONTENTS)
def test_golden_encoder_inputs(oracle, content):
    for n in I.ENC_SIZES:
        if n <= 65536:
            check(oracle, ("%s %d" % (content, n), I.make(content, n), b"", 1))


def test_result_convention():
    src = I.synth_rand(4096, 0)
    assert encmodel.compress(src, 5000)[0] == 4114       # one literal run, as the reference
    src = I.synth_comp(4096, 2)
    r, out = encmodel.compress(src, 1 << 20)
    assert r == len(out) > 0 and encmodel.compress(src, r) == (r, out)
    assert encmodel.compress(src, r - 1) == (0, b"")
    assert encmodel.compress(src, -1) == (0, b"")
    assert encmodel.compress(b"", 1) == (1, b"\0") and encmodel.compress(b"", 0) == (0, b"")
    assert encmodel.compress(bytes(65537), 1 << 20) == (encmodel.ERANGE, b"")
    assert encmodel.compress(src, 1 << 20, acceleration=0) == (r, out)    # <= 1: none
    assert encmodel.compress(src, 1 << 20, acceleration=-5) == (r, out)
    assert encmodel.encode(src, acceleration=1 << 26) == encmodel.encode(src, acceleration=1 << 20)


def test_used_prefix():
    assert [encmodel.used_prefix(100, p) for p in (0, 63, 64, 65, 127, 128, 8192, 65536)] == \
        [0, 0, 64, 64, 64, 128, 8192, 65408]
    assert [encmodel.used_prefix(n, 65536) for n in (0, 1, 64, 65, 65472, 65473, 65536)] == \
        [65536, 65472, 65472, 65408, 64, 0, 0]


def _plain_cases():
    small = [c for c in size_cases() + accel_cases() if len(c[1]) <= 1100]
    pre = [c for c in prefix_cases() if len(c[1]) + len(c[2]) <= 9000 or c[0] in (
        "prefix 65536 n 457", "prefix 60000 + n 5536", "stream chunk 9")]
    return small + crafted_cases() + pre + bench_cases()[:1] + \
        [c for c in accel_cases() if len(c[1]) == 65536][::4]


def test_the_vectorised_form_is_the_plain_one():
    """candidates() and walk() (the table resolved for all positions at once, the walk from
    match to match) restate candidates_plain() and walk_plain(): the same sequences."""
    for name, src, prefix, accel in _plain_cases():
        assert encmodel.parse(src, prefix, accel) == encmodel.parse(src, prefix, accel, plain=True), name
    for rule in WRONG.values():   # and for the wrong rules the next test relies on
        for name, src, prefix, accel in crafted_cases() + [c for c in prefix_cases() if len(c[1]) == 100]:
            assert encmodel.parse(src, prefix, accel, rule=rule) == \
                encmodel.parse(src, prefix, accel, plain=True, rule=rule), (name, rule)


# Every constant of the rule, moved to its neighbour.
WRONG = {
    "backward extension capped at 3": RULE._replace(back=3),
    "a chunk sees its own earlier positions": RULE._replace(own_chunk=True),
    "the last table write one chunk lane early (p + 14 <= N)": RULE._replace(insert_room=14),
    "candidates accepted down to position 0": RULE._replace(min_cand=0),
    "forward length capped at 76": RULE._replace(fwd_cap=76),
    "forward length capped at 76 + 1024": RULE._replace(fwd_cap=76 + 1024),
    "prefix hashed at every position": RULE._replace(prefix_stride=1),
    "prefix used unrounded": RULE._replace(prefix_round=1),
    "probe gap growing after 63 probes": RULE._replace(regime=63),
    "catch-up with acceleration stopped at 4": RULE._replace(acc_more=0),
}
# A table write at p + 8 <= N instead of p + 5 <= N is no neighbour: it is the same function.  A
# position in [N - 7, N - 5] can only be the candidate of a later position, and a match starts at
# N - 12 at the latest; the writes of a chunk follow its lookups, so what such a write replaces
# is not looked up by an earlier position either.  Every bound from p + 5 to p + 13 gives the
# same bytes on every input (the first that differs is p + 14, above).
SAME = {"table writes only at p + 8 <= N": RULE._replace(insert_room=8),
        "table writes only at p + 13 <= N": RULE._replace(insert_room=13)}


def _applies(rule, case):
    if rule.prefix_stride != RULE.prefix_stride or rule.prefix_round != RULE.prefix_round:
        return bool(case[2])
    if rule.regime != RULE.regime or rule.acc_more != RULE.acc_more:
        return case[3] > 1
    return True


@pytest.mark.parametrize("name", list(WRONG))
def test_the_gpu_inputs_tell_the_rule_from_its_neighbour(name):
    """A kernel that followed the wrong rule would write different bytes for at least one input
    of the GPU tests (and so fail there)."""
    rule = WRONG[name]
    cases = sorted((c for c in all_cases() if _applies(rule, c)), key=lambda c: len(c[1]) + len(c[2]))
    hits = []
    for c in cases:
        if encmodel.encode(c[1], c[2], c[3], rule=rule) != model(c[1], c[2], c[3]):
            hits.append(c[0])
            break
    print(name, "->", hits)
    assert hits, name


@pytest.mark.parametrize("name", list(SAME))
def test_the_unobservable_bound_is_unobservable(name):
    rule = SAME[name]
    for c in size_cases() + crafted_cases() + [c for c in prefix_cases() if len(c[1]) <= 4096]:
        if len(c[1]) <= 4096:
            assert encmodel.encode(c[1], c[2], c[3], rule=rule) == model(c[1], c[2], c[3]), c[0]


def _roots(w):
    """Per chunk: the lanes stage 2 measures -- matches of 12 bytes and more (with room for
    more), one per run of consecutive lanes with the same offset."""
    cand = encmodel.candidates(w, 0)
    N = len(w)
    count = {}
    for p in range(1, N - 11):
        def trunc(q):
            return q <= N - 12 and encmodel.has_match(w, cand, q) and \
                encmodel.forward(w, cand[q], q) >= 12 and N - 5 - q > 12
        if trunc(p) and not (p % 64 != 63 and trunc(p + 1) and p + 1 - cand[p + 1] == p - cand[p]):
            count[p // 64] = count.get(p // 64, 0) + 1
    return count


def test_crafted_inputs_are_what_their_names_say():
    cs = {c[0]: c for c in crafted_cases()}
    for L in (75, 76, 77, 76 + 1023, 76 + 1024, 76 + 1025):
        c = cs["match of %d" % L]
        assert [s[1] for s in encmodel.parse(c[1])] == [L]
    c = cs["match ends at n - 5"]
    (lit, ml, off), = encmodel.parse(c[1])
    assert lit + ml == len(c[1]) - 5
    c = cs["match starts at n - 12"]
    (lit, ml, off), = encmodel.parse(c[1])
    assert lit == len(c[1]) - 12 and ml == 7
    assert encmodel.parse(cs["string starts at n - 11"][1]) == []
    assert encmodel.parse(cs["candidate at 3, 7 bytes"][1]) == []
    assert encmodel.parse(cs["candidate at 4, 7 bytes"][1]) == [(100, 7, 96)]
    assert encmodel.parse(cs["candidate at 3, 12 bytes"][1]) == [(100, 12, 97)]   # from 4, 1 back
    c = cs["back stopped by the previous match"]
    a, b = encmodel.parse(c[1])
    assert b[0] == 0 and b[2] == a[0] + a[1] - 1     # no literal between; 3 of the 4 equal bytes
    a, b = encmodel.parse(c[1], b"", 8)
    assert b[0] == 0 and b[2] == a[0] + a[1] - 1     # 10 of the 11
    assert encmodel.parse(cs["back stopped at position 0"][1], b"", 8) == [(300, 40, 300)]
    assert encmodel.parse(cs["the 65th probe"][1], b"", 2) == [(133, 7, 123)]
    c = cs["candidate at n - 13"]
    assert encmodel.parse(c[1]) == [(len(c[1]) - 12, 7, 1)]
    assert max(_roots(cs["more than 16 stage-2 roots"][1]).values()) > 3 * 16   # four passes
    (lit, _, _), = encmodel.parse(cs["literal run past the ring"][1])
    assert lit > 1024
    (lit, _, _), = encmodel.parse(cs["record past the staging buffer"][1])
    assert 512 < lit < 1024


def test_sizes_bracket_the_path_switches():
    """(the kernel's constants, restated: blocks below 128 bytes, the steps without edge code
    from 328 bytes on, two steps more per 128 bytes, the 1 KiB ring and its 64-byte mirror)"""
    for edge in (13, 64, 128, 192, 328, 392, 456, 1024, 1088, 65536):
        assert edge - 1 in SIZES and edge in SIZES and (edge + 1 in SIZES or edge == 65536)
