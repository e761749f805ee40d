"""The prepared-dictionary encoder's rule and compress_destSize's cut on the CPU:
encmodel.encode_cdict and encmodel.dest_size (the definitions of what
APE_LZ4_compress_usingCDict_batch_dev and APE_LZ4_compress_destSize_batch_dev write) against the
oracle -- every block decodes with the reference's decoder -- against their plain forms, and
against their wrong neighbours: every constant, changed, changes the output of at least one case
that tests/test_gpu_cdict_model.py or tests/test_gpu_destsize_model.py runs on the GPU."""
import pytest

import encmodel
import test_gpu_cdict_model as CD
import test_gpu_destsize_model as DS
from encmodel import RULE
from lz4util import orc_decompress
from test_enc_model import decode_with_prefix


# ---------------- the prepared dictionary ----------------
def test_window():
    assert [encmodel.cdict_window(d, 4096) for d in (0, 63, 64, 65, 100, 127, 128, 130, 61439, 61440, 70000)] == \
        [0, 0, 64, 64, 64, 64, 128, 128, 61376, 61440, 61440]
    assert [encmodel.cdict_window(70000, m) for m in (1, 64, 65, 61440, 65472, 65473, 65536)] == \
        [65472, 65472, 65408, 4096, 64, 0, 0]
    want = {0, 64, 128, 4096, 61440, 65472}
    assert {CD.window_of(("nat", s), m) for s, m in CD.OBJECTS} == want
    assert {CD.window_of(k, m) % 3 for k, m in CD.CRAFTED_OBJECTS[:3]} == {0, 1, 2}


def test_every_block_decodes_with_the_original_dictionary(oracle):
    for name, msg, key, max_src in CD.all_cases():
        out = CD.model(msg, key, max_src)
        n = len(msg)
        assert len(out) <= oracle.orc_compressBound(n), name
        assert decode_with_prefix(oracle, out, n, CD.dictionary(key)) == (n, msg), name


def test_without_a_window_it_is_the_plain_encoder():
    """D == 0: an empty dictionary, one below 64 bytes, one with no room beside maxSrcSize."""
    seen = set()
    for name, msg, key, max_src in CD.size_cases():
        if CD.window_of(key, max_src) == 0:
            seen.add((key[1], max_src))
            assert CD.model(msg, key, max_src) == encmodel.encode(msg), name
    assert seen == {(0, 4096), (63, 4096), (70000, 65536)}


def test_the_vectorised_form_is_the_plain_one():
    """Every case of the GPU lists (about 5 s)."""
    for name, msg, key, max_src in CD.all_cases():
        d = CD.dictionary(key)
        assert encmodel.parse_cdict(msg, d, max_src) == encmodel.parse_cdict(msg, d, max_src, plain=True), name
    for rule in CD_WRONG.values():   # and for the wrong rules the neighbour test relies on
        for name, msg, key, max_src in [c for c in CD.crafted_cases() if c[0].startswith("D 4096")][::7]:
            d = CD.dictionary(key)
            assert encmodel.parse_cdict(msg, d, max_src, rule=rule) == \
                encmodel.parse_cdict(msg, d, max_src, plain=True, rule=rule), (name, rule)


def test_the_recorded_ratios():
    """DESIGN.md 3.10 on test_gpu_cdict's inputs: ratio 2.97 at L = 1024 / Dd = 61440 and 2.53 at
    L = 256 / Dd = 32768; total against the staged withPrefix form x 1.0000 and x 1.0002."""
    from test_gpu_cdict import dict_of, messages
    for L, dd, ratio, staged in ((1024, 61440, "2.97", "1.0000"), (256, 32768, "2.53", "1.0002")):
        d, msgs = dict_of(dd), messages(L)
        total = sum(len(encmodel.encode_cdict(m, d, L)) for m in msgs)
        assert "%.2f" % (sum(map(len, msgs)) / total) == ratio
        assert "%.4f" % (total / sum(len(encmodel.encode(m, d)) for m in msgs)) == staged


# Every constant of the dictionary's rule, moved to its neighbour.
CD_WRONG = {
    "dictionary positions hashed while v + 8 <= N": RULE._replace(ext_hash_end="N"),
    "zone above D narrower by one": RULE._replace(ext_above=2),
    "zone above D wider by one": RULE._replace(ext_above=4),
    "no cut at D": RULE._replace(ext_cut=None),
    "cut at D - 1": RULE._replace(ext_cut=-1),
    "cut at D + 1": RULE._replace(ext_cut=1),
    "D from the message's length": RULE._replace(ext_window="len"),
    "candidates accepted down to window position 0": RULE._replace(min_cand=0),
}
# The zone's lower side is no neighbour: it is the same function.  The table holds a dictionary
# position v only when v + 8 <= D, and a message's own positions lie at D and above, so no
# candidate ever lies in [D - 7, D - 1]: every lower side from D - 7 to D - 1 gives the same bytes
# on every input (the kernel's D - 3 keeps a 4-byte verify inside the window whatever the table
# holds).  Only together with positions hashed up to N would it show.
CD_SAME = {"zone below D narrower by one": RULE._replace(ext_below=2),
           "zone below D wider by one": RULE._replace(ext_below=4),
           "zone below D at D - 7": RULE._replace(ext_below=7)}


@pytest.mark.parametrize("name", list(CD_WRONG))
def test_the_gpu_messages_tell_the_dictionary_rule_from_its_neighbour(name):
    rule = CD_WRONG[name]
    hits = []
    for c in sorted(CD.all_cases(), key=lambda c: len(c[1])):
        if encmodel.parse_cdict(c[1], CD.dictionary(c[2]), c[3], rule=rule) != \
                encmodel.parse_cdict(c[1], CD.dictionary(c[2]), c[3]):
            hits.append(c[0])
            break
    print(name, "->", hits)
    assert hits, name


@pytest.mark.parametrize("name", list(CD_SAME))
def test_the_zone_below_the_dictionary_end_is_unobservable(name):
    rule = CD_SAME[name]
    for c in CD.all_cases():
        assert encmodel.parse_cdict(c[1], CD.dictionary(c[2]), c[3], rule=rule) == \
            encmodel.parse_cdict(c[1], CD.dictionary(c[2]), c[3]), c[0]


def _dict_matches(case):
    """[(window position of the candidate, forward + backward length, message position)] of
    the sequences of a case that come out of the dictionary."""
    name, msg, key, max_src = case
    D = CD.window_of(key, max_src)
    out, pos = [], 0
    for lit, ml, off in encmodel.parse_cdict(msg, CD.dictionary(key), max_src):
        pos += lit
        if off > pos:
            out.append((D + pos - off, ml, pos))
        pos += ml
    return D, out


def test_crafted_messages_are_what_their_names_say():
    cs = {c[0]: c for c in CD.crafted_cases()}
    assert len(cs) == len(CD.crafted_cases())
    # matches of every measurement edge's length that end at D, in every placement
    for L, D in zip(CD.EDGES, (61440, 4096, 8192, 4096, 8192, 61440)):
        assert (D - L) % 3 == 0
        for fill in ("start", "zeros"):
            for where in ("first chunk", "inner chunk", "last chunks"):
                c = cs["D %d: %d to D + %s, %s" % (D, L, fill, where)]
                assert (D - L, L) in [m[:2] for m in _dict_matches(c)[1]], c[0]
    # the last hashed position: D - 9, D - 10, D - 8 for D % 3 = 0, 1, 2 -- a copy of fewer
    # bytes of the dictionary's end finds nothing there, a longer one a match that ends at D
    for D, j0 in ((61440, 9), (4096, 10), (8192, 8)):
        for j in range(1, 13):
            _, ms = _dict_matches(cs["D %d: last %d + start, inner chunk" % (D, j)])
            # (a byte more where the random byte before the copy happens to agree)
            assert [(c + ml, c <= D - j) for c, ml, _ in ms] == ([(D, True)] if j >= j0 else []), (D, j)
        # 64 and more: a chunk whose every lane lies in the copy; the candidates lie 3 apart,
        # so no two neighbouring lanes share an offset out of the dictionary
        _, ms = _dict_matches(cs["D %d: last 200 + start, inner chunk" % D])
        assert [m[:2] for m in ms] == [(D - 200, 200)]
        # backward extension into the dictionary: 0, 1, 2 bytes, and 2 cut to 1 by the pending
        # literals (the previous match takes the copy's first byte)
        for b in (0, 1, 2):
            _, ms = _dict_matches(cs["D %d: interior, %d back, first chunk" % (D, b)])
            assert [m[1] for m in ms] == [40 + b], (D, b)
        _, ms = _dict_matches(cs["D %d: interior, back stopped by the previous match, inner chunk" % D])
        assert [m[1] for m in ms] == [21, 41], D
    # (in the small window: in a large one later positions have taken the first ones' slots)
    _, ms = _dict_matches(cs["D 4096: window start, inner chunk"])
    assert [m[:2] for m in ms] == [(2, 28)]       # found from position 6, 4 back
    _, ms = _dict_matches(cs["D 4096: window position 3, inner chunk"])
    assert [m[:2] for m in ms] == [(3, 27)]       # found from position 6, 3 back
    # the message's own first positions: 0 and 3 are no candidates, 4 is one
    for D in (61440, 4096, 8192, 64, 128):
        for where in (100, 230):
            for at, found in ((0, False), (3, False), (4, True)):
                c = cs["D %d: own position %d, 7 bytes at %d" % (D, at, where)]
                seqs = encmodel.parse_cdict(c[1], CD.dictionary(c[2]), c[3])
                assert seqs == ([(where, 7, where - at)] if found else []), c[0]


def test_one_message_under_two_windows_differs():
    cases = CD.two_window_cases()
    by = {}
    for name, msg, key, max_src in cases:
        by.setdefault(msg, set()).add(CD.model(msg, key, max_src))
    assert sum(len(v) == 2 for v in by.values()) >= 10


# ---------------- compress_destSize ----------------
def _kernel_max_lastrun(room, rem):
    """lz4_destsize.hip's closed form, restated."""
    def ext(L):
        return (L - 15) // 255 + 1 if L >= 15 else 0
    b = room - 1
    L = b - (b + 240) // 255
    while L and L + ext(L) > b:
        L -= 1
    while L + 1 + ext(L + 1) <= b:
        L += 1
    return min(L, rem)


def test_the_fill_rule_is_the_kernels_closed_form():
    for room in list(range(1, 1400)) + [65535, 65536, 66000]:
        for rem in (0, 1, 14, 15, 269, 270, 271, 100000):
            want = encmodel.max_lastrun(room, rem, plain=True) if room < 1400 else None
            got = encmodel.max_lastrun(room, rem)
            assert got == _kernel_max_lastrun(room, rem), (room, rem)
            assert want is None or got == want, (room, rem)


def test_every_cut_fits_and_decodes(oracle):
    for name, src, target in DS.all_cases():
        r, k, out = DS.model(src, target)
        if target < 1:
            assert (r, k, out) == (0, len(src), b""), name
            continue
        assert r == len(out) and 1 <= r <= target and 0 <= k <= len(src), name
        assert orc_decompress(oracle, out, k) == (k, src[:k]), name
        if k:
            assert orc_decompress(oracle, out, k - 1)[0] < 0, name
        if len(DS.parsed(src)[1]) <= target:
            assert (k, out) == (len(src), DS.parsed(src)[1]), name


def test_the_plain_form_of_the_cut():
    """Every case of the GPU lists, the plain parse of each input taken once."""
    plain = {}
    for name, src, target in DS.all_cases():
        if src not in plain:
            plain[src] = encmodel.parse(src, plain=True)
            assert plain[src] == DS.parsed(src)[0], name
        assert encmodel.dest_size(src, target, plain=True, seqs=plain[src]) == DS.model(src, target), name


# Every constant of the cut, moved to its neighbour.
DS_WRONG = {
    "need 4": RULE._replace(ds_need=4),
    "need 6": RULE._replace(ds_need=6),
    "need 5 whatever the match's length": RULE._replace(ds_long=4),
    "11 - ml after a short match": RULE._replace(ds_sum=11),
    "13 - ml after a short match": RULE._replace(ds_sum=13),
    "a tie goes to the later cut": RULE._replace(ds_later=True),
    "one length byte from 14 literals on": RULE._replace(ds_ext1=14),
    "one length byte from 16 literals on": RULE._replace(ds_ext1=16),
    "two length bytes from 269 literals on": RULE._replace(ds_ext2=269),
    "two length bytes from 271 literals on": RULE._replace(ds_ext2=271),
}


@pytest.mark.parametrize("name", list(DS_WRONG))
def test_the_gpu_targets_tell_the_cut_from_its_neighbour(name):
    """(A tie is not unobservable: a match of 4 bytes after 15 or more literals costs the 4
    bytes it saves, so the cut after it consumes what the cut before it does.)"""
    rule = DS_WRONG[name]
    hits = []
    for c in DS.all_cases():
        if encmodel.dest_size(c[1], c[2], rule=rule, seqs=DS.parsed(c[1])[0]) != DS.model(c[1], c[2]):
            hits.append(c[0])
            break
    print(name, "->", hits)
    assert hits, name


def test_destsize_inputs_are_what_their_names_say():
    for ml in (4, 5, 6):
        src = dict(DS.small_inputs())["match of %d" % ml]
        assert [s[1] for s in DS.parsed(src)[0]] == [ml]
        assert DS.parsed(src)[0][0][0] >= 15
    lens = {s[0] for s in DS.parsed(dict(DS.small_inputs())["runs"])[0]}
    assert {524, 14, 15, 16, 269, 270, 271} <= lens
    big = dict(DS.large_inputs())
    sizes = sorted(len(DS.parsed(s)[1]) for s in big.values() if len(s) == 65536)
    assert len(sizes) >= 2 and sizes[0] > 4 * DS.WINDOW
    kinds = set()
    for src in big.values():
        kinds |= DS.refill_kinds(DS.parsed(src)[1])
    assert kinds == {"token", "literal length run", "match length run", "offset", "inside 16"}
    # the targets reach the refills: the walk goes on to a target's end
    for name, src, target in DS.large_cases():
        assert target <= len(DS.parsed(src)[1]) + 1
