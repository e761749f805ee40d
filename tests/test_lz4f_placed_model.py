"""tests/lz4fplacedmodel.py, the definition of the placed framed decode, against what it must
mean: the content of every frame liblz4 wrote (flushed or not), lz4fmodel.decode wherever the
existing call takes the frame, and three wrong neighbours told apart.  No GPU, no product code."""
import pytest

import lz4fmodel as M
import lz4fplacedmodel as P
import lz4util


def _all_fixtures():
    out = [("flush/" + k, v) for k, v in P.fixtures().items()]
    return out + [("full/" + k, v) for k, v in M.fixtures().items()]


def _bound(frame):
    """blocks x maximum: the capacity at which the existing call's -9 (against its decoded
    bound) and the placed call's (against the measured total) cannot differ."""
    inf = M.info(frame)
    return max(inf[5], inf[3] * inf[2])


def test_the_fixture_file_has_every_piece_list_and_mode():
    fx = P.fixtures()
    assert len(fx) == 40
    lists = {tuple(v["pieces"]) for v in fx.values()}
    assert lists == {(1,), (100, 65536, 1), (65537,), (3000,) * 40, (0, 500, 0)}
    for pieces in lists:
        modes = {(v["linked"], v["bsid"], v["block_sums"], v["content_sum"], v["content_size"])
                 for v in fx.values() if tuple(v["pieces"]) == pieces}
        assert modes == {(linked, bsid, full, full, full) for linked in (False, True)
                         for bsid in (4, 5) for full in (False, True)}
    for v in fx.values():
        inf = M.info(v["frame"])
        assert inf[0] == 0 and bool(inf[1] & M.F_INDEP) != v["linked"] and \
            inf[2] == M.block_max(v["bsid"])
        # one block per non-empty piece, a piece above the maximum split
        assert inf[3] == sum(-(-n // inf[2]) for n in v["pieces"]), v["name"]


def test_every_fixture_decodes_to_its_content():
    for name, fx in _all_fixtures():
        n = len(fx["content"])
        for cap in (n, n + 1, _bound(fx["frame"])):
            for flags in (0, M.NO_VERIFY):
                assert P.decode_placed(fx["frame"], cap, flags=flags) == (n, fx["content"]), name
        if n:
            assert P.decode_placed(fx["frame"], n - 1) == (-9, None), name


def test_the_existing_call_refuses_the_flushed_frames():
    """-5 from lz4fmodel.decode on every flush fixture with a short block before the last, at a
    capacity that rules -9 out; the fixtures without one decode there too."""
    seen = 0
    for name, fx in P.fixtures().items():
        got = M.decode(fx["frame"], _bound(fx["frame"]))
        if P.has_short_middle_block(fx["frame"]):
            assert got == (-5, None), name
            seen += 1
        else:
            assert got == (len(fx["content"]), fx["content"]), name
    assert seen == 16   # [100, 65536, 1] and [3000] x 40, in their eight modes each


def test_it_agrees_with_the_existing_call_on_its_corruptions():
    """Every case of lz4fmodel.corruptions() but the -5 ones, which now decode (or, where the
    frame declares another content size, are -8).  The capacity is the case's, raised to blocks
    x maximum where the header stage passes: "at least the decoded bound", and the one at which
    the two calls' -9 rules -- against the bound, against the measured total -- coincide.  At
    the cases' own capacities the two differ exactly where that rule differs (below)."""
    own = {}
    for c in M.corruptions():
        cap = c.cap if c.header_stage else max(c.cap, _bound(c.frame))
        old = M.decode(c.frame, cap, c.max_blocks)
        new = P.decode_placed(c.frame, cap, c.max_blocks)
        if c.code == -5:
            assert old == (-5, None), c.name
            assert new[0] >= 0 or new[0] == -8, (c.name, new[0])
        else:
            assert new == old, (c.name, new[0], old[0])
            if cap == c.cap:
                assert new[0] == c.code, c.name
        if c.lenient is not None:
            assert P.decode_placed(c.frame, cap, c.max_blocks, M.NO_VERIFY) == \
                (len(c.lenient), c.lenient) == M.decode(c.frame, cap, c.max_blocks, M.NO_VERIFY)
        own[c.name] = P.decode_placed(c.frame, c.cap, c.max_blocks)[0]
    differ = {name for c in M.corruptions()
              for name in [c.name] if c.code != -5 and own[name] != c.code}
    # the measured total decides -9: a frame that declares 1 byte and holds a full block no
    # longer starts to decode into 1 byte; a frame whose content fits decodes
    assert differ == {"declared size 1, a full block, then 00", "capacity one short"}
    assert own["declared size 1, a full block, then 00"] == -9
    plain = M.fixtures()["indep_none"]
    assert own["capacity one short"] == len(plain["content"])
    assert own["two 100-byte blocks"] == 200
    assert own["declared size 200, a 100-byte block, then 00"] == -8
    assert own["declared size 0, 1025 blocks 00 at 4 MiB"] == 0


def _reach_past_previous_block(frame):
    """Whether a compressed block of a linked frame has a match that starts before the start of
    the block before it: read from the sequences, not from a decode."""
    code, head, blocks, _, _ = M._stage(frame)
    assert code == 0
    if head.flg & M.F_INDEP:
        return False
    measured = P.sizes(frame, head, blocks)
    for q, b in enumerate(blocks):
        if b.stored or q == 0:
            continue
        at = 0
        for lit, off, ml in lz4util.walk_ok(frame[b.at:b.at + b.size]):
            at += lit
            if ml and off - at > measured[q - 1]:
                return True
            at += ml
    return False


def test_wrong_neighbours_are_told_apart():
    """Every flush fixture with two blocks or more, under each wrong neighbour: another result
    wherever the frame's structure makes the neighbour differ -- a short block before the last
    (positions from q x maximum), a match reaching past the block before (a shortened history),
    a content below blocks x maximum (-9 against that) -- and the same result elsewhere."""
    told = {"grid": 0, "history": 0, "bound": 0}
    for name, fx in P.fixtures().items():
        frame, n = fx["frame"], len(fx["content"])
        if P.blocks_of(frame) < 2:
            continue
        right = P.decode_placed(frame, n)
        assert right == (n, fx["content"]), name
        roomy = _bound(frame)
        expect = {"grid": P.has_short_middle_block(frame),
                  "history": _reach_past_previous_block(frame),
                  "bound": n < roomy}
        for wrong, differs in expect.items():
            cap = n if wrong == "bound" else roomy
            got = P.decode_placed(frame, cap, wrong=wrong)
            assert (got != right) == differs, (name, wrong, got[0])
            told[wrong] += differs
    assert told == {"grid": 16, "history": 4, "bound": 20}, told


def test_the_frame_writer_writes_flushed_frames():
    import inputs
    text = M.content_of([["text", 3000, 1, 20000]])
    rand = inputs.make("rand", 5000, 3)
    for linked in (False, True):
        pieces = [text[:3000], rand, b"", text[3000:9000], text[:1], text[9000:20000]]
        frame = P.frame_of(pieces, linked=linked, block_sums=True, content_sum=True,
                           content_size=True)
        content = b"".join(pieces)
        code, head, blocks, _, _ = M._stage(frame)
        assert code == 0 and [b.stored for b in blocks] == [False, True, False, True, False]
        assert P.sizes(frame, head, blocks) == [len(p) for p in pieces if p]
        assert P.decode_placed(frame, len(content)) == (len(content), content)
        assert M.decode(frame, _bound(frame)) == (-5, None)
        assert _reach_past_previous_block(frame) == linked
    # a linked block is smaller than its independent twin: its matches reach back
    twice = [text[:3000], text[:3000]]
    assert len(P.frame_of(twice, linked=True)) < len(P.frame_of(twice)) - 1000


@pytest.mark.parametrize("linked", [False, True])
def test_a_block_without_a_size_and_a_block_that_reaches_too_far(linked):
    """An offset past the block's start: no size in an independent frame (-4, nothing written);
    in a linked frame it has a size, and the decode finds that it reaches before the frame."""
    import struct
    import decseq
    body, _ = decseq.build([(b"abcdefgh", 20, 8)], b"x" * 16, strict=False)
    flg = 0x40 | (0 if linked else M.F_INDEP)
    frame = M.frame_header(flg, 4) + struct.pack("<I", len(body)) + body + struct.pack("<I", 0)
    code, head, blocks, _, _ = M._stage(frame)
    assert P.sizes(frame, head, blocks) == ([32] if linked else [None])
    assert P.decode_placed(frame, 1 << 16) == (-4, None)


# ---- frames of more than 64 blocks (tests/lz4fmany.py): the CPU half of the GPU tests ----
def test_the_many_block_frames_are_what_the_gpu_tests_take_them_to_be():
    import lz4fmany as X
    frames = X.short_frames()
    assert [P.blocks_of(f) for f, _ in frames] == [64, 64, 65, 65, 130, 130]
    assert [bool(M.info(f)[1] & M.F_INDEP) for f, _ in frames] == [True, False] * 3
    for frame, content in frames:
        n = len(content)
        assert n == 13 * P.blocks_of(frame) and M.info(frame)[1] & (M.F_BSUM | M.F_CSUM | M.F_SIZE) \
            == M.F_BSUM | M.F_CSUM | M.F_SIZE
        assert P.decode_placed(frame, n, X.SHORT_BLOCKS) == (n, content)
        assert P.decode_placed(frame, n - 1, X.SHORT_BLOCKS) == (-9, None)
        assert M.decode(frame, X.bound(frame), X.SHORT_BLOCKS) == (-5, None)
    assert len(frames[5][1]) == 1690
    one, content = X.one_block()
    assert P.blocks_of(one) == 1 and P.decode_placed(one, 13, X.SHORT_BLOCKS) == (13, content)


def test_a_bad_block_beyond_the_first_chunk_of_64():
    import lz4fmany as X
    frame = X.unsized_block_70()
    code, head, blocks, _, _ = M._stage(frame)
    assert code == 0 and len(blocks) == 130 and head.flg & M.F_INDEP
    measured = P.sizes(frame, head, blocks)
    assert [q for q, n in enumerate(measured) if n is None] == [70]
    assert P.decode_placed(frame, 1 << 16, X.SHORT_BLOCKS) == (-4, None)
    frame = X.flipped_block_100()
    code, head, blocks, _, _ = M._stage(frame)
    assert code == 0 and len(blocks) == 130 and not head.flg & M.F_INDEP
    assert [q for q, b in enumerate(blocks) if M.xxh32(frame[b.at:b.at + b.size]) != b.want] == [100]
    assert P.decode_placed(frame, 1690, X.SHORT_BLOCKS) == (-6, None)
    assert P.decode_placed(frame, 1690, X.SHORT_BLOCKS, M.NO_VERIFY)[0] == 1690


def test_full_blocks_beyond_the_first_chunk_of_64():
    import lz4fmany as X
    frames = X.big_frames()
    assert [(P.blocks_of(f), gap) for f, _, gap in frames] == [(66, False)] * 2 + [(67, True)] * 2
    assert [bool(M.info(f)[1] & M.F_INDEP) for f, _, _ in frames] == [True, False] * 2
    for (frame, content, gap), (old, new) in zip(frames, X.big_results()):
        assert len(content) == (4260040 if gap else 4259940)
        assert new == (len(content), content)
        assert old == ((-5, None) if gap else (len(content), content))
