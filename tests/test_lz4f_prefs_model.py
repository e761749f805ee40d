"""tests/lz4fprefsmodel.py, the definition of the frames of include/ape_lz4f_prefs.h, against what
it is built from and against liblz4's reading of its frames (tests/golden/lz4f_prefs_golden.json,
made by tests/golden/gen_lz4f_prefs_golden.py; no liblz4 here).  No GPU."""
import hashlib
import json
import os

import pytest

import lz4fmodel as F
import lz4fprefsmodel as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "lz4f_prefs_golden.json")


@pytest.fixture(scope="module")
def cases():
    """name -> (content, the model's frame, ID, mode, depth, flags), computed once."""
    out = {}
    for name, parts, bsid, mode, depth, flags in P.CASES:
        content = F.content_of(parts)
        out[name] = (content, P.compress(content, bsid, mode, depth, flags), bsid, mode, depth, flags)
    return out


edge = P.edge


def test_at_id_4_the_fast_mode_is_the_existing_frame():
    text = F.content_of([["text", 3000, 1, 200000]])
    rand = F.content_of([["text", 3000, 2, 65536], ["rand", 65536, 9, 65536], ["text", 500, 3, 500]])
    for data in (b"", text[:1], text[:12], text[:65536], text[:65537], text, rand, edge(1290)):
        for flags in range(8):
            assert P.compress(data, 4, 0, 0, flags) == F.compress(data, flags), (len(data), flags)


def test_every_frame_decodes_to_its_input_and_info_reports_the_blocks(cases):
    for name, (content, frame, bsid, mode, depth, flags) in cases.items():
        B = F.block_max(bsid)
        nb = (len(content) + B - 1) // B
        info = F.info(frame)
        assert info[5] == (len(content) if flags & 4 else nb * B), name    # the room decode() asks
        assert F.decode(frame, info[5], max(nb, 1)) == (len(content), content), name
        assert info[0] == 0 and info[2] == B and info[3] == nb and info[4] == len(frame), name
        assert frame[5] == bsid << 4, name
        assert (info[6], info[7]) == ((len(content), 0) if flags & 4 else (-1, -1)), name
        assert len(frame) <= P.compress_bound(len(content), bsid, flags), name


def test_the_fixture_says_liblz4_read_exactly_these_frames(cases):
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["slice"] == P.SLICE
    assert [c["name"] for c in doc["cases"]] == [c[0] for c in P.CASES] and len(P.CASES) >= 12
    for c in doc["cases"]:
        content, frame, bsid, mode, depth, flags = cases[c["name"]]
        assert [c["parts"], c["bsid"], c["mode"], c["depth"], c["flags"]] == \
            [[list(p) for p in next(k[1] for k in P.CASES if k[0] == c["name"])], bsid, mode, depth,
             flags]
        assert hashlib.sha256(frame).hexdigest() == c["frame_sha256"], c["name"]
        assert c["frame_bytes"] == len(frame) and c["content_bytes"] == len(content)
        assert c["liblz4"] == {"blockSizeID": bsid, "decompress_return": 0, "consumed": len(frame),
                               "decoded_sha256": hashlib.sha256(content).hexdigest()}, c["name"]


def test_the_bound_is_reached_by_incompressible_input_and_never_exceeded(cases):
    rand = F.content_of([["rand", 300000, 11, 300000]])
    for bsid, n in ((4, 300000), (5, 300000), (5, 262144), (6, 70000), (7, 1)):
        for mode, depth in ((0, 0), (1, 8), (2, 8)):
            for flags in (0, 7):
                frame = P.compress(rand[:n], bsid, mode, depth, flags)
                assert len(frame) == P.compress_bound(n, bsid, flags), (bsid, n, mode, flags)
                assert all(stored for _, stored in P.blocks_of(frame))
    for name, (content, frame, bsid, mode, depth, flags) in cases.items():
        assert len(frame) <= P.compress_bound(len(content), bsid, flags), name
    # a block that compresses at all is below the bound
    assert len(cases["id5_fast_text_tail"][1]) < P.compress_bound(2 * 262144 + 777, 5, 0)


def test_a_block_is_stored_when_its_bytes_take_the_whole_length():
    """The capacity is len - 1: the block that compresses to exactly len bytes is stored, the one
    that compresses to len - 1 is not -- in all three modes, so the inputs hold a block that is
    stored by that one byte."""
    for mode, depth in ((0, 0), (1, 8), (2, 8)):
        full, fits = edge(1290), edge(1289)
        assert len(P.block_bytes(full, mode, depth)) == len(full)
        assert len(P.block_bytes(fits, mode, depth)) == len(fits) - 1
        for bsid in (4, 5):
            (body, stored), = P.blocks_of(P.compress(full, bsid, mode, depth, 7))
            assert stored and body == full
            (body, stored), = P.blocks_of(P.compress(fits, bsid, mode, depth, 7))
            assert not stored and body == P.block_bytes(fits, mode, depth)


def test_the_model_tells_its_wrong_neighbours_apart(cases):
    """BD left at 0x40; blocks cut at 65536 under a larger ID; the capacity len instead of
    len - 1.  Each gives other bytes on inputs of the tests, and the first two frames that no
    longer decode to the input with this project's decoder model."""
    content, frame, bsid, mode, depth, flags = cases["id5_hc_text_tail"]
    left = P.compress(content, bsid, mode, depth, flags, rule=P.RULE._replace(bd_id=4))
    assert left != frame and left[5] == 0x40 and frame[5] == 0x50
    assert F.decode(left, 2 * 262144, 8)[0] < 0          # a block above the named maximum
    cut = P.compress(content, bsid, mode, depth, flags, rule=P.RULE._replace(cut=65536))
    assert cut != frame and F.info(cut)[3] == 5 and F.info(frame)[3] == 2
    assert F.decode(cut, 2 * 262144, 8)[0] < 0             # short blocks before the last
    # ... which the existing ID-4 frame is not: same cuts, BD 0x40
    content0, frame0 = cases["id4_fast_text"][:2]
    assert P.compress(content0, 5, 0, 0, 7, rule=P.RULE._replace(cut=65536, bd_id=4)) == frame0
    for mode, depth in ((0, 0), (1, 8), (2, 8)):
        data = edge(1290)
        right = P.compress(data, 5, mode, depth, 7)
        wrong = P.compress(data, 5, mode, depth, 7, rule=P.RULE._replace(slack=0))
        assert right != wrong and len(right) == len(wrong)
        assert P.blocks_of(wrong)[0][1] is False and P.blocks_of(right)[0][1] is True
        assert F.decode(wrong, 262144, 1) == (len(data), data)    # valid, but not the rule
