"""APE_LZ4_lz4f_decompress_placed_batch_dev (include/ape_lz4f_placed.h) against
tests/lz4fplacedmodel.py: liblz4's flushed frames (tests/golden/lz4f_flush_golden.json), its
full-block frames, frames the model writes and malformed ones, result for result and byte for
byte; what a frame that is refused before the decode leaves of its destination; the existing
call on the same batches.  No liblz4 here: the fixtures carry its frames."""
import struct

import pytest

import decseq
import inputs
import lz4fmodel as M
import lz4fplacedmodel as P
from gpuutil import CANARY, alloc_out, fetch, ints, pack

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
BLOCKS = 40


def _scratch(cuda, nbytes):
    assert 0 < nbytes < 1 << 31
    return cuda.full((nbytes,), 0x33, dtype=cuda.uint8, device="cuda")


def _decode(cuda, product, frames, caps, max_blocks=BLOCKS, flags=0, placed=True, shift=0):
    """(results, the decoded bytes per frame, whether each destination is untouched)."""
    n = len(frames)
    keep, sptr, _ = pack(cuda, frames, misalign=[(7 * k + 3) % 16 for k in range(n)])
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(5 * k + 1 + shift) % 16 for k in range(n)])
    res = ints(cuda, [POISON] * n)
    if placed:
        scratch = _scratch(cuda, product.lz4f_decompress_placed_scratch_size(n, max_blocks))
        call = product.lz4f_decompress_placed_batch
    else:
        scratch = _scratch(cuda, product.lz4f_decompress_scratch_size(n, max_blocks))
        call = product.lz4f_decompress_batch
    call(sptr, ints(cuda, map(len, frames)), dptr, ints(cuda, caps), res, max_blocks, flags, scratch)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    outs = [fetch(dst, o, max(r, 0)) for o, r in zip(offs, rs)]
    clean = [fetch(dst, o, c) == bytes([CANARY]) * c for o, c in zip(offs, caps)]
    return rs, outs, clean


@pytest.fixture(scope="module")
def written():
    """Frames of the model's writer, [(frame, content)]: short pieces, a stored one, an empty
    one, a full block between short ones; independent and linked, with and without checksums."""
    text = M.content_of([["text", 7000, 1, 66000]])
    rand = inputs.make("rand", 5000, 3)
    lists = [[text[:3000], rand, b"", text[3000:9000], text[:1], text[9000:20000]],
             [text[:100], text[100:100 + 65536], text[:1]],
             [text[k:k + 13] for k in range(0, 13 * 40, 13)]]
    out = []
    for pieces in lists:
        for linked in (False, True):
            for full in (False, True):
                frame = P.frame_of(pieces, linked=linked, block_sums=full, content_sum=full,
                                   content_size=full)
                out.append((frame, b"".join(pieces)))
    return out


def test_every_flushed_frame_decodes_to_its_content(product, cuda, written):
    """Exact capacities, and every destination alignment over the four passes."""
    fx = list(P.fixtures().values())
    frames = [f["frame"] for f in fx] + [w[0] for w in written]
    contents = [f["content"] for f in fx] + [w[1] for w in written]
    caps = [len(c) for c in contents]
    assert max(P.blocks_of(f) for f in frames) == BLOCKS
    for shift in (0, 4, 8, 12):
        rs, outs, _ = _decode(cuda, product, frames, caps, shift=shift)
        assert rs == caps
        assert outs == contents


def _too_far(linked):
    """A frame whose only block has a match that starts 12 bytes before the block."""
    body, _ = decseq.build([(b"abcdefgh", 20, 8)], b"x" * 16, strict=False)
    flg = 0x40 | (0 if linked else M.F_INDEP)
    return M.frame_header(flg, 4) + struct.pack("<I", len(body)) + body + struct.pack("<I", 0)


def _cases():
    """[(name, frame, capacity, max_blocks)]: lz4fmodel's corruptions at their own capacities,
    and the placed call's own early refusals."""
    out = [(c.name, c.frame, c.cap, c.max_blocks) for c in M.corruptions()]
    fx = P.fixtures()
    short = fx["forty_short_linked_id4_all"]
    out.append(("flushed, capacity one short", short["frame"], len(short["content"]) - 1, 40))
    out.append(("flushed, negative capacity", fx["short_full_one_indep_id4_none"]["frame"], -1, 8))
    longer = bytearray(fx["short_full_one_indep_id5_all"]["frame"])
    longer[6:14] = struct.pack("<Q", 65637 + 1)
    out.append(("flushed, changed content size", M._redo_header_sum(longer, 10), 1 << 17, 8))
    out.append(("independent block reaching before itself", _too_far(False), 1 << 16, 8))
    out.append(("linked block reaching before the frame", _too_far(True), 1 << 16, 8))
    ok = M.fixtures()["indep_all"]["frame"]
    _, head = M.header(ok)
    second = M.walk(ok, head)[1][1]
    cut = bytearray(ok)
    cut[second.at + second.size - 1] ^= 0x40                        # the block's last literal
    out.append(("flipped literal, block checksums", bytes(cut), 4 * M.BLOCK, 8))
    out.append(("flushed, one block more than max_blocks", short["frame"], 120000, 39))
    return out


def _mixed(cases):
    """Every case between two good frames, flushed and full-block: (frames, caps)."""
    flush, full = P.fixtures(), M.fixtures()
    good = [flush["forty_short_linked_id4_all"], full["linked_all"],
            flush["short_full_one_indep_id5_all"], full["random_block_all"],
            flush["short_full_one_linked_id4_none"], full["indep_bsum"]]
    frames, caps = [], []
    for k, c in enumerate(cases):
        g = good[k % len(good)]
        frames += [g["frame"], c[1]]
        caps += [len(g["content"]), c[2]]
    frames.append(good[0]["frame"])
    caps.append(len(good[0]["content"]))
    return frames, caps


def test_one_batch_mixes_good_frames_and_every_corruption(product, cuda):
    cases = _cases()
    codes = {}
    for max_blocks in sorted({c[3] for c in cases}):
        batch = [c for c in cases if c[3] == max_blocks]
        frames, caps = _mixed(batch)
        want = [P.decode_placed(f, c, max_blocks) for f, c in zip(frames, caps)]
        # the neighbours are good frames (or have more blocks than this batch's maximum)
        assert all(w[0] in (c, M.ERANGE) for w, c in zip(want[0::2], caps[0::2]))
        rs, outs, clean = _decode(cuda, product, frames, caps, max_blocks=max_blocks)
        assert rs == [w[0] for w in want]
        assert all(o == w[1] for o, w in zip(outs, want) if w[0] >= 0)
        codes.update({c[0]: w[0] for c, w in zip(batch, want[1::2])})
        # refused before the decode: -4 from sizing, -8, -9 (and the header stage) write nothing
        for c, w, ok in zip(batch, want[1::2], clean[1::2]):
            early = w[0] in (-1, -2, -3, -8, -9, M.ERANGE) or c[0] in (
                "independent block reaching before itself",)
            assert ok or not early, c[0]
    assert codes == {"flipped data byte, block checksums": -6, "flipped content checksum": -7,
                     "wrong header checksum": -1, "reserved bit, checksum redone": -1,
                     "dictionary ID": -3, "skippable magic": -3, "cut inside a block": -2,
                     "cut inside the trailer": -2, "changed content size": -8,
                     "two 100-byte blocks": 200,
                     "declared size 1, a full block, then 00": -9,
                     "declared size 200, a 100-byte block, then 00": -8,
                     "declared size 0, 1025 blocks 00 at 4 MiB": 0,
                     "one block more than max_blocks": M.ERANGE,
                     "capacity one short": 196708,
                     "flushed, capacity one short": -9, "flushed, negative capacity": -9,
                     "flushed, changed content size": -8,
                     "independent block reaching before itself": -4,
                     "linked block reaching before the frame": -4,
                     "flipped literal, block checksums": -6,
                     "flushed, one block more than max_blocks": M.ERANGE}


def test_the_existing_call_on_the_same_batch(product, cuda):
    """Given at least blocks x maximum, the two calls agree on every corruption but the -5 ones
    and on every full-block fixture; the existing call gives -5 where its model says so -- the
    flushed fixtures among them -- and the placed call the content."""
    cases = [c for c in M.corruptions() if c.max_blocks == M.DEFAULT_BLOCKS]
    flush = [f for f in P.fixtures().values() if P.blocks_of(f["frame"]) <= M.DEFAULT_BLOCKS]
    frames = [c.frame for c in cases] + [f["frame"] for f in flush] + \
        [f["frame"] for f in M.fixtures().values()]

    def bound(frame):
        inf = M.info(frame)
        return max(inf[5], inf[3] * inf[2], 1)

    caps = [c.cap if c.header_stage else max(c.cap, bound(c.frame)) for c in cases] + \
        [bound(f) for f in frames[len(cases):]]
    old = [M.decode(f, c, M.DEFAULT_BLOCKS) for f, c in zip(frames, caps)]
    new = [P.decode_placed(f, c, M.DEFAULT_BLOCKS) for f, c in zip(frames, caps)]
    rs_old, outs_old, _ = _decode(cuda, product, frames, caps, M.DEFAULT_BLOCKS, placed=False)
    rs_new, outs_new, _ = _decode(cuda, product, frames, caps, M.DEFAULT_BLOCKS)
    assert rs_old == [w[0] for w in old] and rs_new == [w[0] for w in new]
    assert all(o == w[1] for o, w in zip(outs_new, new) if w[0] >= 0)
    refused = [k for k, w in enumerate(old) if w[0] == -5]
    assert len(refused) == 2 + sum(P.has_short_middle_block(f["frame"]) for f in flush) == 10
    for k, (o, w) in enumerate(zip(old, new)):
        if k in refused:
            assert w[0] >= 0 or w[0] == -8, k
        else:
            assert (rs_new[k], outs_new[k]) == (rs_old[k], outs_old[k]) and o == w, k
    for k, f in enumerate(flush):
        assert outs_new[len(cases) + k] == f["content"]


def test_flag_2_refuses_linked_frames_and_flag_1_skips_the_checksums(product, cuda):
    fx = list(P.fixtures().values()) + list(M.fixtures().values())
    frames = [f["frame"] for f in fx]
    caps = [max(len(f["content"]), 1) for f in fx]
    rs, outs, clean = _decode(cuda, product, frames, caps, flags=M.NO_LINKED)
    assert rs == [-3 if f["linked"] else len(f["content"]) for f in fx]
    assert all(o == f["content"] for o, f in zip(outs, fx) if not f["linked"])
    assert all(ok for ok, f in zip(clean, fx) if f["linked"])
    cases = [c for c in _cases() if c[3] == 8]
    frames, caps = _mixed(cases)
    want = [P.decode_placed(f, c, BLOCKS, M.NO_VERIFY) for f, c in zip(frames, caps)]
    strict = [P.decode_placed(f, c, BLOCKS) for f, c in zip(frames, caps)]
    lenient = [k for k, (w, s) in enumerate(zip(want, strict)) if w != s]
    assert len(lenient) == 3 and all(strict[k][0] in (-6, -7) and want[k][0] > 0 for k in lenient)
    rs, outs, _ = _decode(cuda, product, frames, caps, flags=M.NO_VERIFY)
    assert rs == [w[0] for w in want]
    assert all(o == w[1] for o, w in zip(outs, want) if w[0] >= 0)


def test_capture_into_a_graph_and_replay(product, cuda):
    fx = [f for f in P.fixtures().values() if f["name"].startswith(("forty", "short_full"))]
    frames, contents = [f["frame"] for f in fx], [f["content"] for f in fx]
    n = len(frames)
    caps = [len(c) for c in contents]
    keep, sptr, _ = pack(cuda, frames, misalign=[(k + 1) % 16 for k in range(n)])
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(3 * k + 2) % 16 for k in range(n)])
    sizes, capt = ints(cuda, map(len, frames)), ints(cuda, caps)
    res = ints(cuda, [POISON] * n)
    scr = _scratch(cuda, product.lz4f_decompress_placed_scratch_size(n, BLOCKS))
    st = cuda.cuda.Stream()
    st.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=st):
        product.lz4f_decompress_placed_batch(sptr, sizes, dptr, capt, res, BLOCKS, 0, scr, stream=st)
    res.fill_(POISON)
    scr.fill_(0x55)
    dst.fill_(CANARY)
    g.replay()
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == caps
    assert [fetch(dst, o, c) for o, c in zip(offs, caps)] == contents


def test_an_empty_batch_launches_nothing(product, cuda):
    L = product.lib()
    assert L.APE_LZ4_lz4f_decompress_placed_batch_dev(None, None, None, None, None, 0, 4, 0, None,
                                                      0, None) == 0


# ---- more than 64 blocks (tests/lz4fmany.py): the kernels step over a frame's blocks 64 at a
# time; tests/test_lz4f_placed_model.py has the CPU half ----
def test_frames_of_64_65_and_130_short_blocks(product, cuda):
    """Beside a one-block frame, whose other 129 slots are absent: the content at the exact
    capacity, -9 and an untouched destination one byte short, -5 from the existing call."""
    import lz4fmany as X
    made = X.short_frames() + [X.one_block()]
    frames, contents = [m[0] for m in made], [m[1] for m in made]
    caps = [len(c) for c in contents]
    assert caps[5] == 1690
    rs, outs, _ = _decode(cuda, product, frames, caps, max_blocks=X.SHORT_BLOCKS)
    assert rs == caps
    assert outs == contents
    want = [P.decode_placed(f, c - 1, X.SHORT_BLOCKS) for f, c in zip(frames, caps)]
    assert want == [(-9, None)] * len(frames)
    rs, _, clean = _decode(cuda, product, frames, [c - 1 for c in caps], max_blocks=X.SHORT_BLOCKS)
    assert rs == [-9] * len(frames) and all(clean)
    roomy = [X.bound(f) for f in frames]
    old = [M.decode(f, c, X.SHORT_BLOCKS)[0] for f, c in zip(frames, roomy)]
    assert old == [-5] * 6 + [13]
    rs, outs, _ = _decode(cuda, product, frames, roomy, max_blocks=X.SHORT_BLOCKS, placed=False)
    assert rs == old and outs[6] == contents[6]


def test_a_bad_block_beyond_the_first_chunk_of_64(product, cuda):
    """Block 70 without a size: -4 and nothing written.  A flipped literal in block 100: -6."""
    import lz4fmany as X
    good, content = X.short_frames()[2]
    frames = [X.unsized_block_70(), good, X.flipped_block_100(), X.one_block()[0]]
    caps = [1 << 16, len(content), 1690, 13]
    want = [P.decode_placed(f, c, X.SHORT_BLOCKS) for f, c in zip(frames, caps)]
    assert [w[0] for w in want] == [-4, len(content), -6, 13]
    rs, outs, clean = _decode(cuda, product, frames, caps, max_blocks=X.SHORT_BLOCKS)
    assert rs == [w[0] for w in want]
    assert clean[0] and outs[1] == content and outs[3] == want[3][1]


def test_both_calls_on_66_and_67_blocks_with_65_full_ones(product, cuda):
    """65 full blocks and a short last one: both calls give the content.  With a 100-byte block
    at index 64 besides, the existing call gives -5 and the placed call the content."""
    import lz4fmany as X
    made, want = X.big_frames(), X.big_results()
    frames = [m[0] for m in made]
    caps = [X.bound(f) for f in frames]
    assert [w[1][0] for w in want] == [4259940, 4259940, 4260040, 4260040]
    assert [w[0][0] for w in want] == [4259940, 4259940, -5, -5]
    rs_new, outs_new, _ = _decode(cuda, product, frames, caps, max_blocks=X.BIG_BLOCKS)
    rs_old, outs_old, _ = _decode(cuda, product, frames, caps, max_blocks=X.BIG_BLOCKS, placed=False)
    assert rs_new == [w[1][0] for w in want] and rs_old == [w[0][0] for w in want]
    assert outs_new == [m[1] for m in made]
    assert outs_old[:2] == [m[1] for m in made[:2]]
