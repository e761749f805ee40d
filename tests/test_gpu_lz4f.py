"""The LZ4 frame calls on the GPU (include/ape_lz4f.h) against tests/lz4fmodel.py: the frames
APE_LZ4_lz4f_compress_batch_dev writes, byte for byte; what APE_LZ4_lz4f_decompress_batch_dev
makes of them, of liblz4's frames (tests/golden/lz4f_golden.json) and of malformed ones, code
for code; APE_LZ4_lz4f_info_batch_dev.  No liblz4 here: the fixtures carry its frames."""
import struct

import pytest

import lz4fmodel as M
from gpuutil import CANARY, alloc_out, fetch, ints, pack

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
SIZES = [0, 1, 12, 13, 65535, 65536, 65537, 3 * 65536 + 100]
MAX_SRC = max(SIZES)


@pytest.fixture(scope="module")
def contents():
    """One input per size: text that repeats every 3000 bytes (a prefix of the fixtures')."""
    whole = M.content_of([["text", 3000, 1, MAX_SRC]])
    return [whole[:n] for n in SIZES]


def _scratch(cuda, nbytes):
    assert 0 < nbytes < 1 << 31
    return cuda.full((nbytes,), 0x33, dtype=cuda.uint8, device="cuda")


def _compress(cuda, product, inputs, flags, caps=None, max_src=MAX_SRC, sizes=None, stream=None):
    """(results, the bytes written per frame, whether each destination is untouched)."""
    n = len(inputs)
    caps = [len(M.compress(b, flags)) for b in inputs] if caps is None else caps
    keep, sptr, _ = pack(cuda, inputs, misalign=[(5 * k + 1) % 16 for k in range(n)])
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(3 * k + 2) % 16 for k in range(n)])
    res = ints(cuda, [POISON] * n)
    scratch = _scratch(cuda, product.lz4f_compress_scratch_size(n, max_src))
    product.lz4f_compress_batch(sptr, ints(cuda, sizes or map(len, inputs)), dptr,
                                ints(cuda, caps), res, max_src, flags, scratch, stream=stream)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    outs = [fetch(dst, o, max(r, 0)) for o, r in zip(offs, rs)]
    clean = [fetch(dst, o, c) == bytes([CANARY]) * c for o, c in zip(offs, caps)]
    return rs, outs, clean


def _decompress(cuda, product, frames, caps, max_blocks=M.DEFAULT_BLOCKS, flags=0, stream=None):
    """(results, the decoded bytes per frame)."""
    n = len(frames)
    keep, sptr, _ = pack(cuda, frames, misalign=[(7 * k + 3) % 16 for k in range(n)])
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(5 * k + 1) % 16 for k in range(n)])
    res = ints(cuda, [POISON] * n)
    scratch = _scratch(cuda, product.lz4f_decompress_scratch_size(n, max_blocks))
    product.lz4f_decompress_batch(sptr, ints(cuda, map(len, frames)), dptr, ints(cuda, caps), res,
                                  max_blocks, flags, scratch, stream=stream)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    return rs, [fetch(dst, o, max(r, 0)) for o, r in zip(offs, rs)]


def _bound(frame):
    return M.info(frame)[5]


# ---- compress ----
@pytest.mark.parametrize("flags", range(8))
def test_frames_equal_the_model_at_exact_capacity_and_decode_again(product, cuda, contents, flags):
    want = [M.compress(b, flags) for b in contents]
    rs, outs, _ = _compress(cuda, product, contents, flags)
    assert rs == [len(w) for w in want]
    assert outs == want
    assert all(len(w) <= product.lz4f_compress_bound(len(b), flags) for w, b in zip(want, contents))
    ds, back = _decompress(cuda, product, outs, [max(_bound(w), 1) for w in want], flags=2)
    assert ds == [len(b) for b in contents]
    assert back == contents


def test_a_random_block_goes_in_stored(product, cuda):
    data = M.content_of([["rand", 65536, 9, 65536], ["text", 1000, 2, 1000]])
    want = M.compress(data, 7)
    assert struct.unpack_from("<I", want, 15)[0] == 65536 | 0x80000000
    rs, outs, _ = _compress(cuda, product, [data, data[:65536]], 7,
                            caps=[len(want), product.lz4f_compress_bound(65536, 7)])
    assert outs == [want, M.compress(data[:65536], 7)]
    assert rs[1] == product.lz4f_compress_bound(65536, 7)       # all stored: the bound is exact
    ds, back = _decompress(cuda, product, outs, [len(data), 65536])
    assert (ds, back) == ([len(data), 65536], [data, data[:65536]])


@pytest.mark.parametrize("flags", (0, 7))
def test_one_byte_short_gives_0_and_an_untouched_destination(product, cuda, contents, flags):
    caps = [len(M.compress(b, flags)) - 1 for b in contents]
    rs, _, clean = _compress(cuda, product, contents, flags, caps=caps)
    assert rs == [0] * len(contents)
    assert all(clean)


def test_erange_above_max_src_and_0_for_a_negative_size(product, cuda, contents):
    small, big = contents[3], contents[6]
    caps = [product.lz4f_compress_bound(len(big), 5)] * 4
    rs, outs, clean = _compress(cuda, product, [small, big, small, big[:65536]], 5, caps=caps,
                                max_src=65536, sizes=[len(small), len(big), -1, 65536])
    assert rs == [len(M.compress(small, 5)), M.ERANGE, 0, len(M.compress(big[:65536], 5))]
    assert outs[0] == M.compress(small, 5) and outs[3] == M.compress(big[:65536], 5)
    assert clean[1] and clean[2]


def test_two_streams(product, cuda, contents):
    streams = (cuda.cuda.Stream(), cuda.cuda.Stream())
    halves = (contents[0::2], contents[1::2])
    n = [len(h) for h in halves]
    packed = [pack(cuda, h) for h in halves]
    caps = [[product.lz4f_compress_bound(len(b), 3) for b in h] for h in halves]
    outs = [alloc_out(cuda, c) for c in caps]
    res = [ints(cuda, [POISON] * k) for k in n]
    scr = [_scratch(cuda, product.lz4f_compress_scratch_size(k, MAX_SRC)) for k in n]
    sizes = [ints(cuda, map(len, h)) for h in halves]
    capt = [ints(cuda, c) for c in caps]
    for k, st in enumerate(streams):
        st.wait_stream(cuda.cuda.current_stream())
        product.lz4f_compress_batch(packed[k][1], sizes[k], outs[k][1], capt[k], res[k], MAX_SRC,
                                    3, scr[k], stream=st)
    cuda.cuda.synchronize()
    for k in range(2):
        rs = res[k].cpu().tolist()
        got = [fetch(outs[k][0], o, max(r, 0)) for o, r in zip(outs[k][2], rs)]
        assert got == [M.compress(b, 3) for b in halves[k]]


def test_compress_and_decompress_capture_into_a_graph(product, cuda, contents):
    """One stream, no parallel branches: compress, then decode what it wrote."""
    inputs = contents[3:]
    n = len(inputs)
    want = [M.compress(b, 7) for b in inputs]
    keep, sptr, _ = pack(cuda, inputs, misalign=[(k + 1) % 16 for k in range(n)])
    caps = [len(w) for w in want]
    mid, mptr, moffs = alloc_out(cuda, caps)
    back, bptr, boffs = alloc_out(cuda, [max(len(b), 1) for b in inputs])
    sizes, capt = ints(cuda, map(len, inputs)), ints(cuda, caps)
    bcap = ints(cuda, [max(len(b), 1) for b in inputs])
    res, dres = ints(cuda, [POISON] * n), ints(cuda, [POISON] * n)
    cscr = _scratch(cuda, product.lz4f_compress_scratch_size(n, MAX_SRC))
    dscr = _scratch(cuda, product.lz4f_decompress_scratch_size(n, 4))
    st = cuda.cuda.Stream()
    st.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=st):
        product.lz4f_compress_batch(sptr, sizes, mptr, capt, res, MAX_SRC, 7, cscr, stream=st)
        product.lz4f_decompress_batch(mptr, res, bptr, bcap, dres, 4, 0, dscr, stream=st)
    res.fill_(POISON)
    dres.fill_(POISON)
    cscr.fill_(0x44)
    dscr.fill_(0x55)
    g.replay()
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    assert [fetch(mid, o, max(r, 0)) for o, r in zip(moffs, rs)] == want
    assert dres.cpu().tolist() == [len(b) for b in inputs]
    assert [fetch(back, o, len(b)) for o, b in zip(boffs, inputs)] == inputs


# ---- decode: liblz4's frames ----
def test_every_fixture_decodes_to_its_content(product, cuda):
    fx = list(M.fixtures().values())
    frames = [f["frame"] for f in fx]
    caps = [max(_bound(f), 1) for f in frames]
    rs, outs = _decompress(cuda, product, frames, caps)
    assert rs == [len(f["content"]) for f in fx]
    assert outs == [f["content"] for f in fx]
    # without the chained launch the linked frames are unsupported, the others as before
    rs, outs = _decompress(cuda, product, frames, caps, flags=M.NO_LINKED)
    assert rs == [-3 if f["linked"] else len(f["content"]) for f in fx]
    assert all(o == f["content"] for o, f in zip(outs, fx) if not f["linked"])
    assert rs == [M.decode(f, c, M.DEFAULT_BLOCKS, M.NO_LINKED)[0] for f, c in zip(frames, caps)]


def test_bytes_after_the_frame_are_ignored(product, cuda):
    fx = M.fixtures()
    frames = [fx["linked_all"]["frame"] + b"\x04\x22\x4d\x18 trailing", fx["empty"]["frame"] + b"x"]
    rs, outs = _decompress(cuda, product, frames, [196708, 1])
    assert (rs, outs) == ([196708, 0], [fx["linked_all"]["content"], b""])


# ---- decode: malformed frames among good neighbours ----
def _mixed(cases):
    """Every case between two fixtures: (frames, caps, the model's (result, bytes) per frame
    with `flags`)."""
    fx = M.fixtures()
    good = [fx[k] for k in ("linked_all", "indep_bsum", "one_byte", "random_block_all")]
    frames, caps = [], []
    for k, c in enumerate(cases):
        g = good[k % len(good)]
        frames += [g["frame"], c.frame]
        caps += [max(_bound(g["frame"]), 1), c.cap]
    frames.append(good[0]["frame"])
    caps.append(_bound(good[0]["frame"]))
    return frames, caps


def test_each_corruption_gets_its_code_and_the_neighbours_decode(product, cuda):
    cases = M.corruptions()
    codes = {c.name: c.code for c in cases}
    assert codes == {"flipped data byte, block checksums": -6, "flipped content checksum": -7,
                     "wrong header checksum": -1, "reserved bit, checksum redone": -1,
                     "dictionary ID": -3, "skippable magic": -3, "cut inside a block": -2,
                     "cut inside the trailer": -2, "changed content size": -8,
                     "two 100-byte blocks": -5,
                     "declared size 1, a full block, then 00": -4,
                     "declared size 200, a 100-byte block, then 00": -5,
                     "declared size 0, 1025 blocks 00 at 4 MiB": -5,
                     "one block more than max_blocks": M.ERANGE,
                     "capacity one short": -9}
    for max_blocks in sorted({c.max_blocks for c in cases}):
        batch = [c for c in cases if c.max_blocks == max_blocks]
        frames, caps = _mixed(batch)
        want = [M.decode(f, c, max_blocks) for f, c in zip(frames, caps)]
        assert [w[0] for w in want[1::2]] == [c.code for c in batch]
        rs, outs = _decompress(cuda, product, frames, caps, max_blocks=max_blocks)
        assert rs == [w[0] for w in want]
        assert all(o == w[1] for o, w in zip(outs, want) if w[0] >= 0)


def test_without_verification_the_checksum_corruptions_decode(product, cuda):
    cases = [c for c in M.corruptions() if c.max_blocks == M.DEFAULT_BLOCKS]
    frames, caps = _mixed(cases)
    want = [M.decode(f, c, M.DEFAULT_BLOCKS, M.NO_VERIFY) for f, c in zip(frames, caps)]
    lenient = [c for c in cases if c.lenient is not None]
    assert len(lenient) == 2
    for c in lenient:
        assert want[2 * cases.index(c) + 1] == (len(c.lenient), c.lenient)
    rs, outs = _decompress(cuda, product, frames, caps, flags=M.NO_VERIFY)
    assert rs == [w[0] for w in want]
    assert all(o == w[1] for o, w in zip(outs, want) if w[0] >= 0)


# ---- info ----
def test_info_agrees_with_the_model(product, cuda):
    frames = [f["frame"] for f in M.fixtures().values()] + [c.frame for c in M.corruptions()]
    frames += [b"", b"\x04\x22\x4d", M.fixtures()["indep_all"]["frame"][:9]]
    n = len(frames)
    keep, sptr, _ = pack(cuda, frames, misalign=[(k + 5) % 16 for k in range(n)])
    info = cuda.full((8 * n + 2,), POISON, dtype=cuda.int32, device="cuda")
    product.lz4f_info_batch(sptr, ints(cuda, map(len, frames)), info[1:8 * n + 1])
    cuda.cuda.synchronize()
    host = info.cpu().tolist()
    assert host[0] == POISON and host[-1] == POISON
    assert [host[1 + 8 * k:9 + 8 * k] for k in range(n)] == [M.info(f) for f in frames]
    stage = {c.name: M.info(c.frame)[0] for c in M.corruptions()}
    assert all(stage[c.name] == (c.code if c.header_stage else 0) for c in M.corruptions())


def test_empty_batches_launch_nothing(product, cuda):
    L = product.lib()
    assert L.APE_LZ4_lz4f_compress_batch_dev(None, None, None, None, None, 0, 65536, 7, None, 0,
                                             None) == 0
    assert L.APE_LZ4_lz4f_decompress_batch_dev(None, None, None, None, None, 0, 4, 0, None, 0,
                                               None) == 0
    assert L.APE_LZ4_lz4f_info_batch_dev(None, None, None, 0, None) == 0
