"""Framed compress with preferences on the GPU (include/ape_lz4f_prefs.h) against
tests/lz4fprefsmodel.py, byte for byte, and against the calls it is defined by on the device:
every block equals what the mode's large-input call returns for the same range with capacity
len - 1 (which holds even where a model is wrong), ID 4 with the fast encoder equals
APE_LZ4_lz4f_compress_batch_dev, and the frames go back through APE_LZ4_lz4f_info_batch_dev and
the verifying APE_LZ4_lz4f_decompress_batch_dev.  The shapes are the smallest at which plan,
layout and pack can go wrong: ID 5 around one and two blocks, a stored middle block that the
pack moves from the source in four pieces, one block each at IDs 6 and 7."""
import pytest

import lz4fmodel as F
import lz4fprefsmodel as P
from gpuutil import CANARY, alloc_out, fetch, ints, pack

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
EINVAL = -2
B5 = 262144
SIZES5 = [0, 1, 12, 65536, B5 - 1, B5, B5 + 1, 2 * B5, 2 * B5 + 777]
MODES = ((0, 0), (1, 8), (2, 8))


@pytest.fixture(scope="module")
def inputs5():
    """The ID 5 inputs: a text that repeats every 3000 bytes cut at SIZES5, one input whose
    middle block is random (stored, and packed from the source in four pieces), one with a
    random tail of one byte, and the two blocks on either side of the capacity len - 1."""
    whole = F.content_of([["text", 3000, 1, max(SIZES5)]])
    middle = F.content_of([["text", 3000, 2, B5], ["rand", B5, 9, B5], ["text", 3000, 3, 777]])
    tail = F.content_of([["text", 3000, 1, B5], ["rand", 1, 3, 1]])
    return [whole[:n] for n in SIZES5] + [middle, tail, P.edge(1289), P.edge(1290)]


def _scratch(cuda, nbytes):
    assert 0 < nbytes < 1 << 31
    return cuda.full((nbytes,), 0x33, dtype=cuda.uint8, device="cuda")


class Run:
    """One framed call: results, the bytes written per frame, whether each destination is
    untouched, and the sources on the device for the cross-check."""

    def __init__(self, cuda, product, inputs, bsid, mode, depth, flags, caps=None, max_src=None,
                 sizes=None, pass_slices=0, scratch_bytes=None):
        n = len(inputs)
        S = product.compress_large_slice_size()
        self.want = [P.compress(b, bsid, mode, depth, flags, S) for b in inputs]
        caps = [len(w) for w in self.want] if caps is None else caps
        max_src = max(map(len, inputs)) if max_src is None else max_src
        self.src, sptr, self.src_offs = pack(cuda, inputs, misalign=[(2 * k + 1) % 16 for k in range(n)])
        dst, dptr, offs = alloc_out(cuda, caps, misalign=[(6 * k + 3) % 16 for k in range(n)])
        res = ints(cuda, [POISON] * n)
        need = product.lz4f_compress_prefs_scratch_size(n, max_src, bsid, mode, pass_slices)
        scratch = _scratch(cuda, need if scratch_bytes is None else scratch_bytes)
        product.lz4f_compress_prefs_batch(sptr, ints(cuda, sizes or map(len, inputs)), dptr,
                                          ints(cuda, caps), res, max_src, bsid, mode, depth, flags,
                                          scratch)
        cuda.cuda.synchronize()
        self.results = res.cpu().tolist()
        self.outs = [fetch(dst, o, max(r, 0)) for o, r in zip(offs, self.results)]
        self.clean = [fetch(dst, o, c) == bytes([CANARY]) * c for o, c in zip(offs, caps)]


def _large_call(cuda, product, mode, depth, run, inputs, B):
    """[(result, bytes)] of the mode's large-input call for every block range of `inputs`, whose
    bytes lie on the device in `run`, with capacity len - 1."""
    ranges = [(k, lo, min(len(b), lo + B)) for k, b in enumerate(inputs) for lo in range(0, len(b), B)]
    base = run.src.data_ptr()
    ptrs = cuda.tensor([base + run.src_offs[k] + lo for k, lo, _ in ranges], dtype=cuda.int64,
                       device="cuda")
    caps = [hi - lo - 1 for _, lo, hi in ranges]
    dst, dptr, offs = alloc_out(cuda, caps)
    res = ints(cuda, [POISON] * len(ranges))
    args = (ptrs, ints(cuda, [hi - lo for _, lo, hi in ranges]), dptr, ints(cuda, caps), res, B)
    if mode == 0:
        product.compress_large_ptr_batch(*args, acceleration=1)
    elif mode == 1:
        product.compress_large_hc_ptr_batch(*args, depth)
    else:
        product.compress_large_hc_opt_ptr_batch(*args, depth)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    return [(r, fetch(dst, o, max(r, 0))) for r, o in zip(rs, offs)]


def _check_blocks(cuda, product, mode, depth, run, inputs, B):
    """Each block of run's frames: the large call's bytes, or stored where that answered 0."""
    got = [blk for out in run.outs for blk in P.blocks_of(out)]
    large = _large_call(cuda, product, mode, depth, run, inputs, B)
    plain = [b[lo:lo + B] for b in inputs for lo in range(0, len(b), B)]
    assert len(got) == len(large) == len(plain)
    for (body, stored), (r, comp), block in zip(got, large, plain):
        assert r >= 0
        assert (body, stored) == ((comp, False) if r > 0 else (block, True))


def _round_trip(cuda, product, frames, inputs, B, max_blocks):
    """info reports B and the block count; the verifying decode returns the input."""
    n = len(frames)
    keep, sptr, _ = pack(cuda, frames, misalign=[(7 * k + 3) % 16 for k in range(n)])
    sizes = ints(cuda, map(len, frames))
    info = cuda.full((8 * n,), POISON, dtype=cuda.int32, device="cuda")
    product.lz4f_info_batch(sptr, sizes, info)
    cuda.cuda.synchronize()
    rows = [info.cpu().tolist()[8 * k:8 * k + 8] for k in range(n)]
    assert [(r[0], r[2], r[3], r[4]) for r in rows] == \
        [(0, B, (len(b) + B - 1) // B, len(f)) for f, b in zip(frames, inputs)]
    caps = [max(r[5], 1) for r in rows]
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(5 * k + 1) % 16 for k in range(n)])
    res = ints(cuda, [POISON] * n)
    scratch = _scratch(cuda, product.lz4f_decompress_scratch_size(n, max_blocks))
    product.lz4f_decompress_batch(sptr, sizes, dptr, ints(cuda, caps), res, max_blocks,
                                  F.NO_LINKED, scratch)
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == [len(b) for b in inputs]
    assert [fetch(dst, o, len(b)) for o, b in zip(offs, inputs)] == inputs


@pytest.mark.parametrize("flags", (0, 3, 7))
@pytest.mark.parametrize("mode,depth", MODES)
def test_id_5_frames_equal_the_model_and_the_large_call_and_decode_again(product, cuda, inputs5,
                                                                         mode, depth, flags):
    run = Run(cuda, product, inputs5, 5, mode, depth, flags)
    assert run.results == [len(w) for w in run.want]
    assert run.outs == run.want
    assert all(r <= product.lz4f_compress_prefs_bound(len(b), 5, flags)
               for r, b in zip(run.results, inputs5))
    # what the inputs are there for
    middle, tail, fits, full = [P.blocks_of(o) for o in run.outs[len(SIZES5):]]
    assert [s for _, s in middle] == [False, True, False] and len(middle[1][0]) == B5
    assert [s for _, s in tail] == [False, True] and len(tail[1][0]) == 1
    assert [s for _, s in fits] == [False] and [s for _, s in full] == [True]
    _check_blocks(cuda, product, mode, depth, run, inputs5, B5)
    _round_trip(cuda, product, run.outs, inputs5, B5, 3)


@pytest.mark.parametrize("bsid,extra", ((6, 13), (7, 1)))
def test_one_block_and_a_rest_at_ids_6_and_7(product, cuda, bsid, extra):
    B = F.block_max(bsid)
    data = [F.content_of([["text", 3000, 1, B + extra]])]
    for flags in (0, 3, 7):
        run = Run(cuda, product, data, bsid, 0, 0, flags)
        assert run.results == [len(run.want[0])]
        assert run.outs == run.want
    _check_blocks(cuda, product, 0, 0, run, data, B)
    _round_trip(cuda, product, run.outs, data, B, 2)


@pytest.mark.parametrize("flags", range(8))
def test_id_4_with_the_fast_encoder_is_the_existing_call(product, cuda, flags):
    sizes = [0, 1, 12, 13, 65535, 65536, 65537, 3 * 65536 + 100]      # tests/test_gpu_lz4f.py's
    whole = F.content_of([["text", 3000, 1, max(sizes)]])
    inputs = [whole[:n] for n in sizes]
    inputs.append(F.content_of([["rand", 65536, 9, 65536], ["text", 1000, 2, 1000]]))
    n = len(inputs)
    run = Run(cuda, product, inputs, 4, 0, 0, flags)
    keep, sptr, _ = pack(cuda, inputs, misalign=[(5 * k + 1) % 16 for k in range(n)])
    caps = [len(w) for w in run.want]
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(3 * k + 2) % 16 for k in range(n)])
    res = ints(cuda, [POISON] * n)
    scratch = _scratch(cuda, product.lz4f_compress_scratch_size(n, max(map(len, inputs))))
    product.lz4f_compress_batch(sptr, ints(cuda, map(len, inputs)), dptr, ints(cuda, caps), res,
                                max(map(len, inputs)), flags, scratch)
    cuda.cuda.synchronize()
    old = res.cpu().tolist()
    assert run.results == old == [len(F.compress(b, flags)) for b in inputs]
    assert run.outs == [fetch(dst, o, r) for o, r in zip(offs, old)]
    assert run.outs == [F.compress(b, flags) for b in inputs]


@pytest.mark.parametrize("mode,depth", MODES)
def test_capacities_and_error_rows_among_good_neighbours(product, cuda, inputs5, mode, depth):
    """Exact capacity works, one less gives 0 and an untouched destination, a negative size 0,
    a size above maxSrcSize ERANGE; the frames between them are what they are alone."""
    a, b, two, big = inputs5[6], inputs5[3], inputs5[7], inputs5[8]     # B + 1, 65536, 2 B, 2 B + 777
    S = product.compress_large_slice_size()
    fa, fb, ftwo = (P.compress(x, 5, mode, depth, 7, S) for x in (a, b, two))
    batch = [a, a, b, big, b, two, two]
    sizes = [len(a), len(a), -1, len(big), len(b), len(two), len(two)]
    caps = [len(fa), len(fa) - 1, len(fb), product.lz4f_compress_prefs_bound(len(big), 5, 7),
            len(fb), len(ftwo) - 1, len(ftwo)]
    run = Run(cuda, product, batch, 5, mode, depth, 7, caps=caps, max_src=len(two), sizes=sizes)
    assert run.results == [len(fa), 0, 0, P.ERANGE, len(fb), 0, len(ftwo)]
    assert [run.outs[k] for k in (0, 4, 6)] == [fa, fb, ftwo]
    assert all(run.clean[k] for k in (1, 2, 3, 5))


@pytest.mark.parametrize("mode,depth", MODES[1:])
def test_a_smaller_scratch_means_more_passes_and_the_same_bytes(product, cuda, inputs5, mode, depth):
    batch = [inputs5[8], inputs5[9], inputs5[4]]
    n, max_src = len(batch), max(map(len, batch))
    size = product.lz4f_compress_prefs_scratch_size
    one, three, all_ = (size(n, max_src, 5, mode, ps) for ps in (1, 3, 0))
    assert one < three < all_
    whole = Run(cuda, product, batch, 5, mode, depth, 7)
    assert whole.outs == whole.want
    for scratch_bytes in (three, three - 1, one):      # three, two and one slice per pass
        run = Run(cuda, product, batch, 5, mode, depth, 7, scratch_bytes=scratch_bytes)
        assert run.outs == whole.outs and run.results == whole.results


@pytest.mark.parametrize("mode,depth", MODES)
def test_a_scratch_one_byte_short_is_einval(product, cuda, inputs5, mode, depth):
    batch = [inputs5[6]]
    keep, sptr, _ = pack(cuda, batch)
    need = product.lz4f_compress_prefs_scratch_size(1, len(batch[0]), 5, mode, 1)
    dst, dptr, offs = alloc_out(cuda, [1000])
    res, sizes, caps = ints(cuda, [POISON]), ints(cuda, [len(batch[0])]), ints(cuda, [1000])
    scratch = _scratch(cuda, need)
    call = product.lib().APE_LZ4_lz4f_compress_prefs_batch_dev
    args = [sptr.data_ptr(), sizes.data_ptr(), dptr.data_ptr(), caps.data_ptr(), res.data_ptr(), 1,
            len(batch[0]), 5, mode, depth, 7, scratch.data_ptr()]
    assert call(*args, need - 1, None) == EINVAL
    assert product.gpu_last_error().startswith("lz4f_compress_prefs_batch_dev:")
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == [POISON] and fetch(dst, offs[0], 1000) == bytes([CANARY]) * 1000
    assert call(*args, need, None) == 0
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == [0]          # (the frame does not fit 1000 bytes)


@pytest.mark.parametrize("mode,depth", MODES)
def test_the_call_captures_into_a_graph(product, cuda, inputs5, mode, depth):
    """One stream, no parallel branches: one captured call, replayed once."""
    batch = [inputs5[6], inputs5[9], inputs5[0], inputs5[11]]
    n, max_src = len(batch), max(map(len, batch))
    S = product.compress_large_slice_size()
    want = [P.compress(b, 5, mode, depth, 7, S) for b in batch]
    keep, sptr, _ = pack(cuda, batch, misalign=[(k + 1) % 16 for k in range(n)])
    caps = [len(w) for w in want]
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(2 * k + 1) % 16 for k in range(n)])
    sizes, capt, res = ints(cuda, map(len, batch)), ints(cuda, caps), ints(cuda, [POISON] * n)
    scratch = _scratch(cuda, product.lz4f_compress_prefs_scratch_size(n, max_src, 5, mode, 0))
    st = cuda.cuda.Stream()
    st.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=st):
        product.lz4f_compress_prefs_batch(sptr, sizes, dptr, capt, res, max_src, 5, mode, depth, 7,
                                          scratch, stream=st)
    res.fill_(POISON)
    scratch.fill_(0x44)
    dst.fill_(CANARY)
    g.replay()
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    assert rs == caps
    assert [fetch(dst, o, r) for o, r in zip(offs, rs)] == want


def test_an_empty_batch_launches_nothing(product, cuda):
    call = product.lib().APE_LZ4_lz4f_compress_prefs_batch_dev
    for bsid, mode, depth in ((4, 0, 0), (7, 2, 8)):
        assert call(None, None, None, None, None, 0, 65536, bsid, mode, depth, 7, None, 0, None) == 0
