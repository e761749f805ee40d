"""Byte ranges of indexed blocks: what can be checked without a GPU -- the exported symbol, the
argument checks that precede every device call, and the binding's checks of its tensors
(tests/test_gpu_range.py has the rest)."""
import pytest

EINVAL = -2


def test_the_symbol_is_exported(product):
    assert hasattr(product.lib(), "APE_LZ4_decompress_range_indexed_batch_dev")
    assert "decompress_range_indexed_ptr_batch" in product.__all__


def test_bad_arguments_are_rejected_before_any_device_call(product):
    f = product.lib().APE_LZ4_decompress_range_indexed_batch_dev
    a = 16   # (never dereferenced: each call fails its argument check)

    def call(src=a, csz=a, index=a, stride=64, max_seg=4, nblocks=1, block_of=a, start=a, ln=a,
             dst=a, cap=a, window=a, res=a, nreq=3, waves=4):
        return f(src, csz, index, stride, max_seg, nblocks, block_of, start, ln, dst, cap, window,
                 res, nreq, waves, None)

    for hole in ("src", "csz", "index", "start", "ln", "dst", "cap", "window", "res"):
        assert call(**{hole: None}) == EINVAL, hole
    assert call(block_of=None) == EINVAL                 # 3 requests, 1 block: needs the mapping
    assert call(block_of=None, nreq=2, nblocks=3) == EINVAL
    assert "d_blockOf" in product.gpu_last_error()
    assert call(nblocks=-1) == EINVAL and call(nreq=-1) == EINVAL
    assert call(nblocks=-1, nreq=-1, block_of=None) == EINVAL
    assert call(waves=0) == EINVAL and call(waves=-2) == EINVAL
    assert call(nreq=1 << 16, waves=1 << 15) == EINVAL   # 2^31 waves
    assert call(nreq=3, waves=1 << 30) == EINVAL
    assert call(max_seg=0) == EINVAL
    assert call(index=a + 8) == EINVAL                   # misaligned
    assert call(stride=72) == EINVAL                     # not a multiple of 16
    assert call(stride=48) == EINVAL                     # 16 + 8 * 5 = 56 > 48
    assert call(max_seg=6, stride=64) == EINVAL          # 16 + 8 * 7 = 72 > 64
    assert "stride" in product.gpu_last_error()


def test_the_binding_validates_its_tensors(product):
    import torch
    f = product.decompress_range_indexed_ptr_batch
    p1, i1 = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    p3, i3 = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    w = torch.zeros(6, dtype=torch.int32)
    ix = torch.zeros((1, 64), dtype=torch.uint8)
    good = dict(src_ptrs=p1, comp_sizes=i1, index=ix, max_segments=4, range_starts=i3,
                range_lens=i3, dst_ptrs=p3, caps=i3, window=w, results=i3, block_of=i3)
    for name in ("src_ptrs", "comp_sizes", "index", "range_starts", "range_lens", "dst_ptrs",
                 "caps", "window", "results"):
        with pytest.raises(ValueError):
            f(**dict(good, **{name: None}))
    for name in ("comp_sizes", "range_starts", "range_lens", "caps", "window", "results",
                 "block_of"):
        with pytest.raises(ValueError):      # sizes are int32
            f(**dict(good, **{name: good[name].to(torch.int64)}))
    for name in ("src_ptrs", "dst_ptrs"):
        with pytest.raises(ValueError):      # pointers are int64
            f(**dict(good, **{name: good[name].to(torch.int32)}))
    with pytest.raises(ValueError):          # the index is a 2-D uint8 tensor, one row per block
        f(**dict(good, index=ix.to(torch.int32)))
    with pytest.raises(ValueError):          # per-request tensors have one entry per request
        f(**dict(good, range_lens=i1))
    with pytest.raises(ValueError):
        f(**dict(good, window=i3))           # two ints per request
    with pytest.raises(ValueError):          # without block_of: one request per block
        f(**dict(good, block_of=None))
    with pytest.raises(ValueError):          # CPU tensors
        f(**good)
