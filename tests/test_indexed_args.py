"""Indexed large blocks: what can be checked without a GPU -- the two index-size helpers and
the argument checks that precede every device call of the indexed compressor and decoder
(tests/test_gpu_indexed.py has the rest)."""
import pytest

MB = 1 << 20
EINVAL = -2


def test_index_helpers(product):
    S = product.compress_large_slice_size()
    seg, size = product.large_index_segments, product.large_index_size
    assert seg(65536, S) == 1 and seg(1, S) == 1 and seg(16 * MB, 0) == 1
    assert seg(65537, S) == -(-65537 // S)
    assert seg(16 * MB, 8 * S) == 16 * MB // (8 * S)
    assert seg(16 * MB + 1, 8 * S) == 16 * MB // (8 * S) + 1
    assert seg(0x7E000000, S) == -(-0x7E000000 // S)
    for m, r in ((65536, S), (65537, S), (MB, 4 * S), (16 * MB, 8 * S), (16 * MB, 0)):
        assert size(m, r) == (16 + 8 * (seg(m, r) + 1) + 15) // 16 * 16
    assert size(1, 0) == 32
    # monotone: more input never needs fewer segments, a longer period never more
    maxes = (1, 65536, 65537, 200000, MB, 16 * MB, 0x7E000000)
    for r in (S, 2 * S, 8 * S, 32 * S):
        row = [seg(m, r) for m in maxes]
        assert row == sorted(row) and row[0] == 1
        assert [size(m, r) for m in maxes] == sorted(size(m, r) for m in maxes)
    for m in maxes:
        col = [seg(m, r) for r in (S, 2 * S, 8 * S, 32 * S)]
        assert col == sorted(col, reverse=True)
    # out of range: 0
    for f in (seg, size):
        assert f(0, S) == 0 and f(0x7E000001, S) == 0 and f(-1, 0) == 0
        assert f(MB, -S) == 0 and f(MB, S + 1) == 0 and f(MB, S // 2) == 0


def test_compressor_rejects_bad_arguments_before_any_device_call(product):
    L = product.lib()
    S = product.compress_large_slice_size()
    f = L.APE_LZ4_compress_large_indexed_batch_dev
    a = 16   # (never dereferenced: each call fails its argument check)
    big = 1 << 30
    stride = product.large_index_size(MB, S)

    def call(ptrs=(a,) * 5, n=1, max_src=MB, scratch=a, restart=S, index=a, istride=stride):
        return f(*ptrs, n, max_src, 1, scratch, big, restart, index, istride, None)

    assert call(n=-1) == EINVAL
    for hole in range(5):
        ptrs = [a] * 5
        ptrs[hole] = None
        assert call(ptrs=ptrs) == EINVAL
    assert call(scratch=None) == EINVAL
    assert call(max_src=0) == EINVAL and call(max_src=0x7E000001) == EINVAL
    for bad in (S + 1, S - 64, S // 2, -S, -1):
        assert call(restart=bad) == EINVAL
        assert call(restart=bad, index=None) == EINVAL
    assert "slice size" in product.gpu_last_error()
    assert call(index=a + 8) == EINVAL                  # misaligned
    assert call(istride=stride + 8) == EINVAL           # not a multiple of 16
    assert call(istride=stride - 16) == EINVAL          # too small
    assert call(istride=0) == EINVAL
    assert str(stride) in product.gpu_last_error()
    assert call(restart=0, istride=16) == EINVAL and call(max_src=65536, istride=16) == EINVAL


def test_decoder_rejects_bad_arguments_before_any_device_call(product):
    L = product.lib()
    f = L.APE_LZ4_decompress_safe_indexed_batch_dev
    a = 16

    def call(src=a, csz=a, dst=a, cap=a, index=a, stride=64, max_seg=4, res=a, n=1):
        return f(src, csz, dst, cap, index, stride, max_seg, res, n, None)

    assert call(n=-1) == EINVAL
    for hole in ("src", "csz", "dst", "cap", "index", "res"):
        assert call(**{hole: None}) == EINVAL
    assert call(max_seg=0) == EINVAL and call(max_seg=-3) == EINVAL
    assert call(index=a + 4) == EINVAL
    assert call(stride=72) == EINVAL                   # not a multiple of 16
    assert call(stride=48) == EINVAL                   # 16 + 8 * 5 = 56 > 48
    assert call(max_seg=6, stride=64) == EINVAL        # 16 + 8 * 7 = 72 > 64
    # nblocks x maxSegments must stay below 2^31 (the strides here are large enough)
    assert call(n=1 << 16, max_seg=1 << 15, stride=16 + 8 * ((1 << 15) + 1) + 8) == EINVAL
    assert call(n=3, max_seg=1 << 30, stride=(1 << 33) + 32) == EINVAL


def test_bindings_validate_their_tensors(product):
    import torch
    S = product.compress_large_slice_size()
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    ix = torch.zeros((2, 64), dtype=torch.uint8)
    with pytest.raises(ValueError):
        product.compress_large_indexed_ptr_batch(p, None, p, i, i, MB, S)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_large_indexed_ptr_batch(p, i, p, i, i, MB, S, index=ix)
    with pytest.raises(ValueError):
        product.compress_large_indexed_ptr_batch(p, i.to(torch.int64), p, i, i, MB, S)
    with pytest.raises(ValueError):
        product.decompress_indexed_ptr_batch(p, None, p, i, ix, 4, i)
    with pytest.raises(ValueError):   # CPU tensors
        product.decompress_indexed_ptr_batch(p, i, p, i, ix, 4, i)
    with pytest.raises(ValueError):
        product.decompress_indexed_ptr_batch(p, i, p, i.to(torch.int64), ix, 4, i)
    with pytest.raises(ValueError):   # the index is a 2-D uint8 tensor, one row per block
        product.decompress_indexed_ptr_batch(p, i, p, i, ix.to(torch.int32), 4, i)
    with pytest.raises(ValueError):
        product.decompress_indexed_ptr_batch(p, i, p, i, ix[:1], 4, i)
    for name in ("large_index_segments", "large_index_size", "compress_large_indexed_ptr_batch",
                 "decompress_indexed_ptr_batch"):
        assert name in product.__all__
