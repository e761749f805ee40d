"""The high-ratio mode's cost-minimising parse: what can be checked without a GPU -- the scratch
arithmetic and the argument checks that precede every device call of its three launchers
(tests/test_gpu_hc_opt.py and tests/test_gpu_hc_opt_large.py have the rest)."""
import pytest

EINVAL = -2
ENODEV = -1
SLOT = 65536 * (2 + 4 + 4)   # chain (u16) + match (u32) + cost (u32) per position
MB = 1 << 20


def test_scratch_size(product):
    f = product.compress_hc_opt_scratch_size
    assert SLOT == 393216 + 262144 == 655360
    assert f(-1) == 0 and f(-2 ** 31) == 0 and f(0) == 0
    assert f(1) == SLOT
    sizes = [f(n) for n in (1, 2, 7, 120, 1023, 1024, 1025, 100000, 2 ** 31 - 1)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert f(7) == 7 * SLOT and f(1024) == f(1025) == 1024 * SLOT
    assert f(7) - product.compress_hc_scratch_size(7) == 7 * 65536 * 4


def test_large_scratch_size(product):
    f, fast = product.compress_large_hc_opt_scratch_size, product.compress_large_scratch_size
    lazy = product.compress_large_hc_scratch_size
    S = product.compress_large_slice_size()
    for n, m in ((1, 1), (1, 65536), (3, 65537), (4, 200000), (16, 16 * MB), (2000, MB)):
        slots = n * (1 if m <= 65536 else (m + S - 1) // S)
        base = (fast(n, m) + 15) // 16 * 16
        assert f(n, m, 1) == base + SLOT
        assert f(n, m, 0) == base + min(slots, 1024) * SLOT
        assert f(n, m, 5) == base + min(slots, 5) * SLOT
        assert f(n, m, 2 ** 31 - 1) == f(n, m, 0)
        assert f(n, m, 5) - lazy(n, m, 5) == min(slots, 5) * 65536 * 4
    assert f(0, MB, 0) == f(0, MB, 1) > 0
    for n, m in ((-1, MB), (1, 0), (1, -5), (1, 0x7E000001)):
        assert f(n, m, 0) == fast(n, m) == 0
    assert f(1, MB, -1) == 0
    assert f(1 << 20, MB, 0) == fast(1 << 20, MB) == 2 ** 64 - 1


def test_block_call_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_compress_hc_opt_batch_dev
    one = product.compress_hc_opt_scratch_size(1)
    a = 16   # (never dereferenced: each call fails its argument check)
    assert f(a, a, a, a, a, -1, 64, a, one, None) == EINVAL
    for hole in range(5):
        args = [a] * 5
        args[hole] = None
        assert f(*args, 1, 64, a, one, None) == EINVAL
    for depth in (-1, 257, 2 ** 31 - 1, -2 ** 31):
        assert f(a, a, a, a, a, 1, depth, a, one, None) == EINVAL
    assert f(a, a, a, a, a, 1, 64, None, one, None) == EINVAL
    assert f(a, a, a, a, a, 0, 64, None, one, None) == EINVAL
    for mis in (1, 4, 8):
        assert f(a, a, a, a, a, 1, 64, a + mis, one, None) == EINVAL
    assert f(a, a, a, a, a, 1, 64, a, one - 1, None) == EINVAL
    assert str(one) in product.gpu_last_error()
    # the lazy call's scratch is too small for this one
    assert f(a, a, a, a, a, 1, 64, a, product.compress_hc_scratch_size(1), None) == EINVAL
    assert f(a, a, a, a, a, 1, 64, a, 0, None) == EINVAL
    assert f(a, a, a, a, a, 0, 64, a, one - 1, None) == EINVAL


def test_prefix_call_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_compress_hc_opt_withPrefix_batch_dev
    one = product.compress_hc_opt_scratch_size(1)
    a = 16
    assert f(a, a, a, a, a, a, -1, 64, a, one, None) == EINVAL
    for hole in (0, 1, 3, 4, 5):   # (2, the prefix sizes, may be null)
        args = [a] * 6
        args[hole] = None
        assert f(*args, 1, 64, a, one, None) == EINVAL
    for depth in (-1, 257):
        assert f(a, a, a, a, a, a, 1, depth, a, one, None) == EINVAL
    assert f(a, a, a, a, a, a, 1, 64, None, one, None) == EINVAL
    for mis in (1, 4, 8):
        assert f(a, a, a, a, a, a, 1, 64, a + mis, one, None) == EINVAL
    assert f(a, a, a, a, a, a, 1, 64, a, one - 1, None) == EINVAL
    assert f(a, a, a, a, a, a, 1, 64, a, 0, None) == EINVAL


def test_large_call_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_compress_large_hc_opt_batch_dev
    S = product.compress_large_slice_size()
    need = product.compress_large_hc_opt_scratch_size(2, MB, 1)
    stride = product.large_index_size(MB, S)
    a = 16

    def call(arrays=(a,) * 5, n=2, max_src=MB, depth=64, scr=a, nbytes=need, restart=0, ix=None,
             ix_stride=0):
        return f(*arrays, n, max_src, depth, scr, nbytes, restart, ix, ix_stride, None)

    for hole in range(5):
        assert call(arrays=(a,) * hole + (None,) + (a,) * (4 - hole)) == EINVAL
    assert call(n=-1) == EINVAL
    for depth in (-1, 257, 2 ** 31 - 1, -2 ** 31):
        assert call(depth=depth) == EINVAL
    assert call(scr=None) == EINVAL
    for mis in (1, 4, 8):
        assert call(scr=a + mis) == EINVAL
    assert call(nbytes=need - 1) == EINVAL
    assert str(need) in product.gpu_last_error()
    assert "compress_large_hc_opt" in product.gpu_last_error()
    assert call(nbytes=product.compress_large_hc_scratch_size(2, MB, 1)) == EINVAL
    assert call(nbytes=0) == EINVAL
    for max_src in (0, -1, 0x7E000001):
        assert call(max_src=max_src) == EINVAL
    for restart in (-S, 1, S - 64, S + 64):
        assert call(restart=restart) == EINVAL
    assert call(restart=S, ix=a + 8, ix_stride=stride) == EINVAL
    assert call(restart=S, ix=a, ix_stride=stride + 8) == EINVAL
    assert call(restart=S, ix=a, ix_stride=stride - 16) == EINVAL
    assert call(n=1 << 20) == EINVAL      # more slices than one call takes


def test_valid_arguments_without_a_device_give_enodev(product):
    L = product.lib()
    if L.APE_LZ4_gpu_device_count() > 0:
        pytest.skip("a GPU is visible here; covered by the -m gpu suite")
    a = 16
    one = product.compress_hc_opt_scratch_size(1)
    for depth in (0, 1, 64, 256):
        assert L.APE_LZ4_compress_hc_opt_batch_dev(a, a, a, a, a, 3, depth, a, one, None) == ENODEV
    assert L.APE_LZ4_compress_hc_opt_batch_dev(a, a, a, a, a, 0, 0, a, one, None) == ENODEV
    assert L.APE_LZ4_compress_hc_opt_withPrefix_batch_dev(a, a, None, a, a, a, 3, 64, a, one,
                                                          None) == ENODEV
    assert L.APE_LZ4_compress_hc_opt_withPrefix_batch_dev(a, a, a, a, a, a, 3, 0, a, one,
                                                          None) == ENODEV
    need = product.compress_large_hc_opt_scratch_size(2, MB, 1)
    for depth in (0, 1, 256):
        assert L.APE_LZ4_compress_large_hc_opt_batch_dev(a, a, a, a, a, 2, MB, depth, a, need, 0,
                                                         None, 0, None) == ENODEV


def test_bindings_validate_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    scr = torch.zeros(16, dtype=torch.uint8)
    good = [p, i, p, i, i, 64, scr]
    for hole in (0, 1, 2, 3, 4, 6):   # the sizes (1) are checked before their shape is read
        for bad in (None, [0, 0], 7):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                product.compress_hc_opt_ptr_batch(*args)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_hc_opt_ptr_batch(*good)
    with pytest.raises(ValueError):
        product.compress_hc_opt_ptr_batch(p, i.to(torch.int64), p, i, i, 64, scr)
    with pytest.raises(ValueError):
        product.compress_hc_opt_ptr_batch(p, i, p, i, i, 64, scr.to(torch.int16))
    with pytest.raises(ValueError):
        product.compress_hc_opt_ptr_batch(p, i[:1], p, i, i, 64, scr)
    for bad in (None, [0, 0], 7):
        with pytest.raises(ValueError):
            product.compress_large_hc_opt_ptr_batch(p, bad, p, i, i, MB, 64, scratch=scr)
        with pytest.raises(ValueError):
            product.compress_hc_opt_prefix_ptr_batch(p, bad, i, p, i, i, 64, scr)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_large_hc_opt_ptr_batch(p, i, p, i, i, MB, 64, scratch=scr)
    with pytest.raises(ValueError):
        product.compress_hc_opt_prefix_ptr_batch(p, i, None, p, i, i, 64, scr)
    with pytest.raises(ValueError):
        product.compress_hc_opt_prefix_ptr_batch(p, i, i.to(torch.int64), p, i, i, 64, scr)
    with pytest.raises(ValueError):
        product.compress_large_hc_opt_ptr_batch(p, i, p, i[:1], i, MB, 64, scratch=scr)
    with pytest.raises(ValueError):
        product.compress_large_hc_opt_ptr_batch(p, i, p, i, i, MB, 64, scratch=scr.to(torch.int16))
    for name in ("compress_hc_opt_scratch_size", "compress_hc_opt_ptr_batch",
                 "compress_hc_opt_prefix_ptr_batch", "compress_large_hc_opt_scratch_size",
                 "compress_large_hc_opt_ptr_batch"):
        assert name in product.__all__
