"""The high-ratio mode: what can be checked without a GPU -- the scratch arithmetic and the
argument checks that precede every device call (tests/test_gpu_hc.py has the rest)."""
import pytest

EINVAL = -2
ENODEV = -1
SLOT = 65536 * (2 + 4)   # chain (u16) + match (u32) per position (lz4_gpu_internal.h)


def test_scratch_size(product):
    f = product.compress_hc_scratch_size
    assert f(-1) == 0 and f(-2 ** 31) == 0 and f(0) == 0
    assert f(1) == SLOT
    sizes = [f(n) for n in (1, 2, 7, 120, 1023, 1024, 1025, 100000, 2 ** 31 - 1)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert f(7) == 7 * SLOT


def test_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_compress_hc_batch_dev
    one = product.compress_hc_scratch_size(1)
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
    assert f(a, a, a, a, a, 1, 64, a, 0, None) == EINVAL
    assert f(a, a, a, a, a, 0, 64, a, one - 1, None) == EINVAL


def test_valid_arguments_without_a_device_give_enodev(product):
    L = product.lib()
    if L.APE_LZ4_gpu_device_count() > 0:
        pytest.skip("a GPU is visible here; covered by the -m gpu suite")
    one = product.compress_hc_scratch_size(1)
    a = 16
    for depth in (0, 1, 64, 256):
        assert L.APE_LZ4_compress_hc_batch_dev(a, a, a, a, a, 3, depth, a, one, None) == ENODEV
    assert L.APE_LZ4_compress_hc_batch_dev(a, a, a, a, a, 0, 0, a, one, None) == ENODEV


def test_binding_validates_before_any_call(product):
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
                product.compress_hc_ptr_batch(*args)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_hc_ptr_batch(*good)
    with pytest.raises(ValueError):
        product.compress_hc_ptr_batch(p, i.to(torch.int64), p, i, i, 64, scr)
    with pytest.raises(ValueError):
        product.compress_hc_ptr_batch(p, i, p, i, i, 64, scr.to(torch.int16))
    with pytest.raises(ValueError):
        product.compress_hc_ptr_batch(p, i[:1], p, i, i, 64, scr)
