"""compress_large: what can be checked without a GPU -- the slice constant, the scratch size
and the argument checks that precede every device call (tests/test_gpu_large.py has the
rest)."""
import pytest

MB = 1 << 20
EINVAL = -2


def test_slice_size_and_scratch_size(product):
    S = product.compress_large_slice_size()
    assert S % 64 == 0 and 0 < S <= 65536 - 64
    size = product.compress_large_scratch_size
    maxes = (1, 65536, 65537, 200000, MB, 16 * MB, 0x7E000000)
    for n in (0, 1, 2, 8, 100):
        row = [size(n, m) for m in maxes]
        assert row == sorted(row) and row[0] > 0
    for m in maxes:
        col = [size(n, m) for n in (0, 1, 2, 8, 100, 1 << 20)]
        assert col == sorted(col)
    # a large input needs room for every slice's own stream
    assert size(1, 16 * MB) > 16 * MB
    # out of range: no size
    assert size(1, 0) == 0 and size(1, 0x7E000001) == 0 and size(-1, MB) == 0


def test_launcher_rejects_bad_arguments_before_any_device_call(product):
    L = product.lib()
    f = L.APE_LZ4_compress_large_batch_dev
    a = 16   # (never dereferenced: each call fails its argument check)
    assert f(a, a, a, a, a, -1, MB, 1, a, 1 << 30, None) == EINVAL
    for hole in range(5):
        args = [a] * 5
        args[hole] = None
        assert f(*args, 1, MB, 1, a, 1 << 30, None) == EINVAL
    assert f(a, a, a, a, a, 1, MB, 1, None, 1 << 30, None) == EINVAL
    assert f(a, a, a, a, a, 1, 0, 1, a, 1 << 30, None) == EINVAL
    assert f(a, a, a, a, a, 1, 0x7E000001, 1, a, 1 << 30, None) == EINVAL


def test_binding_validates_sizes_before_reading_their_shape(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        product.compress_large_ptr_batch(p, None, p, i, i, MB)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_large_ptr_batch(p, i, p, i, i, MB)
    with pytest.raises(ValueError):
        product.compress_large_ptr_batch(p, i.to(torch.int64), p, i, i, MB)
