"""Prepared dictionaries: what can be checked without a GPU -- the object size, the window
arithmetic and the argument checks that precede every device call (tests/test_gpu_cdict.py has
the rest)."""
import pytest

EINVAL = -2
K_HSIZE = 7328   # the encoder's table entries (lz4_gpu_internal.h)


def test_cdict_size(product):
    n = product.cdict_size()
    assert n > 0 and n % 16 == 0
    assert n >= 65536 + K_HSIZE * 2


def test_cdict_window(product):
    w = product.cdict_window
    assert w(0, 1024) == 0
    assert w(63, 1024) == 0
    assert w(64, 1024) == 64
    assert w(100, 1024) == 64
    assert w(70000, 4096) == 61440
    assert w(65536, 65536) == 0
    assert w(65536, 1) == 65472
    assert w(-1, 1024) == -1
    assert w(100, 0) == -1
    assert w(100, 65537) == -1


def test_prepare_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_cdict_prepare_dev
    size = product.cdict_size()
    a = 16   # (never dereferenced: each call fails its argument check)
    assert f(None, 100, 1024, a, size, None) == EINVAL      # null dictionary of 100 bytes
    assert f(a, 100, 1024, None, size, None) == EINVAL      # null object
    assert f(a, -1, 1024, a, size, None) == EINVAL
    assert f(a, 100, 0, a, size, None) == EINVAL
    assert f(a, 100, 65537, a, size, None) == EINVAL
    assert f(a, 100, 1024, a, size - 1, None) == EINVAL
    assert f(a, 100, 1024, a, 0, None) == EINVAL
    for mis in (1, 4, 8):
        assert f(a, 100, 1024, a + mis, size, None) == EINVAL


def test_compress_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_compress_usingCDict_batch_dev
    a = 16
    assert f(a, a, a, a, a, -1, a, None) == EINVAL
    for hole in range(5):
        args = [a] * 5
        args[hole] = None
        assert f(*args, 1, a, None) == EINVAL
    assert f(a, a, a, a, a, 1, None, None) == EINVAL
    assert f(a, a, a, a, a, 0, None, None) == EINVAL
    assert f(a, a, a, a, a, 1, a + 8, None) == EINVAL


def test_binding_validates_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    obj = torch.zeros(product.cdict_size(), dtype=torch.uint8)
    with pytest.raises(ValueError):   # the sizes tensor is checked before its shape is read
        product.compress_cdict_batch(p, None, p, i, i, obj)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_cdict_batch(p, i, p, i, i, obj)
    with pytest.raises(ValueError):
        product.compress_cdict_batch(p, i.to(torch.int64), p, i, i, obj)
    with pytest.raises(ValueError):
        product.compress_cdict_batch(p, i, p, i, i, None)
    d = torch.zeros(100, dtype=torch.uint8)
    with pytest.raises(ValueError):   # CPU tensors
        product.cdict_prepare(d, 1024, obj)
    with pytest.raises(ValueError):
        product.cdict_prepare(d.to(torch.int32), 1024, obj)
    with pytest.raises(ValueError):
        product.cdict_prepare(None, 1024, obj)
    with pytest.raises(ValueError):
        product.cdict_prepare(d, 1024, obj.to(torch.int16))
