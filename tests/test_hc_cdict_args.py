"""The high-ratio mode against a prepared dictionary: what can be checked without a GPU -- the
object size, the window and scratch arithmetic, and the argument checks that precede every
device call, in C and in the bindings (tests/test_gpu_hc_cdict.py has the rest)."""
import pytest

import hcdictmodel

EINVAL = -2
ENODEV = -1


def slot(max_src):
    """chain (u16) for maxSrcSize + 3 window positions and match (u32) per message position,
    each rounded up to 16 bytes (lz4_gpu_internal.h)."""
    return (2 * (max_src + 3) + 15) // 16 * 16 + (4 * max_src + 15) // 16 * 16


def test_object_size(product):
    n = product.hc_cdict_size()
    assert n % 16 == 0
    # header, head table (2^14 u16), chain region (65536 u16), the window and its pads
    assert n >= 16 + 2 * (1 << 14) + 2 * 65536 + 65536 + 16
    assert n != product.cdict_size()


def test_window(product):
    w = product.hc_cdict_window
    assert w(0, 1024) == 0
    assert w(1, 1024) == 1 and w(63, 1024) == 63 and w(100, 1024) == 100   # not rounded
    assert w(70000, 4096) == 61440 and w(70000, 1000) == 64536
    assert w(65536, 65536) == 0 and w(65536, 1) == 65535
    assert w(-1, 1024) == -1 and w(100, 0) == -1 and w(100, 65537) == -1
    for ds in (0, 1, 3, 4, 63, 100, 4095, 65535, 70000, 2 ** 31 - 1):
        for ms in (1, 12, 1000, 1024, 65535, 65536):
            assert w(ds, ms) == hcdictmodel.window(ds, ms)


def test_scratch_size(product):
    f = product.compress_hc_cdict_scratch_size
    assert f(0, 1024) == 0 and f(-1, 1024) == 0 and f(-2 ** 31, 1024) == 0
    assert f(1, 0) == 0 and f(1, -1) == 0 and f(1, 65537) == 0
    for ms in (1, 5, 13, 255, 256, 257, 1000, 1024, 4096, 65535, 65536):
        assert f(1, ms) == slot(ms), ms
        assert f(7, ms) == 7 * slot(ms)
    assert f(1, 1024) == 6160                      # about 6 x maxSrcSize, not 393216
    assert f(1, 65536) == product.compress_hc_scratch_size(1) + 16
    sizes = [f(n, 1024) for n in (1, 2, 1000, 16384, 65536, 65537, 2 ** 31 - 1)]
    assert all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert f(16384, 1024) == 16384 * 6160
    assert f(2 ** 31 - 1, 1024) == f(65536, 1024)  # one pass: 262144 search workgroups
    assert f(2 ** 31 - 1, 65536) == 1024 * slot(65536)


def test_prepare_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_hc_cdict_prepare_dev
    size = product.hc_cdict_size()
    a = 16   # (never dereferenced: each call fails its argument check)
    assert f(None, 100, 1024, a, size, None) == EINVAL      # null dictionary of 100 bytes
    assert f(a, 100, 1024, None, size, None) == EINVAL      # null object
    assert f(a, -1, 1024, a, size, None) == EINVAL
    assert f(a, 100, 0, a, size, None) == EINVAL
    assert f(a, 100, 65537, a, size, None) == EINVAL
    assert f(a, 100, 1024, a, size - 1, None) == EINVAL
    assert f(a, 100, 1024, a, product.cdict_size(), None) == EINVAL   # the other kind's size
    assert f(a, 100, 1024, a, 0, None) == EINVAL
    for mis in (1, 4, 8):
        assert f(a, 100, 1024, a + mis, size, None) == EINVAL


def test_compress_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_compress_hc_usingCDict_batch_dev
    one = product.compress_hc_cdict_scratch_size(1, 1024)
    a = 16
    assert f(a, a, a, a, a, -1, a, 1024, 8, a, one, None) == EINVAL
    for hole in range(5):
        args = [a] * 5
        args[hole] = None
        assert f(*args, 1, a, 1024, 8, a, one, None) == EINVAL
    for depth in (-1, 257, 2 ** 31 - 1, -2 ** 31):
        assert f(a, a, a, a, a, 1, a, 1024, depth, a, one, None) == EINVAL
    for ms in (0, -1, 65537, 2 ** 31 - 1, -2 ** 31):
        assert f(a, a, a, a, a, 1, a, ms, 8, a, 1 << 30, None) == EINVAL
    assert f(a, a, a, a, a, 1, None, 1024, 8, a, one, None) == EINVAL      # the object
    assert f(a, a, a, a, a, 0, None, 1024, 8, a, one, None) == EINVAL
    for mis in (1, 4, 8):
        assert f(a, a, a, a, a, 1, a + mis, 1024, 8, a, one, None) == EINVAL
    assert f(a, a, a, a, a, 1, a, 1024, 8, None, one, None) == EINVAL      # the scratch
    assert f(a, a, a, a, a, 0, a, 1024, 8, None, one, None) == EINVAL
    for mis in (1, 4, 8):
        assert f(a, a, a, a, a, 1, a, 1024, 8, a + mis, one, None) == EINVAL
    assert f(a, a, a, a, a, 1, a, 1024, 8, a, one - 1, None) == EINVAL
    assert f(a, a, a, a, a, 1, a, 1024, 8, a, 0, None) == EINVAL
    assert f(a, a, a, a, a, 0, a, 1024, 8, a, one - 1, None) == EINVAL
    # the scratch of a smaller maxSrcSize does not do for a larger one
    assert f(a, a, a, a, a, 1, a, 4096, 8, a, one, None) == EINVAL


def test_valid_arguments_without_a_device_give_enodev(product):
    L = product.lib()
    if L.APE_LZ4_gpu_device_count() > 0:
        return   # (a GPU is visible here: tests/test_gpu_hc_cdict.py runs the calls)
    one = product.compress_hc_cdict_scratch_size(1, 1024)
    a = 16
    for depth in (0, 1, 64, 256):
        assert L.APE_LZ4_compress_hc_usingCDict_batch_dev(a, a, a, a, a, 3, a, 1024, depth, a,
                                                          one, None) == ENODEV
    assert L.APE_LZ4_hc_cdict_prepare_dev(a, 100, 1024, a, product.hc_cdict_size(), None) == ENODEV
    assert L.APE_LZ4_hc_cdict_prepare_dev(None, 0, 1024, a, product.hc_cdict_size(), None) == ENODEV


def test_binding_validates_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    obj = torch.zeros(product.hc_cdict_size(), dtype=torch.uint8)
    scr = torch.zeros(16, dtype=torch.uint8)
    good = [p, i, p, i, i, obj, 1024, 8, scr]
    for hole in (0, 1, 2, 3, 4, 5, 8):   # the sizes (1) are checked before their shape is read
        for bad in (None, [0, 0], 7):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                product.compress_hc_cdict_batch(*args)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_hc_cdict_batch(*good)
    with pytest.raises(ValueError):
        product.compress_hc_cdict_batch(p, i.to(torch.int64), p, i, i, obj, 1024, 8, scr)
    with pytest.raises(ValueError):
        product.compress_hc_cdict_batch(p, i[:1], p, i, i, obj, 1024, 8, scr)
    with pytest.raises(ValueError):
        product.compress_hc_cdict_batch(p, i, p, i, i, obj.to(torch.int16), 1024, 8, scr)
    with pytest.raises(ValueError):   # an object of the other kind's size
        product.compress_hc_cdict_batch(p, i, p, i, i, obj[:product.cdict_size()], 1024, 8, scr)
    with pytest.raises(ValueError):
        product.compress_hc_cdict_batch(p, i, p, i, i, obj, 1024, 8, scr.to(torch.int16))
    d = torch.zeros(100, dtype=torch.uint8)
    with pytest.raises(ValueError):   # CPU tensors
        product.hc_cdict_prepare(d, 1024, obj)
    with pytest.raises(ValueError):
        product.hc_cdict_prepare(d.to(torch.int32), 1024, obj)
    with pytest.raises(ValueError):
        product.hc_cdict_prepare(None, 1024, obj)
    with pytest.raises(ValueError):
        product.hc_cdict_prepare(d, 1024, obj.to(torch.int16))


def test_the_symbols_are_exported_and_declared(product):
    import os
    names = ("APE_LZ4_hc_cdict_size", "APE_LZ4_hc_cdict_window", "APE_LZ4_hc_cdict_prepare_dev",
             "APE_LZ4_compress_hc_usingCDict_scratch_size",
             "APE_LZ4_compress_hc_usingCDict_batch_dev")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ape_lz4_gpu.h")).read()
    for name in names:
        assert hasattr(product.lib(), name) and name + "(" in header, name
