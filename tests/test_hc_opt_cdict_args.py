"""The cost-minimising parse against a prepared dictionary: what can be checked without a GPU --
the scratch arithmetic and the argument checks that precede every device call, in C and in the
bindings (tests/test_gpu_hc_opt_cdict.py has the rest)."""
import pytest

EINVAL = -2
ENODEV = -1


def slot(max_src):
    """The lazy call's slot -- chain (u16) for maxSrcSize + 3 window positions and match (u32)
    per message position -- plus cost (u32) per message position, each rounded up to 16 bytes."""
    r16 = lambda x: (x + 15) // 16 * 16
    return r16(2 * (max_src + 3)) + 2 * r16(4 * max_src)


def test_scratch_size(product):
    f, lazy = product.compress_hc_opt_cdict_scratch_size, product.compress_hc_cdict_scratch_size
    assert f(0, 1024) == 0 and f(-1, 1024) == 0 and f(-2 ** 31, 1024) == 0
    assert f(1, 0) == 0 and f(1, -1) == 0 and f(1, 65537) == 0 and f(1, -2 ** 31) == 0
    for ms in (1, 5, 13, 255, 256, 257, 1000, 1024, 4096, 65535, 65536):
        assert f(1, ms) == slot(ms), ms
        assert f(7, ms) == 7 * slot(ms)
        assert f(7, ms) - lazy(7, ms) == 7 * ((4 * ms + 15) // 16 * 16)
    assert f(1, 1024) == 6160 + 4096 == 10256          # about 10 x maxSrcSize, not 655360
    assert f(1, 65536) == product.compress_hc_opt_scratch_size(1) + 16
    sizes = [f(n, 1024) for n in (1, 2, 1000, 16384, 65536, 65537, 2 ** 31 - 1)]
    assert all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert f(16384, 1024) == 16384 * 10256
    # the pass cap is the lazy call's: 262144 / ceil(maxSrcSize / 256) messages
    for ms, cap in ((1, 262144), (256, 262144), (257, 131072), (1000, 65536), (1024, 65536),
                    (4096, 16384), (65536, 1024)):
        assert f(2 ** 31 - 1, ms) == f(cap, ms) == cap * slot(ms), ms
        assert f(cap - 1, ms) == (cap - 1) * slot(ms)
        assert lazy(2 ** 31 - 1, ms) == lazy(cap, ms)


def test_compress_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_compress_hc_opt_usingCDict_batch_dev
    one = product.compress_hc_opt_cdict_scratch_size(1, 1024)
    a = 16   # (never dereferenced: each call fails its argument check)
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
    assert str(one) in product.gpu_last_error() and "compress_hc_opt_usingCDict" in product.gpu_last_error()
    assert f(a, a, a, a, a, 1, a, 1024, 8, a, 0, None) == EINVAL
    assert f(a, a, a, a, a, 0, a, 1024, 8, a, one - 1, None) == EINVAL
    # the lazy call's scratch is too small for this one, and so is a smaller maxSrcSize's
    assert f(a, a, a, a, a, 1, a, 1024, 8, a, product.compress_hc_cdict_scratch_size(1, 1024),
             None) == EINVAL
    assert f(a, a, a, a, a, 1, a, 4096, 8, a, one, None) == EINVAL


def test_valid_arguments_reach_the_device_check(product):
    """Without a device they give ENODEV; with one, an empty batch launches nothing and gives 0
    (tests/test_gpu_hc_opt_cdict.py runs the others)."""
    L = product.lib()
    f = L.APE_LZ4_compress_hc_opt_usingCDict_batch_dev
    one = product.compress_hc_opt_cdict_scratch_size(1, 1024)
    a = 16
    if L.APE_LZ4_gpu_device_count() > 0:
        assert f(a, a, a, a, a, 0, a, 1024, 8, a, one, None) == 0
        assert f(None, None, None, None, None, 0, a, 1024, 0, a, one, None) == 0
        return
    for depth in (0, 1, 64, 256):
        assert f(a, a, a, a, a, 3, a, 1024, depth, a, one, None) == ENODEV
    assert f(None, None, None, None, None, 0, a, 1024, 8, a, one, None) == ENODEV


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
                product.compress_hc_opt_cdict_batch(*args)
    with pytest.raises(ValueError):   # CPU tensors
        product.compress_hc_opt_cdict_batch(*good)
    with pytest.raises(ValueError):
        product.compress_hc_opt_cdict_batch(p, i.to(torch.int64), p, i, i, obj, 1024, 8, scr)
    with pytest.raises(ValueError):
        product.compress_hc_opt_cdict_batch(p, i[:1], p, i, i, obj, 1024, 8, scr)
    with pytest.raises(ValueError):   # an object of the other kind's size
        product.compress_hc_opt_cdict_batch(p, i, p, i, i, obj[:product.cdict_size()], 1024, 8, scr)
    with pytest.raises(ValueError):
        product.compress_hc_opt_cdict_batch(p, i, p, i, i, obj, 1024, 8, scr.to(torch.int16))


def test_the_symbols_are_exported_and_declared(product):
    import os
    names = ("APE_LZ4_compress_hc_opt_usingCDict_scratch_size",
             "APE_LZ4_compress_hc_opt_usingCDict_batch_dev")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ape_lz4_gpu.h")).read()
    for name in names:
        assert hasattr(product.lib(), name) and name + "(" in header, name
    for name in ("compress_hc_opt_cdict_scratch_size", "compress_hc_opt_cdict_batch"):
        assert name in product.__all__ and callable(getattr(product, name))
