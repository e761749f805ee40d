"""Dictionary training: what can be checked without a GPU -- the exported symbols, the scratch
arithmetic, and the argument checks that precede every device call, in C and in the binding
(tests/test_gpu_dict_train.py has the rest)."""
import os

import pytest

import dicttrainmodel as M

EINVAL = -2
ENODEV = -1
TABLE = 4 << 20          # 2^20 u32 counts
MAX_SAMPLE = 0x7E000000


def scratch(nsamples, max_sample, segment):
    """The table, 16 bytes of state, and a 16-byte partial per score workgroup: one workgroup per
    four slots, at least 1 and at most 1024."""
    slots = M.geometry(nsamples, segment, segment, max_sample)[2]
    return TABLE + 16 + 16 * min(1024, max(1, (slots + 3) // 4))


def test_the_symbols_are_exported_and_declared(product):
    """The family has a header of its own, which include/ape_lz4_gpu.h includes; the binding's
    ctypes signatures agree with its prototypes."""
    import ctypes as C
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gpu = open(os.path.join(root, "include", "ape_lz4_gpu.h")).read()
    assert '#include "ape_lz4_dict_train.h"' in gpu
    header = open(os.path.join(root, "include", "ape_lz4_dict_train.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"APE_LZ4_dict_train_scratch_size": ("size_t", 3), "APE_LZ4_dict_train_dev": ("int", 11)}
    for name, (ret, nparams) in want.items():
        m = re.search(r"(\w+)\s+%s\s*\(([^()]*)\)\s*;" % name, header)
        assert m and m.group(1) == ret and m.group(2).count(",") + 1 == nparams, name
        f = getattr(product.lib(), name)
        assert len(f.argtypes) == nparams, name
        assert f.restype is (C.c_int if ret == "int" else C.c_size_t), name
    dev = product.lib().APE_LZ4_dict_train_dev
    assert {k for k, t in enumerate(dev.argtypes) if t is C.c_void_p} == {0, 1, 4, 7, 9, 10}
    assert "dict_train" in product.__all__ and "dict_train_scratch_size" in product.__all__


def test_the_model_restates_the_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "libapenetwork_amd", "csrc", "lz4_gpu_internal.h")).read()
    assert "kDtSub = %d;" % M.D in text and "kDtBits = %d;" % M.F in text
    assert "kDtPrime = 0x%Xull" % M.PRIME in text


def test_scratch_size(product):
    f = product.dict_train_scratch_size
    assert f(0, 1024, 64) == TABLE + 32
    assert f(1, 8, 16) == TABLE + 32              # two slots, one workgroup
    assert f(1, 64, 16) == TABLE + 16 + 16 * 4    # 16 slots
    assert f(512, 1024, 64) == f(16384, 4096, 256) == TABLE + 16 + 16 * 1024
    for n in (0, 1, 3, 64, 4097):
        for ms in (8, 9, 100, 1024, 65536):
            for k in (16, 32, 48, 1024):
                assert f(n, ms, k) == scratch(n, ms, k), (n, ms, k)
                assert f(n, ms, k) % 16 == 0
    assert f(1, MAX_SAMPLE, 1024) == scratch(1, MAX_SAMPLE, 1024)
    assert f((2 ** 31 - 1) // 8, 8, 16) == TABLE + 16 + 16 * 1024
    # out of range: the count, the sample bound, the segment, the product
    assert f(-1, 1024, 64) == 0 and f(-2 ** 31, 1024, 64) == 0
    assert f(1, 7, 64) == 0 and f(1, 0, 64) == 0 and f(1, -1, 64) == 0
    assert f(1, MAX_SAMPLE + 1, 64) == 0 and f(1, 2 ** 31 - 1, 64) == 0
    for k in (0, -16, 8, 15, 17, 24, 1000, 1040, 2048, 2 ** 31 - 1):
        assert f(1, 1024, k) == 0, k
    assert f(2 ** 21, 1024, 64) == 0              # 2^31
    assert f(2 ** 21 - 1, 1024, 64) != 0
    assert f(2, MAX_SAMPLE, 64) == 0


def test_rejects_bad_arguments_before_any_device_call(product):
    f = product.lib().APE_LZ4_dict_train_dev
    need = product.dict_train_scratch_size(4, 1024, 64)
    a = 16   # (never dereferenced: each call fails its argument check)

    def call(samples=a, sizes=a, n=4, ms=1024, d=a, cap=4096, k=64, scr=a, nbytes=need, info=a):
        return f(samples, sizes, n, ms, d, cap, k, scr, nbytes, info, None)

    assert call(samples=None) == EINVAL and call(sizes=None) == EINVAL
    assert call(d=None) == EINVAL and call(info=None) == EINVAL
    assert call(d=None, n=0) == EINVAL and call(info=None, n=0) == EINVAL
    assert call(n=-1) == EINVAL and call(n=-2 ** 31) == EINVAL
    for ms in (7, 0, -1, MAX_SAMPLE + 1, 2 ** 31 - 1, -2 ** 31):
        assert call(ms=ms, nbytes=1 << 30) == EINVAL, ms
    for k in (0, -16, 8, 15, 17, 24, 1000, 1040, 2048):
        assert call(k=k, cap=65536, nbytes=1 << 30) == EINVAL, k
    for cap in (63, 0, -1, 65537, 2 ** 31 - 1, -2 ** 31):
        assert call(cap=cap) == EINVAL, cap
    assert call(n=2 ** 21, nbytes=1 << 30) == EINVAL                 # nsamples * maxSampleSize = 2^31
    assert call(n=2, ms=MAX_SAMPLE, nbytes=1 << 30) == EINVAL
    assert call(scr=None) == EINVAL and call(scr=None, n=0) == EINVAL
    for mis in (1, 4, 8):
        assert call(scr=a + mis) == EINVAL
    assert call(nbytes=need - 1) == EINVAL and call(nbytes=0) == EINVAL
    assert call(n=0, nbytes=product.dict_train_scratch_size(0, 1024, 64) - 1) == EINVAL
    # the scratch of fewer samples does not do for more
    assert call(n=64, nbytes=need) == EINVAL
    # every rejection leaves the call's own message, not an earlier call's
    for bad in (dict(samples=None), dict(sizes=None), dict(d=None), dict(info=None),
                dict(scr=None), dict(n=-1), dict(k=24), dict(cap=63), dict(nbytes=0)):
        assert product.lib().APE_LZ4_compress_batch_dev(None, a, a, a, a, 1, None) == EINVAL
        assert call(**bad) == EINVAL
        assert product.gpu_last_error().startswith("dict_train_dev:"), bad


def test_valid_arguments_without_a_device_give_enodev(product):
    L = product.lib()
    if L.APE_LZ4_gpu_device_count() > 0:
        return   # (a GPU is visible here: tests/test_gpu_dict_train.py runs the calls)
    a = 16
    for n, ms, cap, k in ((4, 1024, 4096, 64), (1, 8, 16, 16), (3, 2048, 65536, 1024),
                          (16384, 4096, 61440, 256)):
        need = product.dict_train_scratch_size(n, ms, k)
        assert L.APE_LZ4_dict_train_dev(a, a, n, ms, a, cap, k, a, need, a, None) == ENODEV
    need = product.dict_train_scratch_size(0, 1024, 64)
    assert L.APE_LZ4_dict_train_dev(None, None, 0, 1024, a, 4096, 64, a, need, a, None) == ENODEV


def test_binding_validates_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    d = torch.zeros(4096, dtype=torch.uint8)
    scr = torch.zeros(16, dtype=torch.uint8)
    info = torch.zeros(4, dtype=torch.int32)
    good = [p, i, 1024, d, 64, scr, info]
    for hole in (0, 1, 3, 5, 6):
        for bad in (None, [0, 0], 7):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                product.dict_train(*args)
    with pytest.raises(ValueError):   # CPU tensors
        product.dict_train(*good)
    with pytest.raises(ValueError):
        product.dict_train(p.to(torch.int32), i, 1024, d, 64, scr, info)
    with pytest.raises(ValueError):
        product.dict_train(p, i.to(torch.int64), 1024, d, 64, scr, info)
    with pytest.raises(ValueError):
        product.dict_train(p, i[:1], 1024, d, 64, scr, info)
    with pytest.raises(ValueError):
        product.dict_train(p, i, 1024, d.to(torch.int16), 64, scr, info)
    with pytest.raises(ValueError):
        product.dict_train(p, i, 1024, d, 64, scr.to(torch.int16), info)
    with pytest.raises(ValueError):
        product.dict_train(p, i, 1024, d, 64, scr, info[:3])
    with pytest.raises(ValueError):
        product.dict_train(p, i, 1024, d, 64, scr, info.to(torch.int64))
