"""The LZ4 frame calls (include/ape_lz4f.h): what can be checked without a GPU -- the argument
checks that precede every device call, each rejection with the call's own name in
APE_LZ4_gpu_last_error(), the size functions, the binding's checks, and the ctypes signatures
against the prototypes of the new header (tests/test_gpu_xxh32.py and tests/test_gpu_lz4f.py
have the rest)."""
import ctypes as C
import os

import pytest

import cheader
import lz4fmodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENODEV, EINVAL = 0, -1, -2
A = 4096        # a pointer that is never dereferenced: each call ends at a check
BIG = 1 << 40
FIVE = [A, A, A, A, A]
DEV = ("xxh32_batch_dev", "lz4f_compress_batch_dev", "lz4f_info_batch_dev",
       "lz4f_decompress_batch_dev")
SIZES = ("lz4f_compress_bound", "lz4f_compress_scratch_size", "lz4f_decompress_scratch_size")
MAX_SRC = 0x7E000000
NEVER = (1 << 64) - 1


def _f(product, name):
    return getattr(product.lib(), "APE_LZ4_" + name)


def _rejected(product, name, args):
    assert _f(product, name)(*args) == EINVAL, (name, args)
    assert product.gpu_last_error().startswith(name + ":"), (name, product.gpu_last_error())


def _valid(name, count=1):
    """(a valid argument list, the positions of its arrays, the position of the count)."""
    if name == DEV[0]:
        return [A, A, 0, A, count, None], (0, 1, 3), 4
    if name == DEV[2]:
        return [A, A, A, count, None], (0, 1, 2), 3
    limit, flags = (65536, 7) if name == DEV[1] else (4, 3)
    return FIVE + [count, limit, flags, A, BIG, None], (0, 1, 2, 3, 4, 8), 5


def _prototypes():
    return cheader.prototypes(os.path.join(ROOT, "include", "ape_lz4f.h"))


def test_the_header_declares_the_seven_and_the_binding_agrees(product):
    protos = _prototypes()
    assert sorted(protos) == sorted("APE_LZ4_" + n for n in DEV + SIZES)
    for name, (ret, nparams) in protos.items():
        f = getattr(product.lib(), name)
        assert f.argtypes is not None and len(f.argtypes) == nparams, name
        if name[len("APE_LZ4_"):] in SIZES:
            assert ret.split()[-1] == "size_t" and f.restype is C.c_size_t, name
        else:
            assert ret.split()[-1] == "int" and f.restype is C.c_int, name
    # a stand-alone header: it includes the main one, which does not know it
    mine = open(os.path.join(ROOT, "include", "ape_lz4f.h")).read()
    assert '#include "ape_lz4_gpu.h"' in mine
    gpu = open(os.path.join(ROOT, "include", "ape_lz4_gpu.h")).read()
    assert "lz4f" not in gpu and "xxh32" not in gpu
    for name in ("xxh32_batch", "lz4f_compress_bound", "lz4f_compress_scratch_size",
                 "lz4f_compress_batch", "lz4f_info_batch", "lz4f_decompress_scratch_size",
                 "lz4f_decompress_batch"):
        assert callable(getattr(product, name))


@pytest.mark.parametrize("name", DEV)
def test_a_null_array_or_a_negative_count_is_rejected(product, name):
    good, arrays, count_at = _valid(name)
    for hole in arrays:
        bad = list(good)
        bad[hole] = None
        _rejected(product, name, bad)
    for n in (-1, -2 ** 31):
        bad = list(good)
        bad[count_at] = n
        _rejected(product, name, bad)


def test_compress_rejects_its_other_arguments(product):
    name = DEV[1]
    good, _, _ = _valid(name, 3)
    need = product.lz4f_compress_scratch_size(3, 65536)
    for at, values in ((6, (-1, MAX_SRC + 1, 2 ** 31 - 1, -2 ** 31)), (7, (8, -1, 16, 2 ** 31 - 1)),
                       (8, (A + 1, A + 4, A + 8)), (9, (0, need - 1))):
        for v in values:
            bad = list(good)
            bad[at] = v
            _rejected(product, name, bad)
    ok = list(good)
    ok[9] = need
    assert _f(product, name)(*ok) != EINVAL
    # 2^24 block slots or more are too many for one call, whatever the scratch
    bad = list(good)
    bad[5], bad[6] = 1 << 12, 1 << 28
    _rejected(product, name, bad)
    # an empty batch still has to make sense, but needs no scratch
    for at, v in ((6, -1), (6, MAX_SRC + 1), (7, 8)):
        bad, _, _ = _valid(name, 0)
        bad[at] = v
        _rejected(product, name, bad)


def test_decompress_rejects_its_other_arguments(product):
    name = DEV[3]
    good, _, _ = _valid(name, 3)
    need = product.lz4f_decompress_scratch_size(3, 4)
    for at, values in ((6, (0, -1, -2 ** 31)), (7, (4, -1, 2 ** 31 - 1)),
                       (8, (A + 1, A + 4, A + 8)), (9, (0, need - 1))):
        for v in values:
            bad = list(good)
            bad[at] = v
            _rejected(product, name, bad)
    ok = list(good)
    ok[9] = need
    assert _f(product, name)(*ok) != EINVAL
    bad = list(good)
    bad[5], bad[6] = 1 << 12, 1 << 12
    _rejected(product, name, bad)
    for at, v in ((6, 0), (7, 4)):
        bad, _, _ = _valid(name, 0)
        bad[at] = v
        _rejected(product, name, bad)


def test_a_rejection_never_leaves_another_calls_message(product):
    for first, second in zip(DEV, DEV[1:] + DEV[:1]):
        for name in (first, second):
            bad, arrays, _ = _valid(name)
            bad[arrays[0]] = None
            _rejected(product, name, bad)
        assert not product.gpu_last_error().startswith(first + ":"), (first, second)


def test_valid_arguments_reach_the_device_check(product):
    """Without a device they end at ENODEV, an empty batch too (arguments, then device); with
    one, an empty batch launches nothing and returns 0, null arrays and scratch included."""
    device = product.lib().APE_LZ4_gpu_device_count() > 0
    for name in DEV:
        empty, arrays, _ = _valid(name, 0)
        nulls = list(empty)
        for at in arrays:
            nulls[at] = None
        if name in (DEV[1], DEV[3]):
            nulls[9] = 0
        if device:
            assert _f(product, name)(*empty) == OK, name
            assert _f(product, name)(*nulls) == OK, name
            continue
        for args in (_valid(name)[0], _valid(name, 3)[0], empty, nulls):
            assert _f(product, name)(*args) == ENODEV, (name, args)
            assert "no HIP device" in product.gpu_last_error()


def test_compress_bound_is_the_all_stored_frame(product):
    for n in (0, 1, 65535, 65536, 65537, 3 * 65536 + 100):
        data = bytes(n)
        for flags in range(8):
            bound = product.lz4f_compress_bound(n, flags)
            assert bound == len(M.compress(data, flags, all_stored=True)), (n, flags)
            assert bound == M.compress_bound(n, flags)
    assert product.lz4f_compress_bound(MAX_SRC, 7) == M.compress_bound(MAX_SRC, 7) < 1 << 31
    for n, flags in ((-1, 0), (MAX_SRC + 1, 0), (-2 ** 31, 7), (100, 8), (100, -1)):
        assert product.lz4f_compress_bound(n, flags) == 0 == M.compress_bound(n, flags)


def _up16(x):
    return (x + 15) // 16 * 16


def test_the_scratch_sizes(product):
    cs, ds = product.lz4f_compress_scratch_size, product.lz4f_decompress_scratch_size
    for nframes, max_src in ((1, 1), (1, 65536), (1, 65537), (7, 3 * 65536 + 100), (3, 0)):
        slots = nframes * max(1, (max_src + 65535) // 65536)
        want = slots * 65536 + 2 * _up16(8 * slots) + 5 * _up16(4 * slots) + 2 * _up16(4 * nframes)
        assert cs(nframes, max_src) == want, (nframes, max_src)
    for nframes, max_blocks in ((1, 1), (7, 3), (16, 256)):
        slots = nframes * max_blocks
        want = 16 + _up16(32 * nframes) + 5 * _up16(8 * slots) + 12 * _up16(4 * slots)
        assert ds(nframes, max_blocks) == want, (nframes, max_blocks)
    assert cs(0, 65536) == 0 and cs(16384, 65536) == 16384 * (65536 + 36 + 8)
    # out of range: 0; too many block slots for one call: (size_t)-1
    for args in ((-1, 65536), (1, -1), (1, MAX_SRC + 1)):
        assert cs(*args) == 0, args
    for args in ((-1, 4), (1, 0), (1, -1)):
        assert ds(*args) == 0, args
    assert cs(1, MAX_SRC) < NEVER and cs((1 << 24) - 1, 65536) < NEVER
    assert cs(1 << 24, 65536) == NEVER and cs(1 << 12, 1 << 28) == NEVER
    assert ds((1 << 24) - 1, 1) < NEVER
    assert ds(1 << 24, 1) == NEVER and ds(1 << 12, 1 << 12) == NEVER


def test_the_bindings_validate_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    scr = torch.zeros(16, dtype=torch.uint8)
    calls = [(product.lz4f_compress_batch, [p, i, p, i, i, 65536, 0, scr], (0, 1, 2, 3, 4, 7)),
             (product.lz4f_decompress_batch, [p, i, p, i, i, 4, 0, scr], (0, 1, 2, 3, 4, 7)),
             (product.xxh32_batch, [p, i, i], (0, 1, 2)),
             (product.lz4f_info_batch, [p, i, torch.zeros(16, dtype=torch.int32)], (0, 1, 2))]
    for f, good, tensors in calls:
        with pytest.raises(ValueError):            # CPU tensors
            f(*good)
        for hole in tensors:
            for bad in (None, [0, 0], 7):
                args = list(good)
                args[hole] = bad
                with pytest.raises(ValueError):
                    f(*args)
        for hole, bad in ((0, p.to(torch.int32)), (0, p[:1]), (1, i.to(torch.int64))):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                f(*args)
    for seed in (-1, 1 << 32, 1.5, None):
        with pytest.raises(ValueError):
            product.xxh32_batch(p, i, i, seed=seed)
    with pytest.raises(ValueError):                # info: 8 ints per frame
        product.lz4f_info_batch(p, i, torch.zeros(15, dtype=torch.int32))
