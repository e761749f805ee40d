"""The calls of include/ape_lz4f_placed.h: what can be checked without a GPU -- the argument
checks that precede every device call, each rejection with the call's own name in
APE_LZ4_gpu_last_error(), the scratch-size function, the binding's checks, and the ctypes
signatures against the header's prototypes (tests/test_gpu_decode_size.py and
tests/test_gpu_lz4f_placed.py have the rest)."""
import ctypes as C
import os

import pytest

import cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ape_lz4f_placed.h")
OK, ENODEV, EINVAL = 0, -1, -2
A = 4096        # a pointer that is never dereferenced: each call ends at a check
BIG = 1 << 40
SIZER, PLACED = "decompress_safe_size_batch_dev", "lz4f_decompress_placed_batch_dev"
DEV = (SIZER, PLACED)
SIZES = ("lz4f_decompress_placed_scratch_size",)
NEVER = (1 << 64) - 1


def _f(product, name):
    return getattr(product.lib(), "APE_LZ4_" + name)


def _rejected(product, name, args):
    assert _f(product, name)(*args) == EINVAL, (name, args)
    assert product.gpu_last_error().startswith(name + ":"), (name, product.gpu_last_error())


def _valid(name, count=1):
    """(a valid argument list, the positions of its required arrays, the position of the count)."""
    if name == SIZER:
        return [A, A, A, A, A, count, None], (0, 1, 2, 4), 5
    return [A, A, A, A, A, count, 4, 3, A, BIG, None], (0, 1, 2, 3, 4, 8), 5


def _prototypes():
    return cheader.prototypes(HEADER)


def test_the_header_declares_the_three_and_the_binding_agrees(product):
    protos = _prototypes()
    assert sorted(protos) == sorted("APE_LZ4_" + n for n in DEV + SIZES)
    for name, (ret, nparams) in protos.items():
        f = getattr(product.lib(), name)
        assert f.argtypes is not None and len(f.argtypes) == nparams, name
        if name[len("APE_LZ4_"):] in SIZES:
            assert ret.split()[-1] == "size_t" and f.restype is C.c_size_t, name
        else:
            assert ret.split()[-1] == "int" and f.restype is C.c_int, name
    # a stand-alone header: it includes the frame header, and no header includes it
    assert '#include "ape_lz4f.h"' in open(HEADER).read()
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ape_lz4f_placed.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert "placed" not in text and "safe_size" not in text, other
    for name in ("decompress_size_ptr_batch", "lz4f_decompress_placed_scratch_size",
                 "lz4f_decompress_placed_batch"):
        assert callable(getattr(product, name))
        assert name not in product.__all__


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


def test_the_sizer_takes_a_null_dictionary_size_array(product):
    args, _, _ = _valid(SIZER)
    args[3] = None
    assert _f(product, SIZER)(*args) != EINVAL


def test_the_placed_decode_rejects_its_other_arguments(product):
    name = PLACED
    good, _, _ = _valid(name, 3)
    need = product.lz4f_decompress_placed_scratch_size(3, 4)
    for at, values in ((6, (0, -1, -2 ** 31)), (7, (4, -1, 2 ** 31 - 1)),
                       (8, (A + 1, A + 4, A + 8)), (9, (0, need - 1))):
        for v in values:
            bad = list(good)
            bad[at] = v
            _rejected(product, name, bad)
    ok = list(good)
    ok[9] = need
    assert _f(product, name)(*ok) != EINVAL
    # the existing call's scratch is too short for this one
    bad = list(good)
    bad[9] = product.lz4f_decompress_scratch_size(3, 4)
    _rejected(product, name, bad)
    bad = list(good)
    bad[5], bad[6] = 1 << 12, 1 << 12     # 2^24 block slots
    _rejected(product, name, bad)
    for at, v in ((6, 0), (7, 4)):        # an empty batch still has to make sense
        bad, _, _ = _valid(name, 0)
        bad[at] = v
        _rejected(product, name, bad)


def test_a_rejection_never_leaves_another_calls_message(product):
    for first, second in ((SIZER, PLACED), (PLACED, SIZER),
                          ("lz4f_decompress_batch_dev", PLACED)):
        for name in (first, second):
            bad = [None, A, A, A, A, 1, None] if name == SIZER else \
                [None, A, A, A, A, 1, 4, 0, A, BIG, None]
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
        if name == PLACED:
            nulls[9] = 0
        else:
            nulls[3] = None
        if device:
            assert _f(product, name)(*empty) == OK, name
            assert _f(product, name)(*nulls) == OK, name
            continue
        for args in (_valid(name)[0], _valid(name, 3)[0], empty, nulls):
            assert _f(product, name)(*args) == ENODEV, (name, args)
            assert "no HIP device" in product.gpu_last_error()


def _up16(x):
    return (x + 15) // 16 * 16


def test_the_scratch_size(product):
    ps, ds = product.lz4f_decompress_placed_scratch_size, product.lz4f_decompress_scratch_size
    for nframes, max_blocks in ((1, 1), (7, 3), (16, 256), (3, 40)):
        slots = nframes * max_blocks
        want = 16 + _up16(32 * nframes) + 5 * _up16(8 * slots) + 14 * _up16(4 * slots) + \
            _up16(4 * nframes)
        assert ps(nframes, max_blocks) == want, (nframes, max_blocks)
        # the existing call's regions first, then two ints per slot and one per frame
        assert want == ds(nframes, max_blocks) + 2 * _up16(4 * slots) + _up16(4 * nframes)
    assert ps(16, 256) == 16 * 256 * 96 + 16 * 36 + 16
    for args in ((-1, 4), (1, 0), (1, -1), (-2 ** 31, 1)):
        assert ps(*args) == 0, args
    assert ps(0, 1) == 16 and ps((1 << 24) - 1, 1) < NEVER
    assert ps(1 << 24, 1) == NEVER and ps(1 << 12, 1 << 12) == NEVER


def test_the_bindings_validate_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    scr = torch.zeros(16, dtype=torch.uint8)
    calls = [(product.lz4f_decompress_placed_batch, [p, i, p, i, i, 4, 0, scr], (0, 1, 2, 3, 4, 7)),
             (product.decompress_size_ptr_batch, [p, i, i, i], (0, 1, 2, 3)),
             (product.decompress_size_ptr_batch, [p, i, i, i, i], (0, 1, 2, 3, 4))]
    for f, good, tensors in calls:
        with pytest.raises(ValueError):            # CPU tensors
            f(*good)
        for hole in tensors:
            for bad in (None, [0, 0], 7):
                if bad is None and len(good) == 5 and hole == 4:
                    continue                       # dict_sizes may be None
                args = list(good)
                args[hole] = bad
                with pytest.raises(ValueError):
                    f(*args)
        for hole, bad in ((0, p.to(torch.int32)), (0, p[:1]), (1, i.to(torch.int64))):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                f(*args)
    with pytest.raises(ValueError):                # dict_sizes: int32, one per block
        product.decompress_size_ptr_batch(p, i, i, i, dict_sizes=p)
    with pytest.raises(ValueError):
        product.decompress_size_ptr_batch(p, i, i, i, dict_sizes=i[:1])
