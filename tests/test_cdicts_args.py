"""A prepared dictionary per message (include/ape_lz4_cdicts.h): what can be
checked without a GPU -- the argument checks that precede every device call of the five entry
points, each rejection with the call's own name in APE_LZ4_gpu_last_error(), the binding's
checks, and the ctypes signatures against the prototypes of the new header
(tests/test_gpu_cdicts.py has the rest)."""
import ctypes as C
import os
import re

import pytest

import cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENODEV, EINVAL = 0, -1, -2
A = 4096        # a pointer that is never dereferenced: each call ends at a check
BIG = 1 << 40
FIVE = [A, A, A, A, A]
PREPARES = ("cdict_prepare_batch_dev", "hc_cdict_prepare_batch_dev")
HC = ("compress_hc_usingCDicts_batch_dev", "compress_hc_opt_usingCDicts_batch_dev")
FAST = "compress_usingCDicts_batch_dev"
NAMES = PREPARES + (FAST,) + HC


def _f(product, name):
    return getattr(product.lib(), "APE_LZ4_" + name)


def _rejected(product, name, args):
    assert _f(product, name)(*args) == EINVAL, (name, args)
    assert product.gpu_last_error().startswith(name + ":"), (name, product.gpu_last_error())


def _object_size(product, name):
    return product.cdict_size() if name == PREPARES[0] else product.hc_cdict_size()


def _scratch(product, name, max_src=4096):
    f = (product.compress_hc_cdict_scratch_size if name == HC[0]
         else product.compress_hc_opt_cdict_scratch_size)
    return f(1, max_src)


def _valid(product, name, count=1):
    if name in PREPARES:
        return [A, A, 4096, A, _object_size(product, name), count, None]
    if name == FAST:
        return FIVE + [count, A, None]
    return FIVE + [count, A, 4096, 8, A, _scratch(product, name), None]


def _prototypes():
    return cheader.prototypes(os.path.join(ROOT, "include", "ape_lz4_cdicts.h"))


def test_the_header_declares_the_five_and_the_binding_agrees(product):
    protos = _prototypes()
    assert sorted(protos) == sorted("APE_LZ4_" + n for n in NAMES)
    for name, (ret, nparams) in protos.items():
        f = getattr(product.lib(), name)
        assert f.argtypes is not None and len(f.argtypes) == nparams, name
        # (the expression runs on from the preprocessor line before the first prototype)
        assert ret.split()[-1] == "int" and f.restype is C.c_int, name
    # the main header gains the include at its end and no prototype
    gpu = open(os.path.join(ROOT, "include", "ape_lz4_gpu.h")).read()
    assert gpu.rstrip().endswith('#include "ape_lz4_cdicts.h"')
    code = re.sub(r"/\*.*?\*/", "", gpu, flags=re.S)
    assert "CDicts" not in code and "prepare_batch" not in code
    for name in ("cdict_prepare_batch", "hc_cdict_prepare_batch", "compress_cdicts_batch",
                 "compress_hc_cdicts_batch", "compress_hc_opt_cdicts_batch"):
        assert callable(getattr(product, name))


@pytest.mark.parametrize("name", PREPARES)
def test_prepare_batch_rejects_bad_arguments_before_any_device_call(product, name):
    size = _object_size(product, name)
    good = _valid(product, name, 3)
    good[4] = size + 64
    for hole in (0, 1, 3):                        # a null array, null objects
        bad = list(good)
        bad[hole] = None
        _rejected(product, name, bad)
    for at, values in ((5, (-1, -2 ** 31)), (2, (0, -1, 65537, 2 ** 31 - 1, -2 ** 31)),
                       (3, (A + 1, A + 4, A + 8)),
                       (4, (0, 16, size - 16, size - 1, size + 1, size + 8, size + 24))):
        for v in values:
            bad = list(good)
            bad[at] = v
            _rejected(product, name, bad)
    # the other kind's size is this kind's only where it is large enough
    other = product.hc_cdict_size() if name == PREPARES[0] else product.cdict_size()
    bad = list(good)
    bad[4] = other
    if other < size:
        _rejected(product, name, bad)
    # an empty batch still has to make sense
    for at, v in ((2, 0), (2, 65537), (4, size - 16), (4, size + 8), (3, A + 8)):
        bad = _valid(product, name, 0)
        bad[at] = v
        _rejected(product, name, bad)


def test_stride_rules(product):
    """Any multiple of 16 from the object's size on; nothing else.  On an empty batch, which
    checks the stride all the same and launches nothing where there is a device: the pointers
    here are not memory."""
    for name in PREPARES:
        size = _object_size(product, name)
        assert size % 16 == 0
        for stride, ok in ((size, True), (size + 16, True), (size + 64, True), (2 * size, True),
                           (BIG, True), (size - 16, False), (size + 1, False), (size + 15, False),
                           (size + 17, False), (0, False)):
            args = _valid(product, name, 0)
            args[4] = stride
            rc = _f(product, name)(*args)
            assert (rc != EINVAL) == ok, (name, stride, rc)
            assert ok or product.gpu_last_error().startswith(name + ":")


@pytest.mark.parametrize("name", (FAST,) + HC)
def test_compress_rejects_bad_arguments_before_any_device_call(product, name):
    good = _valid(product, name)
    for hole in range(5):
        bad = list(good)
        bad[hole] = None
        _rejected(product, name, bad)
    bad = list(good)
    bad[6] = None                                 # the array of objects, with a message to compress
    _rejected(product, name, bad)
    for n in (-1, -2 ** 31):
        bad = list(good)
        bad[5] = n
        _rejected(product, name, bad)
    if name == FAST:
        return
    one = _scratch(product, name)
    for at, values in ((7, (0, -1, 65537, 2 ** 31 - 1, -2 ** 31)), (8, (-1, 257, 2 ** 31 - 1)),
                       (9, (None, A + 1, A + 4, A + 8)), (10, (0, one - 1))):
        for v in values:
            bad = list(good)
            bad[at] = v
            if at == 7:
                bad[10] = BIG
            _rejected(product, name, bad)
    # the scratch has to hold one message whatever nblocks is, and the lazy call's is too small
    # for the cost-minimising one
    bad = _valid(product, name, 0)
    bad[10] = one - 1
    _rejected(product, name, bad)
    if name == HC[1]:
        bad = list(good)
        bad[10] = _scratch(product, HC[0])
        _rejected(product, name, bad)
        assert str(one) in product.gpu_last_error()


def test_a_rejection_never_leaves_another_calls_message(product):
    for first, second in zip(NAMES, NAMES[1:] + NAMES[:1]):
        for name in (first, second):
            bad = _valid(product, name)
            bad[0] = None
            _rejected(product, name, bad)
        # (one name ends another: a message is its call's when it starts with the name)
        assert not product.gpu_last_error().startswith(first + ":"), (first, second)


def test_valid_arguments_reach_the_device_check(product):
    """Without a device they end at ENODEV, an empty batch too (arguments, then device, as every
    launcher); with one, an empty batch launches nothing and returns 0, null arrays included
    (tests/test_gpu_cdicts.py runs the rest)."""
    device = product.lib().APE_LZ4_gpu_device_count() > 0
    for name in NAMES:
        empty = _valid(product, name, 0)
        nulls = list(empty)
        for at in ((0, 1, 3) if name in PREPARES else (0, 1, 2, 3, 4, 6)):
            nulls[at] = None
        if device:
            assert _f(product, name)(*empty) == OK, name
            assert _f(product, name)(*nulls) == OK, name
            continue
        for args in (_valid(product, name), _valid(product, name, 3), empty, nulls):
            assert _f(product, name)(*args) == ENODEV, (name, args)
            assert "no HIP device" in product.gpu_last_error()


def test_the_bindings_validate_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    scr = torch.zeros(16, dtype=torch.uint8)
    calls = [(product.compress_cdicts_batch, [p, i, p, i, i, p], (0, 1, 2, 3, 4, 5)),
             (product.compress_hc_cdicts_batch, [p, i, p, i, i, p, 4096, 8, scr],
              (0, 1, 2, 3, 4, 5, 8)),
             (product.compress_hc_opt_cdicts_batch, [p, i, p, i, i, p, 4096, 8, scr],
              (0, 1, 2, 3, 4, 5, 8))]
    for f, good, tensors in calls:
        with pytest.raises(ValueError):            # CPU tensors
            f(*good)
        for hole in tensors:                       # the sizes (1) before their shape is read
            for bad in (None, [0, 0], 7):
                args = list(good)
                args[hole] = bad
                with pytest.raises(ValueError):
                    f(*args)
        for hole, bad in ((5, p.to(torch.int32)), (5, p[:1]), (5, p.to(torch.float64)),
                          (1, i.to(torch.int64)), (0, p[:1])):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                f(*args)
    for f, size in ((product.cdict_prepare_batch, product.cdict_size()),
                    (product.hc_cdict_prepare_batch, product.hc_cdict_size())):
        objs = torch.zeros(2 * size, dtype=torch.uint8)
        good = [p, i, 4096, objs, size]
        with pytest.raises(ValueError):            # CPU tensors
            f(*good)
        for hole in (0, 1, 3):
            for bad in (None, [0, 0], 7):
                args = list(good)
                args[hole] = bad
                with pytest.raises(ValueError):
                    f(*args)
        for hole, bad in ((0, p.to(torch.int32)), (0, p[:1]), (1, i.to(torch.int64)),
                          (3, objs.to(torch.int16)), (3, objs[:2 * size - 1]), (4, size - 16),
                          (4, None), (4, 1.5)):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                f(*args)
