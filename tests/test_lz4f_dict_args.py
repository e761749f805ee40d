"""The calls of include/ape_lz4f_dict.h: what can be checked without a GPU -- the argument checks
that precede every device call, each rejection with the call's own name in
APE_LZ4_gpu_last_error(), the bound and the scratch-size functions, the binding's checks, the
ctypes signatures against the header's prototypes, and the header compiled stand-alone as C and
as C++ (tests/test_gpu_lz4f_dict.py has the rest)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import cheader
import lz4fdictmodel as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ape_lz4f_dict.h")
OK, ENODEV, EINVAL = 0, -1, -2
A = 4096        # a pointer that is never dereferenced: each call ends at a check
BIG = 1 << 40
INFO, COMP, DEC = ("lz4f_info_dict_batch_dev", "lz4f_compress_usingCDicts_batch_dev",
                   "lz4f_decompress_usingDicts_batch_dev")
DEV = (INFO, COMP, DEC)
SIZES = ("lz4f_compress_usingCDicts_bound", "lz4f_compress_usingCDicts_scratch_size",
         "lz4f_decompress_usingDicts_scratch_size")
NEVER = (1 << 64) - 1


def _f(product, name):
    return getattr(product.lib(), "APE_LZ4_" + name)


def _rejected(product, name, args):
    assert _f(product, name)(*args) == EINVAL, (name, args)
    assert product.gpu_last_error().startswith(name + ":"), (name, product.gpu_last_error())


def _valid(name, count=1):
    """(a valid argument list, the positions of its required arrays, the position of the count)."""
    if name == INFO:
        return [A, A, A, count, None], (0, 1, 2), 3
    if name == COMP:
        return [A, A, A, A, A, count, A, A, 4096, 1, 8, 7, A, BIG, None], (0, 1, 2, 3, 4, 6, 12), 5
    return [A, A, A, A, A, count, 4, A, A, A, 3, 7, A, BIG, None], (0, 1, 2, 3, 4, 12), 5


def test_the_header_declares_the_six_and_the_binding_agrees(product):
    protos = cheader.prototypes(HEADER)
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
        if other != "ape_lz4f_dict.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert "ape_lz4f_dict" not in text and "usingDicts" not in text, other
    for name in ("lz4f_info_dict_batch", "lz4f_compress_cdicts_bound",
                 "lz4f_compress_cdicts_scratch_size", "lz4f_compress_cdicts_batch",
                 "lz4f_decompress_dicts_scratch_size", "lz4f_decompress_dicts_batch"):
        assert callable(getattr(product, name))
        assert name not in product.__all__
    assert product.LZ4F_ANY_BLOCK_SIZE == DM.ANY_SIZE == 4
    assert product.LZ4F_NO_DICTIONARY == DM.NO_DICTIONARY == -10


@pytest.mark.parametrize("lang, std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_the_header_compiles_on_its_own(tmp_path, lang, std):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no host compiler")
    src = tmp_path / ("alone." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "ape_lz4f_dict.h"\n'
                   "int (*take)(const char *const *, const int *, int *, int, void *) =\n"
                   "    APE_LZ4_lz4f_info_dict_batch_dev;\n")
    run = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                          "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


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


def test_the_compress_call_rejects_its_other_arguments(product):
    name = COMP
    good, _, _ = _valid(name, 3)
    need = [product.lz4f_compress_cdicts_scratch_size(3, 4096, mode) for mode in (0, 1, 2)]
    # maxSrcSize, mode, depth, flags, the scratch's alignment and size
    for at, values in ((8, (0, -1, 65537, 2 ** 31 - 1)), (9, (-1, 3, 2 ** 31 - 1)),
                       (10, (-1, 257)), (11, (8, -1, 2 ** 31 - 1)),
                       (12, (A + 1, A + 4, A + 8)), (13, (0, need[1] - 1))):
        for v in values:
            bad = list(good)
            bad[at] = v
            _rejected(product, name, bad)
    for mode in (0, 1, 2):
        ok = list(good)
        ok[9], ok[10], ok[13] = mode, 8 if mode else 0, need[mode]
        assert _f(product, name)(*ok) != EINVAL, mode
        ok[7] = None                              # no dictionary IDs
        assert _f(product, name)(*ok) != EINVAL, mode
        short = list(ok)
        short[13] = need[mode] - 1
        _rejected(product, name, short)
    bad = list(good)
    bad[9], bad[10] = 0, 1                        # the fast encoder has no depth
    _rejected(product, name, bad)
    bad = list(good)
    bad[5] = 1 << 24
    _rejected(product, name, bad)
    for at, v in ((8, 0), (9, 3), (11, 8)):       # an empty batch still has to make sense
        bad, _, _ = _valid(name, 0)
        bad[at] = v
        _rejected(product, name, bad)


def test_the_decode_call_rejects_its_other_arguments(product):
    name = DEC
    good, _, _ = _valid(name, 3)
    for flags, placed in ((0, False), (3, False), (4, True), (7, True)):
        need = product.lz4f_decompress_dicts_scratch_size(3, 4, flags)
        assert need == (product.lz4f_decompress_placed_scratch_size(3, 4) if placed
                        else product.lz4f_decompress_scratch_size(3, 4))
        ok = list(good)
        ok[11], ok[13] = flags, need
        assert _f(product, name)(*ok) != EINVAL, flags
        bad = list(ok)
        bad[13] = need - 1
        _rejected(product, name, bad)
    for at, values in ((6, (0, -1, -2 ** 31)), (10, (-1, -2 ** 31)), (11, (8, -1, 2 ** 31 - 1)),
                       (12, (A + 1, A + 4, A + 8)), (13, (0,))):
        for v in values:
            bad = list(good)
            bad[at] = v
            _rejected(product, name, bad)
    for hole in (7, 8, 9):                        # a null table array, with entries
        bad = list(good)
        bad[hole] = None
        _rejected(product, name, bad)
    ok = list(good)                               # ... and without
    ok[7] = ok[8] = ok[9] = None
    ok[10] = 0
    assert _f(product, name)(*ok) != EINVAL
    bad = list(good)
    bad[5], bad[6] = 1 << 12, 1 << 12             # 2^24 block slots
    _rejected(product, name, bad)
    for at, v in ((6, 0), (10, -1), (11, 8)):     # an empty batch still has to make sense
        bad, _, _ = _valid(name, 0)
        bad[at] = v
        _rejected(product, name, bad)


def test_a_rejection_never_leaves_another_calls_message(product):
    for first, second in ((INFO, COMP), (COMP, DEC), (DEC, INFO),
                          ("lz4f_decompress_batch_dev", DEC)):
        for name in (first, second):
            if name in DEV:
                bad, _, _ = _valid(name)
                bad[0] = None
            else:
                bad = [None, A, A, A, A, 1, 4, 0, A, BIG, None]
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
        if name != INFO:
            nulls[13] = 0
            nulls[7] = None
        if name == DEC:
            nulls[8] = nulls[9] = None
            nulls[10] = 0
        if device:
            assert _f(product, name)(*empty) == OK, name
            assert _f(product, name)(*nulls) == OK, name
            continue
        for args in (_valid(name)[0], _valid(name, 3)[0], empty, nulls):
            assert _f(product, name)(*args) == ENODEV, (name, args)
            assert "no HIP device" in product.gpu_last_error()


def _up16(x):
    return (x + 15) // 16 * 16


def test_the_bound_and_the_scratch_sizes(product):
    bound = product.lz4f_compress_cdicts_bound
    for n in (0, 1, 13, 4096, 65536):
        for flags in range(8):
            assert bound(n, flags) == DM.compress_bound(n, flags) > 0, (n, flags)
    assert bound(0, 0) == 15 and bound(1, 0) == 20 and bound(65536, 7) == 15 + 4 + 65536 + 8 + 8
    for args in ((-1, 0), (65537, 0), (5, 8), (5, -1)):
        assert bound(*args) == 0 == DM.compress_bound(*args), args
    cs = product.lz4f_compress_cdicts_scratch_size
    for nframes, max_src in ((1, 1), (7, 4096), (100, 1000), (3, 65536)):
        frame = _up16(nframes * _up16(max_src)) + 2 * _up16(8 * nframes) + 7 * _up16(4 * nframes)
        assert cs(nframes, max_src, 0) == frame
        assert cs(nframes, max_src, 1) == frame + _up16(
            product.compress_hc_cdict_scratch_size(nframes, max_src))
        assert cs(nframes, max_src, 2) == frame + _up16(
            product.compress_hc_opt_cdict_scratch_size(nframes, max_src))
    for args in ((-1, 4096, 0), (1, 0, 0), (1, 65537, 0), (1, 4096, 3), (1, 4096, -1)):
        assert cs(*args) == 0, args
    assert cs(0, 4096, 2) == 0 and cs(1 << 24, 16, 0) == NEVER
    ds = product.lz4f_decompress_dicts_scratch_size
    for args in ((1, 4, 8), (1, 4, -1), (-1, 4, 0), (1, 0, 4)):
        assert ds(*args) == 0, args
    assert ds(1 << 12, 1 << 12, 0) == NEVER == ds(1 << 12, 1 << 12, 4)


def test_the_bindings_validate_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    t3p, t3i = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    scr = torch.zeros(16, dtype=torch.uint8)
    calls = [(product.lz4f_compress_cdicts_batch, [p, i, p, i, i, p, i, 4096, 0, 0, 0, scr],
              (0, 1, 2, 3, 4, 5, 6, 11)),
             (product.lz4f_decompress_dicts_batch, [p, i, p, i, i, 4, t3i, t3p, t3i, 0, scr],
              (0, 1, 2, 3, 4, 6, 7, 8, 10)),
             (product.lz4f_info_dict_batch, [p, i, torch.zeros(20, dtype=torch.int32)], (0, 1, 2))]
    for f, good, tensors in calls:
        with pytest.raises(ValueError):            # CPU tensors
            f(*good)
        for hole in tensors:
            for bad in (None, [0, 0], 7):
                if bad is None and f is product.lz4f_compress_cdicts_batch and hole == 6:
                    continue                       # dict_ids may be None
                args = list(good)
                args[hole] = bad
                with pytest.raises(ValueError):
                    f(*args)
        for hole, bad in ((0, p.to(torch.int32)), (0, p[:1]), (1, i.to(torch.int64))):
            args = list(good)
            args[hole] = bad
            with pytest.raises(ValueError):
                f(*args)
    with pytest.raises(ValueError):                # the table's arrays: one length
        product.lz4f_decompress_dicts_batch(p, i, p, i, i, 4, t3i, p, t3i, 0, scr)
    with pytest.raises(ValueError):                # ten ints per frame
        product.lz4f_info_dict_batch(p, i, torch.zeros(16, dtype=torch.int32))
