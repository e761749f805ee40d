"""Framed compress with preferences (include/ape_lz4f_prefs.h): what can be checked without a
GPU -- the host functions' values, every EINVAL row before a device is looked for, each with the
call's own name in APE_LZ4_gpu_last_error(), an empty batch with null arrays, the binding's
checks and the ctypes signatures against the header (tests/test_gpu_lz4f_prefs.py has the
rest)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import cheader
import lz4fprefsmodel as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENODEV, EINVAL = 0, -1, -2
A = 4096        # a pointer that is never dereferenced: each call ends at a check
BIG = 1 << 40
NAME = "lz4f_compress_prefs_batch_dev"
SIZES = ("lz4f_compress_prefs_bound", "lz4f_compress_prefs_scratch_size")
MAX_SRC = 0x7E000000
NEVER = (1 << 64) - 1
# positions in the argument list
N, MAXSRC, BSID, MODE, DEPTH, FLAGS, SCRATCH, BYTES = 5, 6, 7, 8, 9, 10, 11, 12


def _call(product, args):
    return getattr(product.lib(), "APE_LZ4_" + NAME)(*args)


def _rejected(product, args):
    assert _call(product, args) == EINVAL, args
    assert product.gpu_last_error().startswith(NAME + ":"), product.gpu_last_error()


def _valid(count=1, bsid=5, mode=1, depth=8):
    return [A, A, A, A, A, count, 600000, bsid, mode, depth, 7, A, BIG, None]


def test_the_header_declares_the_three_and_the_binding_agrees(product):
    path = os.path.join(ROOT, "include", "ape_lz4f_prefs.h")
    protos = cheader.prototypes(path)
    assert sorted(protos) == sorted("APE_LZ4_" + n for n in SIZES + (NAME,))
    for name, (ret, nparams) in protos.items():
        f = getattr(product.lib(), name)
        assert f.argtypes is not None and len(f.argtypes) == nparams, name
        if name[len("APE_LZ4_"):] in SIZES:
            assert ret.split()[-1] == "size_t" and f.restype is C.c_size_t, name
        else:
            assert ret.split()[-1] == "int" and f.restype is C.c_int, name
    # a stand-alone header: it includes the frame header, and no other header knows it
    assert '#include "ape_lz4f.h"' in open(path).read()
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ape_lz4f_prefs.h":
            assert "prefs" not in open(os.path.join(ROOT, "include", other)).read(), other
    for name in ("lz4f_compress_prefs_bound", "lz4f_compress_prefs_scratch_size",
                 "lz4f_compress_prefs_batch"):
        assert callable(getattr(product, name))
        assert name not in product.__all__


@pytest.mark.parametrize("lang, std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_the_header_compiles_on_its_own(tmp_path, lang, std):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    assert cc is not None, "no host compiler"
    src = tmp_path / ("alone." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "ape_lz4f_prefs.h"\n'
                   "size_t (*take)(int, int, int) = APE_LZ4_lz4f_compress_prefs_bound;\n")
    run = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                          "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_a_null_array_or_a_negative_count_is_rejected(product):
    good = _valid()
    for hole in (0, 1, 2, 3, 4, SCRATCH):
        bad = list(good)
        bad[hole] = None
        _rejected(product, bad)
    for n in (-1, -2 ** 31):
        bad = list(good)
        bad[N] = n
        _rejected(product, bad)


def test_every_other_argument_out_of_range_is_rejected(product):
    good = _valid(3)
    need = product.lz4f_compress_prefs_scratch_size(3, 600000, 5, 1, 1)
    rows = ((MAXSRC, (-1, MAX_SRC + 1, 2 ** 31 - 1, -2 ** 31)), (BSID, (3, 8, 0, -1, 2 ** 31 - 1)),
            (MODE, (-1, 3, 2 ** 31 - 1)), (DEPTH, (-1, 257, -2 ** 31)),
            (FLAGS, (8, -1, 16, 2 ** 31 - 1)), (SCRATCH, (A + 1, A + 4, A + 8)),
            (BYTES, (0, need - 1)))
    for at, values in rows:
        for v in values:
            bad = list(good)
            bad[at] = v
            _rejected(product, bad)
    ok = list(good)
    ok[BYTES] = need
    assert _call(product, ok) != EINVAL
    # the fast encoder has no depth
    for depth in (1, 64, 256):
        _rejected(product, _valid(3, mode=0, depth=depth))
    assert _call(product, _valid(3, mode=0, depth=0)) != EINVAL
    for mode in (1, 2):
        for depth in (0, 1, 256):
            assert _call(product, _valid(3, mode=mode, depth=depth)) != EINVAL
    # 2^24 block slots, or 2^24 slices, are too many for one call, whatever the scratch
    for count, max_src, bsid in ((1 << 12, 1 << 28, 4), (1 << 10, 1 << 29, 7)):
        bad = _valid(count, bsid=bsid)
        bad[MAXSRC] = max_src
        _rejected(product, bad)
    # an empty batch still has to make sense, but needs no scratch
    for at, v in ((MAXSRC, -1), (BSID, 3), (BSID, 8), (MODE, 3), (DEPTH, 257), (FLAGS, 8)):
        bad = _valid(0)
        bad[at] = v
        _rejected(product, bad)
    _rejected(product, _valid(0, mode=0, depth=8))


def test_valid_arguments_reach_the_device_check(product):
    """Without a device they end at ENODEV, an empty batch too (arguments, then device); with
    one, an empty batch launches nothing and returns 0, null arrays and scratch included."""
    device = product.lib().APE_LZ4_gpu_device_count() > 0
    empty = _valid(0)
    nulls = [None] * 5 + empty[5:]
    nulls[SCRATCH], nulls[BYTES] = None, 0
    if device:
        assert _call(product, empty) == OK and _call(product, nulls) == OK
        return
    for args in (_valid(), _valid(3, bsid=7, mode=0, depth=0), empty, nulls):
        assert _call(product, args) == ENODEV, args
        assert "no HIP device" in product.gpu_last_error()


def test_the_bound_is_the_all_stored_frame(product):
    bound = product.lz4f_compress_prefs_bound
    for bsid in (4, 5, 6, 7):
        B = 1 << (8 + 2 * bsid)
        for n in (0, 1, B - 1, B, B + 1, 2 * B + 777):
            for flags in range(8):
                per = 8 if flags & 2 else 4
                want = (15 if flags & 4 else 7) + n + (n + B - 1) // B * per + (8 if flags & 1 else 4)
                assert bound(n, bsid, flags) == want == P.compress_bound(n, bsid, flags)
        assert bound(MAX_SRC, bsid, 7) == P.compress_bound(MAX_SRC, bsid, 7) < 1 << 31
    for flags in range(8):
        for n in (0, 1, 65536, 200001):
            assert bound(n, 4, flags) == product.lz4f_compress_bound(n, flags)
    for args in ((-1, 4, 0), (MAX_SRC + 1, 4, 0), (-2 ** 31, 7, 7), (100, 3, 0), (100, 8, 0),
                 (100, -1, 0), (100, 4, 8), (100, 4, -1)):
        assert bound(*args) == 0 == P.compress_bound(*args), args


def _up16(x):
    return (x + 15) // 16 * 16


def test_the_scratch_sizes(product):
    """The frame layer's part (a slot of B bytes and 36 bytes of arrays per block, 8 per frame),
    then the whole scratch of the mode's large call for the slots as inputs of up to B bytes."""
    size = product.lz4f_compress_prefs_scratch_size
    large = (lambda n, B, ps: product.compress_large_scratch_size(n, B),
             product.compress_large_hc_scratch_size, product.compress_large_hc_opt_scratch_size)
    for nframes, max_src in ((1, 1), (1, 65536), (1, 262145), (7, 3 * 262144 + 100), (3, 0),
                             (2, 5 << 20)):
        for bsid in (4, 5, 6, 7):
            B = 1 << (8 + 2 * bsid)
            slots = nframes * max(1, (max_src + B - 1) // B)
            frame = slots * B + 2 * _up16(8 * slots) + 5 * _up16(4 * slots) + 2 * _up16(4 * nframes)
            for mode in (0, 1, 2):
                for ps in (0, 1, 3):
                    assert size(nframes, max_src, bsid, mode, ps) == frame + large[mode](slots, B, ps), \
                        (nframes, max_src, bsid, mode, ps)
            assert size(nframes, max_src, bsid, 0, 5) == size(nframes, max_src, bsid, 0, 0)
            assert size(nframes, max_src, bsid, 1, 1) <= size(nframes, max_src, bsid, 1, 3) \
                <= size(nframes, max_src, bsid, 1, 0)
    # out of range: 0
    for args in ((-1, 65536, 4, 0, 0), (1, -1, 4, 0, 0), (1, MAX_SRC + 1, 4, 0, 0), (1, 100, 3, 0, 0),
                 (1, 100, 8, 0, 0), (1, 100, 4, -1, 0), (1, 100, 4, 3, 0), (1, 100, 4, 1, -1)):
        assert size(*args) == 0, args
    # too many block slots, or slices, for one call: (size_t)-1
    assert size(1, MAX_SRC, 4, 0, 0) < NEVER and size(1, MAX_SRC, 7, 2, 1) < NEVER
    assert size((1 << 24) - 1, 65536, 4, 0, 0) < NEVER
    assert size(1 << 24, 65536, 4, 0, 0) == NEVER and size(1 << 12, 1 << 28, 4, 0, 0) == NEVER
    slices = (1 << 22) // product.compress_large_slice_size()      # of a 4 MiB block
    frames = (1 << 24) // slices
    assert size(frames - 1, 1 << 22, 7, 0, 0) < NEVER
    assert size(frames, 1 << 22, 7, 0, 0) == NEVER == size(frames, 1 << 22, 7, 1, 1)


def test_the_binding_validates_before_any_call(product):
    import torch
    p = torch.zeros(2, dtype=torch.int64)
    i = torch.zeros(2, dtype=torch.int32)
    scr = torch.zeros(16, dtype=torch.uint8)
    f = product.lz4f_compress_prefs_batch
    good = [p, i, p, i, i, 65536, 5, 1, 8, 0, scr]
    with pytest.raises(ValueError):            # CPU tensors
        f(*good)
    for hole in (0, 1, 2, 3, 4, 10):
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
