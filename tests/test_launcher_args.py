"""Every *_dev / *_host entry point of include/ape_lz4_gpu.h, from one table: a null required
array or a negative count is EINVAL before any device call, the message APE_LZ4_gpu_last_error()
then holds is that call's own (it starts with the entry point's name: the symbol without the
APE_LZ4_ prefix, then a colon), and the binding's ctypes signatures agree with the header.  The
per-family files (tests/test_*_args.py) pin each family's further rules."""
import ctypes as C
import os

import pytest

import cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENODEV, EINVAL, ELAUNCH = 0, -1, -2, -3
A = 4096        # a pointer that is never dereferenced: each call ends at a check
BIG = 1 << 40   # bytes of a scratch or an object behind such a pointer
MB = 1 << 20
FIVE = [A, A, A, A, A]


def _entries(product):
    """name -> (a valid argument list, the position of the count or None, the positions of the
    arrays the call needs, the positions of the pointers it can do without)."""
    L = product.lib()
    S = L.APE_LZ4_compress_large_slice_size()
    ix = L.APE_LZ4_large_index_size(MB, S)
    ms = (C.c_float * 6)()      # the timed calls write their figures: real memory
    plain = (FIVE + [1, None], 5, range(5), [6])
    accel = (FIVE + [1, 1, None], 5, range(5), [7])
    hc = (FIVE + [1, 64, A, BIG, None], 5, [0, 1, 2, 3, 4, 7], [9])
    hc_prefix = (FIVE + [A, 1, 64, A, BIG, None], 6, [0, 1, 3, 4, 5, 8], [2, 10])
    hc_cdict = (FIVE + [1, A, 4096, 64, A, BIG, None], 5, [0, 1, 2, 3, 4, 6, 9], [11])
    large_hc = (FIVE + [1, MB, 64, A, BIG, S, A, ix, None], 5, [0, 1, 2, 3, 4, 8], [11, 13])
    strided = ([A, 64, A, A, 64, A, A, 1, None], 7, [0, 2, 3, 6], [5, 8])
    prepare = ([A, 100, 4096, A, BIG, None], None, [0, 3], [5])
    return {
        "compress_batch_dev": plain,
        "compress_fast_batch_dev": accel,
        "compress_exact_batch_dev": accel,
        "decompress_safe_batch_dev": plain,
        "decompress_safe_partial_batch_dev": (FIVE + [A, 1, None], 6, range(6), [7]),
        "compress_withPrefix_batch_dev": (FIVE + [A, 1, None], 6, range(6), [7]),
        "decompress_safe_usingDict_batch_dev": (FIVE + [A, A, 1, None], 7, range(7), [8]),
        "cdict_prepare_dev": prepare,
        "compress_usingCDict_batch_dev": (FIVE + [1, A, None], 5, [0, 1, 2, 3, 4, 6], [7]),
        "decompress_fast_batch_dev": plain,
        "compress_destSize_batch_dev": plain,
        "compress_destSize_batch_scratch_dev": (FIVE + [1, A, BIG, None], 5,
                                                [0, 1, 2, 3, 4, 6], [8]),
        "compress_hc_batch_dev": hc,
        "compress_hc_withPrefix_batch_dev": hc_prefix,
        "compress_hc_opt_batch_dev": hc,
        "compress_hc_opt_withPrefix_batch_dev": hc_prefix,
        "hc_cdict_prepare_dev": prepare,
        "compress_hc_usingCDict_batch_dev": hc_cdict,
        "compress_hc_opt_usingCDict_batch_dev": hc_cdict,
        "compress_large_batch_dev": (FIVE + [1, MB, 1, A, BIG, None], 5,
                                     [0, 1, 2, 3, 4, 8], [10]),
        "compress_large_timed_dev": (FIVE + [1, MB, 1, A, BIG, None, ms], 5,
                                     [0, 1, 2, 3, 4, 8, 11], [10]),
        "compress_large_indexed_batch_dev": (FIVE + [1, MB, 1, A, BIG, S, A, ix, None], 5,
                                             [0, 1, 2, 3, 4, 8], [11, 13]),
        "decompress_safe_indexed_batch_dev": ([A, A, A, A, A, 64, 4, A, 1, None], 8,
                                              [0, 1, 2, 3, 4, 7], [9]),
        "compress_large_hc_batch_dev": large_hc,
        "compress_large_hc_timed_dev": (FIVE + [1, MB, 64, A, BIG, S, None, ms], 5,
                                        [0, 1, 2, 3, 4, 8, 12], [11]),
        "compress_large_hc_opt_batch_dev": large_hc,
        "decompress_range_indexed_batch_dev": (
            [A, A, A, 64, 4, 1, A, A, A, A, A, A, A, 1, 4, None], 5,
            [0, 1, 2, 7, 8, 9, 10, 11, 12], [6, 15]),
        "compress_batch_strided_dev": strided,
        "decompress_safe_batch_strided_dev": strided,
        "frame_offsets_dev": ([A, A, A, 1, None], 3, range(3), [4]),
        "frame_pack_strided_dev": ([A, 64, A, A, A, 1, None], 5, [0, 2, 3, 4], [6]),
        "decompress_safe_frames_dev": ([A, A, A, 64, A, A, 1, None], 6, [0, 1, 2, 5], [4, 7]),
        "compress_batch_host": (FIVE + [1], 5, range(5), []),
        "decompress_safe_batch_host": (FIVE + [1], 5, range(5), []),
        "synth_blocks_dev": ([A, 64, 64, 0, 1, 1, None], 4, [0], [6]),
    }


# compress_large_timed_dev makes its events before it looks at its arguments (only a null ms4
# is caught earlier), so without a device every other call of it fails there, valid or not.
EVENTS_FIRST, MS4 = "compress_large_timed_dev", 11


def _prototypes():
    return cheader.prototypes(os.path.join(ROOT, "include", "ape_lz4_gpu.h"))


def _call(product, name, args):
    return getattr(product.lib(), "APE_LZ4_" + name)(*args)


def _no_device(product):
    return product.lib().APE_LZ4_gpu_device_count() == 0


def _rejected(product, name, args):
    """The call is EINVAL, and the message it leaves is its own."""
    if name == EVENTS_FIRST and args[MS4] is not None and _no_device(product):
        assert _call(product, name, args) == ELAUNCH
        return
    assert _call(product, name, args) == EINVAL, (name, args)
    assert (name + ":") in product.gpu_last_error(), (name, product.gpu_last_error())


def test_the_table_has_every_device_and_host_entry_point(product):
    declared = {n[len("APE_LZ4_"):] for n in _prototypes() if n.endswith(("_dev", "_host"))}
    table = _entries(product)
    assert len(declared) == 35 and declared == set(table)
    for name, (args, count_at, required, nullable) in table.items():
        f = getattr(product.lib(), "APE_LZ4_" + name)
        pointers = {k for k, t in enumerate(f.argtypes) if t is C.c_void_p}
        assert len(args) == len(f.argtypes), name
        assert pointers == set(required) | set(nullable), name
        assert count_at is None or f.argtypes[count_at] is C.c_int, name


def test_a_null_array_or_a_negative_count_is_rejected_with_the_calls_own_message(product):
    for name, (args, count_at, required, _) in _entries(product).items():
        for hole in required:
            bad = list(args)
            bad[hole] = None
            _rejected(product, name, bad)
        if count_at is not None:
            bad = list(args)
            bad[count_at] = -1
            _rejected(product, name, bad)
            if name == "decompress_range_indexed_batch_dev":   # its other count, the requests
                bad = list(args)
                bad[13] = -1
                _rejected(product, name, bad)


def test_a_rejection_never_leaves_an_earlier_calls_message(product):
    table = _entries(product)
    names = sorted(table)
    for first, second in zip(names, names[1:] + names[:1]):
        for name in (first, second):
            bad = list(table[name][0])
            bad[table[name][2][-1]] = None
            _rejected(product, name, bad)
        assert (first + ":") not in product.gpu_last_error(), (first, second)
    # the pair that showed it: a depth out of range, then a plain call with a null array
    one = product.compress_hc_scratch_size(1)
    assert _call(product, "compress_hc_batch_dev", FIVE + [1, 999, A, one, None]) == EINVAL
    assert "999" in product.gpu_last_error()
    assert _call(product, "compress_batch_dev", [None, A, A, A, A, 1, None]) == EINVAL
    assert "999" not in product.gpu_last_error() and "compress_hc" not in product.gpu_last_error()
    # and the binding's exception carries the message of the call that failed
    import libapenetwork_amd as amd
    with pytest.raises(amd.GpuError, match="compress_batch_dev:"):
        amd._check(_call(product, "compress_batch_dev", [None, A, A, A, A, 1, None]), "x")


def test_valid_arguments_without_a_device_end_at_the_device_check(product):
    if not _no_device(product):
        pytest.skip("a GPU is visible here; covered by the -m gpu suite")
    for name, (args, count_at, _, nullable) in _entries(product).items():
        want = ELAUNCH if name == EVENTS_FIRST else ENODEV
        assert _call(product, name, args) == want, name
        if want == ENODEV:
            assert "no HIP device" in product.gpu_last_error()
        for hole in nullable:           # the pointers a call can do without
            ok = list(args)
            ok[hole] = None
            assert _call(product, name, ok) == want, (name, hole)


def test_the_ctypes_signatures_agree_with_the_header(product):
    L = product.lib()
    protos = _prototypes()
    assert len(protos) >= 70
    checked = 0
    for name, (ret, nparams) in protos.items():
        f = getattr(L, name)
        if f.argtypes is None:      # not in the binding's table: called nowhere through it
            continue
        checked += 1
        assert len(f.argtypes) == nparams, name
        if ret == "void":
            assert f.restype is None, name
        elif "*" in ret or ret in ("size_t", "long long"):
            assert f.restype is not C.c_int, name
            assert C.sizeof(f.restype) == 8, name
        else:
            assert ret == "int" and f.restype is C.c_int, name
    assert checked >= 70
