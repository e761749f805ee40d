"""The Python binding checks every tensor before a pointer reaches C:
wrong dtype, layout, length or device raises ValueError and nothing is launched.  CPU-only:
the structural checks run before the device check, so CPU tensors reach each rule."""
import pytest

torch = pytest.importorskip("torch")
import libapenetwork_amd as amd  # noqa: E402


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def _i32(n):
    return torch.zeros(n, dtype=torch.int32)


def _i64(n):
    return torch.zeros(n, dtype=torch.int64)


def _raises(match, f, *a, **k):
    with pytest.raises(ValueError, match=match):
        f(*a, **k)


@pytest.mark.parametrize("fn", [amd.compress_batch, amd.decompress_batch])
def test_strided_batch_checks(fn):
    n = 4
    src, dst = _u8(n, 64), _u8(n, 96)
    _raises("dtype", fn, src.to(torch.int32), _i32(n), dst, _i32(n))
    _raises("dtype", fn, src, _i64(n), dst, _i32(n))
    _raises("dtype", fn, src, _i32(n), dst, _i32(n).float())
    _raises("contiguous", fn, _u8(n, 128)[:, ::2], _i32(n), dst, _i32(n))
    _raises("contiguous", fn, src, _i32(n), _u8(96, n).t(), _i32(n))
    _raises("2-D", fn, _u8(n * 64), _i32(n), dst, _i32(n))
    _raises("rows", fn, src, _i32(n), _u8(n + 1, 96), _i32(n))
    _raises("elements", fn, src, _i32(n - 1), dst, _i32(n))
    _raises("elements", fn, src, _i32(n), dst, _i32(n), dst_caps=_i32(n + 1))
    _raises("contiguous", fn, src, torch.zeros(2 * n, dtype=torch.int32)[::2], dst, _i32(n))
    # a row narrower than its stride: the C default cap (the stride) would run past it
    _raises("dst_caps", fn, src, _i32(n), _u8(n, 128)[:, :96], _i32(n))
    # structurally right, but host memory
    _raises("CUDA", fn, src, _i32(n), dst, _i32(n))
    _raises("CUDA", fn, src, _i32(n), _u8(n, 128)[:, :96], _i32(n), dst_caps=_i32(n))


def test_pointer_batch_checks():
    n = 3
    ok = dict(src_ptrs=_i64(n), src_sizes=_i32(n), dst_ptrs=_i64(n), caps=_i32(n), results=_i32(n))
    for f, extra in ((amd.compress_fast_ptr_batch, (1,)), (amd.compress_exact_ptr_batch, ())):
        _raises("dtype", f, _i32(n), ok["src_sizes"], ok["dst_ptrs"], ok["caps"], ok["results"], *extra)
        _raises("elements", f, ok["src_ptrs"], ok["src_sizes"], _i64(n + 1), ok["caps"], ok["results"],
                *extra)
        _raises("tensor", f, ok["src_ptrs"], ok["src_sizes"], ok["dst_ptrs"], None, ok["results"], *extra)
        _raises("CUDA", f, *ok.values(), *extra)
    _raises("dtype", amd.decompress_ptr_batch, _i64(n), _i64(n), _i64(n), _i32(n), _i32(n))
    _raises("elements", amd.decompress_partial_batch, _i64(n), _i32(n), _i64(n), _i32(n), _i32(n),
            _i32(n - 1))
    _raises("dtype", amd.decompress_dict_batch, _i64(n), _i32(n), _i64(n), _i32(n), _i32(n), _i32(n),
            _i32(n))
    _raises("dtype", amd.compress_prefix_batch, _i64(n), _i32(n), _i64(n), _i64(n), _i32(n), _i32(n))
    _raises("dtype", amd.decompress_fast_ptr_batch, _i64(n), _i32(n), _i64(n), _i32(n), _i64(n))
    _raises("dtype", amd.compress_destSize_ptr_batch, _i64(n), _i32(n), _i64(n), _i32(n), _u8(n))
    _raises("CUDA", amd.compress_destSize_scratch_ptr_batch, _i64(n), _i32(n), _i64(n), _i32(n),
            _i32(n), _u8(16))


N = 2
P, I = "p", "i"            # an int64 pointer tensor, an int32 size tensor, N entries each
U8, IX = "u8", "ix"        # a uint8 byte tensor (scratch, prepared dictionary), an index [N, 64]
# every pointer-array wrapper: its arguments in positional order (a letter: a tensor of that
# kind; anything else: the value itself), and which position is the sizes tensor that gives the
# batch its length
POINTER_WRAPPERS = {
    "decompress_partial_batch": ((P, I, P, I, I, I), 1),
    "compress_fast_ptr_batch": ((P, I, P, I, I, 1), 1),
    "compress_exact_ptr_batch": ((P, I, P, I, I), 1),
    "compress_destSize_ptr_batch": ((P, I, P, I, I), 1),
    "compress_destSize_scratch_ptr_batch": ((P, I, P, I, I, U8), 1),
    "decompress_fast_ptr_batch": ((P, I, P, I, I), 3),
    "decompress_ptr_batch": ((P, I, P, I, I), 1),
    "compress_prefix_batch": ((P, I, I, P, I, I), 1),
    "decompress_dict_batch": ((P, I, P, I, P, I, I), 1),
    "compress_large_ptr_batch": ((P, I, P, I, I, 1 << 20, 1, U8), 1),
    "compress_large_indexed_ptr_batch": ((P, I, P, I, I, 1 << 20, 0, IX, 1, U8), 1),
    "decompress_indexed_ptr_batch": ((P, I, P, I, IX, 4, I), 1),
    "decompress_range_indexed_ptr_batch": ((P, I, IX, 4, I, I, P, I, "w", I, I), 1),
    "compress_cdict_batch": ((P, I, P, I, I, U8), 1),
    "compress_hc_ptr_batch": ((P, I, P, I, I, 64, U8), 1),
    "compress_hc_prefix_ptr_batch": ((P, I, I, P, I, I, 64, U8), 1),
    "compress_hc_opt_ptr_batch": ((P, I, P, I, I, 64, U8), 1),
    "compress_hc_opt_prefix_ptr_batch": ((P, I, I, P, I, I, 64, U8), 1),
    "compress_hc_cdict_batch": ((P, I, P, I, I, U8, 4096, 64, U8), 1),
    "compress_hc_opt_cdict_batch": ((P, I, P, I, I, U8, 4096, 64, U8), 1),
    "compress_large_hc_ptr_batch": ((P, I, P, I, I, 1 << 20, 64, 0, IX, U8), 1),
    "compress_large_hc_opt_ptr_batch": ((P, I, P, I, I, 1 << 20, 64, 0, IX, U8), 1),
}
SIZES_ONCE_READ_UNCHECKED = (
    "decompress_partial_batch", "compress_fast_ptr_batch", "compress_exact_ptr_batch",
    "compress_destSize_ptr_batch", "compress_destSize_scratch_ptr_batch",
    "decompress_fast_ptr_batch", "decompress_ptr_batch", "compress_prefix_batch",
    "decompress_dict_batch")


def _tensor(kind):
    return {P: lambda: _i64(N), I: lambda: _i32(N), "w": lambda: _i32(2 * N),
            U8: lambda: _u8(1 << 10), IX: lambda: _u8(N, 64)}.get(kind, lambda: kind)()


def _wrong_dtype(t):
    return t.to(torch.int32 if t.dtype == torch.int64 else torch.int64)


def test_the_table_has_every_pointer_array_wrapper():
    public = [n for n in amd.__all__ if n.endswith("_batch") and n not in ("compress_batch",
                                                                          "decompress_batch")]
    assert public and set(public) <= set(POINTER_WRAPPERS)
    assert set(SIZES_ONCE_READ_UNCHECKED) <= set(POINTER_WRAPPERS)


@pytest.mark.parametrize("name", SIZES_ONCE_READ_UNCHECKED)
def test_sizes_are_checked_before_their_shape_is_read(name):
    kinds, sizes_at = POINTER_WRAPPERS[name]
    for bad in (None, [0, 0], 7):
        args = [_tensor(k) for k in kinds]
        args[sizes_at] = bad
        with pytest.raises(ValueError):
            getattr(amd, name)(*args)


@pytest.mark.parametrize("name", sorted(POINTER_WRAPPERS))
def test_every_tensor_position_checks_its_dtype(name):
    kinds, _ = POINTER_WRAPPERS[name]
    for at, kind in enumerate(kinds):
        if not isinstance(kind, str):
            continue
        args = [_tensor(k) for k in kinds]
        args[at] = _wrong_dtype(args[at])
        # the per-block tensors are checked before anything asks where they live, so on these
        # CPU tensors the message is the dtype's; a scratch or an index comes after that
        per_block = kind in (P, I) and name != "decompress_range_indexed_ptr_batch"
        with pytest.raises(ValueError, match="dtype" if per_block else None):
            getattr(amd, name)(*args)
    with pytest.raises(ValueError, match="CUDA"):      # all of them right, but host memory
        getattr(amd, name)(*[_tensor(k) for k in kinds])


def test_frame_checks():
    n = 4
    comp = _u8(n, 80)
    _raises("elements", amd.frame_pack, comp, _i32(n), _i64(n), _u8(1024))
    _raises("dtype", amd.frame_pack, comp, _i32(n), _i64(n + 1).int(), _u8(1024))
    _raises("nblocks", amd.decompress_frames, _u8(1024), _i64(n + 1), _u8(n, 64), _i32(n), nblocks=n + 1)
    _raises("offsets", amd.decompress_frames, _u8(1024), _i64(n), _u8(n, 64), _i32(n))
    _raises("dst_caps", amd.decompress_frames, _u8(1024), _i64(n + 1), _u8(n, 128)[:, :64], _i32(n))
    _raises("elements", amd.frame_offsets, _i32(n), _i64(n))
    _raises("row", amd.synth_blocks, _u8(n, 64), 65, 0, 1)
