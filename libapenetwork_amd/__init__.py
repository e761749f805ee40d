"""libapenetwork_amd -- MI355X-native LZ4 block codec behind libapenetwork's ape_lz4.h.

The product is the C shared library ``libape_lz4_amd.so`` built next to this file
(``make -C libapenetwork_amd/csrc``): it exports the reference's ape_lz4.h ABI
(src/ape_lz4.h:59-467) -- one-shot calls on its host codec by default,
on HIP kernels when ``set_oneshot_host_below`` selects them -- and the batched device
API of include/ape_lz4_gpu.h, whose codec is HIP kernels only.  This module is a thin ctypes
mirror of that ABI for tests and the benchmark -- same function names, same
argument meaning, same return conventions.  There is no Python or CPU fallback:
importing works anywhere, but every call that needs the library raises if it is
missing, and GPU entry points return the library's error codes without a GPU.
"""
import ctypes as _C
import os as _os

__all__ = [
    "lib", "versionNumber", "compressBound", "compress_default", "compress_fast",
    "decompress_safe", "decompress_safe_partial", "compress_batch", "decompress_batch",
    "decompress_partial_batch", "synth_blocks", "gpu_init", "gpu_last_error", "GpuError",
    "MAX_BLOCK", "ERANGE", "frame_offsets", "frame_pack", "decompress_frames",
    "compress_prefix_batch", "decompress_dict_batch", "compress_fast_ptr_batch", "compress_exact_ptr_batch",
    "decompress_fast_ptr_batch", "compress_destSize_ptr_batch", "RxBuf",
    "compress_destSize_scratch_ptr_batch", "destSize_scratch_size",
    "socket_send_blocks", "socket_recv_blocks", "socket_stats", "set_oneshot_host_below",
    "Chain",
    "compress_large_slice_size", "compress_large_scratch_size", "compress_large_ptr_batch",
    "large_index_segments", "large_index_size", "compress_large_indexed_ptr_batch",
    "decompress_indexed_ptr_batch", "decompress_range_indexed_ptr_batch",
    "oneshot_on_gpu",
    "cdict_size", "cdict_window", "cdict_prepare", "compress_cdict_batch",
    "compress_hc_scratch_size", "compress_hc_ptr_batch",
    "compress_hc_prefix_ptr_batch", "compress_large_hc_scratch_size", "compress_large_hc_ptr_batch",
    "compress_hc_opt_scratch_size", "compress_hc_opt_ptr_batch", "compress_hc_opt_prefix_ptr_batch",
    "compress_large_hc_opt_scratch_size", "compress_large_hc_opt_ptr_batch",
    "compress_hc_opt_cdict_scratch_size", "compress_hc_opt_cdict_batch",
    "dict_train_scratch_size", "dict_train",
    "ONESHOT_HOST_ALL",
]

_HERE = _os.path.dirname(_os.path.abspath(__file__))
# APE_LZ4_LIB selects the diagnostic phase-timer build (tools/phase_stats.py) only.
LIB_PATH = _os.environ.get("APE_LZ4_LIB") or _os.path.join(_HERE, "libape_lz4_amd.so")
MAX_BLOCK = 65536
ERANGE = -2147483648
ONESHOT_HOST_ALL = 0x7FFFFFFF   # default one-shot threshold: every one-shot call on the host

_lib = None


class GpuError(RuntimeError):
    pass


def lib():
    """Load libape_lz4_amd.so (raises OSError with the build command if absent)."""
    global _lib
    if _lib is None:
        if not _os.path.exists(LIB_PATH):
            raise OSError("libape_lz4_amd.so not built: run `make -C %s/csrc` "
                          "(or __graft_entry__.build())" % _HERE)
        L = _C.CDLL(LIB_PATH)
        i, p, cp = _C.c_int, _C.c_void_p, _C.c_char_p
        sz, ll = _C.c_size_t, _C.c_longlong
        sig = {
            "APE_LZ4_versionNumber": (i, []),
            "APE_LZ4_compressBound": (i, [i]),
            "APE_LZ4_compress_default": (i, [p, p, i, i]),
            "APE_LZ4_compress_fast": (i, [p, p, i, i, i]),
            "APE_LZ4_decompress_safe": (i, [p, p, i, i]),
            "APE_LZ4_decompress_safe_partial": (i, [p, p, i, i, i]),
            "APE_LZ4_gpu_init": (i, []),
            "APE_LZ4_gpu_device_count": (i, []),
            "APE_LZ4_gpu_last_error": (cp, []),
            "APE_LZ4_gpu_arch": (cp, []),
            "APE_LZ4_gpu_set_oneshot_host_below": (i, [i]),
            "APE_LZ4_compress_batch_dev": (i, [p, p, p, p, p, i, p]),
            "APE_LZ4_compress_fast_batch_dev": (i, [p, p, p, p, p, i, i, p]),
            "APE_LZ4_compress_exact_batch_dev": (i, [p, p, p, p, p, i, i, p]),
            "APE_LZ4_compress_destSize_batch_dev": (i, [p, p, p, p, p, i, p]),
            "APE_LZ4_compress_destSize_scratch_size": (sz, [i]),
            "APE_LZ4_compress_destSize_batch_scratch_dev": (i, [p, p, p, p, p, i, p, sz, p]),
            "APE_LZ4_decompress_fast_batch_dev": (i, [p, p, p, p, p, i, p]),
            "APE_LZ4_decompress_safe_batch_dev": (i, [p, p, p, p, p, i, p]),
            "APE_LZ4_decompress_safe_partial_batch_dev": (i, [p, p, p, p, p, p, i, p]),
            "APE_LZ4_compress_batch_strided_dev": (i, [p, sz, p, p, sz, p, p, i, p]),
            "APE_LZ4_decompress_safe_batch_strided_dev": (i, [p, sz, p, p, sz, p, p, i, p]),
            "APE_LZ4_compress_batch_host": (i, [p, p, p, p, p, i]),
            "APE_LZ4_decompress_safe_batch_host": (i, [p, p, p, p, p, i]),
            "APE_LZ4_synth_blocks_dev": (i, [p, sz, i, ll, i, i, p]),
            "APE_LZ4_frame_scratch_size": (sz, [i]),
            "APE_LZ4_frame_offsets_dev": (i, [p, p, p, i, p]),
            "APE_LZ4_frame_pack_strided_dev": (i, [p, sz, p, p, p, i, p]),
            "APE_LZ4_decompress_safe_frames_dev": (i, [p, p, p, sz, p, p, i, p]),
            "APE_LZ4_compress_withPrefix_batch_dev": (i, [p, p, p, p, p, p, i, p]),
            "APE_LZ4_decompress_safe_usingDict_batch_dev": (i, [p, p, p, p, p, p, p, i, p]),
            "APE_LZ4_compress_large_slice_size": (i, []),
            "APE_LZ4_compress_large_scratch_size": (sz, [i, i]),
            "APE_LZ4_compress_large_batch_dev": (i, [p, p, p, p, p, i, i, i, p, sz, p]),
            "APE_LZ4_compress_large_timed_dev": (i, [p, p, p, p, p, i, i, i, p, sz, p, p]),
            "APE_LZ4_large_index_segments": (i, [i, i]),
            "APE_LZ4_large_index_size": (sz, [i, i]),
            "APE_LZ4_compress_large_indexed_batch_dev": (i, [p, p, p, p, p, i, i, i, p, sz, i, p, sz, p]),
            "APE_LZ4_decompress_safe_indexed_batch_dev": (i, [p, p, p, p, p, sz, i, p, i, p]),
            "APE_LZ4_decompress_range_indexed_batch_dev": (i, [p, p, p, sz, i, i, p, p, p, p, p, p, p, i, i, p]),
            "APE_LZ4_cdict_size": (sz, []),
            "APE_LZ4_cdict_window": (i, [i, i]),
            "APE_LZ4_cdict_prepare_dev": (i, [p, i, i, p, sz, p]),
            "APE_LZ4_compress_usingCDict_batch_dev": (i, [p, p, p, p, p, i, p, p]),
            "APE_LZ4_compress_hc_scratch_size": (sz, [i]),
            "APE_LZ4_compress_hc_batch_dev": (i, [p, p, p, p, p, i, i, p, sz, p]),
            "APE_LZ4_compress_hc_withPrefix_batch_dev": (i, [p, p, p, p, p, p, i, i, p, sz, p]),
            "APE_LZ4_compress_hc_opt_scratch_size": (sz, [i]),
            "APE_LZ4_compress_hc_opt_batch_dev": (i, [p, p, p, p, p, i, i, p, sz, p]),
            "APE_LZ4_compress_hc_opt_withPrefix_batch_dev": (i, [p, p, p, p, p, p, i, i, p, sz, p]),
            "APE_LZ4_compress_large_hc_opt_scratch_size": (sz, [i, i, i]),
            "APE_LZ4_compress_large_hc_opt_batch_dev": (i, [p, p, p, p, p, i, i, i, p, sz, i, p, sz, p]),
            "APE_LZ4_hc_cdict_size": (sz, []),
            "APE_LZ4_hc_cdict_window": (i, [i, i]),
            "APE_LZ4_hc_cdict_prepare_dev": (i, [p, i, i, p, sz, p]),
            "APE_LZ4_compress_hc_usingCDict_scratch_size": (sz, [i, i]),
            "APE_LZ4_compress_hc_usingCDict_batch_dev": (i, [p, p, p, p, p, i, p, i, i, p, sz, p]),
            "APE_LZ4_compress_hc_opt_usingCDict_scratch_size": (sz, [i, i]),
            "APE_LZ4_compress_hc_opt_usingCDict_batch_dev": (i, [p, p, p, p, p, i, p, i, i, p, sz, p]),
            "APE_LZ4_dict_train_scratch_size": (sz, [i, i, i]),
            "APE_LZ4_dict_train_dev": (i, [p, p, i, i, p, i, i, p, sz, p, p]),
            "APE_LZ4_cdict_prepare_batch_dev": (i, [p, p, i, p, sz, i, p]),
            "APE_LZ4_hc_cdict_prepare_batch_dev": (i, [p, p, i, p, sz, i, p]),
            "APE_LZ4_compress_usingCDicts_batch_dev": (i, [p, p, p, p, p, i, p, p]),
            "APE_LZ4_compress_hc_usingCDicts_batch_dev": (i, [p, p, p, p, p, i, p, i, i, p, sz, p]),
            "APE_LZ4_compress_hc_opt_usingCDicts_batch_dev": (i, [p, p, p, p, p, i, p, i, i, p, sz, p]),
            "APE_LZ4_compress_large_hc_scratch_size": (sz, [i, i, i]),
            "APE_LZ4_compress_large_hc_batch_dev": (i, [p, p, p, p, p, i, i, i, p, sz, i, p, sz, p]),
            "APE_LZ4_compress_large_hc_timed_dev": (i, [p, p, p, p, p, i, i, i, p, sz, i, p, p]),
            "APE_LZ4_xxh32_batch_dev": (i, [p, p, _C.c_uint, p, i, p]),
            "APE_LZ4_lz4f_compress_bound": (sz, [i, i]),
            "APE_LZ4_lz4f_compress_scratch_size": (sz, [i, i]),
            "APE_LZ4_lz4f_compress_batch_dev": (i, [p, p, p, p, p, i, i, i, p, sz, p]),
            "APE_LZ4_lz4f_info_batch_dev": (i, [p, p, p, i, p]),
            "APE_LZ4_lz4f_decompress_scratch_size": (sz, [i, i]),
            "APE_LZ4_lz4f_decompress_batch_dev": (i, [p, p, p, p, p, i, i, i, p, sz, p]),
            "APE_LZ4_decompress_safe_size_batch_dev": (i, [p, p, p, p, p, i, p]),
            "APE_LZ4_lz4f_decompress_placed_scratch_size": (sz, [i, i]),
            "APE_LZ4_lz4f_decompress_placed_batch_dev": (i, [p, p, p, p, p, i, i, i, p, sz, p]),
            "APE_LZ4_lz4f_info_dict_batch_dev": (i, [p, p, p, i, p]),
            "APE_LZ4_lz4f_compress_prefs_bound": (sz, [i, i, i]),
            "APE_LZ4_lz4f_compress_prefs_scratch_size": (sz, [i, i, i, i, i]),
            "APE_LZ4_lz4f_compress_prefs_batch_dev": (i, [p, p, p, p, p, i, i, i, i, i, i, p, sz, p]),
            "APE_LZ4_lz4f_compress_usingCDicts_bound": (sz, [i, i]),
            "APE_LZ4_lz4f_compress_usingCDicts_scratch_size": (sz, [i, i, i]),
            "APE_LZ4_lz4f_compress_usingCDicts_batch_dev": (i, [p, p, p, p, p, i, p, p, i, i, i, i, p, sz, p]),
            "APE_LZ4_lz4f_decompress_usingDicts_scratch_size": (sz, [i, i, i]),
            "APE_LZ4_lz4f_decompress_usingDicts_batch_dev": (i, [p, p, p, p, p, i, i, p, p, p, i, i, p, sz, p]),
            "APE_LZ4_rxbuf_new": (p, [sz]),
            "APE_LZ4_rxbuf_prepare": (i, [p, sz]),
            "APE_LZ4_rxbuf_append": (i, [p, p, sz]),
            "APE_LZ4_rxbuf_frames": (i, [p, p, i, i]),
            "APE_LZ4_rxbuf_consume": (None, [p, sz]),
            "APE_LZ4_rxbuf_data": (p, [p]),
            "APE_LZ4_rxbuf_used": (sz, [p]),
            "APE_LZ4_rxbuf_room": (sz, [p]),
            "APE_LZ4_rxbuf_pinned": (i, [p]),
            "APE_LZ4_rxbuf_free": (None, [p]),
            "APE_LZ4_socket_send_blocks": (ll, [i, p, sz, i, i, i]),
            "APE_LZ4_socket_recv_blocks": (ll, [i, p, sz, i, i, i, p]),
            "APE_LZ4_socket_stats": (i, [p, i]),
            "APE_LZ4_chain_new": (p, [i, i]),
            "APE_LZ4_chain_free": (None, [p]),
            "APE_LZ4_chain_send": (ll, [p, p, p, sz, i]),
            "APE_LZ4_chain_recv": (ll, [p, p, p, sz, i, p]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def versionNumber():
    return lib().APE_LZ4_versionNumber()


def compressBound(n):
    return lib().APE_LZ4_compressBound(n)


def gpu_init():
    return lib().APE_LZ4_gpu_init()


def gpu_last_error():
    s = lib().APE_LZ4_gpu_last_error()
    return s.decode() if s else ""


def set_oneshot_host_below(nbytes):
    """APE_LZ4_gpu_set_oneshot_host_below: one-shot calls on blocks smaller than nbytes run
    the host codec, larger ones the GPU (0 = all on the GPU).  Returns the previous value."""
    return lib().APE_LZ4_gpu_set_oneshot_host_below(nbytes)


class oneshot_on_gpu:
    """Context manager: route every one-shot call to the GPU path inside the block."""

    def __enter__(self):
        self._prev = set_oneshot_host_below(0)
        return self

    def __exit__(self, *exc):
        set_oneshot_host_below(self._prev)
        return False


def _buf(b, pad=16):
    return _C.create_string_buffer(bytes(b) + b"\0" * pad, len(b) + pad)


# ---- one-shot ape_lz4.h calls (host buffers; host codec or GPU, see above) ----
def compress_default(src, max_dst=None):
    """APE_LZ4_compress_default: returns (ret, compressed_bytes)."""
    cap = compressBound(len(src)) if max_dst is None else max_dst
    out = _C.create_string_buffer(max(cap, 1))
    r = lib().APE_LZ4_compress_default(_buf(src), out, len(src), cap)
    return r, out.raw[:max(r, 0)]


def compress_fast(src, max_dst=None, acceleration=1):
    cap = compressBound(len(src)) if max_dst is None else max_dst
    out = _C.create_string_buffer(max(cap, 1))
    r = lib().APE_LZ4_compress_fast(_buf(src), out, len(src), cap, acceleration)
    return r, out.raw[:max(r, 0)]


def decompress_safe(comp, max_out):
    """APE_LZ4_decompress_safe: returns (ret, dst[0:ret])."""
    out = _C.create_string_buffer(max(max_out, 1))
    r = lib().APE_LZ4_decompress_safe(_buf(comp), out, len(comp), max_out)
    return r, out.raw[:max(r, 0)]


def decompress_safe_partial(comp, target, max_out):
    out = _C.create_string_buffer(max(max_out, 1))
    r = lib().APE_LZ4_decompress_safe_partial(_buf(comp), out, len(comp), target, max_out)
    return r, out.raw[:max(r, 0)]


# ---- batched device API on torch tensors (device-resident) ----
def _ptr(t):
    return None if t is None else _C.c_void_p(t.data_ptr())


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return _C.c_void_p(stream.cuda_stream)


def _check(rc, what):
    if rc != 0:
        raise GpuError("%s failed (%d): %s" % (what, rc, gpu_last_error()))


# ---- argument checks: every pointer handed to C comes from a tensor of the dtype, device and
# layout the C signature assumes; ValueError before any call ----
def _arr(t, what, dtype, n=None, optional=False, cuda=True):
    """A contiguous 1-D CUDA tensor of `dtype` (and length n when given)."""
    import torch
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: need a torch tensor" % what)
    if t.dtype != dtype:
        raise ValueError("%s: dtype %s, need %s" % (what, t.dtype, dtype))
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError("%s: need a contiguous 1-D tensor" % what)
    if n is not None and t.shape[0] != n:
        raise ValueError("%s: %d elements, need %d" % (what, t.shape[0], n))
    if cuda:
        _on_cuda(what, t)


def _rows(t, what, n=None, cuda=True):
    """A 2-D uint8 CUDA tensor whose rows are contiguous (row i at data_ptr + i * stride(0),
    shape[1] bytes each, rows not overlapping)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: need a torch tensor" % what)
    if t.dtype != torch.uint8:
        raise ValueError("%s: dtype %s, need torch.uint8" % (what, t.dtype))
    if t.dim() != 2:
        raise ValueError("%s: need a 2-D tensor [blocks, bytes]" % what)
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("%s: rows must be contiguous and not overlap" % what)
    if n is not None and t.shape[0] != n:
        raise ValueError("%s: %d rows, need %d" % (what, t.shape[0], n))
    if cuda:
        _on_cuda(what, t)


def _on_cuda(what, *ts):
    for t in ts:
        if t is not None and t.device.type != "cuda":
            raise ValueError("%s: need CUDA tensors" % what)


def _strided_args(src, sizes, dst, results, caps, what):
    """compress_batch / decompress_batch: the C side reads block i at src + i*stride(0) and
    writes dst + i*stride(0) with capacity caps[i] or, without caps, stride(0) -- so a row
    narrower than its stride needs explicit caps."""
    import torch
    _rows(src, what + " src", cuda=False)
    n = src.shape[0]
    _rows(dst, what + " dst", n, cuda=False)
    _arr(sizes, what + " sizes", torch.int32, n, cuda=False)
    _arr(results, what + " results", torch.int32, n, cuda=False)
    _arr(caps, what + " dst_caps", torch.int32, n, optional=True, cuda=False)
    if caps is None and n > 0 and dst.shape[1] != dst.stride(0):
        raise ValueError("%s: dst rows narrower than their stride need dst_caps" % what)
    _on_cuda(what, src, dst, sizes, results, caps)
    return n


def _ptr_args(what, n, optional=(), **arrs):
    """Pointer-array calls: name -> tensor of n elements each, int64 where the name ends in
    _ptrs (pointers), int32 otherwise (sizes); the names in `optional` may be None."""
    import torch
    for name, t in arrs.items():
        _arr(t, "%s %s" % (what, name), torch.int64 if name.endswith("_ptrs") else torch.int32, n,
             optional=name in optional, cuda=False)
    _on_cuda(what, *arrs.values())


def _count(what, name, sizes):
    """The length of a batch, from its int32 sizes tensor -- validated before its shape is
    read, so anything else is a ValueError."""
    import torch
    _arr(sizes, "%s %s" % (what, name), torch.int32, cuda=False)
    return sizes.shape[0]


_FIVE = "src_ptrs src_sizes dst_ptrs caps results"


def _ptr_batch(what, names, src_ptrs, sizes, dst_ptrs, caps, results, optional=(), **more):
    """The pointer-array form: the sizes tensor first, since it gives the batch its length,
    then the standard five tensors (called `names` in messages) and any further per-block
    tensors in `more`, as _ptr_args takes them.  Returns the number of blocks."""
    names = names.split()
    n = _count(what, names[1], sizes)
    _ptr_args(what, n, optional, **dict(zip(names, (src_ptrs, sizes, dst_ptrs, caps, results))),
              **more)
    return n


def _bytes(t, what):
    """A scratch, a prepared dictionary, a dictionary: a contiguous uint8 CUDA tensor."""
    import torch
    _arr(t, what, torch.uint8)


def _large_scratch(what, scratch, like, size_fn, *size_args):
    """The caller's scratch, validated, or a new one of size_fn(*size_args) bytes on the
    device of `like`."""
    if scratch is not None:
        _bytes(scratch, what + " scratch")
        return scratch
    import torch
    need = size_fn(*size_args)
    if need == 0 or need >= 1 << 63:
        raise ValueError("%s: max_src_size outside [1, 0x7E000000] or too many slices for one "
                         "call" % what)
    return torch.empty(need, dtype=torch.uint8, device=like.device)


def _call(symbol, *args):
    _check(getattr(lib(), symbol)(*args), symbol)


def compress_batch(src, src_sizes, dst, results, dst_caps=None, stream=None):
    """N x APE_LZ4_compress_default on device.

    src: uint8 [N, S] CUDA tensor (block i = row i, first src_sizes[i] bytes);
    dst: uint8 [N, D] CUDA tensor; results: int32 [N] (compressed size or 0).
    """
    n = _strided_args(src, src_sizes, dst, results, dst_caps, "compress_batch")
    _call("APE_LZ4_compress_batch_strided_dev", _ptr(src), src.stride(0), _ptr(src_sizes),
          _ptr(dst), dst.stride(0), _ptr(dst_caps), _ptr(results), n, _stream(stream))


def decompress_batch(comp, comp_sizes, dst, results, dst_caps=None, stream=None):
    """N x APE_LZ4_decompress_safe on device (caps default to dst row stride)."""
    n = _strided_args(comp, comp_sizes, dst, results, dst_caps, "decompress_batch")
    _call("APE_LZ4_decompress_safe_batch_strided_dev", _ptr(comp), comp.stride(0),
          _ptr(comp_sizes), _ptr(dst), dst.stride(0), _ptr(dst_caps), _ptr(results), n,
          _stream(stream))


def decompress_partial_batch(src_ptrs, comp_sizes, dst_ptrs, targets, caps, results,
                             stream=None):
    """N x APE_LZ4_decompress_safe_partial, pointer-array form (int64 tensors of pointers)."""
    n = _ptr_batch("decompress_partial_batch", "src_ptrs comp_sizes dst_ptrs caps results",
                   src_ptrs, comp_sizes, dst_ptrs, caps, results, targets=targets)
    _call("APE_LZ4_decompress_safe_partial_batch_dev", _ptr(src_ptrs), _ptr(comp_sizes),
          _ptr(dst_ptrs), _ptr(targets), _ptr(caps), _ptr(results), n, _stream(stream))


def compress_fast_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, acceleration,
                            stream=None):
    """N x APE_LZ4_compress_fast, pointer-array form (int64 tensors of pointers)."""
    n = _ptr_batch("compress_fast_ptr_batch", _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    _call("APE_LZ4_compress_fast_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs),
          _ptr(caps), _ptr(results), n, acceleration, _stream(stream))


def compress_exact_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, acceleration=1,
                             stream=None):
    """Greedy-exact mode: N x APE_LZ4_compress_fast byte for byte (the reference's own
    sequential parse, one wave per block; slow, for debugging)."""
    n = _ptr_batch("compress_exact_ptr_batch", _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    _call("APE_LZ4_compress_exact_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs),
          _ptr(caps), _ptr(results), n, acceleration, _stream(stream))


_DESTSIZE = "src_ptrs src_sizes dst_ptrs targets results"


def compress_destSize_ptr_batch(src_ptrs, src_sizes, dst_ptrs, targets, results, stream=None):
    """N x APE_LZ4_compress_destSize, pointer-array form: src_sizes (int32) is in/out --
    input sizes on entry, consumed input bytes on return; results = bytes written."""
    n = _ptr_batch("compress_destSize_ptr_batch", _DESTSIZE, src_ptrs, src_sizes, dst_ptrs,
                   targets, results)
    _call("APE_LZ4_compress_destSize_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs),
          _ptr(targets), _ptr(results), n, _stream(stream))


def compress_destSize_scratch_ptr_batch(src_ptrs, src_sizes, dst_ptrs, targets, results,
                                        scratch, stream=None):
    """compress_destSize_ptr_batch with caller-owned scratch (uint8 CUDA tensor of at least
    destSize_scratch_size(1) bytes): allocates nothing, so it can be graph-captured."""
    what = "compress_destSize_scratch_ptr_batch"
    n = _ptr_batch(what, _DESTSIZE, src_ptrs, src_sizes, dst_ptrs, targets, results)
    _bytes(scratch, what + " scratch")
    _call("APE_LZ4_compress_destSize_batch_scratch_dev", _ptr(src_ptrs), _ptr(src_sizes),
          _ptr(dst_ptrs), _ptr(targets), _ptr(results), n, _ptr(scratch), scratch.numel(),
          _stream(stream))


def destSize_scratch_size(nblocks):
    return lib().APE_LZ4_compress_destSize_scratch_size(nblocks)


def decompress_fast_ptr_batch(src_ptrs, src_bounds, dst_ptrs, original_sizes, results,
                              stream=None):
    """N x APE_LZ4_decompress_fast, pointer-array form: results = input bytes consumed."""
    n = _ptr_batch("decompress_fast_ptr_batch",
                   "src_ptrs src_bounds dst_ptrs original_sizes results", src_ptrs, src_bounds,
                   dst_ptrs, original_sizes, results)
    _call("APE_LZ4_decompress_fast_batch_dev", _ptr(src_ptrs), _ptr(src_bounds), _ptr(dst_ptrs),
          _ptr(original_sizes), _ptr(results), n, _stream(stream))


_DECODE = "src_ptrs comp_sizes dst_ptrs caps results"


def decompress_ptr_batch(src_ptrs, comp_sizes, dst_ptrs, caps, results, stream=None):
    """N x APE_LZ4_decompress_safe, pointer-array form."""
    n = _ptr_batch("decompress_ptr_batch", _DECODE, src_ptrs, comp_sizes, dst_ptrs, caps, results)
    _call("APE_LZ4_decompress_safe_batch_dev", _ptr(src_ptrs), _ptr(comp_sizes), _ptr(dst_ptrs),
          _ptr(caps), _ptr(results), n, _stream(stream))


def compress_prefix_batch(src_ptrs, src_sizes, prefix_sizes, dst_ptrs, caps, results,
                          stream=None):
    """N chained-stream chunks (compress_fast_continue on a stream whose history is the
    prefix_sizes[i] bytes just before src_ptrs[i]); pointer-array form (int64 tensors)."""
    n = _ptr_batch("compress_prefix_batch", _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results,
                   prefix_sizes=prefix_sizes)
    _call("APE_LZ4_compress_withPrefix_batch_dev", _ptr(src_ptrs), _ptr(src_sizes),
          _ptr(prefix_sizes), _ptr(dst_ptrs), _ptr(caps), _ptr(results), n, _stream(stream))


def compress_large_slice_size():
    """APE_LZ4_compress_large_slice_size: the slice size S of the large-input path."""
    return lib().APE_LZ4_compress_large_slice_size()


def compress_large_scratch_size(nblocks, max_src_size):
    """APE_LZ4_compress_large_scratch_size: scratch bytes compress_large_ptr_batch needs."""
    return lib().APE_LZ4_compress_large_scratch_size(nblocks, max_src_size)


def compress_large_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_src_size,
                             acceleration=1, scratch=None, stream=None):
    """N x APE_LZ4_compress_fast on inputs of any size up to max_src_size, each as ONE LZ4
    block (slices compressed in parallel, then stitched); pointer-array form (int64 tensors of
    pointers).  scratch: uint8 CUDA tensor of at least compress_large_scratch_size(N,
    max_src_size) bytes, 16-byte aligned; None allocates one.  Returns the scratch."""
    what = "compress_large_ptr_batch"
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    scratch = _large_scratch(what, scratch, src_sizes, compress_large_scratch_size, n,
                             max_src_size)
    _call("APE_LZ4_compress_large_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs),
          _ptr(caps), _ptr(results), n, max_src_size, acceleration, _ptr(scratch),
          scratch.numel(), _stream(stream))
    return scratch


def large_index_segments(max_src_size, restart_bytes):
    """APE_LZ4_large_index_segments: the most segments an input of up to max_src_size bytes
    gets with restart points every restart_bytes (0 for arguments out of range)."""
    return lib().APE_LZ4_large_index_segments(max_src_size, restart_bytes)


def large_index_size(max_src_size, restart_bytes):
    """APE_LZ4_large_index_size: bytes of one block's seek index, the least index stride."""
    return lib().APE_LZ4_large_index_size(max_src_size, restart_bytes)


def _index_arg(what, index, n, optional=False):
    """The seek indexes of n blocks: a 2-D uint8 CUDA tensor [n, stride] (16-byte alignment
    and the stride are checked by the C side).  Returns the stride (0 without an index)."""
    if index is None and optional:
        return 0
    _rows(index, what + " index", n)
    return index.stride(0) if n > 1 else index.shape[1]


def compress_large_indexed_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_src_size,
                                     restart_bytes, index=None, acceleration=1, scratch=None,
                                     stream=None):
    """compress_large_ptr_batch with a restart point every restart_bytes (0 or a multiple of the
    slice size), and, when index (uint8 CUDA [N, stride >= large_index_size(max_src_size,
    restart_bytes)]) is given, each block's seek index in its row.  Returns the scratch."""
    what = "compress_large_indexed_ptr_batch"
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    stride = _index_arg(what, index, n, optional=True)
    scratch = _large_scratch(what, scratch, src_sizes, compress_large_scratch_size, n,
                             max_src_size)
    _call("APE_LZ4_compress_large_indexed_batch_dev", _ptr(src_ptrs), _ptr(src_sizes),
          _ptr(dst_ptrs), _ptr(caps), _ptr(results), n, max_src_size, acceleration, _ptr(scratch),
          scratch.numel(), restart_bytes, _ptr(index), stride, _stream(stream))
    return scratch


def decompress_indexed_ptr_batch(src_ptrs, comp_sizes, dst_ptrs, caps, index, max_segments,
                                 results, stream=None):
    """N x APE_LZ4_decompress_safe on blocks with a seek index (uint8 CUDA [N, stride], as
    compress_large_indexed_ptr_batch wrote it), one wave per segment; a block with more than
    max_segments segments gets ERANGE.  Pointer-array form."""
    what = "decompress_indexed_ptr_batch"
    n = _ptr_batch(what, _DECODE, src_ptrs, comp_sizes, dst_ptrs, caps, results)
    stride = _index_arg(what, index, n)
    _call("APE_LZ4_decompress_safe_indexed_batch_dev", _ptr(src_ptrs), _ptr(comp_sizes),
          _ptr(dst_ptrs), _ptr(caps), _ptr(index), stride, max_segments, _ptr(results), n,
          _stream(stream))


def decompress_range_indexed_ptr_batch(src_ptrs, comp_sizes, index, max_segments, range_starts,
                                       range_lens, dst_ptrs, caps, window, results, block_of=None,
                                       waves_per_request=4, stream=None):
    """Byte ranges of indexed blocks (APE_LZ4_decompress_range_indexed_batch_dev): request r
    reads range_lens[r] bytes from range_starts[r] of block block_of[r] (None: block r, one
    request per block) into dst_ptrs[r], decoding only the covering segments.  src_ptrs,
    comp_sizes and index (uint8 CUDA [blocks, stride]) are per block, every other tensor per
    request; window is int32 [2 * requests] and receives {where the range begins in dst, the
    bytes of dst used}; results the bytes read, or a negative code (ERANGE: caps[r] is below
    window[2r + 1])."""
    what = "decompress_range_indexed_ptr_batch"
    nb = _count(what, "comp_sizes", comp_sizes)
    nreq = _count(what, "range_starts", range_starts)
    _ptr_args(what, nb, src_ptrs=src_ptrs, comp_sizes=comp_sizes)
    _ptr_args(what, nreq, ("block_of",), range_starts=range_starts, range_lens=range_lens,
              dst_ptrs=dst_ptrs, caps=caps, results=results, block_of=block_of)
    _ptr_args(what, 2 * nreq, window=window)
    if block_of is None and nreq != nb:
        raise ValueError("%s: %d requests for %d blocks need block_of" % (what, nreq, nb))
    stride = _index_arg(what, index, nb)
    _call("APE_LZ4_decompress_range_indexed_batch_dev", _ptr(src_ptrs), _ptr(comp_sizes),
          _ptr(index), stride, max_segments, nb, _ptr(block_of), _ptr(range_starts),
          _ptr(range_lens), _ptr(dst_ptrs), _ptr(caps), _ptr(window), _ptr(results), nreq,
          waves_per_request, _stream(stream))


def cdict_size():
    """APE_LZ4_cdict_size: bytes of device memory one prepared dictionary takes."""
    return lib().APE_LZ4_cdict_size()


def cdict_window(dict_size, max_src_size):
    """APE_LZ4_cdict_window: bytes of the dictionary's tail a prepared dictionary uses."""
    return lib().APE_LZ4_cdict_window(dict_size, max_src_size)


def _prepare(symbol, what, dict_tensor, max_src_size, cdict_tensor, stream):
    """cdict_prepare and hc_cdict_prepare: the same arguments, another object."""
    _bytes(dict_tensor, what + " dict")
    _bytes(cdict_tensor, what + " cdict")
    _call(symbol, _ptr(dict_tensor) if dict_tensor.numel() else None, dict_tensor.numel(),
          max_src_size, _ptr(cdict_tensor), cdict_tensor.numel(), _stream(stream))
    return cdict_tensor


def cdict_prepare(dict_tensor, max_src_size, cdict_tensor, stream=None):
    """APE_LZ4_cdict_prepare_dev: dict_tensor (uint8 CUDA, any placement; may be empty) ->
    the prepared dictionary in cdict_tensor (uint8 CUDA, >= cdict_size() bytes, 16-byte
    aligned) for messages of up to max_src_size bytes.  Returns cdict_tensor."""
    return _prepare("APE_LZ4_cdict_prepare_dev", "cdict_prepare", dict_tensor, max_src_size,
                    cdict_tensor, stream)


def _cdict_batch(symbol, what, size_fn, src_ptrs, src_sizes, dst_ptrs, caps, results, cdict,
                 stream, *hc):
    """Every compressor against a prepared dictionary of at least size_fn() bytes; hc: the
    high-ratio ones' (max_src_size, depth, scratch)."""
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    _bytes(cdict, what + " cdict")
    if cdict.numel() < size_fn():
        raise ValueError("%s cdict: smaller than %s()" % (what, size_fn.__name__))
    if hc:
        max_src_size, depth, scratch = hc
        _bytes(scratch, what + " scratch")
        hc = (max_src_size, depth, _ptr(scratch), scratch.numel())
    _call(symbol, _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs), _ptr(caps), _ptr(results), n,
          _ptr(cdict), *hc, _stream(stream))


def compress_cdict_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, cdict, stream=None):
    """N x (loadDict ; compress_fast_continue) against one prepared dictionary (cdict_prepare);
    pointer-array form (int64 tensors of pointers)."""
    _cdict_batch("APE_LZ4_compress_usingCDict_batch_dev", "compress_cdict_batch", cdict_size,
                 src_ptrs, src_sizes, dst_ptrs, caps, results, cdict, stream)


def compress_hc_scratch_size(nblocks):
    """APE_LZ4_compress_hc_scratch_size: scratch bytes for one pass over nblocks."""
    return lib().APE_LZ4_compress_hc_scratch_size(nblocks)


def _hc_batch(symbol, what, src_ptrs, src_sizes, dst_ptrs, caps, results, depth, scratch, stream,
              *prefix):
    """The four high-ratio calls on plain blocks; prefix: the withPrefix ones' (prefix_sizes,)."""
    more = dict(prefix_sizes=prefix[0]) if prefix else {}
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results, ("prefix_sizes",),
                   **more)
    _bytes(scratch, what + " scratch")
    _call(symbol, _ptr(src_ptrs), _ptr(src_sizes), *map(_ptr, prefix), _ptr(dst_ptrs), _ptr(caps),
          _ptr(results), n, depth, _ptr(scratch), scratch.numel(), _stream(stream))


def compress_hc_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, depth, scratch,
                          stream=None):
    """The high-ratio mode, pointer-array form (int64 tensors of pointers): depth chain
    candidates per position (1..256, 0 = the default 64); scratch is a uint8 CUDA tensor of at
    least compress_hc_scratch_size(1) bytes (fewer than compress_hc_scratch_size(N): several
    passes, same bytes).  Allocates nothing, so it can be graph-captured."""
    _hc_batch("APE_LZ4_compress_hc_batch_dev", "compress_hc_ptr_batch", src_ptrs, src_sizes,
              dst_ptrs, caps, results, depth, scratch, stream)


def compress_hc_prefix_ptr_batch(src_ptrs, src_sizes, prefix_sizes, dst_ptrs, caps, results, depth,
                                 scratch, stream=None):
    """compress_hc_ptr_batch with history: the prefix_sizes[i] bytes just before src_ptrs[i]
    (int32 CUDA tensor, or None for no history), of which the last min(prefix, 65536 - size)
    are used; each block decodes with decompress_dict_batch given that history."""
    _hc_batch("APE_LZ4_compress_hc_withPrefix_batch_dev", "compress_hc_prefix_ptr_batch",
              src_ptrs, src_sizes, dst_ptrs, caps, results, depth, scratch, stream, prefix_sizes)


def compress_hc_opt_scratch_size(nblocks):
    """APE_LZ4_compress_hc_opt_scratch_size: scratch bytes for one pass over nblocks."""
    return lib().APE_LZ4_compress_hc_opt_scratch_size(nblocks)


def compress_hc_opt_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, depth, scratch,
                              stream=None):
    """compress_hc_ptr_batch with the cost-minimising parse over the same search (smaller or
    equal blocks, other bytes); scratch is a uint8 CUDA tensor of at least
    compress_hc_opt_scratch_size(1) bytes (fewer than compress_hc_opt_scratch_size(N): several
    passes, same bytes).  Allocates nothing, so it can be graph-captured."""
    _hc_batch("APE_LZ4_compress_hc_opt_batch_dev", "compress_hc_opt_ptr_batch", src_ptrs,
              src_sizes, dst_ptrs, caps, results, depth, scratch, stream)


def compress_hc_opt_prefix_ptr_batch(src_ptrs, src_sizes, prefix_sizes, dst_ptrs, caps, results,
                                     depth, scratch, stream=None):
    """compress_hc_prefix_ptr_batch with the cost-minimising parse: history, results and
    decoding are the same; the scratch is compress_hc_opt_ptr_batch's."""
    _hc_batch("APE_LZ4_compress_hc_opt_withPrefix_batch_dev", "compress_hc_opt_prefix_ptr_batch",
              src_ptrs, src_sizes, dst_ptrs, caps, results, depth, scratch, stream, prefix_sizes)


def compress_large_hc_opt_scratch_size(nblocks, max_src_size, pass_slices=0):
    """APE_LZ4_compress_large_hc_opt_scratch_size: the large path's scratch plus the tables of
    the cost-minimising parse for pass_slices slices (0: as many as the batch has, at most
    1024)."""
    return lib().APE_LZ4_compress_large_hc_opt_scratch_size(nblocks, max_src_size, pass_slices)


def _large_hc_batch(symbol, what, size_fn, src_ptrs, src_sizes, dst_ptrs, caps, results,
                    max_src_size, depth, restart_bytes, index, scratch, stream):
    """compress_large_hc_ptr_batch and its cost-minimising twin; size_fn: the scratch size."""
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    stride = _index_arg(what, index, n, optional=True)
    scratch = _large_scratch(what, scratch, src_sizes, size_fn, n, max_src_size)
    _call(symbol, _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs), _ptr(caps), _ptr(results), n,
          max_src_size, depth, _ptr(scratch), scratch.numel(), restart_bytes, _ptr(index), stride,
          _stream(stream))
    return scratch


def compress_large_hc_opt_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_src_size,
                                    depth, restart_bytes=0, index=None, scratch=None, stream=None):
    """compress_large_hc_ptr_batch with the cost-minimising parse on the slices: restart points,
    the index and every decoder as there.  scratch: uint8 CUDA tensor of at least
    compress_large_hc_opt_scratch_size(N, max_src_size, 1) bytes, 16-byte aligned; None
    allocates one for a single pass.  Returns the scratch."""
    return _large_hc_batch("APE_LZ4_compress_large_hc_opt_batch_dev",
                           "compress_large_hc_opt_ptr_batch", compress_large_hc_opt_scratch_size,
                           src_ptrs, src_sizes, dst_ptrs, caps, results, max_src_size, depth,
                           restart_bytes, index, scratch, stream)


def hc_cdict_size():
    """APE_LZ4_hc_cdict_size: bytes of device memory one prepared high-ratio dictionary takes."""
    return lib().APE_LZ4_hc_cdict_size()


def hc_cdict_window(dict_size, max_src_size):
    """APE_LZ4_hc_cdict_window: bytes of the dictionary's tail such an object uses (not rounded)."""
    return lib().APE_LZ4_hc_cdict_window(dict_size, max_src_size)


def hc_cdict_prepare(dict_tensor, max_src_size, cdict_tensor, stream=None):
    """APE_LZ4_hc_cdict_prepare_dev: dict_tensor (uint8 CUDA, any placement; may be empty) ->
    the prepared high-ratio dictionary in cdict_tensor (uint8 CUDA, >= hc_cdict_size() bytes,
    16-byte aligned) for messages of up to max_src_size bytes.  Returns cdict_tensor."""
    return _prepare("APE_LZ4_hc_cdict_prepare_dev", "hc_cdict_prepare", dict_tensor, max_src_size,
                    cdict_tensor, stream)


def compress_hc_cdict_scratch_size(nblocks, max_src_size):
    """APE_LZ4_compress_hc_usingCDict_scratch_size: scratch bytes for one pass over nblocks."""
    return lib().APE_LZ4_compress_hc_usingCDict_scratch_size(nblocks, max_src_size)


def compress_hc_cdict_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, cdict, max_src_size,
                            depth, scratch, stream=None):
    """The high-ratio mode against one prepared high-ratio dictionary (hc_cdict_prepare with the
    same max_src_size); pointer-array form (int64 tensors of pointers).  depth as
    compress_hc_ptr_batch; scratch is a uint8 CUDA tensor of at least
    compress_hc_cdict_scratch_size(1, max_src_size) bytes (fewer than ..._scratch_size(N, ...):
    several passes, same bytes).  Each block decodes with decompress_dict_batch given the
    original dictionary.  Allocates nothing, so it can be graph-captured."""
    _cdict_batch("APE_LZ4_compress_hc_usingCDict_batch_dev", "compress_hc_cdict_batch",
                 hc_cdict_size, src_ptrs, src_sizes, dst_ptrs, caps, results, cdict, stream,
                 max_src_size, depth, scratch)


def compress_hc_opt_cdict_scratch_size(nblocks, max_src_size):
    """APE_LZ4_compress_hc_opt_usingCDict_scratch_size: scratch bytes for one pass over nblocks."""
    return lib().APE_LZ4_compress_hc_opt_usingCDict_scratch_size(nblocks, max_src_size)


def compress_hc_opt_cdict_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, cdict, max_src_size,
                                depth, scratch, stream=None):
    """compress_hc_cdict_batch with the cost-minimising parse of compress_hc_opt_ptr_batch: the
    same object, arguments and decoding.  scratch is a uint8 CUDA tensor of at least
    compress_hc_opt_cdict_scratch_size(1, max_src_size) bytes (fewer than ..._scratch_size(N,
    ...): several passes, same bytes).  A block that does not fit its capacity gets result 0
    and nothing is written to it.  Allocates nothing, so it can be graph-captured."""
    _cdict_batch("APE_LZ4_compress_hc_opt_usingCDict_batch_dev", "compress_hc_opt_cdict_batch",
                 hc_cdict_size, src_ptrs, src_sizes, dst_ptrs, caps, results, cdict, stream,
                 max_src_size, depth, scratch)


def dict_train_scratch_size(nsamples, max_sample_size, segment_size):
    """APE_LZ4_dict_train_scratch_size: scratch bytes of one dict_train call (0 for arguments
    out of range)."""
    return lib().APE_LZ4_dict_train_scratch_size(nsamples, max_sample_size, segment_size)


def dict_train(sample_ptrs, sample_sizes, max_sample_size, dict_tensor, segment_size, scratch,
               info, stream=None):
    """APE_LZ4_dict_train_dev: a dictionary of dict_tensor.numel() bytes (uint8 CUDA tensor, any
    placement; every byte is written) trained on the samples at sample_ptrs (int64 CUDA tensor
    of pointers) of sample_sizes bytes each (int32; samples above max_sample_size are ignored),
    by the rule of tests/dicttrainmodel.py with segments of segment_size bytes.  scratch: uint8
    CUDA tensor of at least dict_train_scratch_size(N, max_sample_size, segment_size) bytes,
    16-byte aligned; info: int32 CUDA tensor of 4, which gets {bytes used, picks, samples
    ignored, 0}.  Allocates nothing, so it can be graph-captured; dict_tensor can go straight
    into cdict_prepare or hc_cdict_prepare on the same stream.  Returns dict_tensor."""
    import torch
    what = "dict_train"
    n = _count(what, "sample_sizes", sample_sizes)
    _ptr_args(what, n, sample_ptrs=sample_ptrs, sample_sizes=sample_sizes)
    _bytes(dict_tensor, what + " dict")
    _bytes(scratch, what + " scratch")
    _arr(info, what + " info", torch.int32, 4)
    _call("APE_LZ4_dict_train_dev", _ptr(sample_ptrs) if n else None,
          _ptr(sample_sizes) if n else None, n, max_sample_size, _ptr(dict_tensor),
          dict_tensor.numel(), segment_size, _ptr(scratch), scratch.numel(), _ptr(info),
          _stream(stream))
    return dict_tensor


# ---- a prepared dictionary per message (include/ape_lz4_cdicts.h) ----
# (Public, as compress_hc_cdict_batch is, without a line in __all__: every *_batch name listed
# there has a row in tests/test_bindings.py's table of pointer-array wrappers, which is as it was.
# tests/test_cdicts_args.py checks these five the same way.)
def _prepare_batch(symbol, what, size_fn, dict_ptrs, dict_sizes, max_src_size, cdicts, stride,
                   stream):
    """cdict_prepare_batch and hc_cdict_prepare_batch: the same arguments, another object."""
    n = _count(what, "dict_sizes", dict_sizes)
    _ptr_args(what, n, dict_ptrs=dict_ptrs, dict_sizes=dict_sizes)
    _bytes(cdicts, what + " cdicts")
    if not isinstance(stride, int) or isinstance(stride, bool):
        raise ValueError("%s stride: need an int" % what)
    if n > 0 and (stride < size_fn() or cdicts.numel() < (n - 1) * stride + size_fn()):
        raise ValueError("%s cdicts: %d bytes with stride %d do not hold %d objects of %s() "
                         "bytes" % (what, cdicts.numel(), stride, n, size_fn.__name__))
    _call(symbol, _ptr(dict_ptrs) if n else None, _ptr(dict_sizes) if n else None, max_src_size,
          _ptr(cdicts) if n else None, stride, n, _stream(stream))
    return cdicts


def cdict_prepare_batch(dict_ptrs, dict_sizes, max_src_size, cdicts, stride, stream=None):
    """APE_LZ4_cdict_prepare_batch_dev: N prepared dictionaries in one launch.  dict_ptrs (int64
    CUDA tensor of N device pointers; an entry may be 0 where its size is 0) and dict_sizes
    (int32) name the dictionaries; object k is written at cdicts[k * stride:] (uint8 CUDA tensor,
    16-byte aligned; stride a multiple of 16, at least cdict_size()) and is byte for byte what
    cdict_prepare writes.  An entry with a negative size, or a null pointer and a positive size,
    gets a zero header: every compress against it gives 0.  Returns cdicts."""
    return _prepare_batch("APE_LZ4_cdict_prepare_batch_dev", "cdict_prepare_batch", cdict_size,
                          dict_ptrs, dict_sizes, max_src_size, cdicts, stride, stream)


def hc_cdict_prepare_batch(dict_ptrs, dict_sizes, max_src_size, cdicts, stride, stream=None):
    """APE_LZ4_hc_cdict_prepare_batch_dev: cdict_prepare_batch for the high-ratio modes' object
    (stride at least hc_cdict_size(); object k is hc_cdict_prepare's)."""
    return _prepare_batch("APE_LZ4_hc_cdict_prepare_batch_dev", "hc_cdict_prepare_batch",
                          hc_cdict_size, dict_ptrs, dict_sizes, max_src_size, cdicts, stride,
                          stream)


def _cdicts_batch(symbol, what, src_ptrs, src_sizes, dst_ptrs, caps, results, cdict_ptrs, stream,
                  *hc):
    """Every compressor against a prepared dictionary per message; hc: the high-ratio ones'
    (max_src_size, depth, scratch)."""
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results,
                   cdict_ptrs=cdict_ptrs)
    if hc:
        max_src_size, depth, scratch = hc
        _bytes(scratch, what + " scratch")
        hc = (max_src_size, depth, _ptr(scratch), scratch.numel())
    _call(symbol, _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs), _ptr(caps), _ptr(results), n,
          _ptr(cdict_ptrs), *hc, _stream(stream))


def compress_cdicts_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, cdict_ptrs, stream=None):
    """APE_LZ4_compress_usingCDicts_batch_dev: compress_cdict_batch with a prepared dictionary
    per message.  cdict_ptrs: int64 CUDA tensor of N device pointers, message i's object (of
    cdict_prepare or cdict_prepare_batch).  Message i gets what compress_cdict_batch gives it
    against that object; a null, misaligned or unprepared object gives that message 0 and leaves
    the others as they are."""
    _cdicts_batch("APE_LZ4_compress_usingCDicts_batch_dev", "compress_cdicts_batch", src_ptrs,
                  src_sizes, dst_ptrs, caps, results, cdict_ptrs, stream)


def compress_hc_cdicts_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, cdict_ptrs,
                             max_src_size, depth, scratch, stream=None):
    """APE_LZ4_compress_hc_usingCDicts_batch_dev: compress_hc_cdict_batch with a prepared
    high-ratio dictionary per message (cdict_ptrs as in compress_cdicts_batch; every object
    prepared for this max_src_size).  scratch: compress_hc_cdict_batch's."""
    _cdicts_batch("APE_LZ4_compress_hc_usingCDicts_batch_dev", "compress_hc_cdicts_batch",
                  src_ptrs, src_sizes, dst_ptrs, caps, results, cdict_ptrs, stream, max_src_size,
                  depth, scratch)


def compress_hc_opt_cdicts_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, cdict_ptrs,
                                 max_src_size, depth, scratch, stream=None):
    """APE_LZ4_compress_hc_opt_usingCDicts_batch_dev: compress_hc_opt_cdict_batch with a prepared
    high-ratio dictionary per message.  scratch: compress_hc_opt_cdict_batch's."""
    _cdicts_batch("APE_LZ4_compress_hc_opt_usingCDicts_batch_dev", "compress_hc_opt_cdicts_batch",
                  src_ptrs, src_sizes, dst_ptrs, caps, results, cdict_ptrs, stream, max_src_size,
                  depth, scratch)


def compress_large_hc_scratch_size(nblocks, max_src_size, pass_slices=0):
    """APE_LZ4_compress_large_hc_scratch_size: the large path's scratch plus the high-ratio
    tables of pass_slices slices (0: as many as the batch has, at most 1024)."""
    return lib().APE_LZ4_compress_large_hc_scratch_size(nblocks, max_src_size, pass_slices)


def compress_large_hc_ptr_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_src_size, depth,
                                restart_bytes=0, index=None, scratch=None, stream=None):
    """compress_large_indexed_ptr_batch in the high-ratio mode (depth as compress_hc_ptr_batch):
    inputs of any size up to max_src_size, each as ONE LZ4 block, with a restart point every
    restart_bytes (0: none) and, when index is given, each block's seek index in its row.
    scratch: uint8 CUDA tensor of at least compress_large_hc_scratch_size(N, max_src_size, 1)
    bytes, 16-byte aligned (fewer than ..._scratch_size(N, max_src_size): several passes, same
    bytes); None allocates one for a single pass.  Returns the scratch."""
    return _large_hc_batch("APE_LZ4_compress_large_hc_batch_dev", "compress_large_hc_ptr_batch",
                           compress_large_hc_scratch_size, src_ptrs, src_sizes, dst_ptrs, caps,
                           results, max_src_size, depth, restart_bytes, index, scratch, stream)


def decompress_dict_batch(src_ptrs, comp_sizes, dst_ptrs, caps, dict_ptrs, dict_sizes, results,
                          stream=None):
    """N x APE_LZ4_decompress_safe_usingDict, pointer-array form (int64 tensors)."""
    n = _ptr_batch("decompress_dict_batch", _DECODE, src_ptrs, comp_sizes, dst_ptrs, caps,
                   results, dict_ptrs=dict_ptrs, dict_sizes=dict_sizes)
    _call("APE_LZ4_decompress_safe_usingDict_batch_dev", _ptr(src_ptrs), _ptr(comp_sizes),
          _ptr(dst_ptrs), _ptr(caps), _ptr(dict_ptrs), _ptr(dict_sizes), _ptr(results), n,
          _stream(stream))


def synth_blocks(dst, block_size, first_block, kind, stream=None):
    """Fill rows of uint8 [N, S] CUDA tensor with SURVEY App. C blocks (kind 0 rand, 1 comp)."""
    _rows(dst, "synth_blocks dst", cuda=False)
    if not 0 <= block_size <= dst.shape[1]:
        raise ValueError("synth_blocks: block_size must fit a row")
    _on_cuda("synth_blocks", dst)
    _check(lib().APE_LZ4_synth_blocks_dev(_ptr(dst), dst.stride(0), block_size, first_block,
                                          dst.shape[0], kind, _stream(stream)),
           "APE_LZ4_synth_blocks_dev")


# ---- framed stream of independent blocks (include/ape_lz4_gpu.h, socket path) ----
def frame_offsets(comp_sizes, offsets, scratch=None, stream=None):
    """offsets (int64 [N+1] CUDA) <- exclusive scan of 4 + comp_sizes[i]; returns scratch."""
    import torch
    _arr(comp_sizes, "frame_offsets comp_sizes", torch.int32, cuda=False)
    n = comp_sizes.shape[0]
    _arr(offsets, "frame_offsets offsets", torch.int64, n + 1, cuda=False)
    if scratch is not None:
        _arr(scratch, "frame_offsets scratch", torch.uint8, cuda=False)
        if scratch.numel() < lib().APE_LZ4_frame_scratch_size(n):
            raise ValueError("frame_offsets: scratch smaller than APE_LZ4_frame_scratch_size")
    _on_cuda("frame_offsets", comp_sizes, offsets, scratch)
    if scratch is None:
        nbytes = lib().APE_LZ4_frame_scratch_size(n)
        scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=comp_sizes.device)
    _check(lib().APE_LZ4_frame_offsets_dev(_ptr(comp_sizes), _ptr(offsets), _ptr(scratch), n,
                                           _stream(stream)), "APE_LZ4_frame_offsets_dev")
    return scratch


def frame_pack(comp, comp_sizes, offsets, frames, stream=None):
    """Framed stream [le32 c][c bytes]... of the compressed rows of comp (uint8 [N, D])."""
    import torch
    _rows(comp, "frame_pack comp", cuda=False)
    n = comp.shape[0]
    _arr(comp_sizes, "frame_pack comp_sizes", torch.int32, n, cuda=False)
    _arr(offsets, "frame_pack offsets", torch.int64, n + 1, cuda=False)
    _arr(frames, "frame_pack frames", torch.uint8, cuda=False)
    _on_cuda("frame_pack", comp, comp_sizes, offsets, frames)
    _check(lib().APE_LZ4_frame_pack_strided_dev(_ptr(comp), comp.stride(0), _ptr(comp_sizes),
                                                _ptr(offsets), _ptr(frames), n, _stream(stream)),
           "APE_LZ4_frame_pack_strided_dev")


def decompress_frames(frames, offsets, dst, results, dst_caps=None, nblocks=None, stream=None):
    """N x APE_LZ4_decompress_safe of the blocks of a framed stream into rows of dst."""
    import torch
    _rows(dst, "decompress_frames dst", cuda=False)
    n = dst.shape[0] if nblocks is None else nblocks
    if not 0 <= n <= dst.shape[0]:
        raise ValueError("decompress_frames: nblocks must be within dst's rows")
    _arr(frames, "decompress_frames frames", torch.uint8, cuda=False)
    _arr(offsets, "decompress_frames offsets", torch.int64, cuda=False)
    if offsets.shape[0] < n + 1:
        raise ValueError("decompress_frames: offsets need nblocks + 1 entries")
    _arr(results, "decompress_frames results", torch.int32, cuda=False)
    if results.shape[0] < n:
        raise ValueError("decompress_frames: results need nblocks entries")
    if dst_caps is not None:
        _arr(dst_caps, "decompress_frames dst_caps", torch.int32, cuda=False)
        if dst_caps.shape[0] < n:
            raise ValueError("decompress_frames: dst_caps need nblocks entries")
    elif n > 0 and dst.shape[1] != dst.stride(0):
        raise ValueError("decompress_frames: dst rows narrower than their stride need dst_caps")
    _on_cuda("decompress_frames", frames, offsets, dst, results, dst_caps)
    _check(lib().APE_LZ4_decompress_safe_frames_dev(_ptr(frames), _ptr(offsets), _ptr(dst),
                                                    dst.stride(0), _ptr(dst_caps), _ptr(results),
                                                    n, _stream(stream)),
           "APE_LZ4_decompress_safe_frames_dev")


# ---- socket path (include/ape_lz4_gpu.h, lz4_sock.hip; BASELINE config 5) ----
class RxBuf:
    """APE_LZ4_rxbuf: the receive buffer of ape_socket (ref src/ape_buffer.c:210-228),
    growable and registered for DMA, with the rewritten frame parser."""

    def __init__(self, initial=0):
        self._b = lib().APE_LZ4_rxbuf_new(initial)
        if not self._b:
            raise MemoryError("APE_LZ4_rxbuf_new")

    def prepare(self, more):
        return lib().APE_LZ4_rxbuf_prepare(self._b, more)

    def append(self, data):
        data = bytes(data)
        return lib().APE_LZ4_rxbuf_append(self._b, data, len(data))

    def frames(self, max_frames, max_block):
        """(n, offsets[0..n]) of the complete frames at the start, or (-1, []) if malformed."""
        off = (_C.c_longlong * (max_frames + 1))()
        n = lib().APE_LZ4_rxbuf_frames(self._b, off, max_frames, max_block)
        return n, (list(off[:n + 1]) if n >= 0 else [])

    def consume(self, n):
        lib().APE_LZ4_rxbuf_consume(self._b, n)

    def used(self):
        return lib().APE_LZ4_rxbuf_used(self._b)

    def room(self):
        return lib().APE_LZ4_rxbuf_room(self._b)

    def pinned(self):
        return bool(lib().APE_LZ4_rxbuf_pinned(self._b))

    def data(self):
        n = self.used()
        return _C.string_at(lib().APE_LZ4_rxbuf_data(self._b), n) if n else b""

    def free(self):
        if self._b:
            lib().APE_LZ4_rxbuf_free(self._b)
            self._b = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def socket_send_blocks(fd, src, block_size, batch):
    """APE_LZ4_socket_send_blocks: rows of src (uint8 numpy [N, S] or CPU tensor, S >=
    block_size) -> GPU encode -> framed stream written to fd.  Returns bytes written."""
    n = int(src.shape[0])
    stride = int(src.strides[0]) if hasattr(src, "strides") else int(src.stride(0))
    ptr = src.ctypes.data if hasattr(src, "ctypes") else src.data_ptr()
    r = lib().APE_LZ4_socket_send_blocks(fd, _C.c_void_p(ptr), stride, block_size, n, batch)
    if r < 0:
        raise GpuError("APE_LZ4_socket_send_blocks failed (%d): %s" % (r, gpu_last_error()))
    return r


def socket_recv_blocks(fd, dst, block_size, batch, results):
    """APE_LZ4_socket_recv_blocks: framed stream read from fd -> GPU decode -> rows of dst
    (uint8 numpy [N, S]); results (int32 numpy [N]) = decompress_safe results."""
    n = int(dst.shape[0])
    r = lib().APE_LZ4_socket_recv_blocks(fd, _C.c_void_p(dst.ctypes.data), int(dst.strides[0]),
                                         block_size, n, batch, _C.c_void_p(results.ctypes.data))
    if r < 0:
        raise GpuError("APE_LZ4_socket_recv_blocks failed (%d): %s" % (r, gpu_last_error()))
    return r


class Chain:
    """APE_LZ4_chain: nconn chained socket streams in the reference wire format (8 KiB
    chunks against the stream's last 64 KiB, [int32 size][block] frames; ref
    src/ape_socket.c:811-871, :1333-1467) with the GPU codec batched across connections."""

    def __init__(self, nconn, msg_len):
        self.nconn, self.msg_len = int(nconn), int(msg_len)
        self._c = lib().APE_LZ4_chain_new(self.nconn, self.msg_len)
        if not self._c:
            raise GpuError("APE_LZ4_chain_new failed: %s" % gpu_last_error())

    def _fds(self, fds):
        if len(fds) != self.nconn:
            raise ValueError("need %d fds" % self.nconn)
        return (_C.c_int * self.nconn)(*fds)

    def _rows(self, a, what):
        """The C side takes one stride: row pitch = nconn x strides[1], >= msg_len contiguous
        bytes per row."""
        import numpy as np
        if (not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3
                or a.shape[1] != self.nconn or a.shape[2] < self.msg_len or a.strides[2] != 1
                or a.strides[1] < self.msg_len or a.strides[0] != self.nconn * a.strides[1]):
            raise ValueError("%s: need a uint8 array [nmsg, %d, >= %d] with contiguous rows"
                             % (what, self.nconn, self.msg_len))

    def send(self, fds, msgs):
        """msgs: uint8 numpy [nmsg, nconn, S >= msg_len] (round m, connection i).  Returns the
        bytes written."""
        self._rows(msgs, "msgs")
        nmsg = int(msgs.shape[0])
        r = lib().APE_LZ4_chain_send(self._c, self._fds(fds), _C.c_void_p(msgs.ctypes.data),
                                     int(msgs.strides[1]), nmsg)
        if r < 0:
            raise GpuError("APE_LZ4_chain_send failed (%d): %s" % (r, gpu_last_error()))
        return r

    def recv(self, fds, out, status):
        """out: uint8 numpy [nmsg, nconn, S >= msg_len]; status: int32 numpy [nconn].  Returns
        the payload bytes (raises on a malformed stream or a failed decode)."""
        import numpy as np
        self._rows(out, "out")
        if (not isinstance(status, np.ndarray) or status.dtype != np.int32
                or status.shape != (self.nconn,) or not status.flags["C_CONTIGUOUS"]):
            raise ValueError("status: need a contiguous int32 array [%d]" % self.nconn)
        nmsg = int(out.shape[0])
        r = lib().APE_LZ4_chain_recv(self._c, self._fds(fds), _C.c_void_p(out.ctypes.data),
                                     int(out.strides[1]), nmsg, _C.c_void_p(status.ctypes.data))
        if r < 0:
            raise GpuError("APE_LZ4_chain_recv failed (%d): %s" % (r, gpu_last_error()))
        return r

    def free(self):
        if self._c:
            lib().APE_LZ4_chain_free(self._c)
            self._c = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- the LZ4 frame format (include/ape_lz4f.h) ----
# (Public without a line in __all__, as the calls of ape_lz4_cdicts.h are; tests/test_lz4f_args.py
# checks these seven.)
LZ4F_CONTENT_CHECKSUM, LZ4F_BLOCK_CHECKSUMS, LZ4F_CONTENT_SIZE = 1, 2, 4   # compress flags
LZ4F_NO_VERIFY, LZ4F_NO_LINKED = 1, 2                                     # decompress flags


def xxh32_batch(src_ptrs, sizes, hashes, seed=0, stream=None):
    """APE_LZ4_xxh32_batch_dev: hashes[i] (int32 CUDA tensor, the hash's 32 bits) = XXH32 with
    `seed` of the max(sizes[i], 0) bytes at src_ptrs[i] (int64 CUDA tensor of pointers)."""
    what = "xxh32_batch"
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 32:
        raise ValueError("%s seed: need an int in [0, 2^32)" % what)
    n = _count(what, "sizes", sizes)
    _ptr_args(what, n, src_ptrs=src_ptrs, sizes=sizes, hashes=hashes)
    _call("APE_LZ4_xxh32_batch_dev", _ptr(src_ptrs), _ptr(sizes), seed, _ptr(hashes), n,
          _stream(stream))


def lz4f_compress_bound(src_size, flags=0):
    """APE_LZ4_lz4f_compress_bound: the most bytes a frame of src_size input bytes takes with
    these flags (0 for arguments out of range)."""
    return lib().APE_LZ4_lz4f_compress_bound(src_size, flags)


def lz4f_compress_scratch_size(nframes, max_src_size):
    """APE_LZ4_lz4f_compress_scratch_size: scratch bytes of one lz4f_compress_batch call."""
    return lib().APE_LZ4_lz4f_compress_scratch_size(nframes, max_src_size)


def lz4f_decompress_scratch_size(nframes, max_blocks):
    """APE_LZ4_lz4f_decompress_scratch_size: scratch bytes of one lz4f_decompress_batch call."""
    return lib().APE_LZ4_lz4f_decompress_scratch_size(nframes, max_blocks)


def _lz4f_batch(symbol, what, src_ptrs, sizes, dst_ptrs, caps, results, limit, flags, scratch,
                stream):
    """Both framed calls: the five arrays, a limit per frame, flags, the scratch."""
    n = _ptr_batch(what, _FIVE, src_ptrs, sizes, dst_ptrs, caps, results)
    _bytes(scratch, what + " scratch")
    _call(symbol, _ptr(src_ptrs), _ptr(sizes), _ptr(dst_ptrs), _ptr(caps), _ptr(results), n, limit,
          flags, _ptr(scratch), scratch.numel(), _stream(stream))


def lz4f_compress_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_src_size, flags,
                        scratch, stream=None):
    """APE_LZ4_lz4f_compress_batch_dev: input i -> one LZ4 frame (64 KiB independent blocks;
    flags: LZ4F_CONTENT_CHECKSUM | LZ4F_BLOCK_CHECKSUMS | LZ4F_CONTENT_SIZE) at dst_ptrs[i];
    results[i] = the frame's bytes, 0 when it does not fit caps[i] (nothing written), ERANGE
    above max_src_size.  Pointer-array form; scratch: uint8 CUDA tensor of at least
    lz4f_compress_scratch_size(N, max_src_size) bytes, 16-byte aligned.  Allocates nothing."""
    _lz4f_batch("APE_LZ4_lz4f_compress_batch_dev", "lz4f_compress_batch", src_ptrs, src_sizes,
                dst_ptrs, caps, results, max_src_size, flags, scratch, stream)


def lz4f_decompress_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_blocks, flags,
                          scratch, stream=None):
    """APE_LZ4_lz4f_decompress_batch_dev: frame i (of up to max_blocks blocks) -> its content at
    dst_ptrs[i]; results[i] = the decoded size or a negative code (include/ape_lz4f.h; flags:
    LZ4F_NO_VERIFY | LZ4F_NO_LINKED).  Pointer-array form; scratch: uint8 CUDA tensor of at least
    lz4f_decompress_scratch_size(N, max_blocks) bytes, 16-byte aligned.  Allocates nothing."""
    _lz4f_batch("APE_LZ4_lz4f_decompress_batch_dev", "lz4f_decompress_batch", src_ptrs, src_sizes,
                dst_ptrs, caps, results, max_blocks, flags, scratch, stream)


def lz4f_info_batch(src_ptrs, src_sizes, info, stream=None):
    """APE_LZ4_lz4f_info_batch_dev: info (int32 CUDA tensor of 8 N) gets, per frame, {code, FLG,
    block maximum, blocks, frame bytes, decoded bound, content size low, high (or -1, -1)}."""
    what = "lz4f_info_batch"
    n = _count(what, "src_sizes", src_sizes)
    _ptr_args(what, n, src_ptrs=src_ptrs, src_sizes=src_sizes)
    _ptr_args(what, 8 * n, info=info)
    _call("APE_LZ4_lz4f_info_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(info), n,
          _stream(stream))


# ---- frames with short blocks (include/ape_lz4f_placed.h) ----
# (Public without a line in __all__, as the calls above; tests/test_lz4f_placed_args.py checks
# these three.)
def decompress_size_ptr_batch(src_ptrs, src_sizes, caps, results, dict_sizes=None, stream=None):
    """APE_LZ4_decompress_safe_size_batch_dev: results[i] = what decompress_safe of block i
    into caps[i] bytes would return (with dict_sizes: decompress_safe_usingDict with that many
    bytes of dictionary) -- the decoded size or -(ip)-1 -- without a destination: nothing but
    results is written.  Pointer-array form, int32 tensors but src_ptrs (int64)."""
    what = "decompress_size_ptr_batch"
    n = _count(what, "src_sizes", src_sizes)
    _ptr_args(what, n, ("dict_sizes",), src_ptrs=src_ptrs, src_sizes=src_sizes, caps=caps,
              results=results, dict_sizes=dict_sizes)
    _call("APE_LZ4_decompress_safe_size_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(caps),
          _ptr(dict_sizes), _ptr(results), n, _stream(stream))


def lz4f_decompress_placed_scratch_size(nframes, max_blocks):
    """APE_LZ4_lz4f_decompress_placed_scratch_size: scratch bytes of one
    lz4f_decompress_placed_batch call."""
    return lib().APE_LZ4_lz4f_decompress_placed_scratch_size(nframes, max_blocks)


def lz4f_decompress_placed_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_blocks, flags,
                                 scratch, stream=None):
    """APE_LZ4_lz4f_decompress_placed_batch_dev: lz4f_decompress_batch for frames whose blocks
    may be short (a producer that flushes): every block is sized first and decoded where it
    belongs; results[i] = the decoded size or a negative code (include/ape_lz4f_placed.h).
    scratch: uint8 CUDA tensor of at least lz4f_decompress_placed_scratch_size(N, max_blocks)
    bytes, 16-byte aligned.  Allocates nothing."""
    _lz4f_batch("APE_LZ4_lz4f_decompress_placed_batch_dev", "lz4f_decompress_placed_batch",
                src_ptrs, src_sizes, dst_ptrs, caps, results, max_blocks, flags, scratch, stream)


# ---- frames with a dictionary (include/ape_lz4f_dict.h) ----
# (Public without a line in __all__, as the calls above; tests/test_lz4f_dict_args.py checks
# these six.)
LZ4F_ANY_BLOCK_SIZE = 4            # decompress flag of lz4f_decompress_dicts_batch: short blocks
LZ4F_NO_DICTIONARY = -10           # a frame names an ID the table has no usable entry for


def lz4f_info_dict_batch(src_ptrs, src_sizes, info, stream=None):
    """APE_LZ4_lz4f_info_dict_batch_dev: info (int32 CUDA tensor of 10 N) gets, per frame, the
    eight ints of lz4f_info_batch -- a dictionary ID is no reason for -3 -- then whether the
    frame carries the ID field and the ID (its 32 bits as an int32), or 0."""
    what = "lz4f_info_dict_batch"
    n = _count(what, "src_sizes", src_sizes)
    _ptr_args(what, n, src_ptrs=src_ptrs, src_sizes=src_sizes)
    _ptr_args(what, 10 * n, info=info)
    _call("APE_LZ4_lz4f_info_dict_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(info), n,
          _stream(stream))


def lz4f_compress_cdicts_bound(src_size, flags=0):
    """APE_LZ4_lz4f_compress_usingCDicts_bound: the most bytes a one-block dictionary frame of
    src_size (0..65536) input bytes takes with these flags (0 for arguments out of range)."""
    return lib().APE_LZ4_lz4f_compress_usingCDicts_bound(src_size, flags)


def lz4f_compress_cdicts_scratch_size(nframes, max_src_size, mode):
    """APE_LZ4_lz4f_compress_usingCDicts_scratch_size: scratch bytes of one
    lz4f_compress_cdicts_batch call in this mode."""
    return lib().APE_LZ4_lz4f_compress_usingCDicts_scratch_size(nframes, max_src_size, mode)


def lz4f_compress_cdicts_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, cdict_ptrs, dict_ids,
                               max_src_size, mode, depth, flags, scratch, stream=None):
    """APE_LZ4_lz4f_compress_usingCDicts_batch_dev: message i (at most max_src_size bytes) -> one
    LZ4 frame of one block compressed against the prepared dictionary cdict_ptrs[i] (int64 CUDA
    tensor of device pointers: objects of cdict_prepare* for mode 0, of hc_cdict_prepare* for
    this max_src_size for mode 1, the lazy parse, and 2, the cost-minimising parse; depth as in
    compress_hc_cdicts_batch, 0 with mode 0).  dict_ids: int32 CUDA tensor (the IDs' 32 bits)
    or None; the frame carries the ID field where its entry is not 0.  flags as
    lz4f_compress_batch.  A bad object gives a valid frame with a stored block.  results[i] =
    the frame's bytes, 0 when it does not fit caps[i] (nothing written), ERANGE above
    max_src_size.  scratch: uint8 CUDA tensor of at least
    lz4f_compress_cdicts_scratch_size(N, max_src_size, mode) bytes, 16-byte aligned."""
    what = "lz4f_compress_cdicts_batch"
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results, ("dict_ids",),
                   cdict_ptrs=cdict_ptrs, dict_ids=dict_ids)
    _bytes(scratch, what + " scratch")
    _call("APE_LZ4_lz4f_compress_usingCDicts_batch_dev", _ptr(src_ptrs), _ptr(src_sizes),
          _ptr(dst_ptrs), _ptr(caps), _ptr(results), n, _ptr(cdict_ptrs), _ptr(dict_ids),
          max_src_size, mode, depth, flags, _ptr(scratch), scratch.numel(), _stream(stream))


def lz4f_decompress_dicts_scratch_size(nframes, max_blocks, flags=0):
    """APE_LZ4_lz4f_decompress_usingDicts_scratch_size: scratch bytes of one
    lz4f_decompress_dicts_batch call with these flags."""
    return lib().APE_LZ4_lz4f_decompress_usingDicts_scratch_size(nframes, max_blocks, flags)


def lz4f_decompress_dicts_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_blocks,
                                table_ids, table_dict_ptrs, table_dict_sizes, flags, scratch,
                                stream=None):
    """APE_LZ4_lz4f_decompress_usingDicts_batch_dev: lz4f_decompress_batch (with
    LZ4F_ANY_BLOCK_SIZE in flags: the short-block decode) for frames written with a
    dictionary.  The table -- table_ids (int32 CUDA tensor, the IDs' 32 bits), table_dict_ptrs
    (int64) and table_dict_sizes (int32), T >= 0 entries each -- maps a dictionary ID to a
    dictionary; a frame's key is its ID, or 0 without the field, and the first entry with that
    key is used.  results[i] = the decoded size or a code; LZ4F_NO_DICTIONARY (-10) for a named
    ID without a usable entry."""
    what = "lz4f_decompress_dicts_batch"
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    t = _count(what, "table_dict_sizes", table_dict_sizes)
    _ptr_args(what, t, table_ids=table_ids, table_dict_ptrs=table_dict_ptrs,
              table_dict_sizes=table_dict_sizes)
    _bytes(scratch, what + " scratch")
    _call("APE_LZ4_lz4f_decompress_usingDicts_batch_dev", _ptr(src_ptrs), _ptr(src_sizes),
          _ptr(dst_ptrs), _ptr(caps), _ptr(results), n, max_blocks,
          _ptr(table_ids) if t else None, _ptr(table_dict_ptrs) if t else None,
          _ptr(table_dict_sizes) if t else None, t, flags, _ptr(scratch), scratch.numel(),
          _stream(stream))


SOCKET_STATS = {"tx_h2d_ms": 0, "tx_encode_ms": 1, "tx_d2h_ms": 2, "tx_write_ms": 3,
                "tx_gpu_wait_ms": 4, "tx_batches": 5, "tx_total_ms": 6, "rx_total_ms": 7,
                "rx_read_ms": 8, "rx_parse_ms": 9, "rx_h2d_ms": 10, "rx_decode_ms": 11,
                "rx_d2h_ms": 12, "rx_gpu_wait_ms": 13, "rx_batches": 14, "rx_prepare_ms": 15}


def socket_stats(reset=True):
    """APE_LZ4_socket_stats: the time split of the socket calls since the last reset."""
    out = (_C.c_double * 16)()
    if lib().APE_LZ4_socket_stats(out, 1 if reset else 0) != 0:
        raise GpuError("APE_LZ4_socket_stats failed")
    return {k: round(out[i], 3) for k, i in SOCKET_STATS.items()}


# ---- framed compress with preferences (include/ape_lz4f_prefs.h) ----
# (Public without a line in __all__, as the calls above; tests/test_lz4f_prefs_args.py checks
# these three.)
def lz4f_compress_prefs_bound(src_size, block_size_id, flags=0):
    """APE_LZ4_lz4f_compress_prefs_bound: the most bytes a frame of src_size input bytes takes at
    this block-size ID (4..7) with these flags (0 for arguments out of range)."""
    return lib().APE_LZ4_lz4f_compress_prefs_bound(src_size, block_size_id, flags)


def lz4f_compress_prefs_scratch_size(nframes, max_src_size, block_size_id, mode, pass_slices=0):
    """APE_LZ4_lz4f_compress_prefs_scratch_size: scratch bytes of one lz4f_compress_prefs_batch
    call; pass_slices as in compress_large_hc_scratch_size, ignored for mode 0."""
    return lib().APE_LZ4_lz4f_compress_prefs_scratch_size(nframes, max_src_size, block_size_id,
                                                          mode, pass_slices)


def lz4f_compress_prefs_batch(src_ptrs, src_sizes, dst_ptrs, caps, results, max_src_size,
                              block_size_id, mode, depth, flags, scratch, stream=None):
    """APE_LZ4_lz4f_compress_prefs_batch_dev: lz4f_compress_batch with a block-size ID (4..7:
    independent blocks of 64 KiB, 256 KiB, 1 MiB, 4 MiB) and an encoder (mode 0 the fast one, 1
    the high-ratio lazy parse, 2 the cost-minimising parse; depth as in compress_large_hc, 0 with
    mode 0).  A block is what the mode's compress_large* call writes for its range, or stored.
    results[i] = the frame's bytes, 0 when it does not fit caps[i] (nothing written), ERANGE above
    max_src_size.  scratch: uint8 CUDA tensor of at least
    lz4f_compress_prefs_scratch_size(N, max_src_size, block_size_id, mode, 1) bytes, 16-byte
    aligned; more, up to pass_slices = 0, means fewer passes and the same bytes."""
    what = "lz4f_compress_prefs_batch"
    n = _ptr_batch(what, _FIVE, src_ptrs, src_sizes, dst_ptrs, caps, results)
    _bytes(scratch, what + " scratch")
    _call("APE_LZ4_lz4f_compress_prefs_batch_dev", _ptr(src_ptrs), _ptr(src_sizes), _ptr(dst_ptrs),
          _ptr(caps), _ptr(results), n, max_src_size, block_size_id, mode, depth, flags,
          _ptr(scratch), scratch.numel(), _stream(stream))
