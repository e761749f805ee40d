"""The high-ratio mode with history and on large inputs, on the GPU:
APE_LZ4_compress_hc_withPrefix_batch_dev and APE_LZ4_compress_large_hc_batch_dev write, byte for
byte, what tests/hclargemodel.py defines for (input bytes, used history, depth, restartBytes) --
whatever the batch, the alignment, the scratch size or the stream -- and the GPU's own decoders
(whole block, with a dictionary, by segments, by byte range) restore the input."""
import functools
import struct

import pytest

import hclargemodel as M
import hcmodel
import indexutil
from gpuutil import CANARY, alloc_out, fetch, ints, pack
from lz4util import I, orc_decompress
from test_hc_large_model import PREFIXES, data, gpu_large_inputs
from test_hc_model import SIZES

pytestmark = pytest.mark.gpu

ERANGE = -2147483648
EINVAL = -2
POISON = -7


# ---- the call with history ----
@functools.lru_cache(maxsize=None)
def prefix_cases(big_only=False):
    """[(window, used history, offered prefix)]: every size x every prefix over the contents in
    turn, a few sizes with more history offered than a window holds, and the large blocks."""
    out = []
    if not big_only:
        k = 0
        for n in SIZES:
            for pre in PREFIXES + ([65536 - n + 9] if n in (0, 13, 277, 4096) else []):
                whole = _history_and_block(I.ENC_CONTENTS[k % len(I.ENC_CONTENTS)])
                h = M.used_history(pre, n)
                out.append((whole[65536 - h:65536 + n], h, pre))
                k += 1
    text, comp = _history_and_block("text"), _history_and_block("comp")
    out.append((text[:65536], 32768, 32768))
    out.append((comp[:65536], 64, 64))
    out.append((text[4096:4096 + 65536], 64, 70000))     # clamps to 65536 - size
    return out


@functools.lru_cache(maxsize=None)
def _history_and_block(content):
    return I.make(content, 65536 + 4096, seed=11)


@functools.lru_cache(maxsize=None)
def prefix_model(depth, big_only=False):
    return [M.compress_prefix(w, h, depth) for w, h, _ in prefix_cases(big_only)]


def encode_prefix(torch, amd, cases, depth, with_prefix=True):
    """One compress_hc_prefix_ptr_batch call; window bases at every residue of 16."""
    n = len(cases)
    src, wptr, _ = pack(torch, [w for w, _, _ in cases], misalign=[i % 16 for i in range(n)])
    hist = torch.tensor([h for _, h, _ in cases], dtype=torch.int64, device="cuda")
    sptr = wptr + hist
    sizes = [len(w) - h for w, h, _ in cases]
    caps = [amd.compressBound(s) for s in sizes]
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [POISON] * n)
    scratch = torch.full((amd.compress_hc_scratch_size(n),), 0xEE, dtype=torch.uint8, device="cuda")
    amd.compress_hc_prefix_ptr_batch(sptr, ints(torch, sizes),
                                     ints(torch, [p for _, _, p in cases]) if with_prefix else None,
                                     dptr, ints(torch, caps), res, depth, scratch)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    outs = [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)]
    # back through the GPU's usingDict decoder, the history as the dictionary
    back, bptr, boffs = alloc_out(torch, sizes)
    bres = ints(torch, [POISON] * n)
    amd.decompress_dict_batch(dptr, res, bptr, ints(torch, sizes), wptr,
                              ints(torch, [h for _, h, _ in cases]), bres)
    torch.cuda.synchronize()
    plain = [(r, fetch(back, o, max(r, 0))) for o, r in zip(boffs, bres.cpu().tolist())]
    return rs, outs, plain


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            at = next((j for j, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            return "block %d: %d bytes, model %d, first difference at %d" % (i, len(g), len(w), at)
    return None


@pytest.mark.parametrize("depth", [1, 8, 64, 256])
def test_prefix_bytes_are_the_models_and_decode(product, cuda, depth):
    big_only = depth == 256
    cases, want = prefix_cases(big_only), prefix_model(depth, big_only)
    rs, outs, plain = encode_prefix(cuda, product, cases, depth)
    assert rs == [len(w) for w in want], first_difference(outs, want)
    assert outs == want, first_difference(outs, want)
    assert plain == [(len(w) - h, w[h:]) for w, h, _ in cases]


def test_a_null_prefix_array_is_the_plain_call(product, cuda):
    cases = prefix_cases()[::7] + prefix_cases()[-3:]
    blocks = [w[h:] for w, h, _ in cases]
    rs, outs, _ = encode_prefix(cuda, product, [(b, 0, 0) for b in blocks], 8, with_prefix=False)
    n = len(blocks)
    src, sptr, _ = pack(cuda, blocks)
    caps = [product.compressBound(len(b)) for b in blocks]
    dst, dptr, doffs = alloc_out(cuda, caps)
    res = ints(cuda, [POISON] * n)
    scratch = cuda.empty(product.compress_hc_scratch_size(n), dtype=cuda.uint8, device="cuda")
    product.compress_hc_ptr_batch(sptr, ints(cuda, map(len, blocks)), dptr, ints(cuda, caps), res, 8,
                                  scratch)
    cuda.cuda.synchronize()
    plain_rs = res.cpu().tolist()
    assert rs == plain_rs == [len(hcmodel.compress(b, 8)) for b in blocks]
    assert outs == [fetch(dst, o, r) for o, r in zip(doffs, plain_rs)]


# ---- the large call ----
@functools.lru_cache(maxsize=None)
def S():
    import libapenetwork_amd as amd
    return amd.compress_large_slice_size()


@functools.lru_cache(maxsize=None)
def inputs():
    return dict(gpu_large_inputs(S()))


@functools.lru_cache(maxsize=None)
def model(name, depth, restart=0):
    return M.compress_large(inputs()[name], depth, restart, S=S())


class Run:
    pass


def run_large(torch, amd, srcs, depth, restart=0, index=False, caps=None, sizes=None, max_src=None,
              pass_slices=0, stream=None, sync=True):
    """One compress_large_hc_ptr_batch launch; sources and destinations at every residue of 16."""
    d = Run()
    nb = len(srcs)
    max_src = max(map(len, srcs)) if max_src is None else max_src
    d.src, sptr, _ = pack(torch, srcs, misalign=[(5 * i + 1) % 16 for i in range(nb)])
    d.caps = [amd.compressBound(len(s)) for s in srcs] if caps is None else caps
    d.dst, d.dptr, d.doffs = alloc_out(torch, d.caps, misalign=[(3 * i) % 16 for i in range(nb)])
    d.res = ints(torch, [POISON] * nb)
    d.index, d.max_seg = None, amd.large_index_segments(max_src, restart)
    if index:
        d.stride = amd.large_index_size(max_src, restart)
        d.index = torch.zeros((nb, d.stride), dtype=torch.uint8, device="cuda")
    need = amd.compress_large_hc_scratch_size(nb, max_src, pass_slices)
    d.scratch = torch.full((need,), 0xEE, dtype=torch.uint8, device="cuda")
    d.args = (sptr, ints(torch, sizes or map(len, srcs)), d.dptr, ints(torch, d.caps), d.res)
    if stream is not None:   # the buffers above were filled on the current stream
        stream.wait_stream(torch.cuda.current_stream())
    amd.compress_large_hc_ptr_batch(*d.args, max_src, depth, restart_bytes=restart, index=d.index,
                                    scratch=d.scratch, stream=stream)
    return collect(torch, d) if sync else d


def collect(torch, d):
    torch.cuda.synchronize()
    d.rs = d.res.cpu().tolist()
    host = d.dst.cpu().numpy()
    d.outs = [host[o:o + max(r, 0)].tobytes() for o, r in zip(d.doffs, d.rs)]
    if d.index is not None:
        raw = d.index.cpu().numpy()
        words = [struct.unpack("<%dI" % (d.stride // 4), raw[i].tobytes()) for i in range(len(d.rs))]
        d.words = [list(w[:4 + 2 * (w[1] + 1)]) for w in words]
    return d


def gpu_decode(torch, amd, d, srcs):
    back, bptr, boffs = alloc_out(torch, [len(s) for s in srcs])
    res = ints(torch, [POISON] * len(srcs))
    amd.decompress_ptr_batch(d.dptr, d.res, bptr, ints(torch, map(len, srcs)), res)
    torch.cuda.synchronize()
    return [(r, fetch(back, o, max(r, 0))) for o, r in zip(boffs, res.cpu().tolist())]


def untouched(dst, off, lo, hi):
    return fetch(dst, off + lo, hi - lo) == bytes([CANARY]) * (hi - lo)


def test_large_bytes_are_the_models_and_decode(product, cuda, oracle):
    names = list(inputs())
    srcs = [inputs()[nm] for nm in names]
    want = [model(nm, 8) for nm in names]
    d = run_large(cuda, product, srcs, 8)
    assert d.rs == [len(w) for w in want], first_difference(d.outs, want)
    assert d.outs == want, first_difference(d.outs, want)
    for s, c in zip(srcs, d.outs):
        assert orc_decompress(oracle, c, len(s)) == (len(s), s)
    assert gpu_decode(cuda, product, d, srcs) == [(len(s), s) for s in srcs]


def test_large_depth_64(product, cuda, oracle):
    names = ["text 200000", "comp 200000"]
    srcs = [inputs()[nm] for nm in names]
    want = [model(nm, 64) for nm in names]
    d = run_large(cuda, product, srcs, 64)
    assert (d.rs, d.outs) == ([len(w) for w in want], want), first_difference(d.outs, want)
    for s, c in zip(srcs, d.outs):
        assert orc_decompress(oracle, c, len(s)) == (len(s), s)
    assert gpu_decode(cuda, product, d, srcs) == [(len(s), s) for s in srcs]
    d0 = run_large(cuda, product, srcs, 0)      # depth 0 is the default, 64
    assert (d0.rs, d0.outs) == (d.rs, d.outs)


@pytest.mark.parametrize("mult", [1, 2])
def test_restart_points_and_the_index(product, cuda, mult):
    R = mult * S()
    names = ["comp 200000", "text 200000", "mixed"]
    srcs = [inputs()[nm] for nm in names]
    want = [model(nm, 8, R) for nm in names]
    d = run_large(cuda, product, srcs, 8, restart=R, index=True)
    assert (d.rs, d.outs) == ([len(w) for w in want], want), first_difference(d.outs, want)
    assert d.words == [indexutil.build_index(w, range(0, len(s), R)) for w, s in zip(want, srcs)]
    # the segment-parallel decoder
    nb = len(srcs)
    back, bptr, boffs = alloc_out(cuda, [len(s) for s in srcs])
    res = ints(cuda, [POISON] * nb)
    product.decompress_indexed_ptr_batch(d.dptr, d.res, bptr, ints(cuda, map(len, srcs)), d.index,
                                         d.max_seg, res)
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == [len(s) for s in srcs]
    assert [fetch(back, o, len(s)) for o, s in zip(boffs, srcs)] == srcs
    # one range read per block, across the restart point at 2 R
    a, ln = 2 * R - 1000, 3000
    rcaps = [len(s) + 64 for s in srcs]   # (a segment's literals may begin long before it)
    out, optr, ooffs = alloc_out(cuda, rcaps)
    win, rres = ints(cuda, [POISON] * (2 * nb)), ints(cuda, [POISON] * nb)
    product.decompress_range_indexed_ptr_batch(d.dptr, d.res, d.index, d.max_seg, ints(cuda, [a] * nb),
                                               ints(cuda, [ln] * nb), optr, ints(cuda, rcaps), win, rres)
    cuda.cuda.synchronize()
    w = win.cpu().tolist()
    assert rres.cpu().tolist() == [ln] * nb
    assert [fetch(out, o + w[2 * k], ln) for k, o in enumerate(ooffs)] == [s[a:a + ln] for s in srcs]


def pass_inputs():
    names = ["comp 200000", "text 65537", "comp %d" % (3 * S() + 13)]
    return names, [inputs()[nm] for nm in names] + [data("comp", 4096)]


def pass_model():
    names, srcs = pass_inputs()
    return [model(nm, 8) for nm in names] + [hcmodel.compress(srcs[-1], 8)]


@pytest.mark.parametrize("pass_slices", [1, 3, 0])
def test_a_smaller_scratch_runs_passes_with_the_same_bytes(product, cuda, pass_slices):
    _, srcs = pass_inputs()
    want = pass_model()
    sizes = [product.compress_large_hc_scratch_size(len(srcs), 200000, p) for p in (1, 3, 0)]
    assert sizes == sorted(sizes) and sizes[1] - sizes[0] == 2 * 65536 * 6
    d = run_large(cuda, product, srcs, 8, pass_slices=pass_slices)
    assert (d.rs, d.outs) == ([len(w) for w in want], want), first_difference(d.outs, want)


def test_two_streams_give_the_same_bytes(product, cuda):
    _, srcs = pass_inputs()
    want = pass_model()
    s1, s2 = cuda.cuda.Stream(), cuda.cuda.Stream()
    k1 = run_large(cuda, product, srcs, 8, stream=s1, sync=False)
    k2 = run_large(cuda, product, srcs, 8, pass_slices=5, stream=s2, sync=False)
    for d in (collect(cuda, k1), collect(cuda, k2)):
        assert (d.rs, d.outs) == ([len(w) for w in want], want)


def test_small_inputs_are_the_block_call(product, cuda):
    """Inputs of at most 65536 bytes beside a large one: compress_hc_ptr_batch's bytes."""
    small = [data("comp", n) for n in (0, 1, 12, 13, 4096, 65536)] + [data("text", 65536)]
    srcs = small[:3] + [inputs()["comp 200000"]] + small[3:]
    d = run_large(cuda, product, srcs, 8)
    n = len(small)
    src, sptr, _ = pack(cuda, small)
    caps = [product.compressBound(len(b)) for b in small]
    dst, dptr, doffs = alloc_out(cuda, caps)
    res = ints(cuda, [POISON] * n)
    scratch = cuda.empty(product.compress_hc_scratch_size(n), dtype=cuda.uint8, device="cuda")
    product.compress_hc_ptr_batch(sptr, ints(cuda, map(len, small)), dptr, ints(cuda, caps), res, 8,
                                  scratch)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    plain = [fetch(dst, o, r) for o, r in zip(doffs, rs)]
    assert plain == [hcmodel.compress(b, 8) for b in small]
    assert d.rs[:3] + d.rs[4:] == rs and d.outs[:3] + d.outs[4:] == plain
    assert d.outs[3] == model("comp 200000", 8)
    # all of them small: one slot per input, nothing to stitch
    d = run_large(cuda, product, small, 8, max_src=65536)
    assert (d.rs, d.outs) == (rs, plain)


def test_capacity_and_sizes_out_of_range(product, cuda):
    names, srcs = pass_inputs()
    want = pass_model()
    exact = [len(w) for w in want]
    d = run_large(cuda, product, srcs, 8, caps=exact)
    assert (d.rs, d.outs) == (exact, want)
    d = run_large(cuda, product, srcs, 8, caps=[c - 1 for c in exact])
    assert d.rs == [0] * len(srcs)
    for o, c in list(zip(d.doffs, exact))[:3]:   # (the small one is encoded in place, inside cap)
        assert untouched(d.dst, o, 0, c + 64)
    # one short capacity among exact ones: the neighbours are unaffected
    caps = list(exact)
    caps[0] -= 1
    d = run_large(cuda, product, srcs, 8, caps=caps)
    assert d.rs == [0] + exact[1:] and d.outs[1:] == want[1:]
    assert untouched(d.dst, d.doffs[0], 0, exact[0] + 64)
    # a negative size and one above maxSrcSize: 0 and ERANGE, the rest as ever
    sizes = [len(s) for s in srcs]
    sizes[1], sizes[2] = -1, 200001
    d = run_large(cuda, product, srcs, 8, sizes=sizes, max_src=200000)
    assert d.rs == [exact[0], 0, ERANGE, exact[3]]
    assert d.outs[0] == want[0] and d.outs[3] == want[3]
    for k in (1, 2):
        assert untouched(d.dst, d.doffs[k], 0, d.caps[k] + 64)


def test_errors_launch_nothing(product, cuda):
    _, srcs = pass_inputs()
    want = pass_model()
    nb, max_src, R = len(srcs), 200000, S()
    L = product.lib()
    need = product.compress_large_hc_scratch_size(nb, max_src, 1)
    scr = cuda.empty(need + 16, dtype=cuda.uint8, device="cuda")
    assert scr.data_ptr() % 16 == 0
    src, sptr, _ = pack(cuda, srcs)
    caps = [product.compressBound(len(s)) for s in srcs]
    dst, dptr, doffs = alloc_out(cuda, caps)
    szs, cps, res = ints(cuda, map(len, srcs)), ints(cuda, caps), ints(cuda, [POISON] * nb)
    stride = product.large_index_size(max_src, R)
    index = cuda.zeros((nb, stride + 16), dtype=cuda.uint8, device="cuda")
    arrays = [sptr.data_ptr(), szs.data_ptr(), dptr.data_ptr(), cps.data_ptr(), res.data_ptr()]

    def call(arrays=arrays, n=nb, max_src=max_src, depth=8, base=scr.data_ptr(), nbytes=need,
             restart=0, ix=None, ix_stride=0):
        return L.APE_LZ4_compress_large_hc_batch_dev(*arrays, n, max_src, depth, base, nbytes,
                                                     restart, ix, ix_stride, None)

    for hole in range(5):
        assert call(arrays=arrays[:hole] + [None] + arrays[hole + 1:]) == EINVAL
    assert call(n=-1) == EINVAL
    for depth in (-1, 257):
        assert call(depth=depth) == EINVAL
    assert call(base=None) == EINVAL
    assert call(base=scr.data_ptr() + 8) == EINVAL
    assert call(nbytes=need - 1) == EINVAL
    assert str(need) in product.gpu_last_error()
    assert call(max_src=0) == EINVAL and call(max_src=0x7E000001) == EINVAL
    for restart in (R + 64, -R, 1):
        assert call(restart=restart) == EINVAL
    assert call(restart=R, ix=index.data_ptr() + 8, ix_stride=stride + 16) == EINVAL
    assert call(restart=R, ix=index.data_ptr(), ix_stride=stride + 8) == EINVAL
    assert call(restart=R, ix=index.data_ptr(), ix_stride=stride - 16) == EINVAL
    assert call(n=0) == 0
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == [POISON] * nb   # none of these launched anything
    assert call(restart=R, ix=index.data_ptr(), ix_stride=stride + 16) == 0
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    assert all(r > 0 for r in rs) and rs[3] == len(want[3])

    # the binding's checks
    with pytest.raises(ValueError):
        product.compress_large_hc_ptr_batch(sptr, None, dptr, cps, res, max_src, 8)
    with pytest.raises(ValueError):
        product.compress_large_hc_ptr_batch(sptr, szs.cpu(), dptr, cps, res, max_src, 8)
    with pytest.raises(ValueError):
        product.compress_large_hc_ptr_batch(sptr, szs, dptr, cps, res, max_src, 8, scratch=scr.cpu())
    with pytest.raises(ValueError):
        product.compress_hc_prefix_ptr_batch(sptr, None, szs, dptr, cps, res, 8, scr)
    with pytest.raises(ValueError):
        product.compress_hc_prefix_ptr_batch(sptr, szs, szs.cpu(), dptr, cps, res, 8, scr)
    f = product.compress_large_hc_scratch_size
    assert f(-1, max_src, 0) == 0 and f(1, 0, 0) == 0 and f(1, 0x7E000001, 0) == 0 and f(1, 1, -1) == 0
    assert f(1 << 20, 1 << 20, 0) == 2 ** 64 - 1
    assert f(nb, max_src, 0) == f(nb, max_src, 10 ** 6) == \
        product.compress_large_scratch_size(nb, max_src) + nb * ((max_src + R - 1) // R) * 65536 * 6


def test_the_call_captures_into_a_graph(product, cuda):
    """No allocation and no sync: a scratch of 15 slices for 28 (two passes) captured on a side
    stream, replayed twice over a scratch refilled with garbage."""
    _, srcs = pass_inputs()
    want = pass_model()
    nb = len(srcs)
    src, sptr, _ = pack(cuda, srcs)
    caps = [product.compressBound(len(s)) for s in srcs]
    dst, dptr, doffs = alloc_out(cuda, caps)
    szs, cps, res = ints(cuda, map(len, srcs)), ints(cuda, caps), ints(cuda, [POISON] * nb)
    scratch = cuda.full((product.compress_large_hc_scratch_size(nb, 200000, 15),), 0xEE,
                        dtype=cuda.uint8, device="cuda")
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.compress_large_hc_ptr_batch(sptr, szs, dptr, cps, res, 200000, 8, scratch=scratch,
                                            stream=s)
    for _ in range(2):
        res.fill_(POISON)
        scratch.fill_(0x11)
        g.replay()
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    assert rs == [len(w) for w in want]
    assert [fetch(dst, o, r) for o, r in zip(doffs, rs)] == want
