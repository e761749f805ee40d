"""The cost-minimising parse on large and indexed blocks, on the GPU:
APE_LZ4_compress_large_hc_opt_batch_dev writes, byte for byte, what tests/hcoptmodel.py
compress_large() defines for (input bytes, used history, depth, restartBytes) -- whatever the
scratch size -- its index is tests/indexutil.py's, and the GPU's own decoders (whole block, by
segments, by byte range) restore the input."""
import functools

import pytest

import hcoptmodel as M
import indexutil
from gpuutil import alloc_out, fetch, ints, pack
from lz4util import orc_decompress
from test_gpu_hc_large import Run, S, collect, first_difference, gpu_decode, untouched
from test_hc_large_model import data

pytestmark = pytest.mark.gpu

POISON = -7
DEPTH = 8


@functools.lru_cache(maxsize=None)
def inputs():
    s = S()
    out = {"comp 65536": data("comp", 65536), "text 65537": data("text", 65537),
           "comp 200000": data("comp", 200000), "text 200000": data("text", 200000),
           "zeros 200000": bytes(200000)}
    for c in ("comp", "text", "zeros"):
        out["%s %d" % (c, 3 * s + 5)] = data(c, 3 * s + 5)
    return out


@functools.lru_cache(maxsize=None)
def model(name, restart=0):
    return M.compress_large(inputs()[name], DEPTH, restart, S=S())


def run_large(torch, amd, srcs, restart=0, index=False, caps=None, max_src=None, pass_slices=0):
    """One compress_large_hc_opt_ptr_batch launch; sources and destinations at every residue of
    16, the scratch filled with 0xEE."""
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
    need = amd.compress_large_hc_opt_scratch_size(nb, max_src, pass_slices)
    d.scratch = torch.full((need,), 0xEE, dtype=torch.uint8, device="cuda")
    d.args = (sptr, ints(torch, map(len, srcs)), d.dptr, ints(torch, d.caps), d.res)
    amd.compress_large_hc_opt_ptr_batch(*d.args, max_src, DEPTH, restart_bytes=restart,
                                        index=d.index, scratch=d.scratch)
    return collect(torch, d)


@pytest.mark.parametrize("restart_slices", [0, 2])
@pytest.mark.parametrize("index", [False, True])
def test_large_bytes_are_the_models_and_decode(product, cuda, oracle, restart_slices, index):
    R = restart_slices * S()
    names = list(inputs())
    srcs = [inputs()[nm] for nm in names]
    want = [model(nm, R) for nm in names]
    d = run_large(cuda, product, srcs, restart=R, index=index)
    assert d.rs == [len(w) for w in want], first_difference(d.outs, want)
    assert d.outs == want, first_difference(d.outs, want)
    for s, c in zip(srcs, d.outs):
        assert orc_decompress(oracle, c, len(s)) == (len(s), s)
    assert gpu_decode(cuda, product, d, srcs) == [(len(s), s) for s in srcs]
    if not index:
        return
    assert d.words == [indexutil.build_index(w, range(0, len(s), R)) if R else
                       indexutil.trivial_index(len(w), len(s)) for w, s in zip(want, srcs)]
    # the segment-parallel decoder
    nb = len(srcs)
    back, bptr, boffs = alloc_out(cuda, [len(s) for s in srcs])
    res = ints(cuda, [POISON] * nb)
    product.decompress_indexed_ptr_batch(d.dptr, d.res, bptr, ints(cuda, map(len, srcs)), d.index,
                                         d.max_seg, res)
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == [len(s) for s in srcs]
    assert [fetch(back, o, len(s)) for o, s in zip(boffs, srcs)] == srcs
    # one range read per block, across the restart point at 2 S (or inside the one segment)
    a, ln = 2 * S() - 1000, 3000
    lens = [min(ln, len(s) - a) for s in srcs]
    rcaps = [len(s) + 64 for s in srcs]   # (a segment's literals may begin long before it)
    out, optr, ooffs = alloc_out(cuda, rcaps)
    win, rres = ints(cuda, [POISON] * (2 * nb)), ints(cuda, [POISON] * nb)
    product.decompress_range_indexed_ptr_batch(d.dptr, d.res, d.index, d.max_seg,
                                               ints(cuda, [a] * nb), ints(cuda, lens), optr,
                                               ints(cuda, rcaps), win, rres)
    cuda.cuda.synchronize()
    w = win.cpu().tolist()
    assert rres.cpu().tolist() == lens
    assert [fetch(out, o + w[2 * k], lens[k]) for k, o in enumerate(ooffs)] == \
        [s[a:a + n] for s, n in zip(srcs, lens)]


def test_an_input_of_one_block_is_the_block_call(product, cuda):
    small = [data("comp", n) for n in (0, 12, 13, 4096, 65536)]
    d = run_large(cuda, product, small + [inputs()["comp 200000"]])
    want = [M.compress(b, DEPTH) for b in small]
    assert d.outs[:-1] == want and d.outs[-1] == model("comp 200000")
    d = run_large(cuda, product, small, max_src=65536)
    assert (d.rs, d.outs) == ([len(w) for w in want], want)


@pytest.mark.parametrize("pass_slices", [1, 0])
def test_one_slice_of_scratch_against_all_of_it(product, cuda, pass_slices):
    names = ["comp 200000", "text 65537", "zeros %d" % (3 * S() + 5), "comp 65536"]
    srcs = [inputs()[nm] for nm in names]
    want = [model(nm) for nm in names]
    f = product.compress_large_hc_opt_scratch_size
    assert f(len(srcs), 200000, 2) - f(len(srcs), 200000, 1) == 65536 * 10
    d = run_large(cuda, product, srcs, pass_slices=pass_slices)
    assert (d.rs, d.outs) == ([len(w) for w in want], want), first_difference(d.outs, want)


def test_a_capacity_one_below_the_size(product, cuda):
    names = ["comp 200000", "text 65537", "comp 65536"]
    srcs = [inputs()[nm] for nm in names]
    exact = [len(model(nm)) for nm in names]
    d = run_large(cuda, product, srcs, caps=exact)
    assert (d.rs, d.outs) == (exact, [model(nm) for nm in names])
    d = run_large(cuda, product, srcs, caps=[c - 1 for c in exact])
    assert d.rs == [0] * len(srcs)
    for o, c in zip(d.doffs, exact):   # nothing is written, for the small input either
        assert untouched(d.dst, o, 0, c + 32)
    caps = [exact[0] - 1] + exact[1:]
    d = run_large(cuda, product, srcs, caps=caps)
    assert d.rs == [0] + exact[1:] and d.outs[1:] == [model(nm) for nm in names[1:]]
    assert untouched(d.dst, d.doffs[0], 0, exact[0] + 32)
