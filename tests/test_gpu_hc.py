"""The high-ratio mode on the GPU: APE_LZ4_compress_hc_batch_dev writes, byte for byte, what
tests/hcmodel.py defines for (input bytes, depth) -- whatever the batch, the alignment, the
scratch size or the stream -- and the GPU's own decoder restores the input."""
import functools

import pytest

import hcmodel
from gpuutil import alloc_out, ints, pack
from lz4util import I
from test_hc_model import SIZES

pytestmark = pytest.mark.gpu

ERANGE = -2147483648
DEPTHS = (1, 8, 64, 256)


@functools.lru_cache(maxsize=None)
def blocks():
    """The CPU size grid over every content, then six 64 KiB blocks."""
    out = [I.make(c, n, seed=n) for c in I.ENC_CONTENTS for n in SIZES]
    out += [I.make("text", 65536, seed=1), I.make("comp", 65536, seed=3),
            I.make("zeros", 65536), I.make("period3", 65536), I.make("rand", 65536),
            I.make("comp", 65535, seed=5)]
    return out


@functools.lru_cache(maxsize=None)
def model(depth):
    return [hcmodel.compress(b, depth) for b in blocks()]


def encode(torch, amd, blobs, depth, caps=None, sizes=None, scratch_blocks=None, stream=None,
           sync=True):
    """(results, outputs) of one compress_hc_ptr_batch call; sources and destinations start at
    every residue of 16."""
    n = len(blobs)
    src, sptr, _ = pack(torch, blobs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [amd.compressBound(len(b)) for b in blobs] if caps is None else caps
    sizes = [len(b) for b in blobs] if sizes is None else sizes
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [-7] * n)
    nscr = amd.compress_hc_scratch_size(max(n, 1) if scratch_blocks is None else scratch_blocks)
    scratch = torch.full((nscr,), 0xEE, dtype=torch.uint8, device="cuda")
    if stream is not None:   # the buffers above were filled on the current stream
        stream.wait_stream(torch.cuda.current_stream())
    sizes, caps = ints(torch, sizes), ints(torch, caps)
    amd.compress_hc_ptr_batch(sptr, sizes, dptr, caps, res, depth, scratch, stream=stream)
    if not sync:   # (with everything the call still reads or writes kept alive)
        return res, dst, doffs, (src, sptr, dptr, sizes, caps, scratch)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    return rs, [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)]


def gpu_decode(torch, amd, comps, sizes):
    src, sptr, _ = pack(torch, comps)
    dst, dptr, doffs = alloc_out(torch, sizes)
    res = ints(torch, [-7] * len(comps))
    amd.decompress_ptr_batch(sptr, ints(torch, map(len, comps)), dptr, ints(torch, sizes), res)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    return [(r, host[o:o + max(r, 0)].tobytes()) for o, r in zip(doffs, rs)]


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            at = next((j for j, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            return "block %d (%d bytes in): %d bytes, model %d, first difference at %d" % (
                i, len(blocks()[i]), len(g), len(w), at)
    return None


@pytest.mark.parametrize("depth", DEPTHS)
def test_bytes_are_the_models_and_decode(product, cuda, depth):
    want = model(depth)
    rs, outs = encode(cuda, product, blocks(), depth)
    assert rs == [len(w) for w in want], first_difference(outs, want)
    assert outs == want, first_difference(outs, want)
    got = gpu_decode(cuda, product, outs, [len(b) for b in blocks()])
    assert got == [(len(b), b) for b in blocks()]


def test_default_depth_is_64(product, cuda):
    pick = blocks()[-6:-4] + blocks()[100:110]
    want = [hcmodel.compress(b, 64) for b in pick]
    assert encode(cuda, product, pick, 0) == ([len(w) for w in want], want)


def test_capacity(product, cuda):
    idx = [len(blocks()) - 6, len(blocks()) - 4, len(blocks()) - 2, 24, 100, 0]
    pick = [blocks()[i] for i in idx]
    want = [model(8)[i] for i in idx]
    exact = [len(w) for w in want]
    assert encode(cuda, product, pick, 8, caps=exact) == (exact, want)
    for caps in ([c - 1 for c in exact], [0] * len(pick), [-1] * len(pick)):
        rs, _ = encode(cuda, product, pick, 8, caps=caps)
        assert rs == [0] * len(pick), caps
    # one short capacity among exact ones: the neighbours are unaffected
    caps = list(exact)
    caps[1] -= 1
    rs, outs = encode(cuda, product, pick, 8, caps=caps)
    assert rs[1] == 0
    assert [(r, o) for i, (r, o) in enumerate(zip(rs, outs)) if i != 1] == \
        [(len(w), w) for i, w in enumerate(want) if i != 1]


def test_sizes_out_of_range(product, cuda):
    idx = list(range(90, 97)) + [len(blocks()) - 5]
    pick = [blocks()[i] for i in idx]
    want = [model(64)[i] for i in idx]
    sizes = [len(b) for b in pick]
    sizes[2], sizes[5] = 65537, -1
    rs, outs = encode(cuda, product, pick, 64, sizes=sizes)
    assert rs[2] == ERANGE and rs[5] == 0
    for i in range(len(pick)):
        if i not in (2, 5):
            assert (rs[i], outs[i]) == (len(want[i]), want[i]), i


@pytest.mark.parametrize("scratch_blocks", [1, 7])
def test_a_smaller_scratch_runs_passes_with_the_same_bytes(product, cuda, scratch_blocks):
    want = model(8)
    rs, outs = encode(cuda, product, blocks(), 8, scratch_blocks=scratch_blocks)
    assert rs == [len(w) for w in want] and outs == want, first_difference(outs, want)


def test_two_streams_give_the_same_bytes(product, cuda):
    want = model(64)
    s1, s2 = cuda.cuda.Stream(), cuda.cuda.Stream()
    k1 = encode(cuda, product, blocks(), 64, stream=s1, sync=False)
    k2 = encode(cuda, product, blocks(), 64, stream=s2, sync=False)
    cuda.cuda.synchronize()
    for res, dst, doffs, _ in (k1, k2):
        rs, host = res.cpu().tolist(), dst.cpu().numpy()
        assert rs == [len(w) for w in want]
        assert [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)] == want


def test_no_blocks(product, cuda):
    rs, outs = encode(cuda, product, [], 64)
    assert rs == [] and outs == []
    scratch = cuda.zeros(product.compress_hc_scratch_size(1), dtype=cuda.uint8, device="cuda")
    rc = product.lib().APE_LZ4_compress_hc_batch_dev(None, None, None, None, None, 0, 64,
                                                     scratch.data_ptr(), scratch.numel(), None)
    assert rc == 0


def test_the_call_captures_into_a_graph(product, cuda):
    """No allocation and no sync: two passes (a scratch of 7 blocks for 12) captured, replayed."""
    pick = blocks()[-6:-4] + blocks()[100:110]
    want = [hcmodel.compress(b, 8) for b in pick]
    n = len(pick)
    src, sptr, _ = pack(cuda, pick, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [product.compressBound(len(b)) for b in pick]
    dst, dptr, doffs = alloc_out(cuda, caps, misalign=[(3 * i) % 16 for i in range(n)])
    sizes, capt, res = ints(cuda, map(len, pick)), ints(cuda, caps), ints(cuda, [-7] * n)
    scratch = cuda.full((product.compress_hc_scratch_size(7),), 0xEE, dtype=cuda.uint8,
                        device="cuda")
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.compress_hc_ptr_batch(sptr, sizes, dptr, capt, res, 8, scratch, stream=s)
    for _ in range(2):
        res.fill_(-7)
        scratch.fill_(0x11)
        g.replay()
    cuda.cuda.synchronize()
    rs, host = res.cpu().tolist(), dst.cpu().numpy()
    assert rs == [len(w) for w in want]
    assert [host[o:o + r].tobytes() for o, r in zip(doffs, rs)] == want
