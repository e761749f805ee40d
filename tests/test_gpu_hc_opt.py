"""The high-ratio mode's cost-minimising parse on the GPU: APE_LZ4_compress_hc_opt_batch_dev and
its withPrefix form write, byte for byte, what tests/hcoptmodel.py defines for (input bytes, used
history, depth) -- whatever the batch, the alignment, the scratch's size and content or the
stream -- the GPU's own decoders restore the input, and the lazy call beside it keeps its bytes."""
import functools

import pytest

import hcmodel
import hcoptmodel as M
from gpuutil import CANARY, alloc_out, fetch, ints, pack
from lz4util import I
from test_gpu_hc import DEPTHS, ERANGE, blocks, first_difference, gpu_decode
from test_gpu_hc import encode as lazy_encode

pytestmark = pytest.mark.gpu

POISON = -7


@functools.lru_cache(maxsize=None)
def model(depth):
    return [M.compress(b, depth) for b in blocks()]


def encode(torch, amd, blobs, depth, caps=None, sizes=None, scratch_blocks=None, stream=None,
           sync=True, poison=0xEE):
    """(results, outputs) of one compress_hc_opt_ptr_batch call; sources and destinations start
    at every residue of 16, the scratch is filled with `poison`."""
    n = len(blobs)
    src, sptr, _ = pack(torch, blobs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [amd.compressBound(len(b)) for b in blobs] if caps is None else caps
    sizes = [len(b) for b in blobs] if sizes is None else sizes
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [POISON] * n)
    nscr = amd.compress_hc_opt_scratch_size(max(n, 1) if scratch_blocks is None else scratch_blocks)
    scratch = torch.full((nscr,), poison, dtype=torch.uint8, device="cuda")
    if stream is not None:   # the buffers above were filled on the current stream
        stream.wait_stream(torch.cuda.current_stream())
    sizes, caps = ints(torch, sizes), ints(torch, caps)
    amd.compress_hc_opt_ptr_batch(sptr, sizes, dptr, caps, res, depth, scratch, stream=stream)
    if not sync:   # (with everything the call still reads or writes kept alive)
        return res, dst, doffs, (src, sptr, dptr, sizes, caps, scratch)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    return rs, [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)]


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
    want = [M.compress(b, 64) for b in pick]
    assert encode(cuda, product, pick, 0) == ([len(w) for w in want], want)


def test_capacity(product, cuda):
    idx = [len(blocks()) - 6, len(blocks()) - 4, len(blocks()) - 2, 24, 100, 0]
    pick = [blocks()[i] for i in idx]
    want = [model(8)[i] for i in idx]
    exact = [len(w) for w in want]
    assert encode(cuda, product, pick, 8, caps=exact) == (exact, want)
    for caps in ([c - 1 for c in exact], [0] * len(pick), [-1] * len(pick)):
        rs, outs = encode(cuda, product, pick, 8, caps=caps)
        assert rs == [0] * len(pick), caps
    # a block that does not fit writes nothing at all: the size is known before the first byte
    n = len(pick)
    src, sptr, _ = pack(cuda, pick)
    dst, dptr, doffs = alloc_out(cuda, [c - 1 for c in exact])
    res = ints(cuda, [POISON] * n)
    scratch = cuda.empty(product.compress_hc_opt_scratch_size(n), dtype=cuda.uint8, device="cuda")
    product.compress_hc_opt_ptr_batch(sptr, ints(cuda, map(len, pick)), dptr,
                                      ints(cuda, [c - 1 for c in exact]), res, 8, scratch)
    cuda.cuda.synchronize()
    assert res.cpu().tolist() == [0] * n
    for o, c in zip(doffs, exact):
        assert fetch(dst, o, c + 32) == bytes([CANARY]) * (c + 32)
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


def test_the_scratch_is_written_before_it_is_read(product, cuda):
    """0xEE everywhere, then 0x11: the same bytes (test_bytes... ran on 0xEE too)."""
    want = model(8)
    for poison in (0xEE, 0x11):
        rs, outs = encode(cuda, product, blocks(), 8, poison=poison)
        assert rs == [len(w) for w in want] and outs == want, (poison, first_difference(outs, want))


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
    scratch = cuda.zeros(product.compress_hc_opt_scratch_size(1), dtype=cuda.uint8, device="cuda")
    rc = product.lib().APE_LZ4_compress_hc_opt_batch_dev(None, None, None, None, None, 0, 64,
                                                         scratch.data_ptr(), scratch.numel(), None)
    assert rc == 0


def test_the_call_captures_into_a_graph(product, cuda):
    """No allocation and no sync: two passes (a scratch of 7 blocks for 12) captured, replayed
    over a scratch refilled with garbage."""
    pick = blocks()[-6:-4] + blocks()[100:110]
    want = [M.compress(b, 8) for b in pick]
    n = len(pick)
    src, sptr, _ = pack(cuda, pick, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [product.compressBound(len(b)) for b in pick]
    dst, dptr, doffs = alloc_out(cuda, caps, misalign=[(3 * i) % 16 for i in range(n)])
    sizes, capt, res = ints(cuda, map(len, pick)), ints(cuda, caps), ints(cuda, [POISON] * n)
    scratch = cuda.full((product.compress_hc_opt_scratch_size(7),), 0xEE, dtype=cuda.uint8,
                        device="cuda")
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.compress_hc_opt_ptr_batch(sptr, sizes, dptr, capt, res, 8, scratch, stream=s)
    for _ in range(2):
        res.fill_(POISON)
        scratch.fill_(0x11)
        g.replay()
    cuda.cuda.synchronize()
    rs, host = res.cpu().tolist(), dst.cpu().numpy()
    assert rs == [len(w) for w in want]
    assert [host[o:o + r].tobytes() for o, r in zip(doffs, rs)] == want


def test_the_lazy_call_keeps_its_bytes_in_the_same_process(product, cuda):
    pick = blocks()[-6:-4] + blocks()[95:110]
    encode(cuda, product, pick, 8)
    want = [hcmodel.compress(b, 8) for b in pick]
    assert lazy_encode(cuda, product, pick, 8) == ([len(w) for w in want], want)
    want = [M.compress(b, 8) for b in pick]
    assert encode(cuda, product, pick, 8) == ([len(w) for w in want], want)


# ---- the call with history ----
@functools.lru_cache(maxsize=None)
def _history_and_block(content):
    return I.make(content, 65536 + 32768, seed=11)


@functools.lru_cache(maxsize=None)
def prefix_cases():
    """[(window, used history, offered prefix)]: block sizes 13 / 100 / 4096 / 32768 x histories
    of 0, 1, 63, 64, 1000 and 65536 - n bytes over the contents in turn, a negative prefix, more
    history offered than a window holds, and a block that repeats its history: one match that
    starts in the history and runs through the block."""
    out, k = [], 0
    for n in (13, 100, 4096, 32768):
        for pre in (0, 1, 63, 64, 1000, 65536 - n, -5, 65536 - n + 9):
            whole = _history_and_block(("comp", "text", "zeros", "period7", "rand")[k % 5])
            h = max(0, min(pre, 65536 - n))
            out.append((whole[65536 - h:65536 + n], h, pre))
            k += 1
    rep = I.synth_rand(3000, 3)
    out.append((rep + rep[:2000], 3000, 3000))
    out.append((rep[:700] + rep[:700] + rep[:700], 700, 700))
    return out


@functools.lru_cache(maxsize=None)
def prefix_model(depth):
    return [M.compress_prefix(w, h, depth) for w, h, _ in prefix_cases()]


def encode_prefix(torch, amd, cases, depth, with_prefix=True):
    """One compress_hc_opt_prefix_ptr_batch call, window bases at every residue of 16, and its
    blocks back through the GPU's usingDict decoder."""
    n = len(cases)
    src, wptr, _ = pack(torch, [w for w, _, _ in cases], misalign=[i % 16 for i in range(n)])
    hist = torch.tensor([h for _, h, _ in cases], dtype=torch.int64, device="cuda")
    sptr = wptr + hist
    sizes = [len(w) - h for w, h, _ in cases]
    caps = [amd.compressBound(s) for s in sizes]
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [POISON] * n)
    scratch = torch.full((amd.compress_hc_opt_scratch_size(n),), 0xEE, dtype=torch.uint8,
                         device="cuda")
    amd.compress_hc_opt_prefix_ptr_batch(
        sptr, ints(torch, sizes), ints(torch, [p for _, _, p in cases]) if with_prefix else None,
        dptr, ints(torch, caps), res, depth, scratch)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    outs = [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)]
    back, bptr, boffs = alloc_out(torch, sizes)
    bres = ints(torch, [POISON] * n)
    amd.decompress_dict_batch(dptr, res, bptr, ints(torch, sizes), wptr,
                              ints(torch, [h for _, h, _ in cases]), bres)
    torch.cuda.synchronize()
    plain = [(r, fetch(back, o, max(r, 0))) for o, r in zip(boffs, bres.cpu().tolist())]
    return rs, outs, plain


@pytest.mark.parametrize("depth", [8, 64])
def test_prefix_bytes_are_the_models_and_decode(product, cuda, depth):
    cases, want = prefix_cases(), prefix_model(depth)
    rs, outs, plain = encode_prefix(cuda, product, cases, depth)
    assert rs == [len(w) for w in want], first_difference(outs, want)
    assert outs == want, first_difference(outs, want)
    assert plain == [(len(w) - h, w[h:]) for w, h, _ in cases]
    # the block that repeats its history is one match from it and the last literals
    assert len(want[-2]) < 24


def test_a_null_prefix_array_is_the_plain_call(product, cuda):
    cases = prefix_cases()[::5]
    blks = [w[h:] for w, h, _ in cases]
    rs, outs, _ = encode_prefix(cuda, product, [(b, 0, 0) for b in blks], 8, with_prefix=False)
    want = [M.compress(b, 8) for b in blks]
    assert (rs, outs) == ([len(w) for w in want], want)
    assert encode(cuda, product, blks, 8) == (rs, outs)
