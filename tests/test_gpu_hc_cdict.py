"""The high-ratio mode against a prepared dictionary on the GPU: APE_LZ4_hc_cdict_prepare_dev +
APE_LZ4_compress_hc_usingCDict_batch_dev.

Two checkers of the bytes: tests/hcdictmodel.py on a handful of messages per case (it costs
tens of milliseconds per message behind a 60 KiB dictionary), and for breadth the staged call
-- compress_hc_prefix_ptr_batch on [dictionary tail | message] per message -- whose bytes the
new call must write without that staging.  Every block also decodes, with the caller's ORIGINAL
dictionary, through the oracle's usingDict decoder and the GPU's.  The dictionary lies in an
allocation of its own at an odd address, sources and destinations are misaligned, and the
canaries behind every destination are checked after each test."""
import functools

import pytest

import hcdictmodel as M
import hcmodel
from gpuutil import alloc_out, ints, pack
from test_gpu_cdict import BASE, ERANGE, dev_dict, dict_of, messages, plain
from test_gpu_cdict import encode as fast_encode
from test_gpu_cdict import prepare as fast_prepare
from test_gpu_hc_large import encode_prefix, first_difference
from test_gpu_stream import gpu_dict_decode, orc_dict_decode
from test_hc_cdict_model import (BOUNDARY_J, DICT_SIZES, FAMILY_DICT_SIZES, FAMILY_MAX_SRC, LENGTHS,
                                 MAX_SRC, boundary_family, grid_messages, tail_family)

pytestmark = pytest.mark.gpu

POISON = -7


@functools.lru_cache(maxsize=None)
def model(dict_size, message, max_src, depth):
    return M.compress(dict_of(dict_size), message, max_src, depth)


def prepare(torch, amd, d, max_src, fill=0x5A, odd=True, stream=None):
    obj = torch.full((amd.hc_cdict_size(),), fill, dtype=torch.uint8, device="cuda")
    amd.hc_cdict_prepare(dev_dict(torch, d, odd), max_src, obj, stream=stream)
    return obj


def new_scratch(torch, amd, nblocks, max_src, fill=0xEE):
    return torch.full((amd.compress_hc_cdict_scratch_size(nblocks, max_src),), fill,
                      dtype=torch.uint8, device="cuda")


def encode(torch, amd, obj, msgs, max_src, depth, caps=None, sizes=None, scratch=None,
           stream=None, sync=True):
    """(results, outputs) of one compress_hc_cdict_batch call."""
    n = len(msgs)
    src, sptr, _ = pack(torch, msgs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [amd.compressBound(len(m)) for m in msgs] if caps is None else caps
    sizes = [len(m) for m in msgs] if sizes is None else sizes
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [POISON] * n)
    scratch = new_scratch(torch, amd, n, max_src) if scratch is None else scratch
    sizes, caps = ints(torch, sizes), ints(torch, caps)
    amd.compress_hc_cdict_batch(sptr, sizes, dptr, caps, res, obj, max_src, depth, scratch,
                                stream=stream)
    if not sync:   # (with everything the launches read, alive until the caller has synchronised)
        return res, dst, doffs, (src, sptr, dptr, sizes, caps, scratch)
    torch.cuda.synchronize()
    return collect(res, dst, doffs)


def collect(res, dst, doffs):
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    return rs, [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)]


def check_decoders(torch, amd, oracle, d, msgs, rs, outs, what):
    """Every block through both usingDict decoders, given the original dictionary."""
    for i, (m, r, c) in enumerate(zip(msgs, rs, outs)):
        assert r > 0, (what, i, r)
        assert orc_dict_decode(oracle, c, len(m), d) == (len(m), m), (what, i)
    got = gpu_dict_decode(torch, amd, outs, [len(m) for m in msgs], [d] * len(msgs), adjacent=False)
    assert got == [(len(m), m) for m in msgs], what


def staged(torch, amd, d, msgs, max_src, depth):
    """The only way before: [dictionary tail | message] staged per message, withPrefix."""
    D = amd.hc_cdict_window(len(d), max_src)
    tail = d[len(d) - D:]
    rs, outs, _ = encode_prefix(torch, amd, [(tail + m, D, D) for m in msgs], depth)
    return rs, outs


@pytest.mark.parametrize("dict_size", DICT_SIZES)
def test_bytes_are_the_models(oracle, product, cuda, dict_size):
    d = dict_of(dict_size)
    assert product.hc_cdict_window(dict_size, MAX_SRC) == M.window(dict_size, MAX_SRC)
    msgs = [m for L in LENGTHS for m in grid_messages(L)]
    want = [model(dict_size, m, MAX_SRC, 8) for m in msgs]
    rs, outs = encode(cuda, product, prepare(cuda, product, d, MAX_SRC), msgs, MAX_SRC, 8)
    assert outs == want, first_difference(outs, want)
    assert rs == [len(w) for w in want]
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, dict_size)


@pytest.mark.parametrize("depth", [1, 64, 256, 0])
def test_depths(oracle, product, cuda, depth):
    d = dict_of(65535)
    msgs = grid_messages(1000) + grid_messages(65, 1)
    want = [model(65535, m, MAX_SRC, depth or 64) for m in msgs]
    rs, outs = encode(cuda, product, prepare(cuda, product, d, MAX_SRC), msgs, MAX_SRC, depth)
    assert outs == want, first_difference(outs, want)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, depth)


def test_a_full_block_leaves_no_window(oracle, product, cuda):
    """maxSrcSize 65536: D = 0, and the bytes are compress_hc_batch_dev's."""
    d = dict_of(4096)
    msgs = messages(65536)
    assert len(msgs) == 1 and product.hc_cdict_window(len(d), 65536) == 0
    rs, outs = encode(cuda, product, prepare(cuda, product, d, 65536), msgs, 65536, 8)
    src, sptr, _ = pack(cuda, msgs)
    caps = [product.compressBound(65536)]
    dst, dptr, doffs = alloc_out(cuda, caps)
    res = ints(cuda, [POISON])
    scratch = cuda.empty(product.compress_hc_scratch_size(1), dtype=cuda.uint8, device="cuda")
    product.compress_hc_ptr_batch(sptr, ints(cuda, [65536]), dptr, ints(cuda, caps), res, 8, scratch)
    cuda.cuda.synchronize()
    assert (rs, outs) == collect(res, dst, doffs)
    assert outs[0] == hcmodel.compress(msgs[0], 8)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, "64 KiB")


@pytest.mark.parametrize("depth", [8, 64])
@pytest.mark.parametrize("L,dd", [(1024, 61440), (256, 32768)])
def test_bytes_are_the_staged_calls(oracle, product, cuda, L, dd, depth):
    d = dict_of(dd)
    msgs = [plain()[BASE + L * k:BASE + L * (k + 1)] for k in range(128)]
    rs, outs = encode(cuda, product, prepare(cuda, product, d, L), msgs, L, depth)
    srs, souts = staged(cuda, product, d, msgs, L, depth)
    assert outs == souts, first_difference(outs, souts)
    assert rs == srs
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, (L, dd, depth))


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_boundary_family(oracle, product, cuda, dict_size):
    """Matches that start j bytes before the message: in the straddling chain positions (j <=
    3), across the boundary inside the search's compare (j >= 4) and inside the parse's
    extension (j = 300)."""
    d = dict_of(dict_size)
    msgs = boundary_family(d)
    assert len(msgs) == len(BOUNDARY_J)
    want = [model(dict_size, m, FAMILY_MAX_SRC, 8) for m in msgs]
    obj = prepare(cuda, product, d, FAMILY_MAX_SRC)
    rs, outs = encode(cuda, product, obj, msgs, FAMILY_MAX_SRC, 8)
    assert outs == want, first_difference(outs, want)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, dict_size)


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_dictionary_tail_family(oracle, product, cuda, dict_size):
    """Messages that continue the dictionary's last j bytes: the model on every third, the
    staged call on all."""
    d = dict_of(dict_size)
    msgs = tail_family(d)
    obj = prepare(cuda, product, d, FAMILY_MAX_SRC, fill=0x00)
    rs, outs = encode(cuda, product, obj, msgs, FAMILY_MAX_SRC, 8)
    want = [model(dict_size, m, FAMILY_MAX_SRC, 8) for m in msgs[::3]]
    assert outs[::3] == want, first_difference(outs[::3], want)
    srs, souts = staged(cuda, product, d, msgs, FAMILY_MAX_SRC, 8)
    assert (rs, outs) == (srs, souts), first_difference(outs, souts)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, dict_size)


def test_limits_and_capacity(product, cuda):
    d = dict_of(61440)
    m = messages(1024)[:7]
    msgs = [m[0], m[1] + b"x", m[2], m[3], m[4], m[5], m[6]]   # block 1: maxSrcSize + 1 bytes
    obj = prepare(cuda, product, d, 1024)
    rs0, outs0 = encode(cuda, product, obj, m, 1024, 8)
    assert min(rs0) > 0
    sizes = [len(x) for x in msgs]
    sizes[3] = -5
    caps = [product.compressBound(1025)] * 7
    caps[5] = rs0[5] - 1
    rs, outs = encode(cuda, product, obj, msgs, 1024, 8, caps=caps, sizes=sizes)
    assert rs[1] == ERANGE and rs[3] == 0 and rs[5] == 0
    for i in (0, 2, 4, 6):
        assert (rs[i], outs[i]) == (rs0[i], outs0[i]), i
    # the exact capacity fits (and the canaries after every slot are checked after the test)
    caps[5] = rs0[5]
    rs, outs = encode(cuda, product, obj, msgs, 1024, 8, caps=caps, sizes=sizes)
    assert (rs[5], outs[5]) == (rs0[5], outs0[5])


def test_rejected_objects_give_zero(product, cuda):
    msgs = messages(1024)[:5]
    for fill in (0x00, 0xA5, 0xFF):     # never prepared
        obj = cuda.full((product.hc_cdict_size(),), fill, dtype=cuda.uint8, device="cuda")
        assert encode(cuda, product, obj, msgs, 1024, 8)[0] == [0] * 5, fill
    d = dict_of(61440)
    obj = prepare(cuda, product, d, 1024)
    assert min(encode(cuda, product, obj, msgs, 1024, 8)[0]) > 0
    for other in (1023, 1025, 4096):    # a maxSrcSize that is not the object's
        short = [m[:1023] for m in msgs]
        assert encode(cuda, product, obj, short, other, 8)[0] == [0] * 5, other
    # an object of one kind given to the other kind's call (the larger allocation holds both)
    size = max(product.hc_cdict_size(), product.cdict_size())
    fast = cuda.zeros(size, dtype=cuda.uint8, device="cuda")
    product.cdict_prepare(dev_dict(cuda, d), 1024, fast)
    assert min(fast_encode(cuda, product, fast, msgs)[0]) > 0
    assert encode(cuda, product, fast, msgs, 1024, 8)[0] == [0] * 5
    assert fast_encode(cuda, product, obj, msgs)[0] == [0] * 5


@pytest.mark.parametrize("dict_size", [0, 100, 70000])
def test_prepare_writes_every_byte(product, cuda, dict_size):
    d = dict_of(dict_size)
    a = prepare(cuda, product, d, 1024, fill=0x00)
    b = prepare(cuda, product, d, 1024, fill=0xFF, odd=False)
    cuda.cuda.synchronize()
    assert cuda.equal(a, b)


def test_scratch_size_and_contents_do_not_matter(product, cuda):
    d = dict_of(61440)
    msgs = messages(1024)[:32] + grid_messages(13) + grid_messages(5)
    n = len(msgs)
    obj = prepare(cuda, product, d, 1024)
    ref = encode(cuda, product, obj, msgs, 1024, 8)
    assert min(ref[0]) > 0
    for nb, fill in ((1, 0xEE), (7, 0xEE), (n, 0x00), (n, 0xFF)):
        got = encode(cuda, product, obj, msgs, 1024, 8, scratch=new_scratch(cuda, product, nb, 1024, fill))
        assert got == ref, (nb, fill)


def test_one_object_two_streams(product, cuda):
    d = dict_of(61440)
    obj = prepare(cuda, product, d, 1024)
    m1, m2 = messages(1024)[:16], messages(1024)[16:]
    ref1, ref2 = encode(cuda, product, obj, m1, 1024, 8), encode(cuda, product, obj, m2, 1024, 8)
    s1, s2 = cuda.cuda.Stream(), cuda.cuda.Stream()
    s1.wait_stream(cuda.cuda.current_stream())
    s2.wait_stream(cuda.cuda.current_stream())
    k1 = encode(cuda, product, obj, m1, 1024, 8, stream=s1, sync=False)
    k2 = encode(cuda, product, obj, m2, 1024, 8, stream=s2, sync=False)
    cuda.cuda.synchronize()
    assert collect(*k1[:3]) == ref1 and collect(*k2[:3]) == ref2


def test_prepare_and_a_two_pass_compress_capture_into_a_graph(oracle, product, cuda):
    d, msgs = dict_of(61440), messages(1024)
    n = len(msgs)
    eager = encode(cuda, product, prepare(cuda, product, d, 1024), msgs, 1024, 8)
    ddev = dev_dict(cuda, d)
    obj = cuda.full((product.hc_cdict_size(),), 0x11, dtype=cuda.uint8, device="cuda")
    src, sptr, _ = pack(cuda, msgs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [product.compressBound(len(m)) for m in msgs]
    dst, dptr, doffs = alloc_out(cuda, caps, misalign=[(3 * i) % 16 for i in range(n)])
    sizes, capt, res = ints(cuda, map(len, msgs)), ints(cuda, caps), ints(cuda, [POISON] * n)
    scratch = new_scratch(cuda, product, (n + 1) // 2, 1024)     # two passes
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.hc_cdict_prepare(ddev, 1024, obj, stream=s)
        product.compress_hc_cdict_batch(sptr, sizes, dptr, capt, res, obj, 1024, 8, scratch, stream=s)
    for _ in range(2):
        res.fill_(POISON)
        obj.fill_(0x22)
        scratch.fill_(0x33)
        g.replay()
    cuda.cuda.synchronize()
    assert collect(res, dst, doffs) == eager
    check_decoders(cuda, product, oracle, d, msgs, *eager, "graph")


def test_the_dictionary_pays(product, cuda):
    """1024 B messages behind 61440 B at depth 8: the model gives ratio 3.82, the reference's
    dictionary mode 2.60 and the high-ratio mode without a dictionary 1.36."""
    d, msgs = dict_of(61440), messages(1024)
    total = sum(encode(cuda, product, prepare(cuda, product, d, 1024), msgs, 1024, 8)[0])
    fast = sum(fast_encode(cuda, product, fast_prepare(cuda, product, d, 1024), msgs)[0])
    alone = sum(staged(cuda, product, b"", msgs, 1024, 8)[0])
    nbytes = sum(map(len, msgs))
    print("hc cdict 1024 B / 61440 B depth 8: ratio %.3f, compress_usingCDict %.3f, high-ratio "
          "without a dictionary %.3f" % (nbytes / total, nbytes / fast, nbytes / alone))
    assert 0 < total < fast and total < alone
