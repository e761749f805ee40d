"""The cost-minimising parse against a prepared dictionary on the GPU:
APE_LZ4_hc_cdict_prepare_dev + APE_LZ4_compress_hc_opt_usingCDict_batch_dev.

Two checkers of the bytes, as in tests/test_gpu_hc_cdict.py: tests/hcoptdictmodel.py on a
handful of messages per case, and for breadth the staged call -- compress_hc_opt_prefix_ptr_batch
on [dictionary tail | message] per message -- whose bytes the new call must write without that
staging.  Every block also decodes, with the caller's ORIGINAL dictionary, through the oracle's
usingDict decoder and the GPU's.  Sources start at every residue of 16, destinations are
misaligned, and the canaries behind every destination are checked after each test."""
import functools

import pytest

import hcoptdictmodel as M
import hcoptmodel
from gpuutil import CANARY, alloc_out, fetch, ints, pack
from test_gpu_cdict import BASE, ERANGE, dev_dict, dict_of, messages, plain
from test_gpu_hc_cdict import check_decoders, collect, prepare
from test_gpu_hc_cdict import encode as lazy_encode
from test_gpu_hc_large import first_difference
from test_gpu_hc_opt import encode as block_encode
from test_gpu_hc_opt import encode_prefix
from test_hc_cdict_model import (DICT_SIZES, FAMILY_DICT_SIZES, FAMILY_MAX_SRC, LENGTHS, MAX_SRC,
                                 boundary_family, grid_messages, tail_family)
from test_hc_opt_cdict_model import long_family, run_family

pytestmark = pytest.mark.gpu

POISON = -7


@functools.lru_cache(maxsize=None)
def model(dict_size, message, max_src, depth):
    return M.compress(dict_of(dict_size), message, max_src, depth)


def new_scratch(torch, amd, nblocks, max_src, fill=0xEE):
    return torch.full((amd.compress_hc_opt_cdict_scratch_size(nblocks, max_src),), fill,
                      dtype=torch.uint8, device="cuda")


def encode(torch, amd, obj, msgs, max_src, depth, caps=None, sizes=None, scratch=None,
           stream=None, sync=True, raw=False):
    """(results, outputs) of one compress_hc_opt_cdict_batch call."""
    n = len(msgs)
    src, sptr, _ = pack(torch, msgs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [amd.compressBound(len(m)) for m in msgs] if caps is None else caps
    sizes = [len(m) for m in msgs] if sizes is None else sizes
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [POISON] * n)
    scratch = new_scratch(torch, amd, n, max_src) if scratch is None else scratch
    sizes, caps = ints(torch, sizes), ints(torch, caps)
    if stream is not None:   # the buffers above were filled on the current stream
        stream.wait_stream(torch.cuda.current_stream())
    amd.compress_hc_opt_cdict_batch(sptr, sizes, dptr, caps, res, obj, max_src, depth, scratch,
                                    stream=stream)
    if not sync:   # (with everything the launches read, alive until the caller has synchronised)
        return res, dst, doffs, (src, sptr, dptr, sizes, caps, scratch)
    torch.cuda.synchronize()
    if raw:
        return res.cpu().tolist(), dst, doffs
    return collect(res, dst, doffs)


def staged(torch, amd, d, msgs, max_src, depth):
    """The only way before: [dictionary tail | message] staged per message, withPrefix."""
    D = amd.hc_cdict_window(len(d), max_src)
    tail = d[len(d) - D:]
    rs, outs, _ = encode_prefix(torch, amd, [(tail + m, D, D) for m in msgs], depth)
    return rs, outs


@pytest.mark.parametrize("dict_size", DICT_SIZES)
def test_bytes_are_the_models(oracle, product, cuda, dict_size):
    d = dict_of(dict_size)
    msgs = [m for L in LENGTHS for m in grid_messages(L)]   # 32: every residue of 16, twice
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
def test_long_matches_across_the_boundary(oracle, product, cuda, dict_size):
    """long_boundary: the extension of a capped match reads its source in the dictionary, across
    the boundary and in the message.  run_message: the run shortcut carries the full length
    from positions whose source is in the message down to those whose source is in the
    dictionary.  The model on every message, and the staged call."""
    d = dict_of(dict_size)
    msgs = long_family(d) + run_family(d)
    want = [model(dict_size, m, FAMILY_MAX_SRC, 8) for m in msgs]
    obj = prepare(cuda, product, d, FAMILY_MAX_SRC)
    rs, outs = encode(cuda, product, obj, msgs, FAMILY_MAX_SRC, 8)
    assert outs == want, first_difference(outs, want)
    assert (rs, outs) == staged(cuda, product, d, msgs, FAMILY_MAX_SRC, 8)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, dict_size)


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_boundary_family(oracle, product, cuda, dict_size):
    d = dict_of(dict_size)
    msgs = boundary_family(d)
    want = [model(dict_size, m, FAMILY_MAX_SRC, 8) for m in msgs]
    obj = prepare(cuda, product, d, FAMILY_MAX_SRC)
    rs, outs = encode(cuda, product, obj, msgs, FAMILY_MAX_SRC, 8)
    assert outs == want, first_difference(outs, want)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, dict_size)


@pytest.mark.parametrize("dict_size", FAMILY_DICT_SIZES)
def test_dictionary_tail_family(oracle, product, cuda, dict_size):
    """Messages that continue the dictionary's last j bytes (the object's pad after them is
    zero, and the 0x00 fill agrees with it): the model on every third, the staged call on all."""
    d = dict_of(dict_size)
    msgs = tail_family(d)
    obj = prepare(cuda, product, d, FAMILY_MAX_SRC, fill=0x00)
    rs, outs = encode(cuda, product, obj, msgs, FAMILY_MAX_SRC, 8)
    want = [model(dict_size, m, FAMILY_MAX_SRC, 8) for m in msgs[::3]]
    assert outs[::3] == want, first_difference(outs[::3], want)
    srs, souts = staged(cuda, product, d, msgs, FAMILY_MAX_SRC, 8)
    assert (rs, outs) == (srs, souts), first_difference(outs, souts)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, dict_size)


def test_a_full_block_leaves_no_window(oracle, product, cuda):
    """maxSrcSize 65536: D = 0, and the bytes are compress_hc_opt_batch_dev's."""
    d = dict_of(4096)
    msgs = messages(65536)
    assert len(msgs) == 1 and product.hc_cdict_window(len(d), 65536) == 0
    rs, outs = encode(cuda, product, prepare(cuda, product, d, 65536), msgs, 65536, 8)
    assert (rs, outs) == block_encode(cuda, product, msgs, 8)
    assert outs[0] == hcoptmodel.compress(msgs[0], 8)
    check_decoders(cuda, product, oracle, d, msgs, rs, outs, "64 KiB")


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
    rs, dst, doffs = encode(cuda, product, obj, msgs, 1024, 8, caps=caps, sizes=sizes, raw=True)
    assert rs[1] == ERANGE and rs[3] == 0 and rs[5] == 0
    # the block that does not fit, the negative size and the size out of range wrote nothing
    for i in (1, 3, 5):
        assert fetch(dst, doffs[i], caps[i] + 32) == bytes([CANARY]) * (caps[i] + 32), i
    for i in (0, 2, 4, 6):
        assert (rs[i], fetch(dst, doffs[i], rs[i])) == (rs0[i], outs0[i]), i
    # the exact capacity fits (and the canaries after every slot are checked after the test)
    caps[5] = rs0[5]
    rs, outs = encode(cuda, product, obj, msgs, 1024, 8, caps=caps, sizes=sizes)
    assert (rs[5], outs[5]) == (rs0[5], outs0[5])
    # every capacity exact, every capacity one short, none at all
    assert encode(cuda, product, obj, m, 1024, 8, caps=rs0) == (rs0, outs0)
    for short in ([r - 1 for r in rs0], [0] * 7, [-1] * 7):
        rs, dst, doffs = encode(cuda, product, obj, m, 1024, 8, caps=short, raw=True)
        assert rs == [0] * 7
        for o, c in zip(doffs, short):
            assert fetch(dst, o, max(c, 1) + 32) == bytes([CANARY]) * (max(c, 1) + 32)
    # messages shorter than 13 bytes are one literal run, and know their size too
    tiny = [x[:k] for k, x in zip((0, 1, 5, 12, 12, 12, 0), m)]
    want = [bytes([len(t) << 4]) + t for t in tiny]
    assert encode(cuda, product, obj, tiny, 1024, 8) == ([len(w) for w in want], want)
    rs, outs = encode(cuda, product, obj, tiny, 1024, 8, caps=[1, 1, 6, 12, 13, 14, 0])
    assert rs == [1, 0, 6, 0, 13, 13, 0]


def test_an_empty_batch_is_no_error(product, cuda):
    obj = prepare(cuda, product, dict_of(100), 1024)
    scratch = new_scratch(cuda, product, 1, 1024)
    e = cuda.zeros(0, dtype=cuda.int64, device="cuda")
    z = cuda.zeros(0, dtype=cuda.int32, device="cuda")
    product.compress_hc_opt_cdict_batch(e, z, e, z, z, obj, 1024, 8, scratch)
    cuda.cuda.synchronize()
    assert bool((scratch == 0xEE).all())


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
    # the fast encoder's object (the larger allocation holds both kinds)
    size = max(product.hc_cdict_size(), product.cdict_size())
    fast = cuda.zeros(size, dtype=cuda.uint8, device="cuda")
    product.cdict_prepare(dev_dict(cuda, d), 1024, fast)
    assert encode(cuda, product, fast, msgs, 1024, 8)[0] == [0] * 5


def test_scratch_size_and_contents_do_not_matter(product, cuda):
    d = dict_of(61440)
    msgs = messages(1024)[:32] + grid_messages(13) + grid_messages(5) + run_family(d)
    n = len(msgs)
    obj = prepare(cuda, product, d, 1024)
    ref = encode(cuda, product, obj, msgs, 1024, 8)
    assert min(ref[0]) > 0
    for nb, fill in ((1, 0xEE), (7, 0xEE), (1, 0x11), (7, 0x11), (n, 0x11), (n, 0x00), (n, 0xFF)):
        got = encode(cuda, product, obj, msgs, 1024, 8, scratch=new_scratch(cuda, product, nb, 1024, fill))
        assert got == ref, (nb, fill)


def test_one_object_two_streams(product, cuda):
    d = dict_of(61440)
    obj = prepare(cuda, product, d, 1024)
    m1, m2 = messages(1024)[:16], messages(1024)[16:]
    ref1, ref2 = encode(cuda, product, obj, m1, 1024, 8), encode(cuda, product, obj, m2, 1024, 8)
    s1, s2 = cuda.cuda.Stream(), cuda.cuda.Stream()
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
        product.compress_hc_opt_cdict_batch(sptr, sizes, dptr, capt, res, obj, 1024, 8, scratch,
                                            stream=s)
    res.fill_(POISON)
    obj.fill_(0x22)
    scratch.fill_(0x33)
    g.replay()
    cuda.cuda.synchronize()
    assert collect(res, dst, doffs) == eager
    check_decoders(cuda, product, oracle, d, msgs, *eager, "graph")


def test_the_parse_pays(product, cuda):
    """1024 B messages behind 61440 B at depth 8, DESIGN.md 3.15's first row (32 messages): the
    models give ratio 3.824 for the lazy parse and 4.106 for this one."""
    d, msgs = dict_of(61440), messages(1024)
    obj = prepare(cuda, product, d, 1024)
    rs = encode(cuda, product, obj, msgs, 1024, 8)[0]
    lazy = lazy_encode(cuda, product, obj, msgs, 1024, 8)[0]
    nbytes = sum(map(len, msgs))
    print("hc opt cdict 1024 B / 61440 B depth 8, %d messages: ratio %.3f, lazy parse %.3f"
          % (len(msgs), nbytes / sum(rs), nbytes / sum(lazy)))
    assert min(rs) > 0 and min(lazy) > 0
    assert nbytes / sum(rs) >= nbytes / sum(lazy)
