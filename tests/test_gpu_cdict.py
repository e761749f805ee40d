"""Prepared dictionaries on the GPU: APE_LZ4_cdict_prepare_dev +
APE_LZ4_compress_usingCDict_batch_dev (N x loadDict ; compress_fast_continue on fresh streams,
ref src/ape_lz4.c:1101-1133, :1160-1220).

The checker of every block is the reference's decoder as the oracle restates it:
orc_decompress_safe_usingDict with the caller's ORIGINAL dictionary (any size, any placement)
must return the message.  The dictionary lies in an allocation of its own, at an odd address.
"""
import functools

import numpy as np
import pytest

from gpuutil import alloc_out, fetch, ints, pack
from lz4util import I, walk_ok
from test_gpu_stream import gpu_dict_decode, orc_dict_decode

pytestmark = pytest.mark.gpu

ERANGE = -2147483648
BASE = 70000


@functools.lru_cache(maxsize=None)
def plain():
    return I.make("comp", 400000, seed=7)


def dict_of(dd):
    return plain()[BASE - dd:BASE]


def messages(L, most=128):
    if L == 0:
        return [b"", b""]
    return [plain()[s:s + L] for s in range(BASE, 102768, L)][:most]


def dev_dict(torch, d, odd=True):
    """The dictionary in its own allocation (at an odd address): a 1-D uint8 view."""
    off = 3 if odd else 0
    h = np.zeros(len(d) + off + 64, np.uint8)
    h[off:off + len(d)] = np.frombuffer(d, np.uint8)
    dev = torch.from_numpy(h).cuda()
    assert dev.data_ptr() % 2 == 0
    return dev[off:off + len(d)]


def prepare(torch, amd, d, max_src, fill=0x5A, odd=True, stream=None):
    obj = torch.full((amd.cdict_size(),), fill, dtype=torch.uint8, device="cuda")
    amd.cdict_prepare(dev_dict(torch, d, odd), max_src, obj, stream=stream)
    return obj


def encode(torch, amd, obj, msgs, caps=None, sizes=None, stream=None, sync=True):
    """(results, outputs, (dst, offsets)) of one compress_cdict_batch call."""
    n = len(msgs)
    src, sptr, _ = pack(torch, msgs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [amd.compressBound(len(m)) for m in msgs] if caps is None else caps
    sizes = [len(m) for m in msgs] if sizes is None else sizes
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [-7] * n)
    amd.compress_cdict_batch(sptr, ints(torch, sizes), dptr, ints(torch, caps), res, obj,
                             stream=stream)
    if not sync:
        return res, dst, doffs, src
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    return rs, [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)]


def check_round_trip(oracle, d, msgs, rs, outs, what):
    for i, (m, r, c) in enumerate(zip(msgs, rs, outs)):
        assert r > 0, (what, i, r)
        assert orc_dict_decode(oracle, c, len(m), d) == (len(m), m), (what, i)


LENGTHS = (0, 1, 5, 12, 13, 64, 65, 127, 128, 1024, 4096)


@pytest.mark.parametrize("dict_size", [0, 1, 63, 64, 100, 4095, 4096, 65535, 65536, 70000])
def test_round_trip_through_the_reference_decoder(oracle, product, cuda, dict_size):
    d = dict_of(dict_size)
    sub_c, sub_m = [], []
    for L in LENGTHS:
        msgs = messages(L)
        for max_src in sorted({max(L, 1), 4096}):
            obj = prepare(cuda, product, d, max_src)
            rs, outs = encode(cuda, product, obj, msgs)
            check_round_trip(oracle, d, msgs, rs, outs, (L, dict_size, max_src))
            sub_c += outs[::8]
            sub_m += msgs[::8]
    # the GPU's own usingDict decoder agrees (a sample: every eighth block of every case)
    got = gpu_dict_decode(cuda, product, sub_c, [len(m) for m in sub_m], [d] * len(sub_c),
                          adjacent=False)
    assert got == [(len(m), m) for m in sub_m]


def test_round_trip_full_block_leaves_no_window(oracle, product, cuda):
    d = dict_of(4096)
    msgs = messages(65536)
    assert len(msgs) == 1 and product.cdict_window(len(d), 65536) == 0
    obj = prepare(cuda, product, d, 65536)
    rs, outs = encode(cuda, product, obj, msgs)
    check_round_trip(oracle, d, msgs, rs, outs, "64 KiB")
    assert gpu_dict_decode(cuda, product, outs, [65536], [d], adjacent=False) == [(65536, msgs[0])]


@pytest.mark.parametrize("dict_size", [61440, 100])
def test_matches_stop_at_the_dictionary_end(oracle, product, cuda, dict_size):
    """Messages that continue the dictionary's last j bytes: the best match of their first
    bytes lies in the dictionary's last bytes and would, unchecked, run on into the object's
    pad (which is zero: the 0x00 fill makes the message agree with it) -- and a candidate in
    the dictionary's last 3 bytes has its 4-byte check compare pad."""
    d = dict_of(dict_size)
    msgs = []
    for j in (1, 2, 3, 4, 7, 8, 9, 20, 63, 64, 200):
        for fill in (0x00, 0xFF, 0xCD):
            first = d[-j:] + bytes([fill]) * 48 + I.make("rand", 100, seed=j)
            msgs += [first, d[-j:] + d[-j:] + first]
    assert max(map(len, msgs)) <= 1024
    obj = prepare(cuda, product, d, 1024)
    rs, outs = encode(cuda, product, obj, msgs)
    check_round_trip(oracle, d, msgs, rs, outs, dict_size)
    got = gpu_dict_decode(cuda, product, outs, [len(m) for m in msgs], [d] * len(msgs),
                          adjacent=False)
    assert got == [(len(m), m) for m in msgs]


def _plain_encode(torch, amd, msgs):
    src, sptr, _ = pack(torch, msgs)
    caps = [amd.compressBound(len(m)) for m in msgs]
    dst, dptr, _ = alloc_out(torch, caps)
    res = ints(torch, [-7] * len(msgs))
    amd.compress_fast_ptr_batch(sptr, ints(torch, map(len, msgs)), dptr, ints(torch, caps), res, 1)
    torch.cuda.synchronize()
    return res.cpu().tolist()


def _staged_prefix_encode(torch, amd, d, msgs):
    """What a caller could do before: [dictionary | message] staged per message, withPrefix."""
    blobs = [d + m for m in msgs]
    src, sptr, _ = pack(torch, blobs)
    caps = [amd.compressBound(len(m)) for m in msgs]
    dst, dptr, _ = alloc_out(torch, caps)
    res = ints(torch, [-7] * len(msgs))
    amd.compress_prefix_batch(sptr + len(d), ints(torch, map(len, msgs)),
                              ints(torch, [len(d)] * len(msgs)), dptr, ints(torch, caps), res)
    torch.cuda.synchronize()
    return res.cpu().tolist()


@pytest.mark.parametrize("L,dd", [(1024, 61440), (256, 32768)])
def test_the_dictionary_is_used_and_used_well(oracle, product, cuda, L, dd):
    """Reference on the same inputs (loadDict + compress_fast_continue): ratio 2.60 with /
    1.28 without the dictionary at L = 1024, Dd = 61440; 2.36 / 1.12 at L = 256, Dd = 32768."""
    d, msgs = dict_of(dd), messages(L)
    obj = prepare(cuda, product, d, L)
    rs, outs = encode(cuda, product, obj, msgs)
    check_round_trip(oracle, d, msgs, rs, outs, (L, dd))
    # (a) some sequence reaches back beyond its own message
    reach = 0
    for c in outs:
        pos = 0
        for lit, off, ml in walk_ok(c):
            pos += lit
            reach += off > pos
            pos += ml
    total = sum(rs)
    without = sum(_plain_encode(cuda, product, msgs))
    staged = sum(_staged_prefix_encode(cuda, product, d, msgs))
    nbytes = sum(map(len, msgs))
    print("cdict L=%d Dd=%d: %d sequences into the dictionary; ratio %.3f, without %.3f, "
          "staged withPrefix %.3f (cdict / staged = %.4f)"
          % (L, dd, reach, nbytes / total, nbytes / without, nbytes / staged, total / staged))
    assert reach > 0
    assert total < without                      # (b)
    assert total <= 1.02 * staged               # (c)


def test_limits_and_capacity(oracle, product, cuda):
    d = dict_of(61440)
    m = messages(1024)[:7]
    msgs = [m[0], m[1] + b"x", m[2], m[3], m[4], m[5], m[6]]   # block 1: maxSrcSize + 1 bytes
    obj = prepare(cuda, product, d, 1024)
    rs0, outs0 = encode(cuda, product, obj, m)
    assert min(rs0) > 0
    sizes = [len(x) for x in msgs]
    sizes[3] = -5
    caps = [product.compressBound(1025)] * 7
    caps[5] = rs0[5] - 1
    rs, outs = encode(cuda, product, obj, msgs, caps=caps, sizes=sizes)
    assert rs[1] == ERANGE and rs[3] == 0 and rs[5] == 0
    for i in (0, 2, 4, 6):
        assert (rs[i], outs[i]) == (rs0[i], outs0[i]), i
    # the exact capacity fits (and the canaries after every slot are checked after the test)
    caps[5] = rs0[5]
    rs, outs = encode(cuda, product, obj, msgs, caps=caps, sizes=sizes)
    assert (rs[5], outs[5]) == (rs0[5], outs0[5])


@pytest.mark.parametrize("dict_size", [0, 100, 70000])
def test_prepare_writes_every_byte(product, cuda, dict_size):
    d = dict_of(dict_size)
    a = prepare(cuda, product, d, 1024, fill=0x00)
    b = prepare(cuda, product, d, 1024, fill=0xFF, odd=False)
    cuda.cuda.synchronize()
    assert cuda.equal(a, b)


def test_one_object_two_streams(product, cuda):
    d = dict_of(61440)
    obj = prepare(cuda, product, d, 1024)
    m1, m2 = messages(1024)[:16], messages(1024)[16:]
    ref1, ref2 = encode(cuda, product, obj, m1), encode(cuda, product, obj, m2)
    s1, s2 = cuda.cuda.Stream(), cuda.cuda.Stream()
    s1.wait_stream(cuda.cuda.current_stream())
    s2.wait_stream(cuda.cuda.current_stream())
    k1 = encode(cuda, product, obj, m1, stream=s1, sync=False)
    k2 = encode(cuda, product, obj, m2, stream=s2, sync=False)
    cuda.cuda.synchronize()
    for (res, dst, doffs, _), ref in ((k1, ref1), (k2, ref2)):
        rs = res.cpu().tolist()
        assert (rs, [fetch(dst, o, max(r, 0)) for o, r in zip(doffs, rs)]) == ref


def test_unprepared_object_gives_zero(product, cuda):
    for fill in (0x00, 0xA5, 0xFF):
        obj = cuda.full((product.cdict_size(),), fill, dtype=cuda.uint8, device="cuda")
        rs, _ = encode(cuda, product, obj, messages(1024)[:5])
        assert rs == [0] * 5, fill


def test_prepare_and_compress_capture_into_a_graph(oracle, product, cuda):
    d, msgs = dict_of(61440), messages(1024)
    eager = encode(cuda, product, prepare(cuda, product, d, 1024), msgs)
    n = len(msgs)
    ddev = dev_dict(cuda, d)
    obj = cuda.full((product.cdict_size(),), 0x11, dtype=cuda.uint8, device="cuda")
    src, sptr, _ = pack(cuda, msgs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [product.compressBound(len(m)) for m in msgs]
    dst, dptr, doffs = alloc_out(cuda, caps, misalign=[(3 * i) % 16 for i in range(n)])
    sizes, capt, res = ints(cuda, map(len, msgs)), ints(cuda, caps), ints(cuda, [-7] * n)
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.cdict_prepare(ddev, 1024, obj, stream=s)
        product.compress_cdict_batch(sptr, sizes, dptr, capt, res, obj, stream=s)
    for _ in range(2):
        res.fill_(-7)
        obj.fill_(0x22)
        g.replay()
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    assert (rs, [fetch(dst, o, max(r, 0)) for o, r in zip(doffs, rs)]) == eager
    check_round_trip(oracle, d, msgs, *eager, "graph")
