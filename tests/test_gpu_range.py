"""Byte ranges of indexed blocks (include/ape_lz4_gpu.h):
APE_LZ4_decompress_range_indexed_batch_dev reads [a, a + m) of a block that has a seek index
by decoding only the covering segments, one request per batch entry.

The judge is the Python model of the documented rules in tests/rangeutil.py (results, windows
and bytes), and for compressor-written blocks the source itself."""
import functools
import random
import struct
import types

import numpy as np
import pytest

import indexutil as X
import rangeutil as RU
from gpuutil import CANARY, alloc_out, ints, pack
from lz4util import I
from test_range_model import counter_example_block, run_block

pytestmark = pytest.mark.gpu

MB = 1 << 20
CONTENTS = ("comp", "text", "rand", "zeros", "period7")


@functools.lru_cache(maxsize=None)
def _master(content):
    return I.make(content, MB)


def data(content, n):
    return _master(content)[:n]


def mixed():
    return I.synth_rand(100000, 7) + data("comp", 150000) + I.synth_rand(40000, 8) + bytes(70000)


def index_stride(max_seg):
    return (16 + 8 * (max_seg + 1) + 15) // 16 * 16


def compressed(torch, amd, srcs, R):
    """One compress_large_indexed launch, kept on the device; the blocks and index words also
    on the host, for the model."""
    nb, max_src = len(srcs), max(map(len, srcs))
    d = types.SimpleNamespace(srcs=srcs, nb=nb)
    d.src, sptr, _ = pack(torch, srcs)
    caps = [amd.compressBound(len(s)) for s in srcs]
    d.dst, d.sptr, offs = alloc_out(torch, caps)
    d.csz = ints(torch, [-7] * nb)
    stride = amd.large_index_size(max_src, R)
    d.max_seg = amd.large_index_segments(max_src, R)
    d.index = torch.zeros((nb, stride), dtype=torch.uint8, device="cuda")
    amd.compress_large_indexed_ptr_batch(sptr, ints(torch, map(len, srcs)), d.sptr, ints(torch, caps),
                                         d.csz, max_src, R, index=d.index)
    torch.cuda.synchronize()
    rs = d.csz.cpu().tolist()
    assert all(r > 0 for r in rs)
    host = d.dst.cpu().numpy()
    d.blocks = [host[o:o + r].tobytes() for o, r in zip(offs, rs)]
    raw = d.index.cpu().numpy()
    d.words = [list(struct.unpack("<%dI" % (stride // 4), raw[i].tobytes())) for i in range(nb)]
    d.words = [w[:4 + 2 * (w[1] + 1)] for w in d.words]
    return d


def uploaded(torch, blocks, words, max_seg):
    """Host-side blocks and index word lists on the device."""
    d = types.SimpleNamespace(blocks=blocks, words=words, nb=len(blocks), max_seg=max_seg)
    d.src, d.sptr, _ = pack(torch, blocks)
    d.csz = ints(torch, map(len, blocks))
    stride = index_stride(max_seg)
    raw = b"".join(X.index_bytes(w[:stride // 4], stride) for w in words)
    d.index = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).view(len(blocks), stride).cuda()
    return d


def read_ranges(torch, amd, d, reqs, caps, waves, identity=False):
    """One launch of reqs = [(block, a, length)]: (results, windows, the cap bytes of each dst)."""
    nreq = len(reqs)
    dst, dptr, offs = alloc_out(torch, caps)
    res, win = ints(torch, [-7] * nreq), ints(torch, [-7] * (2 * nreq))
    amd.decompress_range_indexed_ptr_batch(
        d.sptr, d.csz, d.index, d.max_seg, ints(torch, (q[1] for q in reqs)),
        ints(torch, (q[2] for q in reqs)), dptr, ints(torch, caps), win, res,
        block_of=None if identity else ints(torch, (q[0] for q in reqs)), waves_per_request=waves)
    torch.cuda.synchronize()
    host, w = dst.cpu().numpy(), win.cpu().tolist()
    return (res.cpu().tolist(), [(w[2 * r], w[2 * r + 1]) for r in range(nreq)],
            [host[o:o + c].tobytes() for o, c in zip(offs, caps)])


def modelled(d, reqs, caps=None):
    """The model's (result, window, bytes) of every request (without caps: room for any)."""
    memos, want = {}, []
    for k, (i, a, ln) in enumerate(reqs):
        memo = memos.setdefault(i, {})
        cap = caps[k] if caps is not None else 1 << 30
        want.append(RU.decode_range(d.blocks[i], d.words[i], a, ln, cap, d.max_seg, memo=memo))
    return want


def check(got, want, caps, reqs):
    """Results, windows and bytes against the model; the canaries of dst past need (nothing at
    all is written for a request the plan refuses)."""
    rs, wins, bufs = got
    for k, ((er, ewin, edata), cap) in enumerate(zip(want, caps)):
        r, buf = rs[k], bufs[k]
        assert r == er, (k, reqs[k], r, er)
        assert wins[k] == ewin, (k, reqs[k], wins[k], ewin)
        written = 0 if er == RU.ERANGE else ewin[1]
        assert buf[written:] == bytes([CANARY]) * (cap - written), (k, reqs[k], "canary")
        if er > 0:
            assert buf[ewin[0]:ewin[0] + er] == edata, (k, reqs[k], "bytes")


# ---- 1. round trip on compressor-written blocks ----
_ROUND = {}


def round_trip_case(torch, amd):
    """The blocks (five contents x six sizes around the restart points at R = 2 S, and mixed()),
    about 40 requests each and what the model says of them: built once for the three runs."""
    if not _ROUND:
        R = 2 * amd.compress_large_slice_size()
        sizes = [65537, R - 1, R, R + 1, 2 * R + 1, 3 * R + 5]
        d = compressed(torch, amd, [data(c, n) for c in CONTENTS for n in sizes] + [mixed()], R)
        reqs = []
        for i, (s, w) in enumerate(zip(d.srcs, d.words)):
            n, nseg = len(s), w[1]
            assert w[2] == n
            points = {w[5 + 2 * j] for j in range(nseg + 1)} | set(range(0, n + 1, R))
            starts = sorted({p + e for p in points for e in (-1, 0, 1) if 0 <= p + e <= n})
            lengths = (0, 1, 2, R, n)
            mine = {(a, lengths[(q + t) % 5]) for q, a in enumerate(starts) for t in (0, 1, 3)}
            mine |= {(a, ln) for a in starts[:2] + starts[-3:] for ln in lengths}
            mine |= {(0, n), (n - 1, 1), (n, 0), (n, 5), (n + 1, 1), (n + 1, 0), (-1, 1)}
            reqs += [(i, a, ln) for a, ln in sorted(mine)]
        want = modelled(d, reqs)
        for (i, a, ln), (er, ewin, edata) in zip(reqs, want):
            n = len(d.srcs[i])
            if 0 <= a <= n:   # the model is a true decoder: the source's bytes
                assert er == min(ln, n - a) and edata == d.srcs[i][a:a + er], (i, a, ln, er)
            else:
                assert er == -1
        _ROUND["v"] = (d, reqs, want, [w[1][1] + 64 for w in want])
    return _ROUND["v"]


@pytest.mark.parametrize("waves", [1, 2, 7])
def test_round_trip_on_compressor_written_blocks(cuda, product, waves):
    d, reqs, want, caps = round_trip_case(cuda, product)
    print("%d requests on %d blocks" % (len(reqs), d.nb))
    assert len(reqs) >= 30 * d.nb
    check(read_ranges(cuda, product, d, reqs, caps, waves), want, caps, reqs)


def test_identity_mapping_reads_one_range_per_block(cuda, product):
    d, _, _, _ = round_trip_case(cuda, product)
    reqs = [(i, len(s) // 3, 5000) for i, s in enumerate(d.srcs)]
    want = modelled(d, reqs)
    caps = [w[1][1] + 64 for w in want]
    check(read_ranges(cuda, product, d, reqs, caps, 4, identity=True), want, caps, reqs)
    assert all(w[2] == s[len(s) // 3:len(s) // 3 + 5000] for w, s in zip(want, d.srcs))


# ---- 2. stop edges ----
def test_stop_edges(cuda, product):
    """Handcrafted blocks of many short segments, empty ones among them, the stop of one
    within 84 bytes of the 2304-byte stage boundary: ranges that start and end in every
    segment.  Results equal the model, codes included."""
    blocks, words = [], []
    for seed, sized in enumerate((None, 2220, 2221, 2262, 2303, 2304, 2305, 2388)):
        b, w, _ = RU.stop_edge_block(seed, sized)
        blocks.append(b)
        words.append(w)
    d = uploaded(cuda, blocks, words, max(w[1] for w in words) + 3)
    reqs = []
    for i, w in enumerate(words):
        nseg, n = w[1], w[2]
        edges = sorted({w[5 + 2 * j] for j in range(nseg + 1)})
        for k in range(len(edges) - 1):
            s, e = edges[k], edges[k + 1]
            mid = (s + e) // 2
            far = edges[min(k + 3, len(edges) - 1)]
            reqs += [(i, s, 1), (i, mid, 1), (i, e - 1, 1), (i, mid, e - mid + 1), (i, s, e - s),
                     (i, mid, far - mid), (i, max(s - 1, 0), 2), (i, s, far - s + 1)]
        reqs += [(i, 0, n), (i, 1, n), (i, n - 1, 1)]
    want = modelled(d, reqs)
    assert all(w[0] > 0 for w in want)
    caps = [w[1][1] + 64 for w in want]
    for waves in (1, 3):
        check(read_ranges(cuda, product, d, reqs, caps, waves), want, caps, reqs)


# ---- 3. the final-run shortcut ----
def test_final_run_shortcut(cuda, product):
    R = 2 * product.compress_large_slice_size()
    rand = compressed(cuda, product, [data("rand", 3 * R + 5)], R)
    n = 3 * R + 5
    w = rand.words[0]
    assert w[1] == 4
    blocks, words = [rand.blocks[0]], [w]
    print("compressor-written random block: pairs", w[4:])
    for L in (14, 15, 16, 269, 270, 271, 15 + 2 * 255):
        b, wd, _, _ = run_block(L)
        blocks.append(b)
        words.append(wd)
    b, wd = counter_example_block()
    blocks.append(b)
    words.append(wd)
    one = X.emit([(rand.srcs[0], 0, 0)])   # the same bytes as one run, whatever matches the
    blocks.append(one)                     # compressor happened to find in them
    words.append([X.MAGIC, 4, n, len(one)] + [0] * 8 + [len(one), n])
    blocks.append(b"\x00")   # a final run of no bytes
    words.append(X.trivial_index(1, 0))
    op_last = w[5 + 2 * 3]
    reqs = [(0, 12345, 4096), (0, n - 4096, 4096), (0, n - 1, 1), (0, op_last, 1), (0, 0, n),
            (0, max(op_last - 1, 0), 40), (0, R - 7, R + 20), (0, 5, 1), (0, 77777, 100001)]
    handmade = len(reqs)
    reqs += [(len(blocks) - 2, a, ln) for _, a, ln in reqs]
    for i in range(1, len(blocks) - 2):
        m = words[i][2]
        reqs += [(i, 20, m - 20), (i, 21, 3), (i, m - 1, 1), (i, m - 7, 7),     # inside, to n
                 (i, 17, 4), (i, 19, 2), (i, 0, m), (i, 5, m),                   # straddling
                 (i, 0, 20), (i, 3, 9)]                                          # before the run
    reqs += [(len(blocks) - 1, 0, 5), (len(blocks) - 1, 1, 1)]
    # a forged op_2 near 2^32 over the one-run block: op_{j1+1} + 16 must not wrap; the window
    # is [op_1, n) and the segment fails its pair check
    blocks.append(one)
    words.append([X.MAGIC, 4, n, len(one), 0, 0, 0, 0, 0, 0xFFFFFFFD, 0, 0, len(one), n])
    reqs.append((len(blocks) - 1, n - 30, 1233))
    d = uploaded(cuda, blocks, words, 4)
    want = modelled(d, reqs)
    assert [x[:2] for x in want[-3:]] == [(0, (0, 0)), (-1, (0, 0)), (-1, (n - 30, n))]
    assert all(x[0] > 0 for x in want[:-3])
    assert want[handmade][:2] == (4096, (0, 4096))   # a 4 KiB read needs a 4 KiB destination
    caps = [x[1][1] + 64 for x in want]
    for k in (0, 1, handmade, handmade + 1):         # ... and gets exactly what it needs
        caps[k] = want[k][1][1]
    check(read_ranges(cuda, product, d, reqs, caps, 2), want, caps, reqs)
    src = rand.srcs[0]
    for k in list(range(9)) + list(range(handmade, handmade + 9)):
        assert want[k][2] == src[reqs[k][1]:reqs[k][1] + reqs[k][2]]


# ---- 4. capacity ----
def test_capacity(cuda, product):
    d, _, _, _ = round_trip_case(cuda, product)
    picks = [i for i, s in enumerate(d.srcs) if len(s) > 190000]   # 3 R + 5 and mixed()
    reqs = [(i, a, ln) for i in picks for a, ln in ((70000, 3000), (65000, 70000), (190000, 1000))]
    free = modelled(d, reqs)
    need = [x[1][1] for x in free]
    assert all(x[0] > 0 for x in free)
    tight = modelled(d, reqs, caps=[c - 1 for c in need])
    assert all(x[0] == RU.ERANGE and x[1] == y[1] for x, y in zip(tight, free))
    both = reqs + reqs
    caps = [c - 1 for c in need] + need
    got = read_ranges(cuda, product, d, both, caps, 4)
    check(got, tight + free, caps, both)
    k = len(reqs)
    assert got[0][:k] == [product.ERANGE] * k and [w[1] for w in got[1][:k]] == need
    for buf in got[2][:k]:
        assert buf == bytes([CANARY]) * len(buf)


# ---- 5. malformed input ----
def test_malformed_input_is_judged_as_the_model_judges_it(cuda, product):
    """Wrong index words and flipped stream bytes, three requests each (first segment, middle,
    last): a result is negative if and only if the model's is; a positive one equals the
    model's in value and bytes (a stream with a zero offset by value only: such a match
    copies dst bytes that nobody wrote); nothing is written past need."""
    S = product.compress_large_slice_size()
    srcs = [data("text", 2 * S + 3000), data("comp", 2 * S + 3000)]
    good = compressed(cuda, product, srcs, S)
    assert good.max_seg == 3
    blocks, words, base, erange = [], [], [], []
    for i, (s, comp) in enumerate(zip(srcs, good.blocks)):
        w = good.words[i]
        assert w[1] == 3 and len(w) == 12
        n = len(s)

        def add(wd, stream=comp):
            blocks.append(stream)
            words.append(list(wd))
            base.append(i)

        add(w)
        for k in range(4, 12):                 # every ip and op, +-1
            for e in (1, -1):
                m = list(w)
                m[k] = (m[k] + e) & 0xFFFFFFFF
                add(m)
        for a, b in ((1, 2), (0, 1), (2, 3)):  # swapped pairs
            m = list(w)
            m[4 + 2 * a:6 + 2 * a], m[4 + 2 * b:6 + 2 * b] = w[4 + 2 * b:6 + 2 * b], w[4 + 2 * a:6 + 2 * a]
            add(m)
        add([w[0] ^ 1] + w[1:])
        add([w[0] + (1 << 24)] + w[1:])
        for k, vals in ((1, (0, 1, 2)), (2, (n - 1, n + 1, 0)), (3, (len(comp) - 1, len(comp) + 1, 0))):
            for v in vals:
                m = list(w)
                m[k] = v
                add(m)
        erange.append(len(blocks))
        add(w[:1] + [4] + w[2:] + [0, 0])      # nseg = maxSegments + 1
        rng = random.Random(1000 + i)
        for _ in range(200):                   # single bits of the stream
            at = rng.randrange(len(comp))
            flipped = bytearray(comp)
            flipped[at] ^= 1 << rng.randrange(8)
            add(w, bytes(flipped))
    d = uploaded(cuda, blocks, words, 3)
    n = len(srcs[0])
    three = ((1000, 500), (S + 1000, 500), (n - 1000, 500))
    reqs = [(k, a, ln) for k in range(len(blocks)) for a, ln in three]
    memos = {}
    want = []
    for k, a, ln in reqs:   # (mutations of one source block share the segments they left alone)
        want.append(RU.decode_range(blocks[k], words[k], a, ln, 1 << 30, 3,
                                    memo=memos.setdefault(base[k], {})))
    caps = [x[1][1] + 64 for x in want]
    rs, wins, bufs = read_ranges(cuda, product, d, reqs, caps, 2)
    negative = 0
    for q, ((k, a, ln), (er, ewin, edata)) in enumerate(zip(reqs, want)):
        assert (rs[q] < 0) == (er < 0), (q, k, a, rs[q], er)
        if k in erange:
            assert rs[q] == product.ERANGE
        assert wins[q] == ewin, (q, k, a)
        written = 0 if er == RU.ERANGE else ewin[1]
        assert bufs[q][written:] == bytes([CANARY]) * (caps[q] - written), (q, k, a)
        if er < 0:
            negative += 1
            continue
        assert rs[q] == er, (q, k, a)
        assert bufs[q][ewin[0]:ewin[0] + er] == edata or RU.has_offset0(blocks[k]), (q, k, a)
    for i, first in enumerate((0, erange[0] + 201)):   # the unmutated blocks
        assert blocks[first] == good.blocks[i] and words[first] == good.words[i]
        for t, (a, ln) in enumerate(three):
            assert rs[3 * first + t] == ln and want[3 * first + t][2] == srcs[i][a:a + ln]
    assert negative > 100
    print("%d of %d requests on malformed input rejected" % (negative, len(reqs)))


# ---- 6. graph capture ----
def test_graph_capture_with_the_compressor(cuda, product):
    R = 2 * product.compress_large_slice_size()
    srcs = [data("comp", 300000), data("text", 4 * R + 1)]
    max_src = 300000
    caps = [product.compressBound(len(s)) for s in srcs]
    src, sptr, _ = pack(cuda, srcs)
    szs, cps = ints(cuda, map(len, srcs)), ints(cuda, caps)
    scr = cuda.empty(product.compress_large_scratch_size(2, max_src), dtype=cuda.uint8, device="cuda")
    stride, max_seg = product.large_index_size(max_src, R), product.large_index_segments(max_src, R)
    index = cuda.zeros((2, stride), dtype=cuda.uint8, device="cuda")
    dst, dptr, _ = alloc_out(cuda, caps)
    res = ints(cuda, [-7, -7])
    reqs = [(0, 100, 5000), (1, R - 10, 2 * R), (0, 299000, 5000), (1, 4 * R, 1), (1, 0, 4 * R + 1),
            (0, 300001, 1)]
    rcaps = [ln + 2 * R + 64 for _, _, ln in reqs]
    back, bptr, boffs = alloc_out(cuda, rcaps)
    block_of, starts = ints(cuda, (q[0] for q in reqs)), ints(cuda, (q[1] for q in reqs))
    lens, rc = ints(cuda, (q[2] for q in reqs)), ints(cuda, rcaps)
    win, rres = ints(cuda, [-7] * (2 * len(reqs))), ints(cuda, [-7] * len(reqs))
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.compress_large_indexed_ptr_batch(sptr, szs, dptr, cps, res, max_src, R, index=index,
                                                 scratch=scr, stream=s)
        product.decompress_range_indexed_ptr_batch(dptr, res, index, max_seg, starts, lens, bptr, rc,
                                                   win, rres, block_of=block_of, waves_per_request=3,
                                                   stream=s)
    for _ in range(2):
        g.replay()
    cuda.cuda.synchronize()
    rs, w, host = rres.cpu().tolist(), win.cpu().tolist(), back.cpu().numpy()
    for k, (i, a, ln) in enumerate(reqs):
        m = min(ln, len(srcs[i]) - a)
        if m < 0:
            assert rs[k] == -1
            continue
        assert rs[k] == m and 0 <= w[2 * k] and w[2 * k] + m <= w[2 * k + 1] <= rcaps[k]
        o = boffs[k] + w[2 * k]
        assert host[o:o + m].tobytes() == srcs[i][a:a + m], k
