"""Large blocks with restart points and a seek index (include/ape_lz4_gpu.h):
APE_LZ4_compress_large_indexed_batch_dev places a restart point every R bytes and writes the
index; APE_LZ4_decompress_safe_indexed_batch_dev decodes one wave per segment.

The checkers are the oracle's decompress_safe (and the reference's own, when built), a Python
stitch of compress_prefix_batch's slices, and the Python model of the format in
tests/indexutil.py."""
import base64
import ctypes as C
import functools
import random
import struct

import numpy as np
import pytest

import gen_golden
import indexutil as X
from gpuutil import CANARY, alloc_out, fetch, ints, pack
from lz4util import I, buf, orc_compress, orc_decompress, ref_lib, sha, walk_ok

pytestmark = pytest.mark.gpu

MB = 1 << 20


@functools.lru_cache(maxsize=None)
def _master(content):
    return I.make(content, MB)


def data(content, n):
    return _master(content)[:n]


def mixed():
    return I.synth_rand(100000, 7) + data("comp", 150000) + I.synth_rand(40000, 8) + bytes(70000)


def check_block(oracle, src, comp):
    n = len(src)
    assert orc_decompress(oracle, comp, n) == (n, src)
    ref = ref_lib()
    if ref is not None:
        out = C.create_string_buffer(n + 64)
        assert ref.APE_LZ4_decompress_safe(buf(comp), out, len(comp), n) == n and out.raw[:n] == src


def words_of(index, i, count=None):
    raw = bytes(index[i].cpu().numpy().tobytes())
    w = list(struct.unpack("<%dI" % (len(raw) // 4), raw))
    return w if count is None else w[:count]


class Packed:
    """One compress_large_indexed launch, kept on the device for a decode."""

    def __init__(self, torch, amd, srcs, R, caps=None, with_index=True, max_src=None):
        self.srcs = srcs
        nb = len(srcs)
        self.max_src = max_src or max(map(len, srcs))
        self.src, self.sptr, _ = pack(torch, srcs)
        self.caps = caps or [amd.compressBound(len(s)) for s in srcs]
        self.dst, self.dptr, self.doffs = alloc_out(torch, self.caps)
        self.res = ints(torch, [-7] * nb)
        self.szs = ints(torch, map(len, srcs))
        self.stride = amd.large_index_size(self.max_src, R)
        self.max_seg = amd.large_index_segments(self.max_src, R)
        self.index = None
        if with_index:
            self.index = torch.full((nb, self.stride), CANARY, dtype=torch.uint8, device="cuda")
        amd.compress_large_indexed_ptr_batch(self.sptr, self.szs, self.dptr, ints(torch, self.caps),
                                             self.res, self.max_src, R, index=self.index)
        torch.cuda.synchronize()
        self.rs = self.res.cpu().tolist()
        self.outs = [fetch(self.dst, o, max(r, 0)) for o, r in zip(self.doffs, self.rs)]


def run_decode(torch, amd, blocks, caps, indexes, max_seg, stride=None):
    """One indexed decode of host-side blocks and index word lists: (results, outputs)."""
    nb = len(blocks)
    stride = stride or (16 + 8 * (max_seg + 1) + 15) // 16 * 16
    src, sptr, _ = pack(torch, blocks)
    dst, dptr, doffs = alloc_out(torch, caps)
    raw = b"".join(X.index_bytes(w, stride) for w in indexes)
    index = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).view(nb, stride).cuda()
    res = ints(torch, [-7] * nb)
    amd.decompress_indexed_ptr_batch(sptr, ints(torch, map(len, blocks)), dptr, ints(torch, caps),
                                     index, max_seg, res)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    return rs, [fetch(dst, o, r) for o, r in zip(doffs, rs)]


def run_plain(torch, amd, blocks, caps):
    src, sptr, _ = pack(torch, blocks)
    dst, dptr, doffs = alloc_out(torch, caps)
    res = ints(torch, [-7] * len(blocks))
    amd.decompress_ptr_batch(sptr, ints(torch, map(len, blocks)), dptr, ints(torch, caps), res)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    return rs, [fetch(dst, o, r) for o, r in zip(doffs, rs)]


# ---- 1. restart placement ----
def restart_slices(torch, amd, srcs, S, R):
    """Every slice of every input through compress_prefix_batch with the history the restart
    rule gives it: slice at `start` gets prefix min(start - group start, 65536 - len)."""
    src, sptr, _ = pack(torch, srcs)
    base = sptr.cpu().tolist()
    ptrs, lens, pres, owner = [], [], [], []
    for i, s in enumerate(srcs):
        for st in range(0, len(s), S):
            ln = min(S, len(s) - st)
            ptrs.append(base[i] + st)
            lens.append(ln)
            pres.append(min(st - st // R * R, 65536 - ln))
            owner.append(i)
    caps = [amd.compressBound(n) for n in lens]
    dst, dptr, doffs = alloc_out(torch, caps)
    res = ints(torch, [-7] * len(lens))
    amd.compress_prefix_batch(torch.tensor(ptrs, dtype=torch.int64, device="cuda"), ints(torch, lens),
                              ints(torch, pres), dptr, ints(torch, caps), res)
    torch.cuda.synchronize()
    out = [[] for _ in srcs]
    for i, o, r in zip(owner, doffs, res.cpu().tolist()):
        assert r > 0
        out[i].append(fetch(dst, o, r))
    return out


def test_restart_placement_is_exactly_the_rule(cuda, product, oracle):
    S = product.compress_large_slice_size()
    srcs = [data("text", 200000), data("comp", 3 * S + 777), mixed()]
    for R in (S, 2 * S, 4 * S):
        want = [X.stitch(st) for st in restart_slices(cuda, product, srcs, S, R)]
        got = Packed(cuda, product, srcs, R, with_index=False)
        for s, w, r, c in zip(srcs, want, got.rs, got.outs):
            assert r == len(w) and c == w, (R, len(s))
            check_block(oracle, s, c)
    # no restart point inside the input: the plain call's bytes
    plain = Packed(cuda, product, srcs, 0, with_index=False)
    caps = plain.caps
    dst, dptr, doffs = alloc_out(cuda, caps)
    res = ints(cuda, [-7] * len(srcs))
    product.compress_large_ptr_batch(plain.sptr, plain.szs, dptr, ints(cuda, caps), res, plain.max_src)
    cuda.cuda.synchronize()
    base_r = res.cpu().tolist()
    base = [fetch(dst, o, r) for o, r in zip(doffs, base_r)]
    assert plain.rs == base_r and plain.outs == base
    far = Packed(cuda, product, srcs, 16 * S)   # R >= n
    assert far.rs == base_r and far.outs == base
    # history costs ratio only where it is withheld
    text = [data("text", MB)]
    r8, r1 = Packed(cuda, product, text, 8 * S).rs[0], Packed(cuda, product, text, S).rs[0]
    r0 = Packed(cuda, product, text, 0).rs[0]
    print("1 MiB text: R = 0 %d, R = 8 S %d, R = S %d bytes" % (r0, r8, r1))
    assert 0 < r8 < r1


# ---- 2. the index ----
CONTENTS = ("comp", "text", "rand", "zeros", "period7")


_BATCH = []


def batch(torch, amd):
    """Five contents x six sizes around the restart points, R = 2 S: compressed once, shared by
    the index test and the round trip."""
    if not _BATCH:
        R = 2 * amd.compress_large_slice_size()
        sizes = [65537, R - 1, R, R + 1, 2 * R + 1, 3 * R + 5]
        _BATCH.append((Packed(torch, amd, [data(c, n) for c in CONTENTS for n in sizes], R), R))
    return _BATCH[0]


def check_index(S, R, src, comp, w, oracle):
    n, c = len(src), len(comp)
    nseg = 1 if n <= 65536 or n <= R else -(-n // R)
    assert w[:4] == [X.MAGIC, nseg, n, c], (n, w[:4])
    pairs = [(w[4 + 2 * j], w[5 + 2 * j]) for j in range(nseg + 1)]
    assert pairs[0] == (0, 0) and pairs[-1] == (c, n) and pairs == sorted(pairs)
    ip, op, seqs = 0, 0, []
    for lit, off, ml in walk_ok(comp):
        seqs.append((ip, op, lit, off, ml))
        ip += 1 + len(X._length(lit)) + lit + (2 + len(X._length(ml - 4)) if ml else 0)
        op += lit + ml
    assert (ip, op) == (c, n)
    at = {s[0]: s[1] for s in seqs}
    for j, (pi, po) in enumerate(pairs[:-1]):
        assert at.get(pi) == po, (n, j)   # a token, and its literals start there
        assert po <= j * R, (n, j)
    j = 0
    for pi, po, lit, off, ml in seqs:
        while j + 1 < nseg and pairs[j + 1][0] <= pi:
            j += 1
        if ml:
            assert po + lit - off >= pairs[j][1], (n, j, pi)
    check_block(oracle, src, comp)


def test_index_is_true(cuda, product, oracle):
    S = product.compress_large_slice_size()
    b, R = batch(cuda, product)
    assert all(r > 0 for r in b.rs)
    for i, (s, c) in enumerate(zip(b.srcs, b.outs)):
        check_index(S, R, s, c, words_of(b.index, i), oracle)
    # 65 slices: the offsets kernel's second trip of 64
    long_src = (data("comp", MB) + data("text", MB) + data("comp", MB))[:64 * S + 100]
    one = Packed(cuda, product, [long_src], R)
    assert one.rs[0] > 0
    check_index(S, R, long_src, one.outs[0], words_of(one.index, 0), oracle)
    # a block that does not fit: no segments, nothing written
    srcs = [data("text", 3 * R + 5), data("comp", 65537)]
    fit = Packed(cuda, product, srcs, R)
    tight = Packed(cuda, product, srcs, R, caps=[r - 1 for r in fit.rs])
    assert tight.rs == [0, 0]
    for i, (o, r) in enumerate(zip(tight.doffs, fit.rs)):
        assert words_of(tight.index, i, 2) == [X.MAGIC, 0]
        assert fetch(tight.dst, o, r + 64) == bytes([CANARY]) * (r + 64)


# ---- 3. round trip ----
def test_round_trip_and_graph_capture(cuda, product):
    b, R = batch(cuda, product)
    nb = len(b.srcs)
    sizes = [len(s) for s in b.srcs]

    def decode(stream=None):
        back, bptr, boffs = alloc_out(cuda, sizes)
        dres = ints(cuda, [-7] * nb)
        product.decompress_indexed_ptr_batch(b.dptr, b.res, bptr, b.szs, b.index, b.max_seg, dres,
                                             stream=stream)
        return back, boffs, dres

    back, boffs, dres = decode()
    cuda.cuda.synchronize()
    assert dres.cpu().tolist() == sizes
    for s, o in zip(b.srcs, boffs):
        assert fetch(back, o, len(s)) == s          # (the canaries around it: conftest)

    # compressor and decoder captured together on a side stream, replayed twice
    srcs = [data("comp", 300000), data("text", 4 * R + 1)]
    caps = [product.compressBound(len(s)) for s in srcs]
    src, sptr, _ = pack(cuda, srcs)
    szs, cps = ints(cuda, map(len, srcs)), ints(cuda, caps)
    scr = cuda.empty(product.compress_large_scratch_size(2, 300000), dtype=cuda.uint8, device="cuda")
    stride, max_seg = product.large_index_size(300000, R), product.large_index_segments(300000, R)
    index = cuda.zeros((2, stride), dtype=cuda.uint8, device="cuda")
    dst, dptr, doffs = alloc_out(cuda, caps)
    back, bptr, boffs = alloc_out(cuda, [len(s) for s in srcs])
    res, dres = ints(cuda, [-7, -7]), ints(cuda, [-7, -7])
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.compress_large_indexed_ptr_batch(sptr, szs, dptr, cps, res, 300000, R, index=index,
                                                 scratch=scr, stream=s)
        product.decompress_indexed_ptr_batch(dptr, res, bptr, szs, index, max_seg, dres, stream=s)
    for _ in range(2):
        g.replay()
    cuda.cuda.synchronize()
    assert dres.cpu().tolist() == [len(x) for x in srcs]
    for x, o in zip(srcs, boffs):
        assert fetch(back, o, len(x)) == x


# ---- 4. reference-made blocks ----
def stitched_case(oracle):
    sizes = (70000, 13, 65536, 100000, 1)
    text = data("text", sum(sizes))
    starts = [sum(sizes[:k]) for k in range(len(sizes))]
    streams = [orc_compress(oracle, text[a:a + n])[1] for a, n in zip(starts, sizes)]
    block = X.stitch(streams)
    return text, block, X.build_index(block, starts)


def test_decoder_against_reference_made_blocks(cuda, product, oracle):
    text, block, words = stitched_case(oracle)
    n = len(text)
    blocks, caps = [block] * 3, [n, n + 17, n - 1]
    idx = [words, words, words]
    rs, outs = run_decode(cuda, product, blocks, caps, idx, 5)
    assert rs[:2] == [n, n] and outs[0] == text and outs[1] == text
    assert rs[2] == -1   # n > cap: the header check
    prs, pouts = run_plain(cuda, product, blocks[:2], caps[:2])
    assert (rs[:2], outs[:2]) == (prs, pouts)
    assert X.decode_indexed(block, words, n) == (n, text)


# ---- 5. one segment ----
def test_one_segment_is_the_plain_decoder(cuda, product, golden):
    cases = golden["decode"]
    comps = [base64.b64decode(d["comp_b64"]) for d in cases]
    caps = [d["cap"] for d in cases]
    idx = [X.trivial_index(len(c), max(d["ret"], 0)) for c, d in zip(comps, cases)]
    rs, outs = run_decode(cuda, product, comps, caps, idx, 1)
    prs, pouts = run_plain(cuda, product, comps, caps)
    for d, r, out, pr, pout in zip(cases, rs, outs, prs, pouts):
        assert r == d["ret"] == pr, d["name"]
        if r > 0 and not d["has_offset0"]:
            assert sha(out) == d["out_sha256"] and out == pout, d["name"]


# ---- 6. stop edges ----
def _seq(kind, rng, avail):
    """One sequence with a match: (literals, offset, match length); avail = bytes of the
    segment written before its literals."""
    if kind == "lit":      # 15 + 255 + 3 literals: two length bytes, the scalar path
        lits = bytes(rng.randrange(256) for _ in range(273))
    else:
        lits = bytes([rng.randrange(256)])
    reach = avail + len(lits)
    off = 1 + rng.randrange(min(reach, 300))
    ml = 4 + 15 + 255 if kind == "match" else 4   # 19 + 255: two match-length bytes
    return lits, off, ml


def _segment_of(k, last_kind, rng, five=0, plain=False):
    """k sequences; the last one (directly before the stop) of last_kind, every 37th of the
    others complex too (the first one: directly after the previous stop) unless `plain`;
    `five` of them with two literals (5 bytes instead of 4) to place the stop at any byte."""
    seqs, avail = [], 0
    for q in range(k):
        kind = "simple" if plain or q % 37 else ("lit", "match", "simple")[q // 37 % 3]
        if q == k - 1:
            kind = last_kind
        lits, off, ml = _seq(kind, rng, avail)
        if kind == "simple" and five > 0:
            lits += bytes([rng.randrange(256)])
            five -= 1
        seqs.append((lits, off, ml))
        avail += len(lits) + ml
    return seqs


def stop_edge_block(seed, sized=None):
    rng = random.Random(seed)
    segs = []
    for k in (1, 2, 63, 64, 65, 107, 108, 200):
        for kind in ("simple", "lit", "match"):
            segs.append(_segment_of(k, kind, rng))
            if rng.randrange(3) == 0:
                segs.append([])                      # an empty segment
    if sized is not None:   # a segment of `sized` compressed bytes: 4-byte sequences and fives
        segs.insert(3, _segment_of(sized // 4, "simple", rng, five=sized % 4, plain=True))
        segs.insert(3, [])
    tail = bytes(rng.randrange(256) for _ in range(40))
    flat, pairs, ip, op = [], [], 0, 0
    for sg in segs:
        pairs.append((ip, op))
        for s in sg:
            flat.append(s)
            ip += len(X.emit([s]))
            op += len(s[0]) + s[2]
    if not segs[-1]:
        pairs[-1] = (ip, op)
    pairs.append((ip, op))   # the last segment: the final run alone
    block = X.emit(flat + [(tail, 0, 0)])
    n = op + len(tail)
    nseg = len(pairs)
    words = [X.MAGIC, nseg, n, len(block)] + [v for p in pairs for v in p] + [len(block), n]
    return block, words, n


def test_stop_edges(cuda, product, oracle):
    blocks, idx, ns = [], [], []
    # the stop within 84 bytes of the 2304-byte stage boundary (either side), and far from it
    for seed, sized in enumerate((None, 2220, 2221, 2262, 2303, 2304, 2305, 2388)):
        b, w, n = stop_edge_block(seed, sized)
        blocks.append(b)
        idx.append(w)
        ns.append(n)
    want = []
    for b, w, n in zip(blocks, idx, ns):
        r, out = X.decode_indexed(b, w, n)
        assert r == n
        assert orc_decompress(oracle, b, n) == (n, out)   # (the model is a true decoder)
        want.append(out)
    max_seg = max(w[1] for w in idx)
    rs, outs = run_decode(cuda, product, blocks, ns, idx, max_seg)
    assert rs == ns
    for k, (o, w) in enumerate(zip(outs, want)):
        assert o == w, k
    rs, outs = run_decode(cuda, product, blocks, [n + 100 for n in ns], idx, max_seg + 3)
    assert rs == ns and outs == want


# ---- 7. malformed input ----
def test_malformed_input_is_rejected_in_bounds(cuda, product, oracle):
    """Wrong index words and flipped stream bytes: every result is negative, or it is the
    oracle's decompress_safe of that stream, value and bytes (a stream with a zero offset by
    value only: the reference then copies uninitialised dst bytes); nothing is
    written outside dst[0, cap) (the canaries, checked after the test)."""
    S = product.compress_large_slice_size()
    R = 3 * S
    srcs = [data("text", 200000), data("comp", 200000)]
    good = Packed(cuda, product, srcs, R)
    assert good.max_seg == 3
    blocks, idx, caps = [], [], []
    erange = []
    for i, (s, comp) in enumerate(zip(srcs, good.outs)):
        w = words_of(good.index, i, 4 + 2 * 4)
        assert w[1] == 3
        n = len(s)

        def add(words, stream=comp):
            blocks.append(stream)
            idx.append(list(words))
            caps.append(n)

        add(w)
        for k in range(4, 12):                 # every ip and op, +-1
            for d in (1, -1):
                m = list(w)
                m[k] = (m[k] + d) & 0xFFFFFFFF
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
        add(w[:1] + [4] + w[2:])               # nseg = maxSegments + 1
        rng = random.Random(1000 + i)
        for _ in range(200):                   # single bytes of the stream
            at = rng.randrange(len(comp))
            flipped = bytearray(comp)
            flipped[at] ^= 1 << rng.randrange(8)
            add(w, bytes(flipped))
    rs, outs = run_decode(cuda, product, blocks, caps, idx, 3)
    negative = 0
    for k, (b, cap, r, out) in enumerate(zip(blocks, caps, rs, outs)):
        if k in erange:
            assert r == product.ERANGE, k
        if r < 0:
            negative += 1
            continue
        er, eout = orc_decompress(oracle, b, cap)
        assert r == er, k
        assert out == eout or gen_golden.has_offset0(b), k
    assert rs[0] == caps[0] and negative > 40
    print("%d of %d malformed inputs rejected" % (negative, len(blocks)))
