"""GPU fast encoder against tests/encmodel.py, byte for byte.

The encoder's output is a pure function of (input bytes, used prefix, acceleration); encmodel
states that function.  Every assertion here is byte equality with the model: at the sizes where
the kernel changes path (blocks below 128 bytes, the general edge steps, the steps without edge
code from 328 bytes on), at every alignment, on inputs built for each rule's edge, through every
entry point that runs the kernel, with acceleration and with a history prefix.

The case lists are plain functions, so that tests/test_enc_model.py (CPU) can show that these
inputs tell the model from its wrong neighbours."""
import ctypes as C
import functools
import random

import pytest

import encmodel
from gpuutil import alloc_out, fetch, ints, pack
from lz4util import I, buf

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 12, 13, 14, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 327, 328, 329, 391, 392,
         393, 455, 456, 457, 1023, 1024, 1025, 1087, 1088, 1089, 4096, 65535, 65536]
SMALL_SIZES = [n for n in SIZES if n <= 4096]
CONTENTS = ["comp", "text", "zeros", "period7", "rand"]
ACCELS = [2, 3, 8, 65, 1 << 26]
PREFIXES = [0, 63, 64, 65, 127, 128, 8192, 65536]


@functools.lru_cache(maxsize=None)
def model(src, prefix=b"", accel=1):
    """The model's block of one case, computed once for the whole session."""
    return encmodel.encode(src, prefix, accel)


# ---------------- the inputs (no GPU needed to build them) ----------------
def _rand(seed, n):
    return random.Random(seed).randbytes(n)


def _repeat_of(seed, length, gap=70, follow=b""):
    """Random bytes in which one string of `length` bytes occurs twice, `gap` random bytes apart,
    the bytes before and after the two occurrences differing: one match of exactly `length`."""
    s = _rand(seed, length)
    g = _rand(seed + 1, gap)
    return _rand(seed + 2, 63) + b"\x01" + s + b"\x02" + g + b"\x03" + s + b"\x04" + follow


def _many_roots():
    """64 consecutive positions whose candidates all have different offsets and 13 bytes of
    match: every lane of the chunk is a stage-2 root (four passes of 16)."""
    x = _rand(40, 64 + 13)
    out = bytearray(_rand(41, 64))
    for j in range(64):
        out += x[j:j + 13] + bytes([x[j + 13] ^ 0xFF])
    out += b"\x00" * (-len(out) % 64)
    return bytes(out) + x + _rand(42, 30)


def crafted_cases():
    """(name, src, prefix, acceleration) of the inputs built for one rule's edge each."""
    from test_gpu_encode import _boundary_copies
    cs = []
    for L in (75, 76, 77, 76 + 1023, 76 + 1024, 76 + 1025):
        cs.append(("match of %d" % L, _repeat_of(L, L, follow=_rand(7, 40)), b"", 1))
    t = _rand(11, 60)
    # the second copy runs to the block's end: cut at n - 5
    cs.append(("match ends at n - 5", _rand(12, 64) + t + _rand(13, 70) + t[:45], b"", 1))
    cs.append(("match starts at n - 12", _rand(14, 100) + t[:20] + _rand(15, 64) + t[:12], b"", 1))
    cs.append(("string starts at n - 11", _rand(14, 100) + t[:20] + _rand(15, 64) + t[:11], b"", 1))
    for at in (3, 4):
        for L in (7, 12):   # (7: the key alone, so that no later position finds the copy)
            b = bytearray(_rand(16, 300))
            b[100:100 + L] = b[at:at + L]
            b[100 + L] = b[at + L] ^ 0x55
            cs.append(("candidate at %d, %d bytes" % (at, L), bytes(b), b"", 1))
    # the block's start again right after a match: positions 1..3 are no candidates, position 4
    # is one, its 4 equal bytes before it (the previous match's last byte is the block's first)
    # cut to 3 by the previous match end
    v = _rand(17, 40)
    s = _rand(18, 39) + v[:1]
    blk = v + _rand(19, 30) + b"\x05" + s + _rand(20, 90) + b"\x06"
    cs.append(("back stopped by the previous match", blk + s + v[1:] + _rand(21, 30), b"", 1))
    # the same with acceleration: the first probe with a candidate lies 10 bytes after the match
    # end, and the catch-up's 11 equal bytes are cut to 10
    cs.append(("catch-up stopped by the previous match", blk + s + v[1:] + _rand(21, 30), b"", 8))
    # a probe lands 6 bytes into a copy of the block's start: the catch-up stops at position 0
    cs.append(("back stopped at position 0", v + _rand(22, 260) + v + _rand(23, 30), b"", 8))
    # 7 bytes found only by the 65th probe after the block's start (3, then 64 with gap 2, then
    # gap 3: position 2 + 128 + 3)
    s7 = _rand(33, 7)
    cs.append(("the 65th probe", _rand(34, 10) + s7 + _rand(35, 116) + s7 + _rand(36, 30), b"", 2))
    # the last position whose table entry can be used: n - 13, the last lane of its chunk, found
    # from n - 12 (a later position starts no match, so whether it is written cannot show)
    cs.append(("candidate at n - 13", _rand(37, 190) + b"B" + b"A" * 13, b"", 1))
    cs.append(("more than 16 stage-2 roots", _many_roots(), b"", 1))
    lens = [11, 12, 13, 15, 16, 17, 19, 20, 21, 75, 76, 77, 79, 80, 81, 83, 84, 85, 86]
    cs.append(("measurement edges", _boundary_copies(4099, 4299, lens), b"", 1))
    s30 = _rand(28, 30)
    cs.append(("literal run past the ring", s30 + _rand(29, 1500) + s30 + _rand(30, 20), b"", 1))
    cs.append(("record past the staging buffer", s30 + _rand(31, 600) + s30 + _rand(32, 20), b"", 1))
    return cs


def size_cases():
    return [("%s %d" % (c, n), I.make(c, n, seed=n), b"", 1) for c in CONTENTS for n in SIZES]


def accel_cases():
    cs = [("comp 65536/%d x%d" % (b, a), I.synth_comp(65536, 100 + b), b"", a)
          for a in ACCELS for b in range(4)]
    cs += [("%s %d x%d" % (c, n, a), I.make(c, n, seed=n + 1), b"", a)
           for a in ACCELS for c in ("comp", "text", "period7") for n in SMALL_SIZES]
    return cs


STREAM = 16 * 8192


@functools.lru_cache(maxsize=None)
def _stream_bytes():
    return I.synth_comp(STREAM // 2, 77) + I.text(STREAM // 2, 5)


def prefix_cases():
    hist = I.text(65536, 9)[:40000] + I.synth_comp(25536, 31)
    cs = []
    for pre in PREFIXES:
        for n in (13, 100, 457, 4096):
            # (copies of the history's last 40 and 100 bytes first: what a prefix of 63 .. 128
            # bytes can give)
            src = (hist[-40:-20] + hist[-100:-80] + hist[-3000:n // 2 - 3000] +
                   I.make("comp", n, seed=pre))[:n]
            cs.append(("prefix %d n %d" % (pre, n), src, hist[65536 - pre:], 1))
    for tot in (65535, 65536, 65537):
        for pre in (64, 200, 4096, 60000):
            n = tot - pre
            cs.append(("prefix %d + n %d" % (pre, n), (hist[pre:] + hist)[:n], hist[:pre], 1))
    s = _stream_bytes()
    cs += [("stream chunk %d" % k, s[8192 * k:8192 * (k + 1)], s[:8192 * k], 1) for k in range(16)]
    return cs


def bench_cases():
    return [("App. C block %d" % b, I.synth_comp(65536, b), b"", 1) for b in range(16)]


def all_cases():
    return size_cases() + crafted_cases() + accel_cases() + prefix_cases() + bench_cases()


# ---------------- running the kernel ----------------
def run(torch, amd, cases, caps=None, in_mis=None, out_mis=None, stream=None):
    """One launch for cases that share (prefixed or not, acceleration): (results, blocks)."""
    srcs = [c[1] for c in cases]
    pres = [c[2] for c in cases]
    accel = cases[0][3]
    assert all(c[3] == accel for c in cases)
    with_prefix = any(pres)
    assert not (with_prefix and accel != 1)
    caps = [amd.compressBound(len(s)) for s in srcs] if caps is None else caps
    src, sptr, _ = pack(torch, [p + s for p, s in zip(pres, srcs)], misalign=in_mis)
    sptr = sptr + torch.tensor([len(p) for p in pres], dtype=torch.int64, device="cuda")
    dst, dptr, doffs = alloc_out(torch, caps, misalign=out_mis)
    res = ints(torch, [-7] * len(srcs))
    sizes, capt, psz = ints(torch, map(len, srcs)), ints(torch, caps), ints(torch, map(len, pres))
    if stream is not None:   # (the buffers above were filled on the current stream)
        stream.wait_stream(torch.cuda.current_stream())
    if with_prefix:
        amd.compress_prefix_batch(sptr, sizes, psz, dptr, capt, res, stream=stream)
    elif accel != 1 or stream is not None:
        amd.compress_fast_ptr_batch(sptr, sizes, dptr, capt, res, accel, stream=stream)
    else:
        rc = amd.lib().APE_LZ4_compress_batch_dev(sptr.data_ptr(), sizes.data_ptr(), dptr.data_ptr(),
                                                  capt.data_ptr(), res.data_ptr(), len(srcs), None)
        assert rc == 0, amd.gpu_last_error()
    if stream is not None:
        return lambda: _collect(torch, res, dst, doffs, (src, sptr, sizes, capt, psz))
    torch.cuda.synchronize()
    return _collect(torch, res, dst, doffs, None)


def _collect(torch, res, dst, doffs, keep):
    rs = res.cpu().tolist()
    return rs, [fetch(dst, o, r) for o, r in zip(doffs, rs)]


def expect(cases):
    return [model(c[1], c[2], c[3]) for c in cases]


def assert_model(cases, rs, comps):
    for c, r, got, want in zip(cases, rs, comps, expect(cases)):
        assert r == len(want), (c[0], r, len(want))
        assert got == want, (c[0], next(i for i in range(r) if got[i] != want[i]))


def by_launch(cases):
    """The cases grouped by what one launch can take: (prefixed, acceleration)."""
    groups = {}
    for c in cases:
        groups.setdefault((bool(c[2]), c[3]), []).append(c)
    return list(groups.values())


# ---------------- the tests ----------------
def test_sizes_and_contents(cuda, product):
    cases = size_cases()
    assert_model(cases, *run(cuda, product, cases))


def test_every_alignment(cuda, product):
    """Source and destination misaligned by 0..15 bytes each, all 256 pairs, on blocks of each
    path."""
    base = [("comp %d" % n, I.make("comp", n, seed=3 + n), b"", 1) for n in (100, 457, 1089)] + \
           [("text 4096", I.text(4096, 2), b"", 1)]
    for c in base:
        cases = [c] * 256
        rs, comps = run(cuda, product, cases, in_mis=[i % 16 for i in range(256)],
                        out_mis=[i // 16 for i in range(256)])
        assert_model(cases, rs, comps)


def test_crafted_inputs(cuda, product):
    for cases in by_launch(crafted_cases()):
        assert_model(cases, *run(cuda, product, cases))


def _mix():
    return [c for c in size_cases() if c[0] in (
        "comp 0", "comp 13", "text 127", "comp 128", "text 329", "comp 457", "period7 1025",
        "comp 4096", "rand 4096", "zeros 65535", "comp 65536", "text 65536")] + \
        [c for c in crafted_cases() if c[3] == 1]


def test_alone_and_in_a_mixed_batch(cuda, product):
    mix = _mix()
    for c in mix[:8] + mix[-2:]:
        assert_model([c], *run(cuda, product, [c]))
    rng = random.Random(5)
    small = [c for c in mix if len(c[1]) <= 4096]
    batch = [rng.choice(small) for _ in range(300)]
    for at, c in zip((0, 1, 63, 64, 150, 298, 299), mix[-7:]):
        batch[at] = c
    for at, c in zip((7, 100, 200, 250), [c for c in mix if len(c[1]) > 4096]):
        batch[at] = c
    assert_model(batch, *run(cuda, product, batch))


def test_capacities(cuda, product):
    """The bytes do not depend on the capacity; one byte too few gives 0 and writes nothing
    outside the slot (the canaries around every slot are checked after the test)."""
    mix = _mix()
    want = expect(mix)
    for d in (0, 1):
        assert_model(mix, *run(cuda, product, mix, caps=[len(w) + d for w in want]))
    rs, _ = run(cuda, product, mix, caps=[len(w) - 1 for w in want])
    assert rs == [0] * len(mix)
    for mis in (3, 8):
        rs, _ = run(cuda, product, mix, caps=[len(w) - 1 for w in want], out_mis=[mis] * len(mix))
        assert rs == [0] * len(mix)
        assert_model(mix, *run(cuda, product, mix, caps=[len(w) for w in want],
                               out_mis=[mis] * len(mix)))


def test_two_streams_at_once(cuda, product):
    mix = _mix() * 4
    s1, s2 = cuda.cuda.Stream(), cuda.cuda.Stream()
    s1.wait_stream(cuda.cuda.current_stream())
    s2.wait_stream(cuda.cuda.current_stream())
    k1 = run(cuda, product, mix, stream=s1)
    k2 = run(cuda, product, mix[::-1], stream=s2)
    cuda.cuda.synchronize()
    assert_model(mix, *k1())
    assert_model(mix[::-1], *k2())


def test_strided_form_without_capacities(cuda, product):
    torch = cuda
    mix = [c for c in _mix() if len(c[1]) <= 4096]
    stride = 4096 + 48
    slot = (product.compressBound(4096) + 15) // 16 * 16
    host = bytearray(stride * len(mix))
    for i, c in enumerate(mix):
        host[stride * i:stride * i + len(c[1])] = c[1]
    src = torch.tensor(host, dtype=torch.uint8).view(len(mix), stride).cuda()
    dst = torch.full((len(mix), slot), 0xCB, dtype=torch.uint8, device="cuda")
    res = ints(torch, [-7] * len(mix))
    product.compress_batch(src, ints(torch, [len(c[1]) for c in mix]), dst, res)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    out = dst.cpu().numpy()
    assert_model(mix, rs, [out[i, :max(r, 0)].tobytes() for i, r in enumerate(rs)])


def test_host_batch(cuda, product):
    mix = _mix()
    nb = len(mix)
    keep = [buf(c[1]) for c in mix]
    caps = [product.compressBound(len(c[1])) for c in mix]
    outs = [C.create_string_buffer(cap + 16) for cap in caps]
    res = (C.c_int * nb)()
    rc = product.lib().APE_LZ4_compress_batch_host(
        (C.c_void_p * nb)(*[C.addressof(k) for k in keep]), (C.c_int * nb)(*[len(c[1]) for c in mix]),
        (C.c_void_p * nb)(*[C.addressof(o) for o in outs]), (C.c_int * nb)(*caps), res, nb)
    assert rc == 0, product.gpu_last_error()
    assert_model(mix, list(res), [outs[i].raw[:max(res[i], 0)] for i in range(nb)])


def test_large_path_up_to_one_block(cuda, product):
    """An input of at most 65536 bytes through the large-input path is the fast encoder's
    block, with acceleration too."""
    torch = cuda
    for cases in ([c for c in _mix()], [c for c in accel_cases() if c[3] == 8][:12]):
        srcs = [c[1] for c in cases]
        caps = [product.compressBound(len(s)) for s in srcs]
        src, sptr, _ = pack(torch, srcs)
        dst, dptr, doffs = alloc_out(torch, caps)
        res = ints(torch, [-7] * len(srcs))
        sizes, capt = ints(torch, map(len, srcs)), ints(torch, caps)
        scratch = product.compress_large_ptr_batch(sptr, sizes, dptr, capt, res, 65536,
                                                   acceleration=cases[0][3])
        torch.cuda.synchronize()
        rs = res.cpu().tolist()
        assert_model(cases, rs, [fetch(dst, o, r) for o, r in zip(doffs, rs)])
        del scratch


def test_destsize_with_room(cuda, product):
    """compress_destSize with a target the block fits: the fast encoder's block, all input
    consumed."""
    torch = cuda
    mix = _mix()
    want = expect(mix)
    cases, tgts = [], []
    for c, w in zip(mix, want):
        for t in (len(w), len(w) + 1, product.compressBound(len(c[1]))):
            cases.append(c)
            tgts.append(t)
    srcs = [c[1] for c in cases]
    src, sptr, _ = pack(torch, srcs)
    dst, dptr, doffs = alloc_out(torch, tgts)
    sizes, tg = ints(torch, map(len, srcs)), ints(torch, tgts)
    res = ints(torch, [-7] * len(srcs))
    product.compress_destSize_ptr_batch(sptr, sizes, dptr, tg, res)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    assert sizes.cpu().tolist() == [len(s) for s in srcs]
    assert_model(cases, rs, [fetch(dst, o, r) for o, r in zip(doffs, rs)])


def test_acceleration(cuda, product):
    for cases in by_launch(accel_cases()):
        assert_model(cases, *run(cuda, product, cases))


def test_with_prefix(cuda, product):
    cases = prefix_cases()
    assert_model(cases, *run(cuda, product, cases))
    # and with the history and the destination at odd addresses
    assert_model(cases, *run(cuda, product, cases, in_mis=[(5 * i + 1) % 16 for i in range(len(cases))],
                             out_mis=[(3 * i + 2) % 16 for i in range(len(cases))]))


def test_stream_of_chunks_in_place(cuda, product):
    """16 chunks of 8 KiB of one stream, each with all of the stream before it as its prefix,
    in one launch on the stream's own buffer (as the socket path sends them)."""
    torch = cuda
    s = _stream_bytes()
    cases = [c for c in prefix_cases() if c[0].startswith("stream chunk")]
    dev = torch.tensor(bytearray(s + bytes(64)), dtype=torch.uint8).cuda()
    sptr = torch.tensor([dev.data_ptr() + 8192 * k for k in range(16)], dtype=torch.int64,
                        device="cuda")
    caps = [product.compressBound(8192)] * 16
    dst, dptr, doffs = alloc_out(torch, caps)
    res = ints(torch, [-7] * 16)
    sizes, capt, psz = ints(torch, [8192] * 16), ints(torch, caps), ints(torch, [8192 * k for k in range(16)])
    product.compress_prefix_batch(sptr, sizes, psz, dptr, capt, res)
    torch.cuda.synchronize()
    rs = res.cpu().tolist()
    assert_model(cases, rs, [fetch(dst, o, r) for o, r in zip(doffs, rs)])


def test_benchmark_blocks(cuda, product):
    cases = bench_cases()
    assert_model(cases, *run(cuda, product, cases))
