"""GPU compress_destSize (lz4_destsize_kernel behind APE_LZ4_compress_destSize_batch_dev and
its _scratch form) against tests/encmodel.py: result, consumed size and bytes.

encmodel.dest_size states the cut of a block that does not fit its target: the first k
sequences and the longest final literal run that fits, for the k that consumes the most, a cut
being legal when that run has the literals the last match needs.  Here every target from 1 to
the block's size + 1 of a few small inputs (text, dense short matches, literal runs around the
lengths where the run's header grows, matches shorter than 7 bytes), and on three 64 KiB inputs
and a 5 KiB text the targets around every refill of the kernel's 2048-byte window over the block.

The case lists are plain functions, so that tests/test_cdict_destsize_model.py (CPU) can show
that these inputs tell the model from its wrong neighbours."""
import functools
import random

import pytest

import encmodel
from gpuutil import alloc_out, ints, pack
from lz4util import I

pytestmark = pytest.mark.gpu

WINDOW = 2048     # the kernel's window over the block, refilled from a 16-byte boundary


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


# ---------------- the inputs (no GPU needed to build them) ----------------
def _dense(n, seed):
    """Copies of 4..9 bytes from anywhere before, 0..3 fresh bytes between them."""
    rng = random.Random(seed)
    out = bytearray(rng.randbytes(40))
    while len(out) < n:
        at = rng.randrange(len(out) - 9)
        out += out[at:at + rng.randrange(4, 10)]
        out += rng.randbytes(rng.randrange(4))
    return bytes(out[:n])


def _runs(lens, seed):
    """Literal runs of the given lengths (the first of 100 bytes or more), between them 8-byte
    strings out of the first run, each another (a match of 8 each)."""
    first = _rand(seed, lens[0])
    out = bytearray(first)
    for i, ln in enumerate(lens[1:]):
        out += first[8 * i + 8:8 * i + 16] + _rand(seed + 1 + i, ln)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def short_match(ml, back=0):
    """An input whose parse holds a match of ml + back < 7 bytes (after 70 literals: with the
    second length byte the sequence's 4 bytes of header are a match of 4's whole gain).  The
    table's key covers 7 bytes, so this takes two 7-byte strings that share ml bytes and no
    more, and their slot; the second lies in the chunk after the first's.  (ml = 6 does not
    exist: the key's last byte alone moves the hash by more than a slot.  `back` equal bytes
    before the two strings make the 6.)"""
    rng = random.Random(400 + ml)
    for _ in range(200):
        a = rng.randbytes(7)
        for _ in range(4000):
            b = a[:ml] + bytes([a[ml] ^ rng.randrange(1, 256)]) + rng.randbytes(6 - ml)
            if encmodel.hashk(a, 0) == encmodel.hashk(b, 0):
                x = _rand(409, back)
                src = _rand(410, 40 - back) + x + a + _rand(411, 23 - back) + x + b + _rand(412, 150)
                if any(s[1] == ml + back for s in encmodel.parse(src)):
                    return src
    raise AssertionError("no colliding pair")


def small_inputs():
    return [("text", I.text(900, 3)),
            ("dense", _dense(700, 21)),
            ("runs", _runs([524, 14, 15, 16, 269, 270, 271, 271, 30], 31)),
            ("match of 4", short_match(4)),
            ("match of 5", short_match(5)),
            ("match of 6", short_match(5, back=1))]


def _long_fields(n, seed, lead):
    """`lead` literals, then literal runs and matches of 3..40 and of 280..600 bytes in turn:
    fields of one, two and three length bytes all along the block, each one byte further on
    in it with each byte of lead."""
    rng = random.Random(seed)
    out = bytearray(_rand(seed + 1, lead))
    while len(out) < n:
        out += rng.randbytes(rng.choice([rng.randrange(3, 40), rng.randrange(280, 600)]))
        ln = rng.choice([rng.randrange(4, 40), rng.randrange(280, 600)])
        at = rng.randrange(len(out) - ln)
        out += out[at:at + ln]
    return bytes(out[:n])


def large_inputs():
    """Blocks of 19 KB and 33 KB (9 and 15 refills), and what they do not hold: the leads that
    put a literal length's and a match length's second byte first past the first window, and a
    text whose walk finds an offset there."""
    return [("App. C 64 KiB", I.synth_comp(65536, 3)),
            ("long fields 64 KiB, lead 983", _long_fields(65536, 51, 983)),
            ("long fields 64 KiB, lead 986", _long_fields(65536, 51, 986)),
            ("text 5 KiB", I.text(5000, 8))]


@functools.lru_cache(maxsize=None)
def parsed(src):
    seqs = encmodel.parse(src)
    return seqs, encmodel.emit(src, seqs)


def refills(block):
    """The kernel's walk over a block, restated for its window only: [(i, kind, w0)] per
    refill -- the byte i whose read refills the window (from i rounded down to 16), what that
    byte is ("token", or "literal length" / "match length" with the number of that field's
    bytes read before it) and the start of the window left behind."""
    ev, w = [], None
    op, n = 0, len(block)

    def read(i, kind):
        nonlocal w
        if w is None or i - w >= WINDOW:
            ev.append((i, kind, w))
            w = i & ~15
        return block[i]

    while op < n:
        tok = read(op, ("token", 0))
        op += 1
        lit = tok >> 4
        if lit == 15:
            k = 0
            while True:
                s = read(op, ("literal length", k))
                op, k, lit = op + 1, k + 1, lit + s
                if s != 255:
                    break
        op += lit
        if op + 2 > n:
            break
        op += 2
        if tok & 15 == 15:
            k = 0
            while True:
                s = read(op, ("match length", k))
                op, k = op + 1, k + 1
                if s != 255:
                    break
    return ev[1:]


def refill_kinds(block):
    """What the refills of a block's walk meet: a token first in the new window; a length field
    lying across the old window's end (its first bytes read from the old one); an offset lying
    across it (skipped, the next read refills); the refilling byte not on a 16-byte boundary."""
    kinds = set()
    for i, (what, k), w0 in refills(block):
        if what == "token":
            kinds.add("token")
        elif k >= 1:
            kinds.add(what + " run")
        # (the two bytes before a token or a match length's first byte are an offset)
        if (what == "token" or (what == "match length" and k == 0)) and i - 1 == w0 + WINDOW:
            kinds.add("offset")
        if i % 16:
            kinds.add("inside 16")
    return kinds


def small_cases():
    """(name, src, target): every target from 1 to the block's size + 1, and 0 and -1."""
    cs = []
    for name, src in small_inputs():
        c = len(parsed(src)[1])
        cs += [("%s -> %d" % (name, t), src, t) for t in range(-1, c + 2)]
    return cs


def large_cases():
    """Targets around every refill of the walk (the walk goes on while the target has room),
    around the window's size, and just below the block's."""
    cs = []
    for name, src in large_inputs():
        blk = parsed(src)[1]
        c = len(blk)
        ts = {WINDOW - 1, WINDOW, WINDOW + 1, WINDOW + 17, 2 * WINDOW, 2 * WINDOW + 1, c // 2, c - 300,
              c - 2, c - 1, c, c + 1}
        for i, _, _ in refills(blk):
            ts |= {i - 1, i, i + 1, i + 2, i + 3, i + 8, i + 20}
        cs += [("%s -> %d" % (name, t), src, t) for t in sorted(ts) if 0 < t <= c + 1]
    return cs


def all_cases():
    return small_cases() + large_cases()


@functools.lru_cache(maxsize=None)
def model(src, target):
    return encmodel.dest_size(src, target, seqs=parsed(src)[0])


# ---------------- running the kernel ----------------
def run(torch, amd, cases, scratch_blocks=None):
    """[(result, consumed, bytes)] of one call; scratch_blocks: through the _scratch form with
    scratch for that many blocks."""
    srcs = list(dict.fromkeys(c[1] for c in cases))
    src, sptr, _ = pack(torch, srcs, misalign=[(5 * i + 1) % 16 for i in range(len(srcs))])
    at = {s: i for i, s in enumerate(srcs)}
    sptr = sptr[torch.tensor([at[c[1]] for c in cases], device="cuda")].contiguous()
    tgts = [c[2] for c in cases]
    dst, dptr, doffs = alloc_out(torch, [max(t, 0) for t in tgts],
                                 misalign=[(3 * i) % 16 for i in range(len(cases))], extra=16)
    sizes, tg = ints(torch, [len(c[1]) for c in cases]), ints(torch, tgts)
    res = ints(torch, [-7] * len(cases))
    if scratch_blocks is None:
        amd.compress_destSize_ptr_batch(sptr, sizes, dptr, tg, res)
    else:
        scr = torch.empty(amd.destSize_scratch_size(scratch_blocks), dtype=torch.uint8, device="cuda")
        amd.compress_destSize_scratch_ptr_batch(sptr, sizes, dptr, tg, res, scr)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    rs, ks = res.cpu().tolist(), sizes.cpu().tolist()
    return [(r, k, host[o:o + max(r, 0)].tobytes()) for r, k, o in zip(rs, ks, doffs)]


def assert_model(cases, got):
    for c, (r, k, comp) in zip(cases, got):
        wr, wk, want = model(c[1], c[2])
        assert (r, k) == (wr, wk), (c[0], (r, k), (wr, wk))
        assert comp == want, (c[0], next(i for i in range(r) if comp[i] != want[i]))


# ---------------- the tests ----------------
def test_every_target_of_small_inputs(cuda, product):
    cases = small_cases()
    assert_model(cases, run(cuda, product, cases))


def test_targets_around_the_window_refills(cuda, product):
    cases = large_cases()
    assert_model(cases, run(cuda, product, cases))


def test_scratch_form_with_one_block_of_scratch(cuda, product):
    cases = all_cases()
    assert_model(cases, run(cuda, product, cases, scratch_blocks=1))
