"""LZ4 blocks written from sequence lists, the plain decoder, and the copy-phase corpus.

build() writes a block token by token from (literal bytes, offset, match length) triples and
returns it with the output the byte-at-a-time definition gives (out.append(out[-off]); offset 0
appends a zero byte).  That output is the reference for BYTES in
tests/test_gpu_decode_copy.py; the oracle stays the reference for return values.

The corpus (grid, edges, slides, chains, dictionary, multi-batch, flush edges) aims every class
of the decoder's copy scheduler (lz4_decode.hip copy_segment / coop_match / lane_match) at the
offsets, lengths and window positions where its arithmetic changes; tests/deccopyclass.py says
which class a sequence takes and tests/test_dec_copy_classes.py proves what the corpus reaches.
Literals are random bytes, and a fresh random run of at least FRESH bytes precedes every probe
whose offset is below FRESH, so a wrongly sourced byte differs with probability 255/256.
"""
import functools
import random

import deccopyclass as K

FRESH = 80
TAIL = 16            # final literals: keeps every match clear of the block-end rules


def _ext(c, v):
    while v >= 255:
        c.append(255)
        v -= 255
    c.append(v)


def build(seqs, tail, history=b"", strict=True):
    """(compressed, expected output).  seqs: (literal bytes, offset, match length >= 4).
    strict=False: an offset past the history is allowed; the expected output is then None."""
    c, out, h = bytearray(), bytearray(history), len(history)
    for lits, off, ml in seqs:
        assert ml >= 4 and 0 <= off <= 65535
        c.append((min(len(lits), 15) << 4) | min(ml - 4, 15))
        if len(lits) >= 15:
            _ext(c, len(lits) - 15)
        c += lits
        c += off.to_bytes(2, "little")
        if ml - 4 >= 15:
            _ext(c, ml - 4 - 15)
        if out is None:
            continue
        out += lits
        if off > len(out):
            assert not strict, (off, len(out))
            out = None
            continue
        for _ in range(ml):
            out.append(out[-off] if off else 0)
    c.append(min(len(tail), 15) << 4)
    if len(tail) >= 15:
        _ext(c, len(tail) - 15)
    c += tail
    if out is not None:
        out += tail
    return bytes(c), (None if out is None else bytes(out[h:]))


def layout(seqs, tail):
    """Per sequence (o, m, me): literals at output [o, m), match [m, me); then the tail's (o, m, m)."""
    pos, lay = 0, []
    for lits, _, ml in seqs:
        lay.append((pos, pos + len(lits), pos + len(lits) + ml))
        pos += len(lits) + ml
    lay.append((pos, pos + len(tail), pos + len(tail)))
    return lay


class Block:
    """One corpus block.  probes: indices into seqs of the sequences the block is about."""
    __slots__ = ("part", "seqs", "tail", "hist", "comp", "out", "probes", "note")

    def __init__(self, part, seqs, tail, probes, hist=b"", note="", strict=True):
        self.part, self.seqs, self.tail, self.hist = part, seqs, tail, hist
        self.probes, self.note = probes, note
        self.comp, self.out = build(seqs, tail, hist[-65536:], strict)

    @property
    def size(self):
        return sum(len(s[0]) + s[2] for s in self.seqs) + len(self.tail)

    def single_batch(self):
        return K.single_batch(len(self.seqs) + 1, len(self.comp))

    def describe(self, dict_mode=False, da=0):
        """The probes as (off, n, position) with their classes: for failure messages."""
        lay = layout(self.seqs, self.tail)
        txt = ["%s %s" % (self.part, self.note)]
        cls = {}
        if self.single_batch():
            for p in K.classify(self.seqs, self.tail, len(self.hist) if dict_mode else None, da):
                cls.setdefault(p.seq, []).append(p.label())
        for i in self.probes:
            txt.append("probe(off=%d, n=%d, at=%d)%s" % (
                self.seqs[i][1], self.seqs[i][2], lay[i][1],
                " " + "+".join(cls[i]) if i in cls else ""))
        return "; ".join(txt)


# ------------------------------------------------------------------ corpus
GRID_OFFS = list(range(1, FRESH + 1))
GRID_LENS = list(range(4, 141))
EXT_OFFS = GRID_OFFS + [255, 256, 257]
EXT_LENS = [18, 19, 20, 273, 274, 275, 528, 529, 530]


def _pack_probes(part, rng, probes, max_out, front=(), note=""):
    """Blocks of up to 20 probes (off, n), each after fresh literals, while the output stays
    within max_out and the block a single batch."""
    blocks, seqs, size, csz = [], list(front), 0, 0
    fsz = sum(len(s[0]) + s[2] for s in front)

    def close():
        nonlocal seqs, size, csz
        if len(seqs) > len(front):
            blocks.append(Block(part, seqs, rng.randbytes(TAIL), list(range(len(front), len(seqs))),
                                note=note))
        seqs, size, csz = list(front), 0, 0

    for off, n in probes:
        lit = FRESH if off <= fsz + size + FRESH else off
        if (len(seqs) - len(front) >= 20 or size + lit + n + TAIL > max_out or
                (not front and csz + lit + 8 + TAIL + 4 > K.CONST["kStage"] - K.CONST["kWinNeed"])):
            close()
            lit = FRESH if off <= fsz + FRESH else off
        seqs.append((rng.randbytes(lit), off, n))
        size += lit + n
        csz += lit + 8
    close()
    return blocks


@functools.lru_cache(None)
def grid():
    """(a) every off 1..80 x n 4..140, and the extension-byte lengths, window base 0."""
    rng = random.Random(1001)
    probes = [(off, n) for n in GRID_LENS for off in GRID_OFFS]
    probes += [(off, n) for n in EXT_LENS for off in EXT_OFFS]
    return _pack_probes("grid", rng, probes, K.CONST["kWinB"])


# boundary pairs of the grid: one per lane-path disjunct and per whole-wave reason
EDGE_PROBES = [(0, 20), (0, 100), (1, 4), (1, 40), (7, 70), (8, 12), (15, 16), (15, 64), (16, 17),
               (16, 64), (17, 33), (31, 64), (32, 65), (33, 49), (40, 140), (63, 64), (63, 130),
               (64, 65), (65, 64), (65, 140), (200, 15), (200, 16), (300, 48)]
FILL_PERIOD = 211    # the filler's period: no probe offset, no multiple of 16


def _filler(rng, upto, cut=None):
    """Random literals expanded by matches of offset FILL_PERIOD to `upto` output bytes."""
    assert upto >= FILL_PERIOD + 4
    seqs, n = [], upto - FILL_PERIOD
    first = cut if cut and 4 <= cut <= n - 4 else n
    seqs.append((rng.randbytes(FILL_PERIOD), FILL_PERIOD, first))
    if first < n:
        seqs.append((b"", FILL_PERIOD, n - first))
    return seqs


def _placed(part, rng, off, n, at, hist=b"", note=""):
    """One probe (off, n) whose match starts at output position `at`, behind a filler."""
    lit = FRESH
    seqs = _filler(rng, at - lit, rng.choice((None, 70, 300))) + [(rng.randbytes(lit), off, n)]
    return Block(part, seqs, rng.randbytes(TAIL), [len(seqs) - 1], hist, note)


def edge_positions(which):
    e1 = K.CONST["kWinB"]
    e = e1 if which == 1 else list(K.segments(3 * e1, 0))[1][1]
    return e, range(e - 80, e + 81)


@functools.lru_cache(None)
def edges(which):
    """(b) the probe list at every position 80 below to 80 above segment edge 1 or 2."""
    rng = random.Random(2000 + which)
    e, pos = edge_positions(which)
    return [_placed("edge%d" % which, rng, off, n, at, note="edge=%d" % e)
            for off, n in EDGE_PROBES for at in pos]


SLIDE_LENS = (4, 15, 16, 17, 33, 64, 65, 100)


@functools.lru_cache(None)
def slides():
    """(b) after two slides: every relation of the source to the window base and to the
    drained history, offsets up to 4096."""
    rng = random.Random(2003)
    segs = list(K.segments(3 * K.CONST["kWinB"], 0))
    s0, _, base, gdone = segs[2]
    at = max(s0 + 616, 4096 + 8)
    assert at + 200 < segs[2][1]
    blocks = []
    for n in SLIDE_LENS:
        offs = set(range(at - base - n - 2, at - base + 3))
        offs |= set(range(at - gdone - 2, at - gdone + n + 3))
        offs |= set(range(at - base + 2, 4097, 16))
        for off in sorted(o for o in offs if 0 < o <= at and o % FILL_PERIOD):
            blocks.append(_placed("slide", rng, off, n, at, note="base=%d gdone=%d" % (base, gdone)))
    # a long match cut by the next edge whose source straddles the window base
    at = segs[2][1] - 100
    for off in range(at - base + 1, at - base + 100, 2):
        if off % FILL_PERIOD:
            blocks.append(_placed("slide", rng, off, 200, at, note="base=%d gdone=%d" % (base, gdone)))
    return blocks


@functools.lru_cache(None)
def chains():
    """(c) dependent passes: sequence k+1's source is sequence k's match, depths 1..20; with a
    whole-wave item in the middle; with a source spanning three earlier sequences; with
    self-overlapping members; at base 0 and across the first segment edge."""
    blocks = []
    e1 = K.CONST["kWinB"]
    for depth in range(1, 21):
        for variant in ("lane", "wave-long", "wave-off", "span3", "overlap"):
            for rep in range(4):
                rng = random.Random(3000 + 100 * depth + 10 * rep + len(variant))
                front = 100 if rep < 2 else e1 - rng.randrange(40, 40 + 12 * depth)
                seqs = [] if front == 100 else _filler(rng, front - 100)
                pos = front
                seqs.append((rng.randbytes(100), 30, 8))
                pm, pn = pos, 8
                pos += 8
                probes = []
                for k in range(depth):
                    lit = rng.choice((0, 0, 1, 3))
                    ma = pos + lit
                    mid = k == depth // 2
                    if variant == "span3" and mid:
                        # three short sequences, then one match whose source covers all three
                        for _ in range(3):
                            seqs.append((rng.randbytes(1), rng.randrange(20, 90), 5))
                        ma = pos + 18 + lit
                        ps, n = pos - 2, 22
                        pos += 18
                    elif variant == "wave-long" and mid:
                        ps, n = rng.randrange(pm, pm + pn), rng.randrange(65, 120)
                        if ma - ps < 64:
                            ps = ma - 64 - rng.randrange(0, 8)
                    elif variant == "wave-off" and mid:
                        ps, n = ma - rng.randrange(1, 16), rng.randrange(16, 50)
                    elif variant == "overlap" and k % 2:
                        ps = min(rng.randrange(pm, pm + pn), ma - 16)
                        n = min(64, ma - ps + rng.randrange(1, 20))
                    else:
                        ps = min(rng.randrange(pm, pm + pn), ma - 4)
                        n = rng.randrange(4, min(64, ma - ps) + 1)
                    seqs.append((rng.randbytes(lit), ma - ps, n))
                    probes.append(len(seqs) - 1)
                    pm, pn, pos = ma, n, ma + n
                blocks.append(Block("chain", seqs, rng.randbytes(TAIL), probes,
                                    note="%s depth=%d front=%d" % (variant, depth, front)))
    return blocks


DICT_SIZES = (1, 15, 16, 17, 100, 65535, 65536, 70000)
DICT_LENS = (4, 15, 16, 17, 40, 64, 65, 130)


@functools.lru_cache(None)
def dictionary():
    """(d) sources wholly inside the dictionary with >= 16 bytes to its end, ending exactly at
    its end, in its last 1..15 bytes, straddling its end (also self-overlapping), starting at
    its first byte; behind a filler too, so the probe meets the first segment edge.
    Returns (valid blocks, blocks whose probe offset is one past what is allowed)."""
    rng = random.Random(4001)
    good, bad = [], []
    e1 = K.CONST["kWinB"]
    for D in DICT_SIZES:
        hist = rng.randbytes(D)
        de = min(D, 65536)
        # (at < FRESH: the fresh run is the dictionary's end and `at` literals, so that offsets
        # below 64 reach into the dictionary)
        for at in (4, 20, 40, FRESH, 333, e1 - 10, e1 + 40):
            for n in DICT_LENS:
                # first byte; >= 16 bytes to the end; ending at it; straddling it; its last bytes
                starts = {-de, -de + 1, -n - 17, -n - 16, -n - 15, -n - 1, -n, -n + 1, -n // 2,
                          -17, -16, -15, -8, -2, -1}
                for ps in sorted(starts):
                    off = at - ps
                    if not (-de <= ps < 0 and off <= 65535):
                        continue
                    if at <= FRESH:
                        seqs = [(rng.randbytes(at), off, n)]
                    else:
                        seqs = _filler(rng, at - FRESH) + [(rng.randbytes(FRESH), off, n)]
                    good.append(Block("dict", seqs, rng.randbytes(TAIL), [len(seqs) - 1], hist,
                                      note="dict=%d ps=%d" % (D, ps)))
            if at + de + 1 <= 65535:
                seqs = ([] if at <= FRESH else _filler(rng, at - FRESH))
                seqs = seqs + [(rng.randbytes(min(at, FRESH)), at + de + 1, 8)]
                bad.append(Block("dict-bad", seqs, rng.randbytes(TAIL), [len(seqs) - 1], hist,
                                 note="dict=%d one past" % D, strict=False))
    return good, bad


def _short_front(rng, nseq):
    """nseq short sequences (1-3 literals, a 4..8-byte match) over 40 random bytes."""
    seqs, size = [(rng.randbytes(40), 17, 4)], 44
    for _ in range(nseq - 1):
        lit, n = rng.randrange(1, 4), rng.randrange(4, 9)
        seqs.append((rng.randbytes(lit), rng.randrange(1, min(size + lit, 4000) + 1), n))
        size += lit + n
    return seqs


@functools.lru_cache(None)
def multibatch(kind):
    """(e) the grid's probes behind 64..200 short sequences ('short': several copy batches,
    descriptors carried over) or behind more than kStage compressed bytes ('restage')."""
    rng = random.Random(5001 + len(kind))
    probes = [(off, n) for n in GRID_LENS for off in GRID_OFFS]
    probes += [(off, n) for n in EXT_LENS for off in EXT_OFFS]
    blocks = []
    for k in range(0, len(probes), 20):
        if kind == "short":
            front = _short_front(rng, rng.randrange(64, 201))
        else:
            front = [(rng.randbytes(rng.randrange(200, 300)), rng.randrange(1, 200), rng.randrange(4, 40))
                     for _ in range(rng.randrange(10, 14))]
        blocks += _pack_probes("multi-" + kind, rng, probes[k:k + 20], 1 << 30, tuple(front))
    return blocks


@functools.lru_cache(None)
def flush_edges():
    """(f) single-literal and literal+match blocks of output sizes 1..80 and kWinB -+ 20; the
    test runs each at all 16 dst misalignments.  Returns [(block, out_mis)]."""
    rng = random.Random(6001)
    e1 = K.CONST["kWinB"]
    out = []
    for size in list(range(1, 81)) + list(range(e1 - 20, e1 + 21)):
        for mis in range(16):
            out.append((Block("flush", [], rng.randbytes(size), [], note="literal size=%d mis=%d" % (size, mis)), mis))
            if size >= 1 + 4 + 12:
                lit = min(size - 4 - 12, 200)
                n = size - 12 - lit
                seqs = [(rng.randbytes(lit), rng.randrange(1, lit + 1), n)]
                out.append((Block("flush", seqs, rng.randbytes(12), [0],
                                  note="match size=%d mis=%d" % (size, mis)), mis))
    return out


def dense_replay():
    """The blocks of tests/test_gpu_decode.py::test_dense_sequences_vs_oracle (its seed, its
    mix) as sequence lists: [(block, decoded whole there?)] -- the others it mutates or cuts."""
    from lz4util import walk_ok
    from test_gpu_decode import _dense_block
    rng = random.Random(77)
    blocks = []
    for k in range(240):
        mix = [(0.0, 0.0, 0.0), (0.02, 0.01, 0.05), (0.1, 0.05, 0.2)][k % 3]
        c, out = _dense_block(rng, rng.choice((3, 40, 400, 1500)), *mix)
        # the draws the test makes between two blocks, in its order (value before index)
        if k % 4 == 1:
            for _ in range(rng.randrange(1, 4)):
                rng.randrange(256), rng.randrange(len(c))
        elif k % 4 == 2:
            rng.randrange(1, len(c) + 1)
        rng.choice((1, 2, 3, 4))
        rng.randrange(0, len(out) + 8)
        seqs, pos = [], 0
        for lit, off, ml in walk_ok(c):
            seqs.append((out[pos:pos + lit], off, ml))
            pos += lit + ml
        tail = seqs.pop()[0]
        b = Block("dense", seqs, tail, [], note="k=%d" % k)
        assert b.comp == c and b.out == out
        blocks.append((b, k % 4 in (0, 3)))
    return blocks
