"""A Python model of indexed LZ4 blocks (include/ape_lz4_gpu.h, "large blocks with restart
points and a seek index"): the stitch of independent streams into one block, the index built
by walking a block, and a decoder that applies the documented rules segment by segment -- the
header checks, the match floor, the segment stop and the tiling of the output.  No product or
oracle code: it pins the specification on the CPU and builds inputs for the GPU tests."""
import struct

MAGIC = 0x3158494C   # "LIX1"
ERANGE = -2 ** 31


# ---- streams as sequences ----
def parse(comp):
    """A valid LZ4 stream as [(literal bytes, offset, match length)], the last (bytes, 0, 0)."""
    seqs, ip, n = [], 0, len(comp)
    while True:
        tok = comp[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                s = comp[ip]
                ip += 1
                lit += s
                if s != 255:
                    break
        lits = bytes(comp[ip:ip + lit])
        ip += lit
        if ip == n:
            seqs.append((lits, 0, 0))
            return seqs
        off = comp[ip] | (comp[ip + 1] << 8)
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                s = comp[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        seqs.append((lits, off, ml + 4))


def _length(v):
    out = bytearray()
    if v >= 15:
        v -= 15
        out += b"\xff" * (v // 255)
        out.append(v % 255)
    return out


def emit(seqs):
    out = bytearray()
    for lits, off, ml in seqs:
        m = ml - 4 if ml else 0
        out.append((min(len(lits), 15) << 4) | min(m, 15))
        out += _length(len(lits)) + lits
        if ml:
            out += bytes([off & 255, off >> 8]) + _length(m)
    return bytes(out)


def stitch(streams):
    """The documented stitch: a stream's final literal run joins the literals of the next
    sequence that has a match; the block ends with one final run."""
    out, carry = [], b""
    for st in streams:
        for lits, off, ml in parse(st):
            if ml:
                out.append((carry + lits, off, ml))
                carry = b""
            else:
                carry += lits
    return emit(out + [(carry, 0, 0)])


def walk(block):
    """[(token position, output position of the literals, literals, offset, match length)] of a
    valid block; the final run has offset 0 and match length 0."""
    out, ip, op = [], 0, 0
    for lits, off, ml in parse(block):
        out.append((ip, op, len(lits), off, ml))
        ip += 1 + len(_length(len(lits))) + len(lits) + (2 + len(_length(ml - 4)) if ml else 0)
        op += len(lits) + ml
    assert ip == len(block)
    return out


# ---- the index ----
def build_index(block, boundaries):
    """The index of a valid block whose matches never reach across a boundary (output positions,
    the first one 0): entry j is the first sequence whose match is written at or after
    boundaries[j] -- its literals may start before -- or the final run.  Returns the words."""
    seqs = walk(block)
    n = seqs[-1][1] + seqs[-1][2]
    pairs = []
    for b in boundaries:
        hit = next((s for s in seqs if s[4] and s[1] + s[2] >= b), seqs[-1])
        pairs.append((hit[0], hit[1]))
    assert pairs[0] == (0, 0)
    pairs.append((len(block), n))
    return [MAGIC, len(boundaries), n, len(block)] + [v for p in pairs for v in p]


def trivial_index(c, n):
    """One segment: the whole block."""
    return [MAGIC, 1, n & 0xFFFFFFFF, c & 0xFFFFFFFF, 0, 0, c & 0xFFFFFFFF, n & 0xFFFFFFFF]


def index_bytes(words, stride):
    raw = struct.pack("<%dI" % len(words), *[w & 0xFFFFFFFF for w in words])
    assert len(raw) <= stride
    return raw + bytes(stride - len(raw))


# ---- the decoder ----
class _Bad(Exception):
    def __init__(self, p):
        self.p = p


def _segment(src, c, out, cap, ip, op, floor, stop):
    """decompress_safe's loop from token `ip`, output position `op`, against the block's true
    end c and capacity cap; matches no further back than `floor`.  stop: the token position at
    which the segment ends (None: at the final run).  Returns (output position, reached the
    stop); raises _Bad(position) as the reference reports it (stepping over the stop: the
    segment's first token)."""
    first = ip

    def byte(k):
        return src[k] if k < c else 0

    while True:
        if stop is not None and ip >= stop:
            if ip > stop:
                raise _Bad(first)
            return op, True
        tok = byte(ip)
        ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                s = byte(ip)
                ip += 1
                lit += s
                if not (ip < c - 15 and s == 255):
                    break
        cpy = op + lit
        if cpy > cap - 12 or ip + lit > c - 8:
            if ip + lit != c or cpy > cap:
                raise _Bad(ip)
            out[op:cpy] = src[ip:ip + lit]
            return cpy, False
        out[op:cpy] = src[ip:ip + lit]
        ip += lit
        op = cpy
        off = byte(ip) | (byte(ip + 1) << 8)
        ip += 2
        if op - off < floor:
            raise _Bad(ip)
        ml = tok & 15
        if ml == 15:
            while True:
                if ip > c - 5:
                    raise _Bad(ip)
                s = byte(ip)
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += 4
        if op + ml > cap - 5:
            raise _Bad(ip)
        if off == 0:
            out[op:op + ml] = bytes(ml)
        elif off >= ml:
            out[op:op + ml] = out[op - off:op - off + ml]
        else:
            pat = bytes(out[op - off:op])
            out[op:op + ml] = (pat * (ml // off + 1))[:ml]
        op += ml


def decode_indexed(block, words, cap, max_segments=None):
    """(result, bytes): the documented decode of `block` with the index `words`.  A positive
    result is n with its n bytes; a negative one is -1 / ERANGE from the header checks, or
    -(p)-1 with the smallest p over the failing segments."""
    c = len(block)
    w = list(words) + [0] * 8
    magic, nseg, n, wc = w[0], w[1], w[2], w[3]
    if magic != MAGIC or nseg == 0 or wc != c or n > cap:
        return -1, b""
    if max_segments is not None and nseg > max_segments:
        return ERANGE, b""
    if len(words) < 4 + 2 * (nseg + 1):
        return ERANGE, b""
    pairs = [(w[4 + 2 * j], w[5 + 2 * j]) for j in range(nseg + 1)]
    if pairs[0] != (0, 0) or pairs[-1] != (c, n):
        return -1, b""
    out = bytearray(cap)
    fails = []
    for j in range(nseg):
        (ip0, op0), (ip1, op1) = pairs[j], pairs[j + 1]
        last = j == nseg - 1
        if not (ip0 <= ip1 <= c and op0 <= op1 <= n):
            fails.append(ip0)
            continue
        if ip0 == ip1:
            if last or op0 != op1:
                fails.append(ip0)
            continue
        try:
            end, hit = _segment(block, c, out, cap, ip0, op0, op0, None if last else ip1)
        except _Bad as e:
            fails.append(e.p)
            continue
        if hit == last or end != op1:
            fails.append(ip0)
    if fails:
        return -min(fails) - 1, b""
    return n, bytes(out[:n])
