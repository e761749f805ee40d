"""A Python model of byte-range reads from indexed LZ4 blocks (include/ape_lz4_gpu.h, "byte
ranges of indexed blocks"), built on indexutil's segment decoder and written from the header's
text: the same binary search of the op column, the same test for a final literal run, the
same window and the smallest-p rule.  No product or oracle code: it pins the specification on
the CPU and judges the GPU tests."""
import random

import indexutil as X

ERANGE = X.ERANGE
INT_MAX = 0x7FFFFFFF


def lenbytes(L):
    return 0 if L < 15 else (L - 15) // 255 + 1


def find_segment(op, nseg, x):
    """The documented binary search of the op column."""
    lo, hi = 0, nseg
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if op[mid] <= x:
            lo = mid
        else:
            hi = mid
    return lo


def final_run(block, n, ip_last, op_last):
    """Where the bytes of the final literal run start when segment nseg - 1 is one final literal
    run -- the closed form and the bytes that confirm it -- else None."""
    c = len(block)
    if c <= 0 or ip_last >= c or op_last > n:
        return None
    L = n - op_last
    nb = lenbytes(L)
    if c - ip_last != 1 + nb + L:
        return None
    if block[ip_last] >> 4 != min(L, 15):
        return None
    if nb:
        lens = block[ip_last + 1:ip_last + 1 + nb]
        if lens[:-1] != b"\xff" * (nb - 1) or lens[-1] != (L - 15) % 255:
            return None
    return ip_last + 1 + nb


def _decode_segment(block, ip0, op0, stop, hi, memo):
    """One segment decoded against the output end hi: ("ok", end, reached the stop, its bytes)
    or ("bad", p).  A segment reads block[ip0:] only, and block[ip0:stop] only when it reaches
    its stop (every byte of a sequence lies before the next token), so the memo's keys are
    those bytes: a judge of many mutations of one block decodes each distinct segment once."""
    c = len(block)
    short = long = None
    if memo is not None:
        if stop is not None and ip0 <= stop <= c:
            short = (bytes(block[ip0:stop]), c, ip0, op0, hi)
            if short in memo:
                return memo[short]
        long = (bytes(block[ip0:]), c, ip0, op0, stop, hi)
        if long in memo:
            return memo[long]
    out = bytearray(max(hi, 0))
    try:
        end, hit = X._segment(block, c, out, hi, ip0, op0, op0, stop)
        got = ("ok", end, hit, bytes(out[op0:end]))
    except X._Bad as e:
        got = ("bad", e.p)
    if memo is not None:
        memo[short if got[0] == "ok" and got[2] and short is not None else long] = got
    return got


def decode_range(block, words, a, length, cap, max_segments=None, memo=None):
    """(result, (window0, need), bytes): the documented read of `length` bytes from `a` of
    `block` with the index `words` into a destination of `cap` bytes.  result > 0 comes with
    its bytes; a negative one is -1 / ERANGE from the plan (ERANGE for cap < need keeps the
    window), or -(p)-1 with the smallest p over the failing segments."""
    bad = (-1, (0, 0), b"")
    c = len(block)
    w = list(words) + [0] * 8
    magic, nseg, n, wc = w[0], w[1], w[2], w[3]
    if a < 0 or length < 0:
        return bad
    if magic != X.MAGIC or nseg == 0 or wc != c or n > INT_MAX or (nseg > 1 and c <= 0):
        return bad
    if max_segments is not None and nseg > max_segments:
        return ERANGE, (0, 0), b""
    if len(words) < 4 + 2 * (nseg + 1):
        return ERANGE, (0, 0), b""
    ip = [w[4 + 2 * j] for j in range(nseg + 1)]
    op = [w[5 + 2 * j] for j in range(nseg + 1)]
    if (ip[0], op[0]) != (0, 0) or (ip[-1], op[-1]) != (c, n):
        return bad
    if a > n:
        return bad
    m = min(length, n - a)
    if m == 0:
        return 0, (0, 0), b""
    x1 = a + m - 1
    j0, j1 = find_segment(op, nseg, a), find_segment(op, nseg, x1)
    if not (op[j0] <= a < op[j0 + 1] and op[j1] <= x1 < op[j1 + 1] and j0 <= j1):
        return bad
    lit0 = final_run(block, n, ip[j1], op[j1]) if j1 == nseg - 1 else None
    run = lit0 is not None
    lo = a if run and j0 == j1 else op[j0]
    E = a + m if run else op[j1 + 1]
    hi = E if run and j0 == j1 else min(E + 16, n)
    window = (a - lo, hi - lo)
    if cap < hi - lo:
        return ERANGE, window, b""
    out = bytearray(hi)
    fails = []
    for j in range(j0, j1 + 1):
        last = j == nseg - 1
        if last and run:
            k = max(a, op[j])
            out[k:a + m] = block[lit0 + k - op[j]:lit0 + a + m - op[j]]
            continue
        if nseg > 1:
            if not (ip[j] <= ip[j + 1] <= c and op[j] <= op[j + 1] <= n):
                fails.append(ip[j])
                continue
            if ip[j] == ip[j + 1]:
                if last or op[j] != op[j + 1]:
                    fails.append(ip[j])
                continue
            if not lo <= op[j] <= hi:
                fails.append(ip[j])
                continue
        got = _decode_segment(block, ip[j], op[j], None if last else ip[j + 1], hi, memo)
        if got[0] == "bad":
            fails.append(got[1])
            continue
        _, end, hit, data = got
        if hit == last or end != op[j + 1]:
            fails.append(ip[j])
            continue
        out[op[j]:end] = data
    if fails:
        return -min(fails) - 1, window, b""
    return m, window, bytes(out[a:a + m])


# ---- handcrafted multi-segment blocks: test_gpu_indexed.py's builder of stop-edge blocks (a copy:
# that module needs a GPU test's imports) ----
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


def has_offset0(comp):
    """A lenient walk of the token chain: True if any match offset is 0 (the decoders then copy
    bytes of dst that nobody wrote, so only the result's value is comparable)."""
    ip, n = 0, len(comp)
    while ip < n:
        tok = comp[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            while ip < n:
                s = comp[ip]
                ip += 1
                lit += s
                if s != 255:
                    break
        ip += lit
        if ip + 2 > n:
            return False
        if comp[ip] == 0 and comp[ip + 1] == 0:
            return True
        ip += 2
        if tok & 15 == 15:
            while ip < n:
                s = comp[ip]
                ip += 1
                if s != 255:
                    break
    return False
