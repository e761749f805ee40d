"""A Python model of the fast encoder (APE_LZ4_compress_batch_dev, _fast_batch_dev and
_withPrefix_batch_dev; DESIGN.md 3.1, "The parse as a function").  The GPU's output is a pure
function of (input bytes, used prefix, acceleration), and this file is its definition.  No
product or oracle code.

candidates_plain() and walk_plain() state the rule position by position; candidates() and
walk() are the same rule with the table resolved for all positions at once (numpy) and the
walk jumping from match to match, fast enough for the 64 KiB blocks of the GPU tests.
tests/test_enc_model.py holds the two against each other.

RULE holds the rule's constants.  The tests build wrong models from it (RULE._replace) to show
that their inputs tell each constant from its neighbour; the product has one rule, RULE."""
import collections

import numpy as np

HSIZE = 7328          # table entries (kHSize, lz4_gpu_internal.h)
CHUNK = 64            # positions that look the table up together
MAX_BLOCK = 65536
MINLENGTH = 13        # a shorter input is one literal run
MFLIMIT = 12          # a match starts at p <= N - 12 ...
LASTLITERALS = 5      # ... and ends at or before N - 5
MAX_ACCEL = 1 << 20
ERANGE = -2147483647 - 1   # APE_LZ4_GPU_ERANGE

Rule = collections.namedtuple("Rule", [
    "back",           # bytes of backward extension measured with the match
    "own_chunk",      # a position sees the earlier positions of its own chunk
    "insert_room",    # p enters the table when p + insert_room <= N
    "min_cand",       # candidates below this position are no candidates
    "fwd_cap",        # forward length cap (None: the full common length)
    "prefix_stride",  # every prefix_stride-th position of the prefix is hashed
    "prefix_round",   # the used prefix is a multiple of this (and at least this)
    "regime",         # probes per gap size (acceleration > 1)
    "acc_more",       # further bytes of backward extension (acceleration > 1)
])
RULE = Rule(back=4, own_chunk=False, insert_room=5, min_cand=4, fwd_cap=None, prefix_stride=3,
            prefix_round=64, regime=64, acc_more=16)


def used_prefix(n, prefix_len, rule=RULE):
    """D: the bytes of history the encoder uses for an n-byte input."""
    d = max(min(prefix_len, MAX_BLOCK - n), 0)
    d -= d % rule.prefix_round
    return d if d >= rule.prefix_round else 0


def window(src, prefix=b"", rule=RULE):
    """(w, D): the D used bytes of history followed by the input."""
    src, prefix = bytes(src), bytes(prefix)
    d = used_prefix(len(src), len(prefix), rule)
    return prefix[len(prefix) - d:] + src, d


def hashk(w, p):
    """The table slot of the 7 bytes at p (bytes past the window's end read as 0)."""
    b = w[p:p + 7] + bytes(7)
    v = (int.from_bytes(b[0:3], "little") * 0x9E3779 + int.from_bytes(b[3:6], "little") * 0xC2B2AE +
         b[6] * 0x27D4EB) & 0xFFFFFFFF
    return (v * HSIZE) >> 32


def _prefix_positions(N, D, rule):
    return [v for v in range(0, D, rule.prefix_stride) if v + 8 <= N]


def candidates_plain(w, D, rule=RULE):
    """cand[p] for every window position (0 below D): what the table holds under p's hash when
    p's chunk looks it up.  One position at a time, with the table itself."""
    N = len(w)
    tab = [0] * HSIZE
    cand = [0] * N
    for v in _prefix_positions(N, D, rule):
        tab[hashk(w, v)] = v
    for lo in range(D - D % CHUNK, N, CHUNK):
        ps = range(max(lo, D), min(lo + CHUNK, N))
        if rule.own_chunk:
            for p in ps:
                h = hashk(w, p)
                cand[p] = tab[h]
                if p + rule.insert_room <= N:
                    tab[h] = p
            continue
        for p in ps:                        # every position reads ...
            cand[p] = tab[hashk(w, p)]
        for p in ps:                        # ... then every hashable position is written
            if p + rule.insert_room <= N:
                tab[hashk(w, p)] = p
    return cand


def candidates(w, D, rule=RULE):
    """candidates_plain for all positions at once: the latest position written under the same
    slot before p's chunk (before p, for own_chunk)."""
    N = len(w)
    if N == 0:
        return []
    a = np.zeros(N + 8, np.uint64)
    a[:N] = np.frombuffer(w, np.uint8)
    lo3 = a[0:N] | (a[1:N + 1] << np.uint64(8)) | (a[2:N + 2] << np.uint64(16))
    hi3 = a[3:N + 3] | (a[4:N + 4] << np.uint64(8)) | (a[5:N + 5] << np.uint64(16))
    v = (lo3 * np.uint64(0x9E3779) + hi3 * np.uint64(0xC2B2AE) + a[6:N + 6] * np.uint64(0x27D4EB)) \
        & np.uint64(0xFFFFFFFF)
    h = ((v * np.uint64(HSIZE)) >> np.uint64(32)).astype(np.int64)
    pos = np.arange(N, dtype=np.int64)
    written = np.concatenate([np.array(_prefix_positions(N, D, rule), np.int64),
                              pos[(pos >= D) & (pos + rule.insert_room <= N)]])
    if written.size == 0:
        return [0] * N
    keys = np.sort(h[written] * (1 << 20) + written)   # (prefix positions lie below D: position
    #                                                     order is the order of the writes)
    # writes below `seen` are visible (every prefix position to the block's first chunk)
    seen = pos if rule.own_chunk else np.maximum(pos - pos % CHUNK, D)
    at = np.searchsorted(keys, h * (1 << 20) + seen) - 1
    hit = keys[np.maximum(at, 0)]
    cand = np.where((at >= 0) & ((hit >> 20) == h), hit & ((1 << 20) - 1), 0)
    cand[:D] = 0
    return cand.tolist()


def has_match(w, cand, p, rule=RULE):
    N, c = len(w), cand[p]
    return 1 <= p <= N - MFLIMIT and rule.min_cand <= c < p and w[c:c + 4] == w[p:p + 4]


def forward(w, c, p, rule=RULE):
    """Bytes equal from (c, p) on, at most up to the match limit N - 5."""
    mx = len(w) - LASTLITERALS - p
    if rule.fwd_cap is not None:
        mx = min(mx, rule.fwd_cap)
    L, step = 0, 32
    while L < mx:                           # (in growing pieces: most matches are short)
        k = min(step, mx - L)
        a, b = w[p + L:p + L + k], w[c + L:c + L + k]
        if a != b:
            x = int.from_bytes(a, "little") ^ int.from_bytes(b, "little")
            return L + (((x & -x).bit_length() - 1) >> 3)
        L += k
        step *= 2
    return mx


def backward(w, c, p, room, accel, rule=RULE):
    """Bytes equal before (c, p): at most `back`, the candidate's position and the pending
    literals (room).  With acceleration a run of `back` goes on for up to acc_more bytes."""
    lim = min(rule.back, c, room)
    b = 0
    while b < lim and w[p - 1 - b] == w[c - 1 - b]:
        b += 1
    if accel > 1 and b == rule.back:
        lim = min(rule.back + rule.acc_more, c, room)
        while b < lim and w[p - 1 - b] == w[c - 1 - b]:
            b += 1
    return b


def probes(e, accel, last, rule=RULE):
    """The positions compress_fast's search visits after a match end e, up to `last`."""
    for p in (e, e + 1, e + 2):
        if p > last:
            return
        yield p
    p, gap = e + 2, accel
    while True:
        for _ in range(rule.regime):
            p += gap
            if p > last:
                return
            yield p
        gap += 1


def _take(w, cand, p, e, accel, rule):
    c = cand[p]
    L = forward(w, c, p, rule)
    b = backward(w, c, p, p - e, accel, rule)
    return (p - b - e, L + b, p - c), p + L


def walk_plain(w, D, cand, accel=1, rule=RULE):
    """The greedy walk, one position (or probe) at a time: [(literals, match length, offset)]."""
    N = len(w)
    seqs, e = [], D
    if N - D < MINLENGTH:
        return seqs
    accel = min(accel, MAX_ACCEL)
    last = N - MFLIMIT
    while True:
        visit = range(e, last + 1) if accel <= 1 else probes(e, accel, last, rule)
        for p in visit:
            if has_match(w, cand, p, rule):
                break
        else:
            return seqs
        s, e = _take(w, cand, p, e, accel, rule)
        seqs.append(s)


def walk(w, D, cand, accel=1, rule=RULE):
    """walk_plain over the positions that have a match only."""
    N = len(w)
    seqs, e = [], D
    if N - D < MINLENGTH:
        return seqs
    accel = min(accel, MAX_ACCEL)
    last = N - MFLIMIT
    a = np.frombuffer(w, np.uint8).astype(np.uint32)
    w4 = a[:N - 3] | (a[1:N - 2] << 8) | (a[2:N - 1] << 16) | (a[3:N] << 24)
    c = np.asarray(cand, np.int64)[:last + 1]
    p = np.arange(last + 1, dtype=np.int64)
    ok = (p >= max(D, 1)) & (c >= rule.min_cand) & (c < p)
    ok &= w4[np.where(ok, c, 0)] == w4[:last + 1]
    if accel <= 1:
        at = np.nonzero(ok)[0].tolist()
        i = 0
        while True:
            while i < len(at) and at[i] < e:
                i += 1
            if i == len(at):
                return seqs
            s, e = _take(w, cand, at[i], e, accel, rule)
            seqs.append(s)
    ok = ok.tolist()
    while True:
        for q in probes(e, accel, last, rule):
            if ok[q]:
                break
        else:
            return seqs
        s, e = _take(w, cand, q, e, accel, rule)
        seqs.append(s)


def parse(src, prefix=b"", acceleration=1, plain=False, rule=RULE):
    """The sequence list [(literals, match length, offset)] of (src, prefix, acceleration)."""
    w, D = window(src, prefix, rule)
    if plain:
        return walk_plain(w, D, candidates_plain(w, D, rule), acceleration, rule)
    return walk(w, D, candidates(w, D, rule), acceleration, rule)


def _length_bytes(v):
    """The bytes after the token for a length field whose value is v (>= 15)."""
    v -= 15
    return b"\xff" * (v // 255) + bytes([v % 255])


def emit(src, seqs):
    """The LZ4 block of a sequence list: the standard encoding, then the final literal run."""
    src = bytes(src)
    out = bytearray()
    at = 0
    for lits, mlen, off in seqs:
        out.append((min(lits, 15) << 4) | min(mlen - 4, 15))
        if lits >= 15:
            out += _length_bytes(lits)
        out += src[at:at + lits]
        out += off.to_bytes(2, "little")
        if mlen - 4 >= 15:
            out += _length_bytes(mlen - 4)
        at += lits + mlen
    lits = len(src) - at
    out.append(min(lits, 15) << 4)
    if lits >= 15:
        out += _length_bytes(lits)
    out += src[at:]
    return bytes(out)


def encode(src, prefix=b"", acceleration=1, plain=False, rule=RULE):
    """The block the GPU writes for (src, prefix, acceleration); len(src) <= 65536."""
    assert len(src) <= MAX_BLOCK
    return emit(src, parse(src, prefix, acceleration, plain, rule))


def compress(src, cap, prefix=b"", acceleration=1):
    """The launcher's per-block result: (result, the bytes written when result > 0)."""
    if len(src) > MAX_BLOCK:
        return ERANGE, b""
    if cap < 0:
        return 0, b""
    out = encode(src, prefix, acceleration)
    return (len(out), out) if len(out) <= cap else (0, b"")
