"""A Python model of the fast encoder (APE_LZ4_compress_batch_dev, _fast_batch_dev and
_withPrefix_batch_dev; DESIGN.md 3.1, "The parse as a function").  The GPU's output is a pure
function of (input bytes, used prefix, acceleration), and this file is its definition.  No
product or oracle code.

candidates_plain() and walk_plain() state the rule position by position; candidates() and
walk() are the same rule with the table resolved for all positions at once (numpy) and the
walk jumping from match to match, fast enough for the 64 KiB blocks of the GPU tests.
tests/test_enc_model.py holds the two against each other.

encode_cdict() is APE_LZ4_compress_usingCDict_batch_dev: the same rule on
window = dictionary[-D:] + message, D = min(dictionary, 65536 - maxSrcSize) rounded down to 64
(0 below 64) whatever the message's length, with the three changes a dictionary that does not
lie before the message brings: dictionary position v is hashed when v % 3 == 0 and v + 8 <= D,
a candidate c with D - 3 <= c <= D + 3 is none, and a match from a candidate below D ends at D.
candidates_cdict() takes the dictionary's table from dict_table(), built once per (dictionary, D).

dest_size() is compress_destSize's cut (lz4_destsize_kernel): a block that fits
its target is kept; otherwise the first k sequences of parse() and the longest final literal
run L with 1 + length bytes + L <= the room left, for the k that consumes the most input (the
earliest of equals), a cut after a match of ml bytes being legal when L >= 5, or 12 - ml for
ml < 7.

RULE holds the rule's constants.  The tests build wrong models from it (RULE._replace) to show
that their inputs tell each constant from its neighbour; the product has one rule, RULE."""
import collections
import functools

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
    # a prepared dictionary (encode_cdict); D is the window's dictionary part
    "ext_window",     # D comes from "max_src" (the object's), not from the message's "len"
    "ext_hash_end",   # dictionary position v is hashed when v + 8 <= "D" (not the window's "N")
    "ext_below",      # a candidate c with D - ext_below <= c ...
    "ext_above",      # ... <= D + ext_above is no candidate
    "ext_cut",        # a match from a candidate below D ends at D + ext_cut (None: no cut)
    # compress_destSize (dest_size)
    "ds_long",        # after a last match of ds_long bytes or more the final run needs ...
    "ds_need",        # ... ds_need literals,
    "ds_sum",         # after a shorter one ds_sum - its length
    "ds_later",       # of two cuts that consume the same, the later one is taken
    "ds_ext1",        # a final run of ds_ext1 literals or more has one length byte,
    "ds_ext2",        # of ds_ext2 or more two (and one more per 255 from there)
])
RULE = Rule(back=4, own_chunk=False, insert_room=5, min_cand=4, fwd_cap=None, prefix_stride=3,
            prefix_round=64, regime=64, acc_more=16,
            ext_window="max_src", ext_hash_end="D", ext_below=3, ext_above=3, ext_cut=0,
            ds_long=7, ds_need=5, ds_sum=12, ds_later=False, ds_ext1=15, ds_ext2=270)


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


def _prefix_positions(N, D, rule, ext=False):
    """The hashed positions of the history: with an adjacent prefix the 8 bytes may run on into
    the input, in a prepared dictionary (ext) they end with it."""
    end = D if ext and rule.ext_hash_end == "D" else N
    return [v for v in range(0, D, rule.prefix_stride) if v + 8 <= end]


def candidates_plain(w, D, rule=RULE, ext=False):
    """cand[p] for every window position (0 below D): what the table holds under p's hash when
    p's chunk looks it up.  One position at a time, with the table itself."""
    N = len(w)
    tab = [0] * HSIZE
    cand = [0] * N
    for v in _prefix_positions(N, D, rule, ext):
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


def _hashes(w):
    """hashk of every position of w."""
    N = len(w)
    a = np.zeros(N + 8, np.uint64)
    a[:N] = np.frombuffer(w, np.uint8)
    lo3 = a[0:N] | (a[1:N + 1] << np.uint64(8)) | (a[2:N + 2] << np.uint64(16))
    hi3 = a[3:N + 3] | (a[4:N + 4] << np.uint64(8)) | (a[5:N + 5] << np.uint64(16))
    v = (lo3 * np.uint64(0x9E3779) + hi3 * np.uint64(0xC2B2AE) + a[6:N + 6] * np.uint64(0x27D4EB)) \
        & np.uint64(0xFFFFFFFF)
    return ((v * np.uint64(HSIZE)) >> np.uint64(32)).astype(np.int64)


def _latest(h, written, seen):
    """Per position: the latest of the `written` positions below seen[p] in p's slot, or -1."""
    if written.size == 0:
        return np.full(h.size, -1, np.int64)
    keys = np.sort(h[written] * (1 << 20) + written)   # (position order is the order of the writes)
    at = np.searchsorted(keys, h * (1 << 20) + seen) - 1
    hit = keys[np.maximum(at, 0)]
    return np.where((at >= 0) & ((hit >> 20) == h), hit & ((1 << 20) - 1), -1)


def candidates(w, D, rule=RULE):
    """candidates_plain for all positions at once: the latest position written under the same
    slot before p's chunk (before p, for own_chunk)."""
    N = len(w)
    if N == 0:
        return []
    h = _hashes(w)
    pos = np.arange(N, dtype=np.int64)
    written = np.concatenate([np.array(_prefix_positions(N, D, rule), np.int64),
                              pos[(pos >= D) & (pos + rule.insert_room <= N)]])
    # writes below `seen` are visible (every prefix position to the block's first chunk)
    seen = pos if rule.own_chunk else np.maximum(pos - pos % CHUNK, D)
    cand = np.maximum(_latest(h, written, seen), 0)
    cand[:D] = 0
    return cand.tolist()


def dict_table(dictionary, D, rule=RULE):
    """The table a prepared dictionary carries: slot -> the latest hashed position of the
    dictionary's last D bytes alone, 0 where there is none.  Built once per (dictionary, D):
    give the same bytes object for every message of a batch, its hash is taken once."""
    return _dict_table(dictionary, D, rule.prefix_stride)


@functools.lru_cache(maxsize=64)
def _dict_table(dictionary, D, stride):
    head = dictionary[len(dictionary) - D:]
    tab = np.zeros(HSIZE, np.int64)
    v = np.arange(0, max(D - 7, 0), stride, dtype=np.int64)      # v + 8 <= D
    if v.size:
        hv = _hashes(head)[v]
        order = np.argsort(hv, kind="stable")                     # per slot: the last v wins
        hs, vs = hv[order], v[order]
        keep = np.r_[hs[1:] != hs[:-1], True]
        tab[hs[keep]] = vs[keep]
    return tab


def candidates_cdict(w, D, dictionary, rule=RULE):
    """candidates_plain(w, D, rule, ext=True) for all positions at once: the message's own
    writes as in candidates(), and below them the table of the dictionary (whose last D bytes
    are w[:D]), built once per (dictionary, D)."""
    N = len(w)
    if rule.ext_hash_end != "D":                 # (a wrong rule: the table depends on the message)
        tab = np.zeros(HSIZE, np.int64)
        for v in _prefix_positions(N, D, rule, True):
            tab[hashk(w, v)] = v
    else:
        tab = dict_table(dictionary, D, rule)
    h = _hashes(w[D:])
    pos = np.arange(N - D, dtype=np.int64)       # (D is a multiple of CHUNK)
    written = pos[D + pos + rule.insert_room <= N]
    own = _latest(h, written, pos if rule.own_chunk else pos - pos % CHUNK)
    return [0] * D + np.where(own >= 0, own + D, tab[h]).tolist()


def has_match(w, cand, p, rule=RULE, ext=None):
    """ext: D of a prepared dictionary, whose bytes do not lie before the message's: a candidate
    whose 4 bytes (below D) or whose 4 bytes of backward context (from D on) cross D is none."""
    N, c = len(w), cand[p]
    if ext is not None and ext - rule.ext_below <= c <= ext + rule.ext_above:
        return False
    return 1 <= p <= N - MFLIMIT and rule.min_cand <= c < p and w[c:c + 4] == w[p:p + 4]


def forward(w, c, p, rule=RULE, ext=None):
    """Bytes equal from (c, p) on, at most up to the match limit N - 5 -- and, from a candidate
    in a prepared dictionary (ext: its D), up to the dictionary's end."""
    mx = len(w) - LASTLITERALS - p
    if rule.fwd_cap is not None:
        mx = min(mx, rule.fwd_cap)
    if ext is not None and rule.ext_cut is not None and c < ext:
        mx = min(mx, ext + rule.ext_cut - c)
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


def _take(w, cand, p, e, accel, rule, ext=None):
    c = cand[p]
    L = forward(w, c, p, rule, ext)
    b = backward(w, c, p, p - e, accel, rule)
    return (p - b - e, L + b, p - c), p + L


def walk_plain(w, D, cand, accel=1, rule=RULE, ext=False):
    """The greedy walk, one position (or probe) at a time: [(literals, match length, offset)].
    ext: [0, D) is a prepared dictionary's window."""
    N = len(w)
    ext = D if ext else None
    seqs, e = [], D
    if N - D < MINLENGTH:
        return seqs
    accel = min(accel, MAX_ACCEL)
    last = N - MFLIMIT
    while True:
        visit = range(e, last + 1) if accel <= 1 else probes(e, accel, last, rule)
        for p in visit:
            if has_match(w, cand, p, rule, ext):
                break
        else:
            return seqs
        s, e = _take(w, cand, p, e, accel, rule, ext)
        seqs.append(s)


def walk(w, D, cand, accel=1, rule=RULE, ext=False):
    """walk_plain over the positions that have a match only."""
    N = len(w)
    ext = D if ext else None
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
    if ext is not None:
        ok &= (c < D - rule.ext_below) | (c > D + rule.ext_above)
    ok &= w4[np.where(ok, c, 0)] == w4[:last + 1]
    if accel <= 1:
        at = np.nonzero(ok)[0].tolist()
        i = 0
        while True:
            while i < len(at) and at[i] < e:
                i += 1
            if i == len(at):
                return seqs
            s, e = _take(w, cand, at[i], e, accel, rule, ext)
            seqs.append(s)
    ok = ok.tolist()
    while True:
        for q in probes(e, accel, last, rule):
            if ok[q]:
                break
        else:
            return seqs
        s, e = _take(w, cand, q, e, accel, rule, ext)
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


# ---------------- a prepared dictionary (APE_LZ4_compress_usingCDict_batch_dev) ----------------
def cdict_window(dict_len, max_src, rule=RULE):
    """D of a dictionary prepared for messages of up to max_src bytes: min(dict_len, 65536 -
    max_src) rounded down to 64, and 0 below 64.  Every message of the object gets this D,
    whatever its own length."""
    return used_prefix(max_src, dict_len, rule)


def parse_cdict(src, dictionary, max_src, plain=False, rule=RULE):
    """The sequence list of a message against a dictionary prepared for max_src: the rule of
    parse() on window = dictionary[-D:] + src, except that the dictionary's bytes do not lie in
    memory before the message's, so nothing of the dictionary reads on into the message:
      - dictionary position v is hashed when v % 3 == 0 and v + 8 <= D;
      - a candidate within 3 bytes of D on either side is no candidate (has_match);
      - a match from a candidate below D ends at D at the latest (forward)."""
    src = bytes(src)
    dictionary = dictionary if type(dictionary) is bytes else bytes(dictionary)
    assert 1 <= max_src <= MAX_BLOCK and len(src) <= max_src
    D = cdict_window(len(dictionary), max_src if rule.ext_window == "max_src" else len(src), rule)
    w = dictionary[len(dictionary) - D:] + src
    if plain:
        return walk_plain(w, D, candidates_plain(w, D, rule, True), 1, rule, True)
    return walk(w, D, candidates_cdict(w, D, dictionary, rule), 1, rule, True)


def encode_cdict(src, dictionary, max_src, plain=False, rule=RULE):
    """The block the GPU writes for a message of a batch against a prepared dictionary."""
    return emit(src, parse_cdict(src, dictionary, max_src, plain, rule))


# ---------------- compress_destSize (lz4_destsize_kernel) ----------------
def _run_bytes(L, rule=RULE):
    """Token and length bytes of a final run of L literals."""
    if L < rule.ds_ext1:
        return 1
    return 2 if L < rule.ds_ext2 else 3 + (L - rule.ds_ext2) // 255


def max_lastrun(room, rem, plain=False, rule=RULE):
    """The fill rule: the longest final literal run L <= rem with token + length bytes + L <=
    room (room >= 1)."""
    if plain:                         # (from the top: the first L that fits is the longest)
        L = min(rem, room)
        while L and _run_bytes(L, rule) + L > room:
            L -= 1
        return L
    lo, hi = 0, min(rem, room)        # (_run_bytes(L) + L grows with L)
    while lo < hi:
        L = (lo + hi + 1) // 2
        if _run_bytes(L, rule) + L <= room:
            lo = L
        else:
            hi = L - 1
    return lo


def dest_size(src, target, plain=False, rule=RULE, seqs=None):
    """(result, consumed, bytes) of compress_destSize.  A block that fits the target is kept.
    Otherwise the cut is the first k sequences of parse(src) and then the longest final
    literal run the target has room for, for the k that consumes the most input (the earliest
    such k); after a last match of ml bytes the run must have 5 literals, after one shorter
    than 7 (which the decoder wants to start 12 bytes before the end) 12 - ml.  k = 0, a
    literal run alone, needs nothing.  (seqs: parse(src), for a caller that has it.)"""
    src = bytes(src)
    n = len(src)
    assert n <= MAX_BLOCK
    if target < 1:
        return 0, n, b""
    seqs = parse(src, plain=plain) if seqs is None else seqs
    out = emit(src, seqs)
    if len(out) <= target:
        return len(out), n, out
    k, at, best = 0, 0, max_lastrun(target, n, plain, rule)
    op = pos = 0
    for i, (lits, ml, _) in enumerate(seqs):
        op += 1 + len(_length_bytes(lits) if lits >= 15 else b"") + lits + 2 + \
            len(_length_bytes(ml - 4) if ml - 4 >= 15 else b"")
        pos += lits + ml
        if op + 1 > target:               # no room for the final run's token
            break
        need = rule.ds_need if ml >= rule.ds_long else rule.ds_sum - ml
        L = max_lastrun(target - op, n - pos, plain, rule)
        if L >= need and (pos + L > best or (rule.ds_later and pos + L == best)):
            k, at, best = i + 1, pos, pos + L
    out = emit(src[:best], seqs[:k])
    return len(out), best, out
