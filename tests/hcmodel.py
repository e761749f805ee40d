"""A Python model of the high-ratio encoder (APE_LZ4_compress_hc_batch_dev):
hash chains, a search of the first `depth` chain members of every position, and a sequential
parse with a one-step lazy rule.  The GPU's output is a pure function of (input bytes, depth),
and this file is its definition.  No product or oracle code.

search_plain() states the search position by position; search() is the same rule over all
positions at once (numpy), fast enough for 64 KiB blocks at depth 256.  tests/test_hc_model.py
holds the two against each other."""
import numpy as np

CAP = 272        # longest match the search reports (kHcCap, lz4_gpu_internal.h)
HBITS = 14       # bits of the chain hash (kHcHashBits)
HMUL = 2654435761
MAX_BLOCK = 65536
MFLIMIT = 12     # a match starts at p <= n - 12 ...
LASTLITERALS = 5  # ... and ends at or before n - 5


def hash4(word):
    """The chain hash of the 4 bytes at p, given as a little-endian integer."""
    return ((word * HMUL) & 0xFFFFFFFF) >> (32 - HBITS)


def chains(src):
    """prev[p] for p in [0, n - 4]: the nearest earlier position with the same hash, or -1."""
    n = len(src)
    prev, head = [-1] * max(n - 3, 0), {}
    for p in range(n - 3):
        h = hash4(int.from_bytes(src[p:p + 4], "little"))
        prev[p] = head.get(h, -1)
        head[h] = p
    return prev


def common_prefix(src, q, p, mx):
    a, b = src[p:p + mx], src[q:q + mx]
    if a == b:
        return mx
    x = int.from_bytes(a, "little") ^ int.from_bytes(b, "little")
    return ((x & -x).bit_length() - 1) >> 3


def search_plain(src, depth):
    """M[p] = (L, q) for p in [0, n - 12] (L = 0: none), one position at a time."""
    n = len(src)
    prev = chains(src)
    M = []
    for p in range(n - MFLIMIT + 1):
        mx = min(CAP, n - LASTLITERALS - p)
        best, bq, q = 0, 0, prev[p]
        for _ in range(depth):
            if q < 0:
                break
            L = common_prefix(src, q, p, mx)
            if L >= 4 and L > best:     # strictly longer: a tie stays with the nearer one
                best, bq = L, q
            if L == mx:
                break
            q = prev[q]
        M.append((best, bq))
    return M


def _prefix_lengths(w8, q, p, mx):
    """Common prefix of src[q..] and src[p..] capped at mx, for arrays of pairs."""
    L = np.zeros(q.shape[0], np.int64)
    live = np.arange(q.shape[0])
    k = 0
    while live.size:
        x = w8[q[live] + k] ^ w8[p[live] + k]
        same = np.zeros(live.shape[0], np.int64)
        run = np.ones(live.shape[0], bool)
        for b in range(8):
            run &= ((x >> np.uint64(8 * b)) & np.uint64(0xFF)) == 0
            same += run
        L[live] = np.minimum(k + same, mx[live])
        live = live[(same == 8) & (k + 8 < mx[live])]
        k += 8
    return L


def search(src, depth):
    """search_plain over all positions at once: arrays (L, q) over p in [0, n - 12]."""
    n = len(src)
    P = max(n - MFLIMIT + 1, 0)
    best, bq = np.zeros(P, np.int64), np.zeros(P, np.int64)
    if n < MFLIMIT + 1:
        return best, bq
    a = np.zeros(n + CAP + 16, np.uint64)      # (the pad is never counted: L stops at mx)
    a[:n] = np.frombuffer(src, np.uint8)
    w8 = np.zeros(n + CAP + 8, np.uint64)
    for b in range(8):
        w8 |= a[b:b + w8.shape[0]] << np.uint64(8 * b)
    h = ((w8[:n - 3] & np.uint64(0xFFFFFFFF)) * np.uint64(HMUL) & np.uint64(0xFFFFFFFF)) \
        >> np.uint64(32 - HBITS)
    order = np.argsort(h, kind="stable")
    prev = np.full(n - 3, -1, np.int64)
    same = h[order[1:]] == h[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    pos = np.arange(P)
    mx = np.minimum(CAP, n - LASTLITERALS - pos)
    cur = prev[:P].copy()
    idx = pos[cur >= 0]
    for _ in range(depth):
        if not idx.size:
            break
        q = cur[idx]
        L = _prefix_lengths(w8, q, idx, mx[idx])
        better = (L >= 4) & (L > best[idx])
        best[idx[better]] = L[better]
        bq[idx[better]] = q[better]
        nxt = prev[q]
        cur[idx] = nxt
        idx = idx[(L < mx[idx]) & (nxt >= 0)]
    return best, bq


def _length_bytes(v):
    """The bytes after the token for a length field whose value is v (>= 15)."""
    v -= 15
    return b"\xff" * (v // 255) + bytes([v % 255])


def parse(src, ML, MQ):
    """The sequential walk over M = (ML, MQ): the LZ4 block."""
    n = len(src)
    out = bytearray()
    p = anchor = 0
    last = n - MFLIMIT
    while p <= last:
        if ML[p] == 0:
            p += 1
            continue
        while p + 1 <= last and ML[p + 1] > ML[p]:      # the lazy step
            p += 1
        L, q = int(ML[p]), int(MQ[p])
        if L == min(CAP, n - LASTLITERALS - p):          # capped: extend forward
            while p + L < n - LASTLITERALS and src[q + L] == src[p + L]:
                L += 1
        lits, ml = p - anchor, L - 4
        out.append((min(lits, 15) << 4) | min(ml, 15))
        if lits >= 15:
            out += _length_bytes(lits)
        out += src[anchor:p]
        out += (p - q).to_bytes(2, "little")
        if ml >= 15:
            out += _length_bytes(ml)
        p += L
        anchor = p
    lits = n - anchor
    out.append(min(lits, 15) << 4)
    if lits >= 15:
        out += _length_bytes(lits)
    out += src[anchor:]
    return bytes(out)


def compress(src, depth=64, plain=False):
    """The block the GPU writes for (src, depth); depth in 1..256, len(src) <= 65536."""
    assert 1 <= depth <= 256 and len(src) <= MAX_BLOCK
    src = bytes(src)
    if plain:
        M = search_plain(src, depth)
        return parse(src, [m[0] for m in M], [m[1] for m in M])
    ML, MQ = search(src, depth)
    return parse(src, ML.tolist(), MQ.tolist())
