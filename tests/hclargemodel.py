"""A Python model of the high-ratio mode with history and on large inputs
(APE_LZ4_compress_hc_withPrefix_batch_dev, APE_LZ4_compress_large_hc_batch_dev).
The GPU's output is a pure function of (input bytes, used history, depth, restartBytes), and
this file is its definition, on top of tests/hcmodel.py (the search rule and the parse) and
tests/indexutil.py (the stitch and the index).  No product or oracle code.

compress_prefix() is hcmodel.compress() on a window = history + block: the chains run over the
whole window, so candidates may lie in the history; only the block's positions are searched and
parsed.  compress_large() cuts an input at multiples of S, compresses slice k against the bytes
before it (back to the last restart point, when there are any) and stitches the streams."""
import collections

import numpy as np

import hcmodel
import indexutil
from hcmodel import CAP, HBITS, HMUL, LASTLITERALS, MAX_BLOCK, MFLIMIT

SLICE = 32768    # S of the CPU tests; the GPU tests pass compress_large_slice_size()
MINLENGTH = MFLIMIT + 1   # a block shorter than this is one literal run, whatever its history

# The large path's rule, and the handles by which tests/test_hc_large_model.py moves it to its
# wrong neighbours: slices see history at all; as much of it as the window holds beside the
# slice (a number: that many bytes at the most, whatever the slice's length); a match is capped
# against the slice's end (False: against the input's end, the bytes after the slice in sight).
Rule = collections.namedtuple("Rule", "history fixed mx_slice")
RULE = Rule(history=True, fixed=None, mx_slice=True)


def used_history(prefix_size, size):
    """The bytes of history a block of `size` bytes uses out of prefix_size offered: a window of
    u16 positions holds 65536 bytes, and nothing is rounded."""
    return max(0, min(prefix_size, MAX_BLOCK - size))


def search(window, prefix, depth, ahead=0):
    """hcmodel.search's rule for the positions p in [prefix, len(window) - 12] alone, with chains
    over the whole window: arrays (L, q) indexed by window position (zero before prefix).
    (ahead, for a wrong neighbour only: the block ends that many bytes before the window does.)"""
    n = len(window)
    P = max(n - ahead - MFLIMIT + 1, 0)
    best, bq = np.zeros(P, np.int64), np.zeros(P, np.int64)
    if n - ahead - prefix < MINLENGTH:
        return best, bq
    a = np.zeros(n + CAP + 16, np.uint64)      # (the pad is never counted: L stops at mx)
    a[:n] = np.frombuffer(window, np.uint8)
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
    idx = pos[(cur >= 0) & (pos >= prefix)]
    for _ in range(depth):
        if not idx.size:
            break
        q = cur[idx]
        L = hcmodel._prefix_lengths(w8, q, idx, mx[idx])
        better = (L >= 4) & (L > best[idx])
        best[idx[better]] = L[better]
        bq[idx[better]] = q[better]
        nxt = prev[q]
        cur[idx] = nxt
        idx = idx[(L < mx[idx]) & (nxt >= 0)]
    return best, bq


def parse(window, prefix, ML, MQ, ahead=0):
    """hcmodel.parse's walk over the window, starting with p = anchor = prefix."""
    n = len(window)
    out = bytearray()
    p = anchor = prefix
    last = n - ahead - MFLIMIT
    while p <= last:
        if ML[p] == 0:
            p += 1
            continue
        while p + 1 <= last and ML[p + 1] > ML[p]:      # the lazy step
            p += 1
        L, q = int(ML[p]), int(MQ[p])
        if L == min(CAP, n - LASTLITERALS - p):          # capped: extend forward
            while p + L < n - LASTLITERALS and window[q + L] == window[p + L]:
                L += 1
        lits, ml = p - anchor, L - 4
        out.append((min(lits, 15) << 4) | min(ml, 15))
        if lits >= 15:
            out += hcmodel._length_bytes(lits)
        out += window[anchor:p]
        out += (p - q).to_bytes(2, "little")
        if ml >= 15:
            out += hcmodel._length_bytes(ml)
        p += L
        anchor = p
    lits = max(n - ahead - anchor, 0)
    out.append(min(lits, 15) << 4)
    if lits >= 15:
        out += hcmodel._length_bytes(lits)
    out += window[anchor:anchor + lits]
    return bytes(out)


def compress_prefix(window, prefix, depth, ahead=0):
    """The block the GPU writes for window[prefix:] with window[:prefix] as its used history
    (len(window) <= 65536); it decodes with decompress_safe_usingDict given that history."""
    assert 1 <= depth <= 256 and 0 <= prefix <= len(window) - ahead <= MAX_BLOCK
    window = bytes(window)
    ML, MQ = search(window, prefix, depth, ahead)
    return parse(window, prefix, ML.tolist(), MQ.tolist(), ahead)


def slices(n, S=SLICE, restart=0, rule=RULE):
    """[(start, length, used history)] of an input of n > 65536 bytes, as large_plan_kernel
    cuts it: history back to the last restart point, at most 65536 - length bytes of it."""
    out = []
    for start in range(0, n, S):
        ln = min(S, n - start)
        offered = (start % restart if restart > 0 else start) if rule.history else 0
        h = used_history(offered, ln) if rule.fixed is None else min(offered, rule.fixed)
        out.append((start, ln, h))
    return out


def compress_large(src, depth, restart=0, S=SLICE, rule=RULE):
    """The block the GPU writes for an input of any size; its index is
    indexutil.build_index(block, range(0, len(src), restart)) when restart > 0."""
    src = bytes(src)
    if len(src) <= MAX_BLOCK:
        return hcmodel.compress(src, depth)
    assert restart >= 0 and restart % S == 0
    streams = []
    for st, ln, h in slices(len(src), S, restart, rule):
        ahead = 0 if rule.mx_slice else min(len(src) - st - ln, CAP)
        streams.append(compress_prefix(src[st - h:st + ln + ahead], h, depth, ahead))
    return indexutil.stitch(streams)
