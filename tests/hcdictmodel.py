"""A Python model of the high-ratio mode against a prepared dictionary
(APE_LZ4_hc_cdict_prepare_dev + APE_LZ4_compress_hc_usingCDict_batch_dev).
No new policy: the block of message m is hclargemodel.compress_prefix() on the window
[the dictionary's last D bytes | m], D = min(dictSize, 65536 - maxSrcSize), not rounded.  This
file holds that window rule, the call, and the handles by which tests/test_hc_cdict_model.py
moves the rule to its wrong neighbours.  No product or oracle code."""
import collections

import hclargemodel
import hcmodel
from hcmodel import CAP, LASTLITERALS, MAX_BLOCK, MFLIMIT

# The rule and its wrong neighbours: D rounded down to a multiple of 64 (the fast prepared
# dictionary's rule); a match that starts in the dictionary ends at the dictionary's end (the
# fast call's); the window positions D-3 .. D-1, whose 4 bytes straddle dictionary and message,
# are chain members; the dictionary is history at all.
Rule = collections.namedtuple("Rule", "round64 stop_at_dict straddle history")
RULE = Rule(round64=False, stop_at_dict=False, straddle=True, history=True)


def window(dict_size, max_src_size, rule=RULE):
    """D: the bytes of the dictionary's tail a prepared high-ratio dictionary uses."""
    assert dict_size >= 0 and 1 <= max_src_size <= MAX_BLOCK
    if not rule.history:
        return 0
    D = min(dict_size, MAX_BLOCK - max_src_size)
    return D & ~63 if rule.round64 else D


def search_plain(win, D, depth, rule=RULE):
    """hcmodel.search_plain's rule on the window, one position at a time, for the message's
    positions alone: lists (L, q) by window position.  With RULE it is hclargemodel.search
    (tests/test_hc_cdict_model.py holds the two against each other); the neighbours live here."""
    n = len(win)
    P = max(n - MFLIMIT + 1, 0)
    ML, MQ = [0] * P, [0] * P
    if n - D < MFLIMIT + 1:
        return ML, MQ
    prev, head = [-1] * (n - 3), {}
    for p in range(n - 3):
        if not rule.straddle and D - 3 <= p < D:
            continue
        h = hcmodel.hash4(int.from_bytes(win[p:p + 4], "little"))
        prev[p] = head.get(h, -1)
        head[h] = p
    for p in range(D, P):
        mx = min(CAP, n - LASTLITERALS - p)
        q = prev[p]
        for _ in range(depth):
            if q < 0:
                break
            L = hcmodel.common_prefix(win, q, p, mx)
            if rule.stop_at_dict and q < D:
                L = min(L, D - q)
            if L >= 4 and L > ML[p]:
                ML[p], MQ[p] = L, q
            if L == mx:
                break
            q = prev[q]
    return ML, MQ


def compress(dictionary, message, max_src_size, depth, rule=RULE):
    """The block the GPU writes for `message` (at most max_src_size bytes) against an object
    prepared from `dictionary` for max_src_size; it decodes with decompress_safe_usingDict given
    the whole dictionary."""
    assert len(message) <= max_src_size
    D = window(len(dictionary), max_src_size, rule)
    win = bytes(dictionary[len(dictionary) - D:]) + bytes(message)
    if rule == RULE:
        return hclargemodel.compress_prefix(win, D, depth)
    ML, MQ = search_plain(win, D, depth, rule)
    return hclargemodel.parse(win, D, ML, MQ)
