"""A Python model of the high-ratio mode's cost-minimising parse
(APE_LZ4_compress_hc_opt_batch_dev, APE_LZ4_compress_hc_opt_withPrefix_batch_dev,
APE_LZ4_compress_large_hc_opt_batch_dev).  The GPU's output is a pure function of
(input bytes, used history, depth, restartBytes), and this file is its definition, on top of
tests/hclargemodel.py (the search over a window, the slices) and tests/indexutil.py (the stitch).
No product or oracle code.

The search is the lazy mode's, unchanged: M[p] = (L, q), the longest match among the first `depth`
chain members of p.  What differs is the walk over M.  Every offset costs two bytes, so a price
needs one source per position only, and any prefix of the longest match is as cheap to reference
as the match itself.  A backward pass gives every position the cost A[p] of the cheapest encoding
of window[p:] it can see -- a literal, or a match of any length from 4 up to the match's full
length E(p) -- and a forward pass emits the choices.  R[p], the literals that lead the chosen
continuation, makes the literal-length bytes exact along the chosen path, so A[prefix] is the
emitted size; it is the run of the CHOSEN continuation only, so the parse is cost-minimising,
not a proven optimum."""
import collections

import numpy as np

import hclargemodel
import hcmodel
import indexutil
from hcmodel import CAP, LASTLITERALS, MAX_BLOCK, MFLIMIT
from hclargemodel import SLICE

# The rule, and the handles by which tests/test_hc_opt_model.py moves it to its wrong
# neighbours: among equally cheap match lengths the longest is taken; a match as cheap as the
# literal is taken; the match's full length (past the search's cap) is a candidate; a literal
# pays for the length byte it adds to its run.
Rule = collections.namedtuple("Rule", "longest match_wins_ties full_length literal_term")
RULE = Rule(longest=True, match_wins_ties=True, full_length=True, literal_term=True)


def lb(v):
    """The bytes a length field of value v takes after the token."""
    return 0 if v < 15 else 1 + (v - 15) // 255


# lb(l - 4) for a match of l bytes, l in [0, CAP]
_MATCH_LB = np.array([lb(max(l - 4, 0)) for l in range(CAP + 1)], np.int64)


def full_length_plain(window, prefix, ML, MQ):
    """E(p) for every p with a match, byte by byte: the common prefix of window[q:] and
    window[p:], limited to len(window) - 5 - p.  (0 where M[p] has no match.)"""
    W = len(window)
    E = [0] * len(ML)
    for p in range(prefix, W - MFLIMIT + 1):
        if ML[p]:
            q, e = MQ[p], 0
            while p + e < W - LASTLITERALS and window[q + e] == window[p + e]:
                e += 1
            E[p] = e
    return E


def full_length(window, prefix, ML, MQ):
    """The same, cheaply.  L below its cap min(CAP, W - 5 - p) is E.  A capped match is extended
    -- unless the nearest later position with a match, p' <= p + L, has the same offset: then the
    two are one repetition and E(p) = p' + E(p') - p, so a run of capped matches at one offset
    costs one extension in all."""
    W = len(window)
    E = [0] * len(ML)
    run_off = run_p = run_end = -1
    for p in range(W - MFLIMIT, prefix - 1, -1):
        L = ML[p]
        if not L:
            continue
        q, lim = MQ[p], W - LASTLITERALS - p
        if L < min(CAP, lim) or L == lim:
            e = L
        elif p - q == run_off and run_p <= p + L:
            e = run_end - p
        else:
            e = L + hcmodel.common_prefix(window, q + L, p + L, lim - L)
        E[p] = e
        run_off, run_p, run_end = p - q, p, p + e
    return E


def price(window, prefix, ML, MQ, rule=RULE):
    """The backward pass: (A, C) over window positions, A[p] the cost of window[p:] (A[W] = 1,
    the final run's token) and C[p] the chosen match length at p, 0 for a literal."""
    W = len(window)
    E = full_length(window, prefix, ML, MQ)
    A = np.zeros(W + 1, np.int64)
    C = [0] * (W + 1)
    A[W] = 1
    a1, r1 = 1, 0            # A[p + 1], R[p + 1]
    last = W - MFLIMIT if W - prefix > MFLIMIT else -1
    for p in range(W - 1, prefix - 1, -1):
        lit = 1 + a1 + (lb(r1 + 1) - lb(r1) if rule.literal_term else 0)
        best_l = 0
        if p <= last and ML[p]:
            e = E[p]
            near = min(e, CAP)
            cost = A[p + 4:p + near + 1] + _MATCH_LB[4:near + 1]
            if rule.longest:
                k = near - 4 - int(np.argmin(cost[::-1]))
            else:
                k = int(np.argmin(cost))
            best, best_l = 3 + int(cost[k]), 4 + k
            if e > CAP and rule.full_length:
                far = 3 + lb(e - 4) + int(A[p + e])
                if far <= best if rule.longest else far < best:
                    best, best_l = far, e
            if not (best <= lit if rule.match_wins_ties else best < lit):
                best_l = 0
        if best_l:
            a1, r1 = best, 0
        else:
            a1, r1 = lit, r1 + 1
        A[p], C[p] = a1, best_l
    return A, C


def parse_opt(window, prefix, ML, MQ, rule=RULE):
    """The cost-minimising walk over M = (ML, MQ) for window[prefix:]: the LZ4 block."""
    W = len(window)
    A, C = price(window, prefix, ML, MQ, rule)
    out = bytearray()
    p = anchor = prefix
    while p < W:
        l = C[p]
        if l == 0:
            p += 1
            continue
        lits, ml = p - anchor, l - 4
        out.append((min(lits, 15) << 4) | min(ml, 15))
        if lits >= 15:
            out += hcmodel._length_bytes(lits)
        out += window[anchor:p]
        out += (p - int(MQ[p])).to_bytes(2, "little")
        if ml >= 15:
            out += hcmodel._length_bytes(ml)
        p += l
        anchor = p
    lits = W - anchor
    out.append(min(lits, 15) << 4)
    if lits >= 15:
        out += hcmodel._length_bytes(lits)
    out += window[anchor:]
    if rule == RULE:
        assert int(A[prefix]) == len(out), (int(A[prefix]), len(out))
    return bytes(out)


def compress_prefix(window, prefix, depth, rule=RULE):
    """The block the GPU writes for window[prefix:] with window[:prefix] as its used history
    (len(window) <= 65536); it decodes with decompress_safe_usingDict given that history."""
    assert 1 <= depth <= 256 and 0 <= prefix <= len(window) <= MAX_BLOCK
    window = bytes(window)
    ML, MQ = hclargemodel.search(window, prefix, depth)
    return parse_opt(window, prefix, ML.tolist(), MQ.tolist(), rule)


def compress(src, depth=64, rule=RULE):
    """The block the GPU writes for (src, depth); depth in 1..256, len(src) <= 65536."""
    return compress_prefix(src, 0, depth, rule)


def compress_large(src, depth, restart=0, S=SLICE):
    """The block the GPU writes for an input of any size; its index is
    indexutil.build_index(block, range(0, len(src), restart)) when restart > 0."""
    src = bytes(src)
    if len(src) <= MAX_BLOCK:
        return compress(src, depth)
    assert restart >= 0 and restart % S == 0
    return indexutil.stitch([compress_prefix(src[st - h:st + ln], h, depth)
                             for st, ln, h in hclargemodel.slices(len(src), S, restart)])
