"""Which path of the decoder's copy scheduler a sequence takes: a Python restatement of the
arithmetic of copy_batch (segments, slide condition, new base, gdone) and of the masks of
copy_segment (off0m, ovlm, inwm, ingm, indm, lpom, lenm, r1m, the need mask and the pass loop)
in libapenetwork_amd/csrc/lz4_decode.hip.

DOCUMENTATION-BOUND: this file follows the kernel, not the other way round.  It exists only to
prove what the corpus of tests/decseq.py reaches (tests/test_dec_copy_classes.py) and to name a
branch in a failure message.  No byte a GPU test checks comes from here: bytes are compared
with decseq.build's plain decoder, return values with the oracle.

SCOPE: single-batch blocks only -- at most 63 descriptors (sequences and the final literal
run) and a compressed size of at most kStage - kWinNeed bytes.  Such a block is staged once and
copied as one batch, B0 = 0 and B1 = the output size, so the geometry is exact.

The constants are read from the kernel's text, so a retuned window moves the cases with it.
"""
import os
import re

_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "libapenetwork_amd", "csrc", "lz4_decode.hip")


def _constants():
    text = open(_HIP).read()
    pat = {
        "kWinB": r"#define APE_LZ4_DWIN (\d+)",
        "kKeep": r"#define APE_LZ4_DKEEP (\d+)",
        "kStage": r"#define APE_LZ4_DSTAGE (\d+)",
        "kWinNeed": r"constexpr int kWinNeed = (\d+);",
        "kBatch": r"constexpr int kBatch = (\d+);",
        "kLaneMax": r"constexpr uint32_t kLaneMax = (\d+);",
    }
    out = {}
    for k, p in pat.items():
        m = re.search(p, text)
        if not m:
            raise RuntimeError("lz4_decode.hip: constant %s not found (pattern %r)" % (k, p))
        out[k] = int(m.group(1))
    for k, macro in (("kWinB", "APE_LZ4_DWIN"), ("kKeep", "APE_LZ4_DKEEP"), ("kStage", "APE_LZ4_DSTAGE")):
        if not re.search(r"constexpr \w+ %s = %s;" % (k, macro), text):
            raise RuntimeError("lz4_decode.hip: %s is no longer %s" % (k, macro))
    return out


CONST = _constants()
POISON = -1


def single_batch(ndesc, csize):
    return ndesc <= CONST["kBatch"] - 1 and csize <= CONST["kStage"] - CONST["kWinNeed"]


def segments(B1, da=0):
    """copy_batch for B0 = 0, last = true: [(S0, S1, base, gdone)].  da = dst address & 15."""
    W, Kp = CONST["kWinB"], CONST["kKeep"]
    base = fl = gdone = S0 = 0
    out = []
    while S0 < B1:
        if B1 > base + W and S0 >= base + Kp + 16:
            gdone = fl
            base = (S0 - Kp) & ~15
        S1 = min(B1, base + W)
        out.append((S0, S1, base, gdone))
        sa = (S1 + da) & ~15
        F1 = S1 if S1 == B1 else (sa - da if sa > da else 0)
        if F1 > fl:
            fl = F1
        S0 = S1
    return out


class Piece:
    """The part of one sequence's match that one segment produces."""
    __slots__ = ("seg", "seq", "ma", "nm", "off", "ps", "cls", "rnd", "cut", "base", "gdone", "need")

    def label(self):
        return "%s[%s%s]" % (self.cls, "r1" if self.rnd == 0 else "pass%d" % self.rnd,
                             ",cut" if self.cut else "")


def _name(off, nm, ps, pe0, base, lp, ovl, inw, ing, lenok):
    if off == 0:
        return "zero.lane" if lenok else "zero.wave"
    if lp:
        return "lane.overlap" if ovl else "lane.win" if inw else "lane.hist" if ing else "lane.dict"
    if nm > CONST["kLaneMax"]:
        if off < 64:
            return "wave.long.per-dict" if ps < 0 else "wave.long.per"
        if ps >= base:
            return "wave.long.win"
        if ps < 0:
            return "wave.long.dict" if pe0 <= 0 else "wave.long.straddle-dict"
        return "wave.long.hist" if pe0 <= base else "wave.long.straddle-base"
    if nm < 4:
        return "wave.cut"
    if ps < 0:
        return "wave.dict-overlap" if ovl else "wave.dict-end"
    if ovl:
        return "wave.off<16" if off < 16 else "wave.overlap-below-base"
    return "wave.straddle-base" if pe0 > base else "wave.hist-cap"


CLASSES = ("zero.lane", "zero.wave", "lane.win", "lane.hist", "lane.dict", "lane.overlap",
           "wave.long.per", "wave.long.per-dict", "wave.long.win", "wave.long.hist",
           "wave.long.straddle-base", "wave.long.dict", "wave.long.straddle-dict", "wave.cut",
           "wave.off<16", "wave.dict-end", "wave.dict-overlap", "wave.overlap-below-base",
           "wave.straddle-base", "wave.hist-cap")

FAULTS = {
    "overlap-read-all": "self-overlap 16 <= off < n <= 64 copied read-all-then-write",
    "lpo8": "offsets 8..15 taken by the 16-byte unit-after-unit copy",
    "per32": "the periodic whole-wave form limited to off < 32",
    "round-up": "the last unit rounded up to 16 bytes: clobbers the following literal",
    "base-from-window": "a source straddling the window base read wholly from the window",
    "dict-one-side": "a source straddling the dictionary's end read wholly from the dictionary",
    "cut-restart": "a cut match's second piece restarts from the match's first source byte",
    "early": "a dependent match run one pass early",
}
# the classes a fault may change the output of (a block without one decodes as before)
FAULT_CLASSES = {
    "overlap-read-all": ("lane.overlap",),
    "lpo8": ("wave.off<16",),
    "per32": ("wave.long.per", "wave.long.per-dict", "wave.off<16", "wave.cut", "wave.dict-overlap",
              "wave.dict-end"),
    "round-up": ("lane.win", "lane.hist", "lane.dict", "lane.overlap", "zero.lane"),
    "base-from-window": ("wave.long.straddle-base",),
    "dict-one-side": ("wave.long.straddle-dict", "wave.long.per-dict", "wave.dict-end",
                      "wave.dict-overlap", "wave.cut"),
    "cut-restart": None,     # any class, on a cut piece
    "early": None,           # any lane class in a dependent pass
}


def simulate(seqs, tail, dict_size=None, da=0, fault=None, history=b"", cap=None):
    """The copy phase of a single-batch block, segment by segment in the kernel's order, on a
    byte array in which an unwritten byte is POISON.  Returns (pieces, output list).
    dict_size: None = the plain instantiation, else the dictionary instantiation (history =
    the dictionary's bytes).  fault: a key of FAULTS, the class slipping; None = the kernel."""
    from decseq import layout
    lay = layout(seqs, tail)
    nd = len(lay)
    B1 = lay[-1][1]
    assert fault is None or fault in FAULTS
    dict_mode = dict_size is not None
    hist = history[-65536:] if dict_mode else b""
    cap = B1 if cap is None else cap
    lane_max = CONST["kLaneMax"]
    out = [POISON] * (B1 + 80)
    lits = [s[0] for s in seqs] + [tail]
    offs = [s[1] for s in seqs] + [0]
    starts = [l[0] for l in lay] + [B1] * (64 - nd)
    islit = bytearray(B1 + 80)
    if fault == "round-up":
        for o, m, _ in lay:
            islit[o:m] = b"\1" * (m - o)
    pieces = []

    def owner(x):
        k, st = 0, 32
        while st >= 1:
            if starts[k + st] <= x:
                k += st
            st >>= 1
        return k

    for si, (S0, S1, base, gdone) in enumerate(segments(B1, da)):
        def rd(p):   # window (>= base), drained dst history (< base) or the dictionary (< 0)
            if p >= 0:
                return out[p]
            return hist[p] if dict_mode and -p <= len(hist) else POISON

        lanes = []
        for k in range(nd):
            o, m, me = lay[k]
            ma, mb = max(m, S0), min(me, S1)
            nm = mb - ma if mb > ma else 0
            if not nm:
                continue
            off = offs[k]
            ps = ma - off
            off0 = off == 0
            ovl = not off0 and off < nm
            pe0 = ps + nm
            inw = ps >= base
            ing = pe0 <= gdone and (nm >= 16 or ps + 16 <= cap) and (not dict_mode or ps >= 0)
            ind = dict_mode and ps + max(nm, 16) <= 0
            lpo = off >= (8 if fault == "lpo8" else 16) and inw
            lenok = 4 <= nm <= lane_max
            lp = lenok and (off0 or (ovl and lpo) or (not ovl and (inw or ing or ind)))
            pe = -(1 << 31) if off0 else (ma if ovl else pe0)
            r1 = lp and pe <= S0
            P = Piece()
            P.seg, P.seq, P.ma, P.nm, P.off, P.ps = si, k, ma, nm, off, ps
            P.base, P.gdone = base, gdone
            P.cut = m < S0 or me > S1
            P.cls = _name(off, nm, ps, pe0, base, lp, ovl, inw, ing, lenok)
            P.rnd = 0 if r1 else None
            need = ()
            if not r1 and k > 0:
                k0, k1 = owner(max(ps, S0)), min(owner(pe - 1), k - 1)
                need = range(k0, k1 + 1)
            P.need = len(need)     # sequences of this segment the pass loop waits for
            src0 = ps if not (fault == "cut-restart" and ma > m) else m - off
            lanes.append((k, P, lp, ovl, need, src0))
            pieces.append(P)

        def lane_copy(P, ovl, src0, loaded=None):
            ma, nm = P.ma, P.nm
            if P.off == 0:
                vals = [0] * nm
            elif ovl and fault != "overlap-read-all":
                ts = [0] + [t for t, u in ((min(16, nm - 16), nm > 16), (min(32, nm - 16), nm > 32),
                                           (nm - 16, nm > 48)) if u]
                for t in ts:    # unit after unit: 16 bytes read, 16 bytes written
                    v = [rd(src0 + t + i) for i in range(16)]
                    out[ma + t:ma + t + 16] = v
                vals = None
            else:
                vals = loaded if loaded is not None else [rd(src0 + i) for i in range(nm)]
            if vals is not None:
                out[ma:ma + nm] = vals
            if fault == "round-up":
                for p in range(ma + nm, ma + (nm + 15) // 16 * 16):
                    if p < S1 and islit[p]:
                        out[p] = POISON

        def coop(P, src0):
            ma, nm, off = P.ma, P.nm, P.off
            if off == 0:
                out[ma:ma + nm] = [0] * nm
                return
            per = off < (32 if fault == "per32" else 64)
            straddle_b = fault == "base-from-window" and P.ps < base < P.ps + nm
            straddle_d = fault == "dict-one-side" and P.ps < 0 < P.ps + nm
            for t0 in range(0, nm, 64):
                if not per and src0 + t0 >= 0 and not straddle_b and not straddle_d:
                    out[ma + t0:ma + min(t0 + 64, nm)] = out[src0 + t0:src0 + min(t0 + 64, nm)]
                    continue
                v = []
                for t in range(t0, min(t0 + 64, nm)):
                    sp = src0 + (t % off if per else t)
                    if (straddle_b and 0 <= sp < base) or (straddle_d and sp >= 0):
                        v.append(POISON)
                    else:
                        v.append(rd(sp))
                out[ma + t0:ma + t0 + len(v)] = v

        # round 1: sources read, then the literals, then the stores
        loaded = {}
        for k, P, lp, ovl, need, src0 in lanes:
            if P.rnd == 0 and P.off and not (ovl and fault != "overlap-read-all"):
                loaded[k] = [rd(src0 + i) for i in range(P.nm)]
        for k in range(nd):
            o, m, _ = lay[k]
            la, lb = max(o, S0), min(m, S1)
            if lb > la:
                out[la:lb] = lits[k][la - o:lb - o]
        for k, P, lp, ovl, need, src0 in lanes:
            if P.rnd == 0:
                lane_copy(P, ovl, src0, loaded.get(k))
        pend = [x for x in lanes if x[1].rnd is None]
        done = set(range(64)) - {x[0] for x in pend}
        npass = 0
        while pend:
            npass += 1
            ready = [x for x in pend if x[2] and all(j in done for j in x[4])]
            if ready:
                if fault == "early":
                    after = done | {x[0] for x in ready}
                    early = [x for x in pend if x not in ready and x[2] and all(j in after for j in x[4])]
                    got = {x[0]: [rd(x[5] + i) for i in range(x[1].nm)] for x in early}
                    ready = ready + early
                else:
                    got = {}
                for k, P, lp, ovl, need, src0 in ready:
                    P.rnd = npass
                    lane_copy(P, ovl and k not in got, src0, got.get(k))
                    done.add(k)
            else:
                k, P, lp, ovl, need, src0 = pend[0]
                assert not lp
                P.rnd = npass
                coop(P, src0)
                done.add(k)
            pend = [x for x in pend if x[0] not in done]
    return pieces, out[:B1]


def classify(seqs, tail, dict_size=None, da=0):
    """[Piece] of a single-batch block (class, round 1 or pass number, cut by a segment edge)."""
    return simulate(seqs, tail, dict_size, da)[0]
