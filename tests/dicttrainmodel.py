"""The dictionary trainer's rule (APE_LZ4_dict_train_dev): this file is the
definition, and lz4_dict_train.hip is held to it byte for byte.

train(samples, capacity, segment, max_sample) -> (dictionary, info)

  Counts.  freq[idx] = number of positions p with p + 8 <= size_i, over all used samples, whose
  8 bytes have table index idx = (u64 little-endian * PRIME mod 2^64) >> (64 - F).  A sample
  with a negative size is empty; one larger than max_sample is ignored (no counts, no slots).
  Slots.  st = segment / 4, J = ceil(max_sample / st).  Slot c = i * J + j is the segment
  [j * st, j * st + n) of sample i, n = min(segment, size_i - j * st); empty when n < 8.
  Score.  The sum of freq[idx] over the DISTINCT indices of the slot's n - 7 substrings.
  Rounds.  E = capacity // segment rounds; round e looks at the slots [e * M // E,
  (e + 1) * M // E), M = nsamples * J, and picks the highest score, the lowest slot on a tie,
  nothing at score 0.  A pick sets freq[idx] = 0 for every substring of its segment.
  Layout.  Pick 0 is the dictionary's last bytes, pick r ends where pick r - 1 begins, and
  capacity - u zero bytes come first.
  info = [u, picks, samples ignored, 0].

Rule's other fields describe the wrong neighbours tests/test_dict_train_model.py tells the rule
from; corpus() is the quality corpus of that test, of tests/test_gpu_dict_train.py and of
tools/dict_train_bench.py."""
import collections

import numpy as np

D = 8                        # bytes of a counted substring
F = 20                       # the count table has 2^F entries
PRIME = 0x9E3779B185EBCA87
TABLE = 1 << F

Rule = collections.namedtuple(
    "Rule", "distinct zeroing low_tie back_to_front within_sample cut_n")
# distinct: "index" (the rule), "string" or "none" (every occurrence)
RULE = Rule(distinct="index", zeroing=True, low_tie=True, back_to_front=True, within_sample=True,
            cut_n=True)


def index_of(eight):
    """The table index of 8 bytes."""
    assert len(eight) == D
    return ((int.from_bytes(eight, "little") * PRIME) & ((1 << 64) - 1)) >> (64 - F)


def _words(b):
    """The u64 little-endian value of every 8-byte substring of b."""
    a = np.frombuffer(b, dtype=np.uint8)
    n = len(a) - (D - 1)
    if n <= 0:
        return np.zeros(0, np.uint64)
    v = np.zeros(n, np.uint64)
    for j in range(D):
        v |= a[j:j + n].astype(np.uint64) << np.uint64(8 * j)
    return v


def _indices(words):
    return ((words * np.uint64(PRIME)) >> np.uint64(64 - F)).astype(np.int64)


def geometry(nsamples, capacity, segment, max_sample):
    """(st, J, M, E) -- host-known numbers only."""
    st = segment // 4
    J = -(-max_sample // st)
    return st, J, nsamples * J, capacity // segment


def train(samples, capacity, segment, max_sample, sizes=None, rule=RULE):
    """samples: byte strings; sizes (optional): the size the caller states for each, which may be
    negative, or smaller than the buffer."""
    k = segment
    assert k % 16 == 0 and 16 <= k <= 1024 and k <= capacity <= 65536 and max_sample >= D
    sizes = [len(s) for s in samples] if sizes is None else list(sizes)
    st, J, M, E = geometry(len(samples), capacity, k, max_sample)
    ignored = sum(1 for z in sizes if z > max_sample)
    data = [b"" if z > max_sample else bytes(s[:max(z, 0)]) for s, z in zip(samples, sizes)]
    if not rule.within_sample or not rule.cut_n:
        # the wrong neighbours read on into the samples that follow
        after = [b""] * (len(data) + 1)
        for i in range(len(data) - 1, -1, -1):
            after[i] = (data[i] + after[i + 1])[:len(data[i]) + 2 * 1024]
    W = [_words(d) for d in data]
    H = [_indices(w) for w in W]
    freq = np.zeros(TABLE, np.int64)
    for i, h in enumerate(H):
        if not rule.within_sample and len(data[i]):
            h = _indices(_words(after[i][:len(data[i]) + D - 1]))
        np.add.at(freq, h, 1)

    def segment_of(c):
        i, j = divmod(c, J)
        s = j * st
        n = min(k, len(data[i]) - s)
        if n < D:
            return None
        if rule.cut_n:
            return i, s, n, W[i][s:s + n - 7], data[i][s:s + n]
        b = after[i][s:s + k]
        return i, s, len(b), _words(b), b

    picks = []
    for e in range(E):
        best, best_c = 0, -1
        for c in range(e * M // E, (e + 1) * M // E):
            seg = segment_of(c)
            if seg is None:
                continue
            w = seg[3]
            if rule.distinct == "index":
                score = int(freq[np.unique(_indices(w))].sum())
            elif rule.distinct == "string":
                score = int(freq[_indices(np.unique(w))].sum())
            else:
                score = int(freq[_indices(w)].sum())
            if score > best or (not rule.low_tie and score == best and score > 0):
                best, best_c = score, c
        if best_c >= 0:
            seg = segment_of(best_c)
            picks.append(seg[4])
            if rule.zeroing:
                freq[_indices(seg[3])] = 0
    u = sum(map(len, picks))
    body = b"".join(reversed(picks) if rule.back_to_front else picks)
    return bytes(capacity - u) + body, [u, len(picks), ignored, 0]


# ---- the quality corpus: messages built from a pool of 3000 lower-case phrases of 24..64
# bytes, drawn with probability ~ 1 / rank, with a run of 4..19 random bytes a quarter of the
# time; the pool is the same for every seed, so held-out messages share it ----
_POOL = []


def _pool(P=3000):
    if not _POOL:
        r = np.random.RandomState(1234)
        phrases = [r.randint(97, 123, size=r.randint(24, 65), dtype=np.uint8).tobytes()
                   for _ in range(P)]
        w = 1.0 / np.arange(1, P + 1) ** 1.0
        w /= w.sum()
        cdf = w.cumsum()
        cdf /= cdf[-1]
        _POOL.extend([phrases, cdf])
    return _POOL


def corpus(n, length, seed):
    """n messages of `length` bytes.  (The phrase draw is RandomState.choice(P, p=w) written out:
    one uniform double looked up in the cumulative weights.)"""
    phrases, cdf = _pool()
    r = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        parts, size = [], 0
        while size < length:
            if r.rand() < 0.25:
                b = r.randint(0, 256, size=r.randint(4, 20), dtype=np.uint8).tobytes()
            else:
                b = phrases[int(cdf.searchsorted(r.random_sample(), side="right"))]
            parts.append(b)
            size += len(b)
        out.append(b"".join(parts)[:length])
    return out


def naive(samples, capacity, tail=False):
    """What a caller without a trainer does: the samples' first (or last) `capacity` bytes."""
    cat = b"".join(samples)
    return cat[-capacity:] if tail else cat[:capacity]


# the rows of the quality table: samples x bytes -> capacity, segment; trained on corpus(.., 1),
# judged on the 128 messages of corpus(128, .., 2)
QUALITY = ((512, 1024, 16384, 64), (256, 512, 8192, 64), (64, 256, 2048, 32))
