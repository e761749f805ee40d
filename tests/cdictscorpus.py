"""The corpus of the dictionary-per-message tests: a mixed batch whose messages
depend on WHICH dictionary they are compressed against.  Two sets of four dictionaries, the
messages of each cut from the text right after their own dictionary and assigned round-robin
(message j belongs to dictionary j % 4), so neighbouring messages never share an object.

  content : four dictionaries of 60 KiB with different bytes -- two disjoint slices of
            tests/test_gpu_cdict.py's text and two of a second seed's -- at maxSrcSize 4096;
  size    : four dictionaries of different length that end at the same place of one text (0, 100,
            4095, 70000 bytes; 70000 is cut to the window), at maxSrcSize 4096.

tests/test_cdicts_corpus.py proves on the CPU that a kernel which took another set member's
object for a message would write different bytes."""
import functools

from lz4util import I

MAX_SRC = 4096
DICT_BYTES = 61440                      # 60 KiB: the whole window at maxSrcSize 4096
LENGTHS = (0, 1, 12, 13, 64, 65, 1000, 4096)
SIZES = (0, 100, 4095, 70000)
BASE = 70000                            # where the size set's dictionaries end
ROUNDS = 2                              # messages of every length per dictionary
TEXT = 200000


@functools.lru_cache(maxsize=None)
def text(seed):
    return I.make("comp", TEXT, seed=seed)


class Set:
    """dicts[k], and messages[j] assigned to dictionary owner[j]."""

    def __init__(self, name, dicts, after):
        self.name, self.dicts = name, dicts
        self.messages, self.owner = [], []
        pos = [0] * len(dicts)
        for r in range(ROUNDS):
            for L in LENGTHS:
                for k in range(len(dicts)):
                    src = after[k]
                    self.messages.append(src[pos[k]:pos[k] + L])
                    self.owner.append(k)
                    pos[k] += L
        assert min(len(a) for a in after) >= sum(LENGTHS) * ROUNDS

    def of(self, k):
        """indices of the messages assigned to dictionary k"""
        return [j for j, o in enumerate(self.owner) if o == k]

    def small(self, most=1000):
        """indices of the messages of at most `most` bytes (the CPU models' share)"""
        return [j for j, m in enumerate(self.messages) if len(m) <= most]


@functools.lru_cache(maxsize=None)
def content_set():
    slices = [(7, 0), (7, 100000), (11, 0), (11, 100000)]
    dicts = [text(s)[at:at + DICT_BYTES] for s, at in slices]
    after = [text(s)[at + DICT_BYTES:at + 100000] for s, at in slices]
    return Set("content", dicts, after)


@functools.lru_cache(maxsize=None)
def size_set():
    t = text(7)
    return Set("size", [t[BASE - dd:BASE] for dd in SIZES], [t[BASE:]] * len(SIZES))


def sets():
    return [content_set(), size_set()]
