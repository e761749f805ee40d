"""A Python model of framed compress with preferences (include/ape_lz4f_prefs.h):
the frame APE_LZ4_lz4f_compress_prefs_batch_dev writes for (input, blockSizeID, mode, depth,
flags).  This file is its definition, built from existing parts only: the frame pieces of
tests/lz4fmodel.py (frame_header, xxh32, block_max) and the block bytes of the large-input calls
-- mode 0: tests/encmodel.py, above 65536 bytes its slices at multiples of S with the bytes before
them as history, stitched by tests/indexutil.py; mode 1: tests/hclargemodel.py; mode 2:
tests/hcoptmodel.py.  No product or oracle code.

The frame: version 01, block-independent, no dictionary ID, BD = blockSizeID << 4; ceil(n / B)
blocks of B = block_max(blockSizeID) bytes, the last shorter; a block is the mode's bytes when
they take at most len - 1 (the large call's capacity), else it is stored."""
import collections
import functools
import struct

import encmodel
import hclargemodel
import hcoptmodel
import indexutil
import lz4fmodel as F

SLICE = 32768    # S of the CPU tests; the GPU tests pass compress_large_slice_size()
ERANGE = F.ERANGE

# The rule, and the handles by which tests/test_lz4f_prefs_model.py moves it to its wrong
# neighbours: the ID that BD names (None: the one the blocks are cut by), where the blocks are
# cut (None: at the block maximum), and how far below the block's length its encoder's
# capacity lies.
Rule = collections.namedtuple("Rule", "bd_id cut slack")
RULE = Rule(bd_id=None, cut=None, slack=1)


@functools.lru_cache(maxsize=256)
def _xxh32(data):
    return F.xxh32(data)


@functools.lru_cache(maxsize=256)
def block_bytes(block, mode, depth=0, S=SLICE):
    """What the mode's large-input call writes for `block` with room for all of it."""
    assert mode in (0, 1, 2) and 0 <= depth <= 256 and (mode or not depth)
    depth = depth or 64
    if mode == 1:
        return hclargemodel.compress_large(block, depth, S=S)
    if mode == 2:
        return hcoptmodel.compress_large(block, depth, S=S)
    if len(block) <= 65536:
        return encmodel.encode(block)
    return indexutil.stitch([encmodel.encode(block[st:st + S], prefix=block[:st])
                             for st in range(0, len(block), S)])


def frame_block(block, mode, depth, block_sums, S=SLICE, rule=RULE):
    block = bytes(block)
    comp = block_bytes(block, mode, depth, S)
    if len(comp) <= len(block) - rule.slack:
        body, word = comp, len(comp)
    else:
        body, word = block, len(block) | 0x80000000
    out = struct.pack("<I", word) + body
    if block_sums:
        out += struct.pack("<I", _xxh32(body))
    return out


def compress(data, bsid, mode=0, depth=0, flags=0, S=SLICE, rule=RULE):
    """The frame APE_LZ4_lz4f_compress_prefs_batch_dev writes."""
    assert 4 <= bsid <= 7 and 0 <= flags <= 7 and len(data) <= F.MAX_SRC
    data = bytes(data)
    flg = 0x40 | F.F_INDEP | (F.F_BSUM if flags & F.BLOCK_CHECKSUMS else 0) | \
        (F.F_SIZE if flags & F.CONTENT_SIZE else 0) | (F.F_CSUM if flags & F.CONTENT_CHECKSUM else 0)
    out = [F.frame_header(flg, bsid if rule.bd_id is None else rule.bd_id,
                          len(data) if flags & F.CONTENT_SIZE else None)]
    B = F.block_max(bsid) if rule.cut is None else rule.cut
    for at in range(0, len(data), B):
        out.append(frame_block(data[at:at + B], mode, depth, bool(flags & F.BLOCK_CHECKSUMS), S,
                               rule))
    out.append(struct.pack("<I", 0))
    if flags & F.CONTENT_CHECKSUM:
        out.append(struct.pack("<I", _xxh32(data)))
    return b"".join(out)


def result(data, size, cap, max_src, bsid, mode=0, depth=0, flags=0, S=SLICE):
    """(d_result, the bytes written) for an input whose d_srcSize is `size`."""
    if size < 0:
        return 0, b""
    if size > max_src:
        return ERANGE, b""
    frame = compress(data[:size], bsid, mode, depth, flags, S)
    return (len(frame), frame) if len(frame) <= cap else (0, b"")


def compress_bound(n, bsid, flags):
    """APE_LZ4_lz4f_compress_prefs_bound: every block stored."""
    if not 0 <= n <= F.MAX_SRC or not 4 <= bsid <= 7 or not 0 <= flags <= 7:
        return 0
    B = F.block_max(bsid)
    return (15 if flags & F.CONTENT_SIZE else 7) + n + (n + B - 1) // B * \
        (8 if flags & F.BLOCK_CHECKSUMS else 4) + (8 if flags & F.CONTENT_CHECKSUM else 4)


def blocks_of(frame):
    """[(the block's bytes in the frame, stored)] of a frame this model wrote."""
    code, head = F.header(frame)
    assert code == 0
    code, blocks, _ = F.walk(frame, head)
    assert code == 0
    return [(frame[b.at:b.at + b.size], b.stored) for b in blocks]


def edge(tail):
    """A block of 75 + tail bytes: 64 random bytes, their first 11 again, then `tail` more random
    ones.  All three encoders find the one match, and the three literal-length bytes of the last
    run eat what it saves: with tail 1289 every mode's block takes len - 1 bytes and goes in
    compressed, with 1290 it takes exactly len and is stored by that one byte."""
    r = F.content_of([["rand", 4000, 0, 4000]])
    return r[:64] + r[:11] + r[64:64 + tail]


# ---------------- the cases of tests/golden/lz4f_prefs_golden.json ----------------
# name, the content's recipe (lz4fmodel.content_of), ID, mode, depth, flags
CASES = [
    ("id4_fast_text", [["text", 3000, 1, 200000]], 4, 0, 0, 7),
    ("id5_fast_text_tail", [["text", 3000, 1, 2 * 262144 + 777]], 5, 0, 0, 0),
    ("id5_fast_stored_middle", [["text", 3000, 2, 262144], ["rand", 262144, 9, 262144],
                                ["text", 3000, 3, 777]], 5, 0, 0, 7),
    ("id5_hc_text_tail", [["text", 3000, 1, 262144 + 777]], 5, 1, 8, 7),
    ("id5_hc_stored_middle", [["comp", 262144, 4, 262144], ["rand", 262144, 9, 262144],
                              ["text", 3000, 3, 777]], 5, 1, 8, 3),
    ("id5_opt_text_tail", [["text", 3000, 1, 262144 + 777]], 5, 2, 8, 7),
    ("id5_opt_comp", [["comp", 300000, 5, 300000]], 5, 2, 8, 0),
    ("id5_hc_default_depth", [["comp", 70000, 6, 70000]], 5, 1, 0, 4),
    ("id6_fast_comp", [["comp", 1048576 + 13, 7, 1048576 + 13]], 6, 0, 0, 7),
    ("id6_hc_text", [["text", 5000, 8, 400000]], 6, 1, 8, 2),
    ("id7_fast_text", [["text", 3000, 1, 4194304 + 1]], 7, 0, 0, 1),
    ("id7_empty", [], 7, 2, 8, 7),
    ("id5_random_tail_byte", [["text", 3000, 1, 262144], ["rand", 1, 3, 1]], 5, 0, 0, 7),
]
