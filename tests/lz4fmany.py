"""Frames of more than 64 blocks for the tests of the two framed decodes: both step over a
frame's blocks 64 at a time, and these are the inputs that reach the second chunk and the
third.  Built with lz4fplacedmodel.frame_of, once per session; tests/test_lz4f_placed_model.py
checks on the CPU that they are what the GPU tests take them to be.  No product code."""
import functools
import struct

import decseq
import lz4fmodel as M
import lz4fplacedmodel as P

COUNTS = (64, 65, 130)
SHORT_BLOCKS = 130     # max_blocks for the 13-byte pieces: a one-block frame leaves 129 absent
BIG_BLOCKS = 67        # max_blocks for the full blocks


@functools.lru_cache(maxsize=1)
def text():
    return M.content_of([["text", 7000, 1, 66000]])


def pieces(count):
    return [text()[(13 * k) % 5000:][:13] for k in range(count)]


def bound(frame):
    """blocks x maximum (at least the declared size, at least 1): room for the existing call."""
    inf = M.info(frame)
    return max(inf[5], inf[3] * inf[2], 1)


@functools.lru_cache(maxsize=1)
def short_frames():
    """[(frame, content)]: 64, 65 and 130 pieces of 13 bytes, independent and linked, with block
    checksums, content checksum and content size."""
    return [(P.frame_of(pieces(n), linked=linked, block_sums=True, content_sum=True,
                        content_size=True), b"".join(pieces(n)))
            for n in COUNTS for linked in (False, True)]


def one_block():
    """(frame, content) of one block: in a batch of SHORT_BLOCKS its other slots are absent."""
    return P.frame_of([text()[:13]], block_sums=True, content_sum=True, content_size=True), \
        text()[:13]


def _block(frame, q):
    _, head = M.header(frame)
    return M.walk(frame, head)[1][q]


def unsized_block_70():
    """The 130-piece independent frame, block 70 now a compressed block whose match starts 12
    bytes before the block (its checksum redone): the sizer has no size for it."""
    frame = short_frames()[4][0]
    body, _ = decseq.build([(b"abcdefgh", 20, 8)], b"x" * 16, strict=False)
    b = _block(frame, 70)
    new = struct.pack("<I", len(body)) + body + struct.pack("<I", M.xxh32(body))
    return frame[:b.at - 4] + new + frame[b.at + b.size + 4:]


def flipped_block_100():
    """The 130-piece linked frame with the last literal of block 100 flipped."""
    frame = bytearray(short_frames()[5][0])
    b = _block(frame, 100)
    frame[b.at + b.size - 1] ^= 0x40
    return bytes(frame)


@functools.lru_cache(maxsize=1)
def big_frames():
    """[(frame, content, whether a block before the last is short)]: 65 full blocks and one of
    100 bytes, then the same with a 100-byte piece at index 64; each independent and linked,
    with a content checksum."""
    unit = text()[:65536]
    full = [unit] * 65 + [text()[:100]]
    gap = full[:64] + [text()[:100]] + full[64:]
    return [(P.frame_of(p, linked=linked, content_sum=True), b"".join(p), p is gap)
            for p in (full, gap) for linked in (False, True)]


@functools.lru_cache(maxsize=1)
def big_results():
    """[(lz4fmodel.decode, decode_placed)] of big_frames() at capacity bound(frame): the models
    run once for the CPU and the GPU tests."""
    return [(M.decode(f, bound(f), BIG_BLOCKS), P.decode_placed(f, bound(f), BIG_BLOCKS))
            for f, _, _ in big_frames()]
