"""A Python model of the placed framed decode (include/ape_lz4f_placed.h): the
result of APE_LZ4_lz4f_decompress_placed_batch_dev, codes included, and a frame writer for the
tests.  It imports tests/lz4fmodel.py for the header, the walk, XXH32 and the block decoder,
and is the definition of what differs: a block may decode to any size up to the block
maximum, so every block is sized first and placed at the sum of the sizes before it.

decode_placed()'s codes, the first of the list that applies:
  -1, -3, -2, ERANGE  the header stage, as lz4fmodel.decode
  -4 a block has no decoded size: it does not decode into the block maximum -- with NO history
     for a block of an independent frame, with 64 KiB of ANY history for one of a linked frame
     (a block's size does not depend on what its offsets reach, and the true history of a linked
     block is only known once the blocks before it are sized)
  -9 capacity below the sum of the sizes (not below blocks x maximum)
  -8 content size mismatch
    -- up to here nothing of the destination is written --
  -6 block checksum; -4 a block fails to decode into exactly its size with its true history
  (a match of a linked block that reaches before the frame's start); -7 content checksum.
-5 does not occur.  Against lz4fmodel.decode: -4 from sizing, -9 and -8 come before -6, because
they are decided before anything is written; on frames that the existing call takes, with a
capacity of at least blocks x maximum, the two agree.

lz4fmodel.block_decode takes no side on malformed blocks, so every block of a fixture or a
test is well-formed or broken in a way both it and the reference decoder reject."""
import base64
import collections
import functools
import json
import os
import struct

import encmodel
import lz4fmodel as M

ERANGE = M.ERANGE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "lz4f_flush_golden.json")
ANY_HISTORY = bytes(65536)


def block_size(body, bmax, linked):
    """The decoded size of a compressed block, or None."""
    out = M.block_decode(body, bmax, ANY_HISTORY if linked else b"")
    return None if out is None else len(out)


def sizes(frame, head, blocks):
    linked = not head.flg & M.F_INDEP
    return [b.size if b.stored else block_size(frame[b.at:b.at + b.size], head.bmax, linked)
            for b in blocks]


def decode_placed(frame, cap, max_blocks=1 << 20, flags=0, wrong=None):
    """(result, bytes or None) of APE_LZ4_lz4f_decompress_placed_batch_dev for one frame.
    wrong: a wrong neighbour for the tests -- "grid": block q at q x maximum (the existing
    call's placement); "history": a linked block's history stops at the start of the block
    before it; "bound": -9 against blocks x maximum."""
    code, head, blocks, end, _ = M._stage(frame, bool(flags & M.NO_LINKED))
    if code:
        return code, None
    if len(blocks) > max_blocks:
        return ERANGE, None
    measured = sizes(frame, head, blocks)
    if any(n is None for n in measured):
        return -4, None
    total = sum(measured)
    if cap < (len(blocks) * head.bmax if wrong == "bound" else total):
        return -9, None
    if head.content_size is not None and head.content_size != total:
        return -8, None
    verify = not flags & M.NO_VERIFY
    linked = not head.flg & M.F_INDEP
    image = bytearray(total if wrong != "grid" else len(blocks) * head.bmax)
    pos, got, starts = 0, [], []
    for q, (b, n) in enumerate(zip(blocks, measured)):
        body = frame[b.at:b.at + b.size]
        at = q * head.bmax if wrong == "grid" else pos
        starts.append(at)
        if b.stored:
            out = body
        else:
            history = b""
            if linked:
                low = starts[-2] if wrong == "history" and q else 0
                history = bytes(image[max(low, at - 65536):at])
            out = M.block_decode(body, n, history)
            if out is not None and len(out) != n:
                out = None
        got.append(out)
        if out is not None:
            image[at:at + n] = out
        pos += n
    if verify and head.flg & M.F_BSUM:
        for b in blocks:
            if M.xxh32(frame[b.at:b.at + b.size]) != b.want:
                return -6, None
    if any(out is None for out in got):
        return -4, None
    content = bytes(image[:total])
    if verify and head.flg & M.F_CSUM and \
            M.xxh32(content) != struct.unpack_from("<I", frame, end - 4)[0]:
        return -7, None
    return total, content


def has_short_middle_block(frame):
    """Whether a block before the last decodes to less than the block maximum: the frames the
    existing call answers with -5."""
    code, head, blocks, _, _ = M._stage(frame)
    assert code == 0
    return any(n != head.bmax for n in sizes(frame, head, blocks)[:-1])


# ---------------- a frame writer for the tests ----------------
@functools.lru_cache(maxsize=512)
def _encode(piece, prefix):
    return encmodel.encode(piece, prefix)


def frame_of(pieces, linked=False, bsid=4, block_sums=False, content_sum=False,
             content_size=False):
    """A frame with one block per piece (bytes, at most 64 KiB each: the encoder model's limit),
    as a producer that flushes after every piece writes it: independent blocks, or linked ones
    whose matches reach into the pieces before (as far as the encoder's 64 KiB window of history
    + piece allows); a piece the encoder does not shrink is stored; an empty piece writes no
    block."""
    content = b"".join(pieces)
    flg = 0x40 | (0 if linked else M.F_INDEP) | (M.F_BSUM if block_sums else 0) | \
        (M.F_SIZE if content_size else 0) | (M.F_CSUM if content_sum else 0)
    out = [M.frame_header(flg, bsid, len(content) if content_size else None)]
    at = 0
    for piece in pieces:
        piece = bytes(piece)
        assert len(piece) <= min(M.BLOCK, M.block_max(bsid))
        if not piece:
            continue
        room = M.BLOCK - len(piece)
        prefix = content[max(0, at - room):at] if linked and room else b""
        comp = _encode(piece, prefix)
        if len(comp) <= len(piece) - 1:
            body, word = comp, len(comp)
        else:
            body, word = piece, len(piece) | 0x80000000
        out.append(struct.pack("<I", word) + body)
        if block_sums:
            out.append(struct.pack("<I", M.xxh32(body)))
        at += len(piece)
    out.append(struct.pack("<I", 0))
    if content_sum:
        out.append(struct.pack("<I", M.xxh32(content)))
    return b"".join(out)


# ---------------- fixtures (tests/golden/lz4f_flush_golden.json) ----------------
def pieces_of(content, lengths):
    out, at = [], 0
    for n in lengths:
        out.append(content[at:at + n])
        at += n
    assert at == len(content)
    return out


@functools.lru_cache(maxsize=1)
def fixtures():
    """name -> dict(frame, content, pieces (lengths), bsid, linked, block_sums, content_sum,
    content_size): frames liblz4 wrote with a flush after every piece."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = collections.OrderedDict()
    for fx in doc["frames"]:
        fx = dict(fx)
        fx["frame"] = base64.b64decode(fx.pop("frame_b64"))
        fx["content"] = M.content_of(fx["parts"])
        if fx["repeat_to"] is not None:   # the recipe is a unit, repeated up to so many bytes
            unit, n = fx["content"], fx["repeat_to"]
            fx["content"] = (unit * (n // len(unit) + 1))[:n]
        assert len(fx["content"]) == sum(fx["pieces"])
        out[fx["name"]] = fx
    return out


def blocks_of(frame):
    code, _, blocks, _, _ = M._stage(frame)
    assert code == 0
    return len(blocks)
