"""A Python model of LZ4 frames with a dictionary (include/ape_lz4f_dict.h): the
ten ints of APE_LZ4_lz4f_info_dict_batch_dev, the frame
APE_LZ4_lz4f_compress_usingCDicts_batch_dev writes and the result of
APE_LZ4_lz4f_decompress_usingDicts_batch_dev, codes included.  It stands on tests/lz4fmodel.py
(header fields, walk, XXH32, block decoder) and tests/lz4fplacedmodel.py (sizing), and is the
definition of what differs.  The block bytes come from tests/encmodel.py encode_cdict,
tests/hcdictmodel.py and tests/hcoptdictmodel.py.  No product or oracle code.

The format: FLG bit 0 announces a le32 dictionary ID after the optional content size; the header
checksum covers it.  Every block of an independent frame has the dictionary's last 64 KiB as its
only history; the history of a block of a linked frame is the last 64 KiB of (dictionary ++
content so far).

decode()'s codes, the first that applies.  Without ANY_SIZE (the grid placement of lz4fmodel):
  -1, -3, -2, ERANGE  the header stage of lz4fmodel.decode; a dictionary ID is no reason for -3
  -10 the frame names an ID and the table's first entry with it is missing or unusable
  -9, -6, -4, -5, -8, -7  as lz4fmodel.decode
With ANY_SIZE (the placement of lz4fplacedmodel):
  -1, -3, -2, ERANGE, -10  as above
  -4 a block has no decoded size: with the dictionary as history for a block of an independent
     frame and for block 0 of a linked frame with a non-empty dictionary, else as lz4fplacedmodel
  -3 a linked frame with a non-empty dictionary has a later compressed block that starts below
     65536: its history would be the dictionary's tail and the output before it, which the block
     decoder does not take
  -9, -8, then -6, -4, -7  as lz4fplacedmodel
A frame's key is its ID, or 0 without the field; a frame without the field and without an entry
for key 0 is decoded with no dictionary.  An empty dictionary is no dictionary."""
import base64
import collections
import functools
import json
import os
import struct

import encmodel
import lz4fmodel as M
import lz4fplacedmodel as P

ERANGE = M.ERANGE
NO_DICTIONARY = -10
ANY_SIZE = 4                      # decompress flag: blocks of any size (the placed decode)
FAST, HC, HC_OPT = 0, 1, 2        # compress modes
DEFAULT_DEPTH = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "lz4f_dict_golden.json")


# ---------------- reading a frame ----------------
def header(frame, no_linked=False, ids_in_checksum=True):
    """(code, Head or None, the dictionary ID or None): lz4fmodel.header with the ID as a field.
    ids_in_checksum=False: the wrong neighbour whose header checksum stops before the ID."""
    n = len(frame)
    if n < 4:
        return -2, None, None
    magic = struct.unpack_from("<I", frame)[0]
    if magic & 0xFFFFFFF0 == M.SKIPPABLE or magic == M.LEGACY:
        return -3, None, None
    if magic != M.MAGIC:
        return -1, None, None
    if n < 6:
        return -2, None, None
    flg, bd = frame[4], frame[5]
    bsid = (bd >> 4) & 7
    if flg >> 6 != 1 or flg & M.F_RESERVED or bd & 0x8F or bsid < 4:
        return -1, None, None
    dn = 2 + (8 if flg & M.F_SIZE else 0) + (4 if flg & M.F_DICT else 0)
    if n < 4 + dn + 1:
        return -2, None, None
    covered = dn if ids_in_checksum or not flg & M.F_DICT else dn - 4
    if frame[4 + dn] != M.header_checksum(frame[4:4 + covered]):
        return -1, None, None
    size = struct.unpack_from("<Q", frame, 6)[0] if flg & M.F_SIZE else None
    if (no_linked and not flg & M.F_INDEP) or (size is not None and size >= 1 << 31):
        return -3, None, None
    dict_id = struct.unpack_from("<I", frame, 4 + dn - 4)[0] if flg & M.F_DICT else None
    return 0, M.Head(flg, M.block_max(bsid), 4 + dn + 1, size), dict_id


def _stage(frame, no_linked=False, ids_in_checksum=True):
    """(code, head, dictionary ID, blocks, frame bytes, bound)"""
    code, head, dict_id = header(frame, no_linked, ids_in_checksum)
    if code:
        return code, None, None, None, None, None
    code, blocks, end = M.walk(frame, head)
    if code:
        return code, None, None, None, None, None
    bound = head.content_size if head.content_size is not None else len(blocks) * head.bmax
    if bound >= 1 << 31:
        return -3, None, None, None, None, None
    return 0, head, dict_id, blocks, end, bound


def info(frame):
    """The ten ints of APE_LZ4_lz4f_info_dict_batch_dev."""
    code, head, dict_id, blocks, end, bound = _stage(frame)
    if code:
        return [code, 0, 0, 0, 0, 0, -1, -1, 0, 0]
    size = head.content_size
    return [0, head.flg, head.bmax, len(blocks), end, bound,
            -1 if size is None else M._i32(size & M.M32),
            -1 if size is None else M._i32(size >> 32),
            0 if dict_id is None else 1, 0 if dict_id is None else M._i32(dict_id)]


def pick(table, dict_id, missing_is_10=False):
    """(code, dictionary bytes): the table is [(key, bytes, or None for an unusable entry)]; the
    first entry with the frame's key counts.  missing_is_10: the wrong neighbour that refuses a
    frame without the field when the table has no entry for key 0."""
    key = dict_id or 0
    for k, d in table:
        if k == key:
            return (NO_DICTIONARY, None) if d is None else (0, bytes(d))
    if dict_id is not None or missing_is_10:
        return NO_DICTIONARY, None
    return 0, b""


def decode(frame, cap, table=(), max_blocks=1 << 20, flags=0, wrong=None):
    """(result, bytes or None) of APE_LZ4_lz4f_decompress_usingDicts_batch_dev for one frame.
    wrong: a wrong neighbour for the tests -- "block0": in an independent frame only block 0 gets
    the dictionary; "every_linked": every block of a linked frame gets the dictionary in place of
    the output before it; "no_id_sum": the header checksum stops before the ID; "first64k": the
    first 64 KiB of a longer dictionary; "missing": a frame without an ID and without an entry for
    key 0 is -10."""
    code, head, dict_id, blocks, end, bound = _stage(frame, bool(flags & M.NO_LINKED),
                                                     wrong != "no_id_sum")
    if code:
        return code, None
    if len(blocks) > max_blocks:
        return ERANGE, None
    code, dictionary = pick(table, dict_id, wrong == "missing")
    if code:
        return code, None
    dictionary = dictionary[:65536] if wrong == "first64k" else dictionary[-65536:]
    verify = not flags & M.NO_VERIFY
    linked = not head.flg & M.F_INDEP
    bodies = [frame[b.at:b.at + b.size] for b in blocks]

    def history(q, image, at):
        """of compressed block q, which starts at `at` of the output image"""
        if not linked:
            return dictionary if q == 0 or wrong != "block0" else b""
        if wrong == "every_linked" or (q == 0 and dictionary):
            return dictionary
        return bytes(image[max(0, at - 65536):at])

    if flags & ANY_SIZE:
        measured = []
        for q, (b, body) in enumerate(zip(blocks, bodies)):
            if b.stored:
                measured.append(b.size)
            elif not linked or (q == 0 and dictionary):
                out = M.block_decode(body, head.bmax, history(q, b"", 0))
                measured.append(None if out is None else len(out))
            else:
                measured.append(P.block_size(body, head.bmax, True))
        if any(n is None for n in measured):
            return -4, None
        starts = [sum(measured[:q]) for q in range(len(blocks))]
        if linked and dictionary and any(q and not b.stored and starts[q] < 65536
                                         for q, b in enumerate(blocks)):
            return -3, None
        total = sum(measured)
        if cap < total:
            return -9, None
        if head.content_size is not None and head.content_size != total:
            return -8, None
        image, got = bytearray(total), []
        for q, (b, body, n, at) in enumerate(zip(blocks, bodies, measured, starts)):
            out = body if b.stored else M.block_decode(body, n, history(q, image, at))
            if out is not None and len(out) != n:
                out = None
            got.append(out)
            if out is not None:
                image[at:at + n] = out
        if verify and head.flg & M.F_BSUM and any(M.xxh32(body) != b.want
                                                  for b, body in zip(blocks, bodies)):
            return -6, None
        if any(out is None for out in got):
            return -4, None
        content = bytes(image)
    else:
        if cap < bound:
            return -9, None
        image, got = bytearray(), []
        for q, (b, body) in enumerate(zip(blocks, bodies)):
            room = max(0, min(head.bmax, cap - q * head.bmax))
            if room:
                image += bytes(q * head.bmax - len(image))
            if b.stored:
                out = body if b.size <= room else None
            else:
                out = M.block_decode(body, room, history(q, image, len(image)))
            got.append(out)
            image += out or b""
        if verify and head.flg & M.F_BSUM and any(M.xxh32(body) != b.want
                                                  for b, body in zip(blocks, bodies)):
            return -6, None
        if any(out is None for out in got):
            return -4, None
        if any(len(out) != head.bmax for out in got[:-1]):
            return -5, None
        content = bytes(image)
        if head.content_size is not None and head.content_size != len(content):
            return -8, None
    if verify and head.flg & M.F_CSUM and \
            M.xxh32(content) != struct.unpack_from("<I", frame, end - 4)[0]:
        return -7, None
    return len(content), content


# ---------------- writing a frame ----------------
@functools.lru_cache(maxsize=1024)
def block_of(message, dictionary, max_src_size, mode, depth):
    """The block the mode's usingCDicts call gives `message` against an object prepared from
    `dictionary` for max_src_size."""
    if mode == FAST:
        return encmodel.encode_cdict(message, dictionary, max_src_size)
    if mode == HC:
        import hcdictmodel
        return hcdictmodel.compress(dictionary, message, max_src_size, depth or DEFAULT_DEPTH)
    import hcoptdictmodel
    return hcoptdictmodel.compress(dictionary, message, max_src_size, depth or DEFAULT_DEPTH)


def window_bytes(dictionary, max_src_size, mode):
    """The bytes of the dictionary a prepared object holds: the frame depends on these alone."""
    import hcdictmodel
    D = encmodel.cdict_window(len(dictionary), max_src_size) if mode == FAST else \
        hcdictmodel.window(len(dictionary), max_src_size)
    return bytes(dictionary[len(dictionary) - D:])


def compress(message, dictionary, max_src_size, dict_id=0, mode=FAST, depth=0, flags=0):
    """The frame APE_LZ4_lz4f_compress_usingCDicts_batch_dev writes for a message of at most
    max_src_size bytes: one independent block, block-size ID 4, the ID field exactly when
    dict_id != 0.  dictionary: what the message's object was prepared from (window_bytes() of it
    gives the same frame), or None for a bad object: the block is then stored."""
    message = bytes(message)
    assert 0 <= flags <= 7 and len(message) <= max_src_size <= M.BLOCK
    flg = 0x40 | M.F_INDEP | (M.F_BSUM if flags & M.BLOCK_CHECKSUMS else 0) | \
        (M.F_SIZE if flags & M.CONTENT_SIZE else 0) | \
        (M.F_CSUM if flags & M.CONTENT_CHECKSUM else 0) | (M.F_DICT if dict_id else 0)
    out = [M.frame_header(flg, 4, len(message) if flags & M.CONTENT_SIZE else None,
                          dict_id if dict_id else None)]
    if message:
        comp = None if dictionary is None else \
            block_of(message, bytes(dictionary), max_src_size, mode, depth)
        if comp is not None and len(comp) <= len(message) - 1:
            body, word = comp, len(comp)
        else:
            body, word = message, len(message) | 0x80000000
        out.append(struct.pack("<I", word) + body)
        if flags & M.BLOCK_CHECKSUMS:
            out.append(struct.pack("<I", M.xxh32(body)))
    out.append(struct.pack("<I", 0))
    if flags & M.CONTENT_CHECKSUM:
        out.append(struct.pack("<I", M.xxh32(message)))
    return b"".join(out)


def compress_bound(n, flags):
    """APE_LZ4_lz4f_compress_usingCDicts_bound: a stored block and an ID field."""
    if not 0 <= n <= M.BLOCK or not 0 <= flags <= 7:
        return 0
    return (15 if flags & M.CONTENT_SIZE else 7) + 4 + n + \
        ((8 if flags & M.BLOCK_CHECKSUMS else 4) if n else 0) + \
        (8 if flags & M.CONTENT_CHECKSUM else 4)


# ---------------- fixtures (tests/golden/lz4f_dict_golden.json) ----------------
def repeated(parts, repeat_to):
    unit = M.content_of(parts)
    return unit if repeat_to is None else (unit * (repeat_to // len(unit) + 1))[:repeat_to]


@functools.lru_cache(maxsize=1)
def dictionaries():
    """name -> bytes, from the recipes in the fixture file."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    return collections.OrderedDict((name, M.content_of(parts))
                                   for name, parts in doc["dictionaries"].items())


@functools.lru_cache(maxsize=1)
def fixtures():
    """name -> dict(frame, content, dict (a name of dictionaries()), dict_id, bsid, linked (what
    was asked of liblz4; `indep` is what the frame says), pieces (lengths, for a flushed frame,
    else None), block_sums, content_sum, content_size): frames liblz4 wrote with a dictionary."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = collections.OrderedDict()
    for fx in doc["frames"]:
        fx = dict(fx)
        fx["frame"] = base64.b64decode(fx.pop("frame_b64"))
        fx["content"] = repeated(fx["parts"], fx["repeat_to"])
        fx["indep"] = bool(fx["frame"][4] & M.F_INDEP)
        out[fx["name"]] = fx
    return out


def table_for(fx=None):
    """The table the tests decode the fixtures with: three keys first (5 names no frame), and for a
    fixture without an ID its own dictionary under key 0."""
    ds = dictionaries()
    table = [(77, ds["d60k"]), (0x80000001, ds["d70k"]), (5, ds["d4k"])]
    if fx is not None and fx["dict_id"] == 0:
        table.append((0, ds[fx["dict"]]))
    return table


def blocks_of(frame):
    code, _, _, blocks, _, _ = _stage(frame)
    assert code == 0
    return len(blocks)
