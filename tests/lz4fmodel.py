"""A Python model of the LZ4 frame layer (include/ape_lz4f.h): XXH32, the frame
APE_LZ4_lz4f_compress_batch_dev writes, what APE_LZ4_lz4f_info_batch_dev reports and the result
of APE_LZ4_lz4f_decompress_batch_dev, codes included.  This file is their definition; the block
bytes come from tests/encmodel.py.  No product or oracle code.

The frame (LZ4 frame format 1.6.x): le32 magic 0x184D2204; FLG = version 01 << 6 | independent
<< 5 | block checksums << 4 | content size << 3 | content checksum << 2 | reserved << 1 |
dictionary ID; BD = block-size ID << 4 (4..7: 64 KiB, 256 KiB, 1 MiB, 4 MiB), other bits
reserved; le64 content size and le32 dictionary ID where flagged; HC = (XXH32(FLG .. the byte
before HC) >> 8) & 255; then blocks [le32 word: size, bit 31 = stored][bytes][le32 XXH32 of those
bytes, with block checksums]; the end mark, a word whose low 31 bits are 0; le32 XXH32 of the
content, with a content checksum.

decode()'s codes, the first of the list that applies:
  -1 bad magic, version, reserved bit, block-size ID or header checksum; -3 unsupported
  (dictionary ID, skippable or legacy magic, a linked frame when the caller excludes them, a
  decoded bound of 2^31 or more); -2 truncated, or a block reaching past the input or larger
  than the block maximum; ERANGE more blocks than max_blocks; -9 capacity below the decoded
  bound; -6 block checksum; -4 a block fails to decode; -5 a short block before the last; -8
  content size mismatch; -7 content checksum.
The header is judged field by field in header(), each check on the bytes it needs, and a
truncation ends the judging: a frame cut inside its descriptor is -2 even if the missing header
checksum would have been wrong.  The bound is the content size where the frame carries it (so
that -3 is known from the header) and blocks x maximum otherwise (known after the walk)."""
import base64
import collections
import functools
import json
import os
import struct

import encmodel

MAGIC, SKIPPABLE, LEGACY = 0x184D2204, 0x184D2A50, 0x184C2102
ERANGE = -2147483647 - 1
CONTENT_CHECKSUM, BLOCK_CHECKSUMS, CONTENT_SIZE = 1, 2, 4      # compress flags
NO_VERIFY, NO_LINKED = 1, 2                                    # decompress flags
F_INDEP, F_BSUM, F_SIZE, F_CSUM, F_RESERVED, F_DICT = 0x20, 0x10, 0x08, 0x04, 0x02, 0x01
MAX_SRC = 0x7E000000
BLOCK = 65536
M32 = 0xFFFFFFFF
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def xxh32(data, seed=0):
    """XXH32 (xxHash 0.8 specification), a plain restatement."""
    data = bytes(data)
    n = len(data)
    at = 0
    if n >= 16:
        acc = [(seed + P1 + P2) & M32, (seed + P2) & M32, seed & M32, (seed - P1) & M32]
        words = struct.unpack_from("<%dI" % (n // 16 * 4), data)
        for k, x in enumerate(words):
            a = k & 3
            acc[a] = (_rotl((acc[a] + x * P2) & M32, 13) * P1) & M32
        at = n // 16 * 16
        h = (_rotl(acc[0], 1) + _rotl(acc[1], 7) + _rotl(acc[2], 12) + _rotl(acc[3], 18)) & M32
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while at + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, at)[0] * P3) & M32, 17) * P4) & M32
        at += 4
    while at < n:
        h = (_rotl((h + data[at] * P5) & M32, 11) * P1) & M32
        at += 1
    h ^= h >> 15
    h = (h * P2) & M32
    h ^= h >> 13
    h = (h * P3) & M32
    return h ^ (h >> 16)


def block_max(bsid):
    return 1 << (8 + 2 * bsid)


def header_checksum(descriptor, shift=8):
    """shift: the format's 8 (tests build a wrong neighbour with 0)."""
    return (xxh32(descriptor) >> shift) & 0xFF


def frame_header(flg, bsid, content_size=None, dict_id=None, shift=8):
    d = bytes([flg, bsid << 4])
    if content_size is not None:
        d += struct.pack("<Q", content_size)
    if dict_id is not None:
        d += struct.pack("<I", dict_id)
    return struct.pack("<I", MAGIC) + d + bytes([header_checksum(d, shift)])


@functools.lru_cache(maxsize=256)
def _encode_block(block):
    return encmodel.encode(block)


def frame_block(block, block_sums=False, sum_of_decoded=False):
    """One block of compress(): the fast encoder's bytes when they take at most len - 1, else
    the block stored; the checksum covers the bytes as they sit in the frame (sum_of_decoded:
    the wrong neighbour that hashes the content)."""
    comp = _encode_block(bytes(block))
    if len(comp) <= len(block) - 1:
        body, word = comp, len(comp)
    else:
        body, word = bytes(block), len(block) | 0x80000000
    out = struct.pack("<I", word) + body
    if block_sums:
        out += struct.pack("<I", xxh32(block if sum_of_decoded else body))
    return out


def compress(data, flags=0, all_stored=False):
    """The frame APE_LZ4_lz4f_compress_batch_dev writes for (data, flags): version 01,
    independent 64 KiB blocks, block-size ID 4."""
    assert 0 <= flags <= 7 and len(data) <= MAX_SRC
    flg = 0x40 | F_INDEP | (F_BSUM if flags & BLOCK_CHECKSUMS else 0) | \
        (F_SIZE if flags & CONTENT_SIZE else 0) | (F_CSUM if flags & CONTENT_CHECKSUM else 0)
    out = [frame_header(flg, 4, len(data) if flags & CONTENT_SIZE else None)]
    for at in range(0, len(data), BLOCK):
        block = data[at:at + BLOCK]
        if all_stored:
            out.append(struct.pack("<I", len(block) | 0x80000000) + block)
            if flags & BLOCK_CHECKSUMS:
                out.append(struct.pack("<I", xxh32(block)))
        else:
            out.append(frame_block(block, bool(flags & BLOCK_CHECKSUMS)))
    out.append(struct.pack("<I", 0))
    if flags & CONTENT_CHECKSUM:
        out.append(struct.pack("<I", xxh32(data)))
    return b"".join(out)


def compress_bound(n, flags):
    """APE_LZ4_lz4f_compress_bound: every block stored."""
    if not 0 <= n <= MAX_SRC or not 0 <= flags <= 7:
        return 0
    nb = (n + BLOCK - 1) // BLOCK
    return (15 if flags & CONTENT_SIZE else 7) + n + nb * (8 if flags & BLOCK_CHECKSUMS else 4) + \
        (8 if flags & CONTENT_CHECKSUM else 4)


# ---------------- reading a frame ----------------
Head = collections.namedtuple("Head", "flg bmax size content_size")
Block = collections.namedtuple("Block", "at size stored want")


def header(frame, no_linked=False, shift=8):
    """(code, Head or None): the header stage, up to the first block."""
    n = len(frame)
    if n < 4:
        return -2, None
    magic = struct.unpack_from("<I", frame)[0]
    if magic & 0xFFFFFFF0 == SKIPPABLE or magic == LEGACY:
        return -3, None
    if magic != MAGIC:
        return -1, None
    if n < 6:
        return -2, None
    flg, bd = frame[4], frame[5]
    bsid = (bd >> 4) & 7
    if flg >> 6 != 1 or flg & F_RESERVED or bd & 0x8F or bsid < 4:
        return -1, None
    dn = 2 + (8 if flg & F_SIZE else 0) + (4 if flg & F_DICT else 0)
    if n < 4 + dn + 1:
        return -2, None
    if frame[4 + dn] != header_checksum(frame[4:4 + dn], shift):
        return -1, None
    size = struct.unpack_from("<Q", frame, 6)[0] if flg & F_SIZE else None
    if flg & F_DICT or (no_linked and not flg & F_INDEP) or (size is not None and size >= 1 << 31):
        return -3, None
    return 0, Head(flg, block_max(bsid), 4 + dn + 1, size)


def walk(frame, head):
    """(code, blocks, the frame's bytes): the block headers up to the end mark and the trailer."""
    n, p, blocks = len(frame), head.size, []
    extra = 4 if head.flg & F_BSUM else 0
    while True:
        if n - p < 4:
            return -2, None, None
        word = struct.unpack_from("<I", frame, p)[0]
        size = word & 0x7FFFFFFF
        p += 4
        if size == 0:
            break
        if size > head.bmax or n - p < size + extra:
            return -2, None, None
        want = struct.unpack_from("<I", frame, p + size)[0] if extra else None
        blocks.append(Block(p, size, bool(word >> 31), want))
        p += size + extra
    if head.flg & F_CSUM:
        if n - p < 4:
            return -2, None, None
        p += 4
    return 0, blocks, p


def _stage(frame, no_linked=False):
    """Header, walk and bound: (code, head, blocks, frame bytes, bound)."""
    code, head = header(frame, no_linked)
    if code:
        return code, None, None, None, None
    code, blocks, end = walk(frame, head)
    if code:
        return code, None, None, None, None
    bound = head.content_size if head.content_size is not None else len(blocks) * head.bmax
    if bound >= 1 << 31:
        return -3, None, None, None, None
    return 0, head, blocks, end, bound


def info(frame):
    """The eight ints of APE_LZ4_lz4f_info_batch_dev."""
    code, head, blocks, end, bound = _stage(frame)
    if code:
        return [code, 0, 0, 0, 0, 0, -1, -1]
    size = head.content_size
    return [0, head.flg, head.bmax, len(blocks), end, bound,
            -1 if size is None else _i32(size & M32), -1 if size is None else _i32(size >> 32)]


def _i32(x):
    return x - (1 << 32) if x >= 1 << 31 else x


def block_decode(src, cap, history=b""):
    """An LZ4 block -> its bytes, or None: literal runs and matches must stay inside the input,
    the capacity and the history (the last 64 KiB before the block).  A restatement for the
    frames of the tests; where decoders differ on malformed blocks it takes no side."""
    buf = bytearray(history[-65536:])
    base, n, ip = len(buf), len(src), 0
    while True:
        if ip >= n:
            return None
        token = src[ip]
        ip += 1
        run = token >> 4
        if run == 15:
            while True:
                if ip >= n:
                    return None
                run += src[ip]
                ip += 1
                if src[ip - 1] != 255:
                    break
        if ip + run > n or len(buf) - base + run > cap:
            return None
        buf += src[ip:ip + run]
        ip += run
        if ip == n:
            return bytes(buf[base:])
        if ip + 2 > n:
            return None
        offset = src[ip] | src[ip + 1] << 8
        ip += 2
        length = token & 15
        if length == 15:
            while True:
                if ip >= n:
                    return None
                length += src[ip]
                ip += 1
                if src[ip - 1] != 255:
                    break
        length += 4
        if offset == 0 or offset > len(buf) or len(buf) - base + length > cap:
            return None
        if offset >= length:
            start = len(buf) - offset
            buf += buf[start:start + length]
        else:
            pattern = bytes(buf[-offset:])
            buf += (pattern * (length // offset + 1))[:length]


def decode(frame, cap, max_blocks=1 << 20, flags=0, sum_of_decoded=False):
    """(result, bytes or None) of APE_LZ4_lz4f_decompress_batch_dev for one frame: the decoded
    size and the content, or a code.  Block q's output lies at q x block maximum, in room
    min(block maximum, cap - q x block maximum)."""
    code, head, blocks, end, bound = _stage(frame, bool(flags & NO_LINKED))
    if code:
        return code, None
    if len(blocks) > max_blocks:
        return ERANGE, None
    if cap < bound:
        return -9, None
    verify = not flags & NO_VERIFY
    image = bytearray()
    got = []
    for q, b in enumerate(blocks):
        body = frame[b.at:b.at + b.size]
        room = max(0, min(head.bmax, cap - q * head.bmax))
        if room:   # (a short block leaves a gap; without room nothing is placed)
            image += bytes(q * head.bmax - len(image))
        if b.stored:
            out = body if b.size <= room else None
        else:
            linked = not head.flg & F_INDEP
            out = block_decode(body, room, bytes(image[-65536:]) if linked else b"")
        got.append(out)
        image += out or b""
    if verify and head.flg & F_BSUM:
        for b, out in zip(blocks, got):
            hashed = (out or b"") if sum_of_decoded else frame[b.at:b.at + b.size]
            if xxh32(hashed) != b.want:
                return -6, None
    if any(out is None for out in got):
        return -4, None
    if any(len(out) != head.bmax for out in got[:-1]):
        return -5, None
    content = bytes(image)
    if head.content_size is not None and head.content_size != len(content):
        return -8, None
    if verify and head.flg & F_CSUM and xxh32(content) != struct.unpack_from("<I", frame, end - 4)[0]:
        return -7, None
    return len(content), content


# ---------------- fixtures (tests/golden/lz4f_golden.json) and what the tests derive ----------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_golden.json")


def content_of(parts):
    """A fixture's content from its recipe: parts [kind, n, seed, total], each inputs.make(kind,
    n, seed) repeated up to `total` bytes."""
    import inputs
    out = []
    for kind, n, seed, total in parts:
        piece = inputs.make(kind, n, seed)
        out.append((piece * (total // max(n, 1) + 1))[:total] if total else b"")
    return b"".join(out)


@functools.lru_cache(maxsize=1)
def fixtures():
    """name -> dict(frame, content, bsid, linked, block_sums, content_sum, content_size)."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = collections.OrderedDict()
    for fx in doc["frames"]:
        fx = dict(fx)
        fx["frame"] = base64.b64decode(fx.pop("frame_b64"))
        fx["content"] = content_of(fx["parts"])
        out[fx["name"]] = fx
    return out


def _redo_header_sum(frame, dn):
    frame = bytearray(frame)
    frame[4 + dn] = header_checksum(bytes(frame[4:4 + dn]))
    return bytes(frame)


def _flip(frame, at):
    frame = bytearray(frame)
    frame[at] ^= 0x40
    return bytes(frame)


Case = collections.namedtuple(
    "Case", "name frame cap max_blocks code header_stage lenient malformed")
DEFAULT_BLOCKS = 8


def corruptions():
    """The malformed frames of the tests, each from a fixture: Case(name, frame, the capacity
    to decode it with, max_blocks, the code decode() gives, whether info() shows the code, the
    result with NO_VERIFY when that differs, whether the frame breaks the format -- the others
    are well-formed frames that run into a limit of this decoder or of the call)."""
    fx = fixtures()
    plain, sums = fx["indep_none"], fx["indep_all"]
    sized, rand = fx["indep_content_size"], fx["random_block_all"]
    room = 4 * BLOCK
    out = []

    def add(name, frame, code, cap=room, max_blocks=DEFAULT_BLOCKS, header_stage=False,
            lenient=None, malformed=True):
        out.append(Case(name, frame, cap, max_blocks, code, header_stage, lenient, malformed))

    _, head = header(rand["frame"])
    stored = walk(rand["frame"], head)[1][0]
    assert stored.stored
    flipped = _flip(rand["frame"], stored.at + 1000)
    want = bytearray(rand["content"])
    want[1000] ^= 0x40
    add("flipped data byte, block checksums", flipped, -6, lenient=bytes(want))
    add("flipped content checksum", _flip(sums["frame"], len(sums["frame"]) - 1), -7,
        lenient=sums["content"])
    add("wrong header checksum", _flip(plain["frame"], 6), -1, header_stage=True)
    reserved = bytearray(plain["frame"])
    reserved[4] |= F_RESERVED
    add("reserved bit, checksum redone", _redo_header_sum(reserved, 2), -1, header_stage=True)
    with_id = bytearray(plain["frame"])
    with_id[4] |= F_DICT
    with_id[6:7] = struct.pack("<I", 7) + b"\0"
    add("dictionary ID", _redo_header_sum(with_id, 6), -3, header_stage=True, malformed=False)
    add("skippable magic", struct.pack("<I", SKIPPABLE + 3) + plain["frame"][4:], -3,
        header_stage=True, malformed=False)
    _, head = header(sums["frame"])
    second = walk(sums["frame"], head)[1][1]
    add("cut inside a block", sums["frame"][:second.at + second.size // 2], -2, header_stage=True)
    add("cut inside the trailer", sums["frame"][:-2], -2, header_stage=True)
    longer = bytearray(sized["frame"])
    longer[6:14] = struct.pack("<Q", len(sized["content"]) + 1)
    add("changed content size", _redo_header_sum(longer, 10), -8)
    text = sums["content"]
    short = frame_header(0x40 | F_INDEP, 4) + frame_block(text[:100]) + \
        frame_block(text[100:200]) + struct.pack("<I", 0)
    add("two 100-byte blocks", short, -5, malformed=False)
    # A declared content size far below blocks x maximum, the capacity it asks for, and a last
    # block 00, which decodes to 0 bytes in no room at all: the earlier block is what fails (or
    # is short), and nothing past the capacity may be touched, not even read for the checksum.
    flg = 0x40 | F_INDEP | F_SIZE | F_CSUM
    tail = struct.pack("<I", 1) + b"\0" + struct.pack("<II", 0, xxh32(b""))
    add("declared size 1, a full block, then 00",
        frame_header(flg, 4, 1) + frame_block(text[:BLOCK]) + tail, -4, cap=1)
    add("declared size 200, a 100-byte block, then 00",
        frame_header(flg, 4, 200) + frame_block(text[:100]) + tail, -5, cap=200)
    # ... and with 1025 such blocks at 4 MiB, where (blocks - 1) x maximum is 2^32
    many = frame_header(flg, 7, 0) + (struct.pack("<I", 1) + b"\0") * 1025 + \
        struct.pack("<II", 0, xxh32(b""))
    add("declared size 0, 1025 blocks 00 at 4 MiB", many, -5, cap=0, max_blocks=1100,
        malformed=False)
    blocks = info(plain["frame"])[3]
    add("one block more than max_blocks", plain["frame"], ERANGE, max_blocks=blocks - 1,
        malformed=False)
    add("capacity one short", plain["frame"], -9, cap=info(plain["frame"])[5] - 1,
        malformed=False)
    return out
