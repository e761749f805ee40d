"""Writes tests/golden/lz4f_flush_golden.json: LZ4 frames made by the system's liblz4 (1.9.3 when
this was run) the way a streaming producer that flushes makes them, for the placed framed
decode's tests (tests/lz4fplacedmodel.py reads them).  Run once, by hand, on a machine that has
liblz4.so.1 (or liblz4.so.1.9.3 under /usr/lib/x86_64-linux-gnu); no test needs the library.

Each frame is LZ4F_compressBegin, then LZ4F_compressUpdate + LZ4F_flush per piece, then
LZ4F_compressEnd: one block per non-empty piece (a piece above the block maximum gives full
blocks and a rest), so the blocks in the middle are short -- the frames
APE_LZ4_lz4f_decompress_batch_dev answers with -5.  An empty update writes no block.  Only the
frames are stored (base64); the contents are regenerated from tests/golden/inputs.py by their
recipe, as in gen_lz4f_golden.py; with "repeat_to", that content is a unit repeated up to so many
bytes.  The 40 pieces of 3000 bytes cut a unit of 7000 bytes -- seven texts of 50 bytes, each
repeated to 1000 -- so a piece compresses on its own (the independent frames stay small), and in
the linked frame every text's first bytes match 7000 bytes back, across two short blocks (with a
period of 3000 every match would start exactly at the block before)."""
import base64
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import lz4fmodel as M  # noqa: E402
from gen_lz4f_golden import Preferences  # noqa: E402


def liblz4():
    try:
        L = C.CDLL("liblz4.so.1")
    except OSError:
        L = C.CDLL("/usr/lib/x86_64-linux-gnu/liblz4.so.1.9.3")
    L.LZ4F_compressBound.restype = C.c_size_t
    L.LZ4F_compressBound.argtypes = [C.c_size_t, C.c_void_p]
    L.LZ4F_isError.argtypes = [C.c_size_t]
    L.LZ4F_createCompressionContext.argtypes = [C.c_void_p, C.c_uint]
    L.LZ4F_createCompressionContext.restype = C.c_size_t
    L.LZ4F_freeCompressionContext.argtypes = [C.c_void_p]
    for name, args in (("LZ4F_compressBegin", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
                       ("LZ4F_compressUpdate", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.c_size_t, C.c_void_p]),
                       ("LZ4F_flush", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
                       ("LZ4F_compressEnd", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])):
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_size_t, args
    return L


def make_frame(L, content, pieces, bsid, linked, sums, content_size):
    prefs = Preferences()
    prefs.frameInfo.blockSizeID = bsid
    prefs.frameInfo.blockMode = 0 if linked else 1
    prefs.frameInfo.contentChecksumFlag = int(sums)
    prefs.frameInfo.blockChecksumFlag = int(sums)
    prefs.frameInfo.contentSize = len(content) if content_size else 0
    cap = L.LZ4F_compressBound(len(content), C.byref(prefs)) + 64 + 16 * len(pieces) + \
        len(pieces) * 64
    out = C.create_string_buffer(cap)
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(C.byref(ctx), 100))
    at = 0

    def took(r):
        assert not L.LZ4F_isError(r), r
        return r

    at += took(L.LZ4F_compressBegin(ctx, C.byref(out, at), cap - at, C.byref(prefs)))
    done = 0
    for n in pieces:
        piece = content[done:done + n]
        done += n
        at += took(L.LZ4F_compressUpdate(ctx, C.byref(out, at), cap - at, piece, n, None))
        at += took(L.LZ4F_flush(ctx, C.byref(out, at), cap - at, None))
    assert done == len(content)
    at += took(L.LZ4F_compressEnd(ctx, C.byref(out, at), cap - at, None))
    L.LZ4F_freeCompressionContext(ctx)
    return out.raw[:at]


# name, the pieces' lengths, the content's recipe, the bytes its unit is repeated to (or None)
PIECES = [
    ("one_byte", [1], [["byte", 1, 0, 1]], None),
    ("short_full_one", [100, 65536, 1], [["text", 3000, 2, 65637]], None),
    ("full_and_one", [65537], [["text", 3000, 3, 65537]], None),
    ("forty_short", [3000] * 40, [["text", 50, 10 + k, 1000] for k in range(7)], 120000),
    ("empty_updates", [0, 500, 0], [["text", 500, 4, 500]], None),
]


def content_of(parts, repeat_to):
    unit = M.content_of(parts)
    return unit if repeat_to is None else (unit * (repeat_to // len(unit) + 1))[:repeat_to]


def main():
    L = liblz4()
    L.LZ4_versionString.restype = C.c_char_p
    version = L.LZ4_versionString().decode()
    frames = []
    for tag, pieces, parts, repeat_to in PIECES:
        content = content_of(parts, repeat_to)
        for linked in (False, True):
            for bsid in (4, 5):
                for full in (False, True):
                    name = "%s_%s_id%d_%s" % (tag, "linked" if linked else "indep", bsid,
                                              "all" if full else "none")
                    frame = make_frame(L, content, pieces, bsid, linked, full, full)
                    frames.append({"name": name, "bsid": bsid, "linked": linked,
                                   "block_sums": full, "content_sum": full, "content_size": full,
                                   "pieces": pieces, "parts": parts, "repeat_to": repeat_to,
                                   "frame_b64": base64.b64encode(frame).decode()})
                    print("%-36s %7d -> %6d bytes, %d blocks" % (
                        name, len(content), len(frame), M.info(frame)[3]))
    path = os.path.join(HERE, "lz4f_flush_golden.json")
    with open(path, "w") as f:
        # one frame per line
        f.write('{"liblz4": %s, "frames": [\n' % json.dumps(version))
        f.write(",\n".join(json.dumps(fr) for fr in frames))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
