"""Writes tests/golden/lz4f_dict_golden.json: LZ4 frames the system's liblz4 (1.9.3 when this was
run) wrote with a dictionary, for the tests of include/ape_lz4f_dict.h (tests/lz4fdictmodel.py
reads them).  Run once, by hand, on a machine that has liblz4.so.1 (or liblz4.so.1.9.3 under
/usr/lib/x86_64-linux-gnu); no test needs the library.

One-shot frames are LZ4F_compressFrame_usingCDict; flushed ones LZ4F_compressBegin_usingCDict,
then LZ4F_compressUpdate + LZ4F_flush per piece, then LZ4F_compressEnd.  Only the frames are
stored (base64).  The dictionaries are pieces of text from tests/golden/inputs.py, and a content
is a few of its dictionary's own pieces, repeated: every block refers to the dictionary, and a
three-block frame stays below 4 KB.  The script asserts what lets the fixtures tell right from
wrong: every compressed block of every frame fails to decode without history (but the last,
partial block of a linked frame of several blocks: liblz4 1.9.3 was seen to compress that one
without any history, so it decodes on its own), and block 1 of the
three-block linked frames with the 4 KiB dictionary fails with the dictionary as its only history
(the contents' period is longer than that dictionary)."""
import base64
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import lz4fmodel as M  # noqa: E402
import lz4fdictmodel as DM  # noqa: E402
from gen_lz4f_golden import Preferences  # noqa: E402
from gen_lz4f_flush_golden import liblz4 as _liblz4  # noqa: E402


def liblz4():
    L = _liblz4()
    L.LZ4F_createCDict.restype = C.c_void_p
    L.LZ4F_createCDict.argtypes = [C.c_void_p, C.c_size_t]
    L.LZ4F_freeCDict.argtypes = [C.c_void_p]
    L.LZ4F_compressFrame_usingCDict.restype = C.c_size_t
    L.LZ4F_compressFrame_usingCDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.c_size_t, C.c_void_p, C.c_void_p]
    L.LZ4F_compressBegin_usingCDict.restype = C.c_size_t
    L.LZ4F_compressBegin_usingCDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.c_void_p]
    return L


# The dictionaries: pieces of text, [kind, n, seed, total] as lz4fmodel.content_of takes them.
def _piece(name, k):
    return {"d4k": ["text", 256, 100 + k, 256], "d60k": ["text", 256, 300 + k, 256],
            "d70k": ["text", 250, 600 + k, 250]}[name]


DICTS = {"d4k": [_piece("d4k", k) for k in range(16)],        # 4096 bytes
         "d60k": [_piece("d60k", k) for k in range(240)],     # 61440 bytes
         "d70k": [_piece("d70k", k) for k in range(280)]}     # 70000 bytes: pieces 263.. lie past
                                                              # its first 64 KiB
IDS = {"d4k": 0, "d60k": 77, "d70k": 0x80000001}
# a content's unit: pieces of its dictionary (of d70k's, ones its first 64 KiB do not hold)
UNIT = {"d4k": [_piece("d4k", k) for k in (9, 2, 14, 5, 11, 0, 7, 13, 3, 8, 1, 15, 6, 12, 4, 10)] +
        [_piece("d4k", k) for k in (3, 9, 1, 12, 6, 15, 0, 10, 5, 13, 7, 2)],   # 7168 bytes
        "d60k": [_piece("d60k", k) for k in range(239, 0, -17)],
        "d70k": [_piece("d70k", k) for k in (279, 265, 272, 268, 277, 264, 270, 275, 266, 273)]}


def prefs_of(bsid, linked, full, content_size, dict_id):
    prefs = Preferences()
    prefs.frameInfo.blockSizeID = bsid
    prefs.frameInfo.blockMode = 0 if linked else 1
    prefs.frameInfo.contentChecksumFlag = int(full)
    prefs.frameInfo.blockChecksumFlag = int(full)
    prefs.frameInfo.contentSize = content_size
    prefs.frameInfo.dictID = dict_id
    return prefs


def took(L, r):
    assert not L.LZ4F_isError(r), r
    return r


def make_frame(L, cdict, content, pieces, prefs):
    cap = L.LZ4F_compressBound(len(content), C.byref(prefs)) + 256 + 80 * len(pieces or [])
    out = C.create_string_buffer(cap)
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(C.byref(ctx), 100))
    if pieces is None:
        at = took(L, L.LZ4F_compressFrame_usingCDict(ctx, out, cap, content, len(content), cdict,
                                                     C.byref(prefs)))
    else:
        at = took(L, L.LZ4F_compressBegin_usingCDict(ctx, out, cap, cdict, C.byref(prefs)))
        done = 0
        for n in pieces:
            piece = content[done:done + n]
            done += n
            at += took(L, L.LZ4F_compressUpdate(ctx, C.byref(out, at), cap - at, piece, n, None))
            at += took(L, L.LZ4F_flush(ctx, C.byref(out, at), cap - at, None))
        assert done == len(content)
        at += took(L, L.LZ4F_compressEnd(ctx, C.byref(out, at), cap - at, None))
    L.LZ4F_freeCompressionContext(ctx)
    return out.raw[:at]


THREE = 65536 + 65536 + 9000
# tag, dictionary, content bytes, pieces (None: one shot), bsid, linked, checksums and content size
FRAMES = [("one_byte", d, 1, None, 4, False, full) for d, full in
          (("d4k", False), ("d60k", True), ("d70k", False))] + \
    [("hundred", d, 100, None, b, False, full) for d, b, full in
     (("d4k", 5, True), ("d60k", 4, False), ("d70k", 4, True))] + \
    [("four_k", d, 4000, None, 4, linked, full) for d, linked, full in
     (("d4k", False, False), ("d60k", False, True), ("d70k", False, False), ("d70k", True, True),
      ("d4k", True, False))] + \
    [("three", d, THREE, None, b, linked, full) for d, b, linked, full in
     (("d4k", 4, True, False), ("d4k", 4, True, True), ("d60k", 4, False, False),
      ("d70k", 4, False, True), ("d70k", 4, True, False), ("d60k", 4, True, True),
      ("d70k", 5, False, False), ("d4k", 5, True, True))] + \
    [("flush_short", "d60k", 5101, [100, 3000, 1, 2000], 4, False, True),
     ("flush_short", "d70k", 5101, [100, 3000, 1, 2000], 5, False, False),
     ("flush_low", "d4k", 7000, [3000, 3000, 1000], 4, True, False),
     ("flush_low", "d60k", 7000, [3000, 3000, 1000], 4, True, True),
     ("flush_high", "d4k", 65536 + 800, [65536, 500, 300], 4, True, True),
     ("flush_high", "d70k", 65536 + 800, [65536, 500, 300], 4, True, False)]


def check(name, frame, content, dictionary, linked_three):
    """What the fixtures must have to tell right from wrong."""
    code, head, dict_id, blocks, end, _ = DM._stage(frame)
    assert code == 0, name
    for q, b in enumerate(blocks):
        lone = not head.flg & M.F_INDEP and q and q == len(blocks) - 1   # (see the docstring)
        if not b.stored and not lone:
            body = frame[b.at:b.at + b.size]
            assert M.block_decode(body, head.bmax, b"") is None, (name, q, "decodes on its own")
    if linked_three:
        assert not head.flg & M.F_INDEP and len(blocks) == 3 and not blocks[1].stored, name
        b = blocks[1]
        assert M.block_decode(frame[b.at:b.at + b.size], head.bmax, dictionary) is None, name
    table = [(dict_id or 0, dictionary)]
    got = DM.decode(frame, len(content), table, flags=DM.ANY_SIZE)
    assert got == (len(content), content) or got[0] == -3, (name, got[0])
    return len(blocks), got[0]


def main():
    L = liblz4()
    L.LZ4_versionString.restype = C.c_char_p
    version = L.LZ4_versionString().decode()
    frames = []
    for tag, dname, nbytes, pieces, bsid, linked, full in FRAMES:
        dictionary = M.content_of(DICTS[dname])
        cdict = L.LZ4F_createCDict(dictionary, len(dictionary))
        assert cdict
        content = DM.repeated(UNIT[dname], nbytes)
        prefs = prefs_of(bsid, linked, full, len(content) if full else 0, IDS[dname])
        frame = make_frame(L, cdict, content, pieces, prefs)
        L.LZ4F_freeCDict(cdict)
        name = "%s_%s_%s_id%d_%s" % (tag, dname, "linked" if linked else "indep", bsid,
                                     "all" if full else "none")
        nb, placed = check(name, frame, content, dictionary,
                           tag == "three" and linked and bsid == 4 and dname == "d4k")
        frames.append({"name": name, "dict": dname, "dict_id": IDS[dname], "bsid": bsid,
                       "linked": linked, "block_sums": full, "content_sum": full,
                       "content_size": full, "pieces": pieces, "parts": UNIT[dname],
                       "repeat_to": nbytes, "frame_b64": base64.b64encode(frame).decode()})
        print("%-40s %7d -> %6d bytes, %d blocks, FLG %02x, placed %d" % (
            name, len(content), len(frame), nb, frame[4], placed))
    path = os.path.join(HERE, "lz4f_dict_golden.json")
    with open(path, "w") as f:
        f.write('{"liblz4": %s, "dictionaries": %s, "frames": [\n' % (
            json.dumps(version), json.dumps(DICTS)))
        f.write(",\n".join(json.dumps(fr) for fr in frames))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
