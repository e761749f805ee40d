"""Writes tests/golden/lz4f_golden.json: LZ4 frames made by the system's liblz4 (1.9.3 when this
was run), for the frame layer's tests (tests/lz4fmodel.py reads them).  Run once, by hand, on a
machine that has liblz4.so.1; no test needs the library.

Each frame comes from liblz4's streaming calls (LZ4F_compressBegin / compressUpdate on the whole
input / compressEnd), which keep the requested block-size ID and block mode where
LZ4F_compressFrame would lower them for a short input.  Only the frames are stored (base64); the
contents are regenerated from tests/golden/inputs.py by their recipe: parts [kind, n, seed,
total], each inputs.make(kind, n, seed) repeated up to `total` bytes.  The repeated 3000-byte
text makes every block start with matches that reach into the block before it, which linked
frames use and independent ones cannot."""
import base64
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import lz4fmodel as M  # noqa: E402


class FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int),
                ("frameType", C.c_int), ("contentSize", C.c_ulonglong), ("dictID", C.c_uint),
                ("blockChecksumFlag", C.c_int)]


class Preferences(C.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint),
                ("favorDecSpeed", C.c_uint), ("reserved", C.c_uint * 3)]


def liblz4():
    L = C.CDLL("liblz4.so.1")
    L.LZ4F_compressBound.restype = C.c_size_t
    L.LZ4F_compressBound.argtypes = [C.c_size_t, C.c_void_p]
    L.LZ4F_isError.argtypes = [C.c_size_t]
    L.LZ4F_createCompressionContext.argtypes = [C.c_void_p, C.c_uint]
    L.LZ4F_createCompressionContext.restype = C.c_size_t
    L.LZ4F_freeCompressionContext.argtypes = [C.c_void_p]
    for name, args in (("LZ4F_compressBegin", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
                       ("LZ4F_compressUpdate", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.c_size_t, C.c_void_p]),
                       ("LZ4F_compressEnd", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])):
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_size_t, args
    return L


def make_frame(L, content, bsid, linked, block_sums, content_sum, content_size):
    prefs = Preferences()
    prefs.frameInfo.blockSizeID = bsid
    prefs.frameInfo.blockMode = 0 if linked else 1
    prefs.frameInfo.contentChecksumFlag = int(content_sum)
    prefs.frameInfo.blockChecksumFlag = int(block_sums)
    prefs.frameInfo.contentSize = len(content) if content_size else 0
    cap = L.LZ4F_compressBound(len(content), C.byref(prefs)) + 64
    out = C.create_string_buffer(cap)
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(C.byref(ctx), 100))
    at = 0
    for step in (lambda: L.LZ4F_compressBegin(ctx, C.byref(out, at), cap - at, C.byref(prefs)),
                 lambda: L.LZ4F_compressUpdate(ctx, C.byref(out, at), cap - at, content,
                                               len(content), None),
                 lambda: L.LZ4F_compressEnd(ctx, C.byref(out, at), cap - at, None)):
        r = step()
        assert not L.LZ4F_isError(r), r
        at += r
    L.LZ4F_freeCompressionContext(ctx)
    return out.raw[:at]


TEXT = ["text", 3000, 1, 3 * 65536 + 100]
FOUR = [(mode + "_" + tag, 4, mode == "linked", bs, cs, size, [TEXT])
        for mode in ("indep", "linked")
        for tag, bs, cs, size in (("none", False, False, False), ("bsum", True, False, False),
                                  ("content_size", False, True, True), ("all", True, True, True))]
FRAMES = FOUR + [
    ("random_block_all", 4, False, True, True, True, [["rand", 65536, 5, 65536],
                                                      ["text", 1000, 2, 1000]]),
    ("id5_two_blocks", 5, False, False, True, False, [["text", 3000, 3, 262145]]),
    ("id7_short", 7, True, True, False, False, [["text", 500, 4, 500]]),
    ("empty", 4, False, False, True, False, []),
    ("one_byte", 4, False, False, False, True, [["byte", 1, 0, 1]]),
]


def main():
    L = liblz4()
    L.LZ4_versionString.restype = C.c_char_p
    version = L.LZ4_versionString().decode()
    frames = []
    for name, bsid, linked, bs, cs, size, parts in FRAMES:
        content = M.content_of(parts)
        frame = make_frame(L, content, bsid, linked, bs, cs, size)
        frames.append({"name": name, "bsid": bsid, "linked": linked, "block_sums": bs,
                       "content_sum": cs, "content_size": size, "parts": parts,
                       "frame_b64": base64.b64encode(frame).decode()})
        print("%-22s %7d -> %6d bytes" % (name, len(content), len(frame)))
    path = os.path.join(HERE, "lz4f_golden.json")
    with open(path, "w") as f:
        json.dump({"liblz4": version, "frames": frames}, f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
