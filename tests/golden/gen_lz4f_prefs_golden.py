"""Writes tests/golden/lz4f_prefs_golden.json: what the system's liblz4 (1.9.3 when this was run)
makes of the frames tests/lz4fprefsmodel.py defines for its CASES -- (input recipe, block-size ID,
mode, depth, flags).  Run once, by hand, on a machine that has liblz4.so.1 (or liblz4.so.1.9.3
under /usr/lib/x86_64-linux-gnu); no test needs the library.

Per case the file holds the SHA-256 of the model's frame and liblz4's reading of it:
LZ4F_getFrameInfo's blockSizeID, the last LZ4F_decompress return (0: the frame is complete), the
bytes it consumed (the frame's length) and the SHA-256 of what it decoded (the input's).  The
frames are not stored: tests/test_lz4f_prefs_model.py recomputes them and compares the hashes, so
the fixture says "liblz4 read exactly these frames"."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import lz4fmodel as M  # noqa: E402
import lz4fprefsmodel as P  # noqa: E402
from gen_lz4f_golden import FrameInfo  # noqa: E402


def liblz4():
    try:
        L = C.CDLL("liblz4.so.1")
    except OSError:
        L = C.CDLL("/usr/lib/x86_64-linux-gnu/liblz4.so.1.9.3")
    L.LZ4F_isError.argtypes = [C.c_size_t]
    L.LZ4F_createDecompressionContext.restype = C.c_size_t
    L.LZ4F_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]
    L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    L.LZ4F_getFrameInfo.restype = C.c_size_t
    L.LZ4F_getFrameInfo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.LZ4F_decompress.restype = C.c_size_t
    L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]
    return L


def read_frame(L, frame, room):
    """(blockSizeID, last LZ4F_decompress return, bytes consumed, the decoded bytes)."""
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    src = C.create_string_buffer(frame, len(frame))
    info = FrameInfo()
    took = C.c_size_t(len(frame))
    r = L.LZ4F_getFrameInfo(ctx, C.byref(info), src, C.byref(took))
    assert not L.LZ4F_isError(r), r
    at, out, last = took.value, bytearray(), r
    dst = C.create_string_buffer(room + 1)
    while at < len(frame):
        wrote, took = C.c_size_t(room + 1), C.c_size_t(len(frame) - at)
        last = L.LZ4F_decompress(ctx, dst, C.byref(wrote), C.byref(src, at), C.byref(took), None)
        assert not L.LZ4F_isError(last), last
        out += dst.raw[:wrote.value]
        at += took.value
        if last == 0:
            break
    L.LZ4F_freeDecompressionContext(ctx)
    return info.blockSizeID, last, at, bytes(out)


def main():
    L = liblz4()
    L.LZ4_versionString.restype = C.c_char_p
    version = L.LZ4_versionString().decode()
    cases = []
    for name, parts, bsid, mode, depth, flags in P.CASES:
        content = M.content_of(parts)
        frame = P.compress(content, bsid, mode, depth, flags)
        got_id, last, consumed, decoded = read_frame(L, frame, len(content))
        assert (got_id, last, consumed, decoded) == (bsid, 0, len(frame), content), name
        cases.append({"name": name, "parts": parts, "bsid": bsid, "mode": mode, "depth": depth,
                      "flags": flags, "content_bytes": len(content), "frame_bytes": len(frame),
                      "frame_sha256": hashlib.sha256(frame).hexdigest(),
                      "liblz4": {"blockSizeID": got_id, "decompress_return": last,
                                 "consumed": consumed,
                                 "decoded_sha256": hashlib.sha256(decoded).hexdigest()}})
        print("%-26s %8d -> %8d bytes, %d blocks" % (name, len(content), len(frame),
                                                    M.info(frame)[3]))
    path = os.path.join(HERE, "lz4f_prefs_golden.json")
    with open(path, "w") as f:
        f.write('{"liblz4": %s, "slice": %d, "cases": [\n' % (json.dumps(version), P.SLICE))
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
