"""tests/lz4fmodel.py against the outside world, without a GPU: XXH32 against its published
values, the xxhash module (where importable) and every checksum liblz4 put into the fixtures;
the model's decoder on liblz4's frames; liblz4's decoder (where the library loads) on the
model's frames and on the corruptions; and the two wrong neighbours the fixtures tell apart."""
import ctypes as C
import struct

import numpy as np
import pytest

import lz4fmodel as M

SIZES = [0, 1, 65535, 65536, 65537, 3 * 65536 + 100]


def _bytes(n, salt):
    return np.random.RandomState(salt).randint(0, 256, n, dtype=np.uint8).tobytes()


def test_xxh32_published_values():
    assert M.xxh32(b"") == 0x02CC5D05
    assert M.xxh32(b"a") == 0x550D7456


def test_xxh32_equals_the_xxhash_module():
    xxhash = pytest.importorskip("xxhash")
    for n in list(range(49)) + [63, 64, 65, 4095, 4096, 4097, 65536]:
        data = _bytes(n, n)
        for seed in (0, 1, 0x9E3779B1):
            assert M.xxh32(data, seed) == xxhash.xxh32(data, seed=seed).intdigest(), (n, seed)


def test_xxh32_matches_every_checksum_inside_the_fixtures():
    counted = 0
    for name, fx in M.fixtures().items():
        frame = fx["frame"]
        code, head = M.header(frame)      # (checks HC against the model's xxh32)
        assert code == 0, name
        assert bool(head.flg & M.F_BSUM) == fx["block_sums"], name
        assert bool(head.flg & M.F_CSUM) == fx["content_sum"], name
        assert (head.content_size is not None) == fx["content_size"], name
        assert bool(head.flg & M.F_INDEP) != fx["linked"] and head.bmax == M.block_max(fx["bsid"])
        code, blocks, end = M.walk(frame, head)
        assert code == 0 and end == len(frame), name
        for b in blocks:
            if b.want is not None:
                assert M.xxh32(frame[b.at:b.at + b.size]) == b.want, name
                counted += 1
        if fx["content_sum"]:
            assert M.xxh32(fx["content"]) == struct.unpack_from("<I", frame, end - 4)[0], name
            counted += 1
        counted += 1
    assert counted >= 30


def test_the_fixtures_are_the_frames_the_issue_lists():
    fx = M.fixtures()
    assert len(fx) == 13
    for mode in ("indep", "linked"):
        for tag in ("none", "bsum", "content_size", "all"):
            f = fx[mode + "_" + tag]
            assert len(f["content"]) == 3 * 65536 + 100 and M.info(f["frame"])[3] == 4
    # the linked frames reach back: the same content, fewer bytes
    assert len(fx["linked_none"]["frame"]) < len(fx["indep_none"]["frame"]) - 1000
    _, head = M.header(fx["random_block_all"]["frame"])
    assert M.walk(fx["random_block_all"]["frame"], head)[1][0].stored
    assert M.info(fx["id5_two_blocks"]["frame"])[2:4] == [262144, 2]
    assert M.info(fx["id7_short"]["frame"])[2:4] == [4 << 20, 1]
    assert M.info(fx["empty"]["frame"])[3:6] == [0, len(fx["empty"]["frame"]), 0]
    assert fx["one_byte"]["content"] == b"A"


def test_the_model_decodes_every_fixture():
    for name, fx in M.fixtures().items():
        bound = M.info(fx["frame"])[5]
        assert M.decode(fx["frame"], bound) == (len(fx["content"]), fx["content"]), name
        assert M.decode(fx["frame"], bound, flags=M.NO_VERIFY)[0] == len(fx["content"]), name
        want = -3 if fx["linked"] else len(fx["content"])
        assert M.decode(fx["frame"], bound, flags=M.NO_LINKED)[0] == want, name
        if bound:
            assert M.decode(fx["frame"], bound - 1)[0] == -9, name


# ---- liblz4, where it loads ----
@pytest.fixture(scope="module")
def liblz4():
    try:
        L = C.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("no liblz4.so.1 on this machine")
    L.LZ4F_isError.argtypes = [C.c_size_t]
    L.LZ4F_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]
    L.LZ4F_createDecompressionContext.restype = C.c_size_t
    L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    L.LZ4F_decompress.restype = C.c_size_t
    L.LZ4F_decompress.argtypes = [C.c_void_p] * 6
    return L


def _liblz4_run(L, frame, room):
    """(what liblz4 made of the frame, "done" | "error" | "more": it finished the frame,
    reported an error, or still wanted input when the bytes ran out)."""
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        out = C.create_string_buffer(max(room, 1))
        src = C.create_string_buffer(bytes(frame), max(len(frame), 1))
        at, made, hint = 0, 0, 1
        while at < len(frame) and hint:
            dn, sn = C.c_size_t(room - made), C.c_size_t(len(frame) - at)
            hint = L.LZ4F_decompress(ctx, C.byref(out, made), C.byref(dn), C.byref(src, at),
                                     C.byref(sn), None)
            if L.LZ4F_isError(hint):
                return out.raw[:made], "error"
            if not dn.value and not sn.value:
                return out.raw[:made], "error"
            at += sn.value
            made += dn.value
        return out.raw[:made], "more" if hint else "done"
    finally:
        L.LZ4F_freeDecompressionContext(ctx)


def _liblz4_decode(L, frame, room):
    """The content, or None when liblz4 does not finish the frame."""
    out, how = _liblz4_run(L, frame, room)
    return out if how == "done" else None


def test_liblz4_restores_every_model_built_frame(liblz4):
    whole = M.content_of([["text", 3000, 1, max(SIZES)]])
    inputs = [whole[:n] for n in SIZES]
    inputs.append(M.content_of([["rand", 65536, 9, 65536], ["text", 1000, 2, 1000]]))
    for data in inputs:
        for flags in range(8):
            frame = M.compress(data, flags)
            assert len(frame) <= M.compress_bound(len(data), flags)
            assert _liblz4_decode(liblz4, frame, len(data) + 16) == data, (len(data), flags)
    data = inputs[-1]
    for flags in range(8):      # the random block went in stored, the text after it did not
        frame = M.compress(data, flags)
        assert [b.stored for b in M.walk(frame, M.header(frame)[1])[1]] == [True, False]
    assert _liblz4_decode(liblz4, M.compress(data, 7, all_stored=True), len(data)) == data
    assert len(M.compress(data, 7, all_stored=True)) == M.compress_bound(len(data), 7)


def test_liblz4_reads_its_own_fixtures_through_this_harness(liblz4):
    for name, fx in M.fixtures().items():
        assert _liblz4_decode(liblz4, fx["frame"], len(fx["content"]) + 16) == fx["content"], name


# ---- corruptions ----
CODES = {"flipped data byte, block checksums": -6, "flipped content checksum": -7,
         "wrong header checksum": -1, "reserved bit, checksum redone": -1, "dictionary ID": -3,
         "skippable magic": -3, "cut inside a block": -2, "cut inside the trailer": -2,
         "changed content size": -8, "two 100-byte blocks": -5,
         "declared size 1, a full block, then 00": -4,
         "declared size 200, a 100-byte block, then 00": -5,
         "declared size 0, 1025 blocks 00 at 4 MiB": -5,
         "one block more than max_blocks": M.ERANGE, "capacity one short": -9}


def test_every_corruption_gets_its_code():
    cases = M.corruptions()
    assert {c.name: c.code for c in cases} == CODES
    for c in cases:
        assert M.decode(c.frame, c.cap, c.max_blocks)[0] == c.code, c.name
        assert M.info(c.frame)[0] == (c.code if c.header_stage else 0), c.name
        if c.lenient is not None:
            assert M.decode(c.frame, c.cap, c.max_blocks, M.NO_VERIFY) == (len(c.lenient), c.lenient)
        else:
            assert M.decode(c.frame, c.cap, c.max_blocks, M.NO_VERIFY)[0] == c.code, c.name


def test_liblz4_rejects_every_malformed_frame(liblz4):
    """The frames that break the format.  The other cases are well-formed frames that meet a
    limit of this decoder (a dictionary ID, a skippable frame, flushed short blocks) or of the
    call (max_blocks, the capacity): what liblz4 makes of each of those is pinned below."""
    cases = M.corruptions()
    assert sum(c.malformed for c in cases) == 9 and len(cases) == 15
    for c in cases:
        if c.malformed:
            assert _liblz4_decode(liblz4, c.frame, 4 * 65536) is None, c.name
    by_name = {c.name: c for c in cases}
    text = M.fixtures()["indep_all"]["content"]
    assert _liblz4_decode(liblz4, by_name["two 100-byte blocks"].frame, 4 * 65536) == text[:200]
    # a dictionary ID on blocks that use no dictionary: liblz4 decodes them without one
    for name in ("one block more than max_blocks", "capacity one short", "dictionary ID"):
        assert _liblz4_decode(liblz4, by_name[name].frame, 4 * 65536) == text
    # empty blocks are blocks to liblz4: 1025 of them make the declared 0 bytes
    assert _liblz4_decode(liblz4, by_name["declared size 0, 1025 blocks 00 at 4 MiB"].frame, 16) == b""
    # a skippable magic in front of a frame's remains: liblz4 takes the next four bytes (FLG,
    # BD, HC, a size byte) as the length to skip, produces nothing and runs out of input
    assert _liblz4_run(liblz4, by_name["skippable magic"].frame, 4 * 65536) == (b"", "more")


# ---- wrong neighbours ----
def test_the_fixtures_tell_the_header_checksum_from_its_unshifted_neighbour():
    told = 0
    for name, fx in M.fixtures().items():
        d = fx["frame"][4:M.header(fx["frame"])[1].size - 1]
        assert fx["frame"][4 + len(d)] == M.header_checksum(d)
        if M.header_checksum(d, shift=0) != M.header_checksum(d):
            assert M.header(fx["frame"], shift=0)[0] == -1, name
            told += 1
    assert told >= 10


def test_the_fixtures_tell_the_block_checksum_from_one_over_the_decoded_bytes():
    told = 0
    for name, fx in M.fixtures().items():
        if not fx["block_sums"]:
            continue
        bound = M.info(fx["frame"])[5]
        assert M.decode(fx["frame"], bound)[0] == len(fx["content"])
        assert M.decode(fx["frame"], bound, sum_of_decoded=True)[0] == -6, name
        told += 1
    assert told == 6
    # and a frame built with that neighbour's checksums is what the model rejects
    data = M.fixtures()["indep_all"]["content"][:70000]
    head = M.frame_header(0x40 | M.F_INDEP | M.F_BSUM, 4)
    wrong = head + M.frame_block(data[:65536], True, sum_of_decoded=True) + \
        M.frame_block(data[65536:], True, sum_of_decoded=True) + struct.pack("<I", 0)
    assert M.decode(wrong, 2 * 65536)[0] == -6
    assert M.decode(M.compress(data, M.BLOCK_CHECKSUMS), 2 * 65536) == (len(data), data)
