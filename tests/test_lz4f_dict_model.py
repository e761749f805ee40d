"""tests/lz4fdictmodel.py against liblz4's dictionary frames (tests/golden/lz4f_dict_golden.json):
the model decodes every fixture to its content, its wrong neighbours are told apart on the
fixtures whose structure makes them differ, the frames it writes decode under itself and -- where
the system's liblz4 loads -- under LZ4F_decompress_usingDict with the caller's original
dictionary, and the existing models still refuse every frame with an ID.  No GPU."""
import ctypes as C
import struct

import pytest

import inputs
import lz4fdictmodel as DM
import lz4fmodel as M
import lz4fplacedmodel as P


def _fx():
    return DM.fixtures()


def _dict(fx):
    return DM.dictionaries()[fx["dict"]]


def _multi(fx):
    return DM.blocks_of(fx["frame"]) > 1


def test_the_fixtures_cover_what_they_should():
    fx = _fx()
    assert len(fx) == 25 and {len(d) for d in DM.dictionaries().values()} == {4096, 61440, 70000}
    assert {f["dict_id"] for f in fx.values()} == {0, 77, 0x80000001}
    assert {f["bsid"] for f in fx.values()} == {4, 5}
    assert {len(f["content"]) for f in fx.values() if f["pieces"] is None} == \
        {1, 100, 4000, 65536 + 65536 + 9000}
    for f in fx.values():
        flg = f["frame"][4]
        assert bool(flg & M.F_DICT) == (f["dict_id"] != 0), f["name"]
        assert bool(flg & M.F_BSUM) == f["block_sums"] and bool(flg & M.F_SIZE) == f["content_size"]
        # liblz4 marks a frame whose content fits one block as independent
        one = f["pieces"] is None and len(f["content"]) <= M.block_max(f["bsid"])
        assert f["indep"] == (not f["linked"] or one), f["name"]
    assert sum(1 for f in fx.values() if not f["indep"] and _multi(f)) == 8
    assert sum(1 for f in fx.values() if f["indep"] and _multi(f)) == 4
    # the example header of the format facts: ID 77, no content size
    assert M.frame_header(0x61, 4, None, 77).hex() == "04224d1861404d000000de"


def test_the_info_ints():
    for f in _fx().values():
        got = DM.info(f["frame"])
        assert got[0] == 0 and got[3] == DM.blocks_of(f["frame"]) and got[4] == len(f["frame"])
        assert got[8:] == [int(f["dict_id"] != 0), M._i32(f["dict_id"])], f["name"]
        if not f["dict_id"]:
            assert got[:8] == M.info(f["frame"]), f["name"]
        else:
            assert M.info(f["frame"]) == [-3, 0, 0, 0, 0, 0, -1, -1]
    for c in M.corruptions():
        old, new = M.info(c.frame), DM.info(c.frame)
        if c.name == "dictionary ID":
            assert old[0] == -3 and new[0] == 0 and new[8:] == [1, 7]
        else:
            assert new == old + [0, 0], c.name


@pytest.mark.parametrize("flags", [0, DM.ANY_SIZE, M.NO_VERIFY, DM.ANY_SIZE | M.NO_VERIFY])
def test_the_model_decodes_every_fixture(flags):
    shapes = 0
    for f in _fx().values():
        cap = len(f["content"])
        inf = DM.info(f["frame"])
        bound = max(inf[5], inf[3] * inf[2], cap)
        got = DM.decode(f["frame"], bound, DM.table_for(f), flags=flags)
        low = not f["indep"] and f["pieces"] is not None and f["pieces"][0] < 65536
        short = f["pieces"] is not None and any(n != M.block_max(f["bsid"])
                                                for n in f["pieces"][:-1])
        if flags & DM.ANY_SIZE:
            want = (-3, None) if low else (cap, f["content"])
            shapes += low
        else:
            want = (-5, None) if short else (cap, f["content"])
        assert got == want, f["name"]
        if flags & DM.ANY_SIZE and not low:      # the exact capacity, and one short
            assert DM.decode(f["frame"], cap, DM.table_for(f), flags=flags) == want
            assert DM.decode(f["frame"], cap - 1, DM.table_for(f), flags=flags)[0] == -9
    assert shapes == (2 if flags & DM.ANY_SIZE else 0)


def test_the_unsupported_shape_is_decided_after_sizing_and_before_the_capacity():
    f = _fx()["flush_low_d4k_linked_id4_none"]
    table = DM.table_for(f)
    assert DM.decode(f["frame"], 0, table, flags=DM.ANY_SIZE)[0] == -3           # before -9
    assert DM.decode(f["frame"], 7000, [], flags=DM.ANY_SIZE)[0] == -4           # no dictionary
    assert DM.decode(f["frame"], 7000, [(0, b"")], flags=DM.ANY_SIZE)[0] == -4   # an empty one
    assert DM.decode(f["frame"], 7000, table, flags=DM.ANY_SIZE | M.NO_LINKED)[0] == -3
    g = _fx()["flush_low_d60k_linked_id4_all"]
    assert DM.decode(g["frame"], 7000, [], flags=DM.ANY_SIZE)[0] == DM.NO_DICTIONARY
    # a block that cannot be sized comes first
    frame = bytearray(f["frame"])
    _, head, _, blocks, _, _ = DM._stage(bytes(frame))
    frame[blocks[2].at + blocks[2].size - 1:blocks[2].at + blocks[2].size] = b""
    frame[blocks[2].at - 4:blocks[2].at] = struct.pack("<I", blocks[2].size - 1)
    assert DM.decode(bytes(frame), 7000, table, flags=DM.ANY_SIZE)[0] == -4


def _differs(f, wrong, flags=DM.ANY_SIZE, table=None):
    table = DM.table_for(f) if table is None else table
    inf = DM.info(f["frame"])
    cap = max(inf[5], inf[3] * inf[2], len(f["content"]))
    right = DM.decode(f["frame"], cap, table, flags=flags)
    assert right == (len(f["content"]), f["content"]), f["name"]
    return DM.decode(f["frame"], cap, table, flags=flags, wrong=wrong) != right


def test_wrong_neighbours_are_told_apart():
    fx = _fx()
    for flags in (0, DM.ANY_SIZE):
        # the dictionary given to block 0 only, in an independent frame of several blocks
        multi = [f for f in fx.values() if f["indep"] and _multi(f) and (
            flags or f["pieces"] is None)]
        assert len(multi) == (4 if flags else 2)
        assert all(_differs(f, "block0", flags) for f in multi)
        # the dictionary given to every block of a linked frame in place of the output before it
        linked = [f for f in fx.values() if not f["indep"] and f["name"].startswith("three")]
        assert len(linked) == 4 and all(_differs(f, "every_linked", flags) for f in linked)
        # the first instead of the last 64 KiB of the long dictionary
        long = [f for f in fx.values() if f["dict"] == "d70k" and len(f["content"]) >= 100 and
                (f["pieces"] is None or (flags and (f["indep"] or f["pieces"][0] == 65536)))]
        assert len(long) >= 6 and all(_differs(f, "first64k", flags) for f in long)
    # the header checksum without the ID bytes: every frame with an ID, and no other
    for f in fx.values():
        got = DM.decode(f["frame"], 1 << 18, DM.table_for(f), flags=DM.ANY_SIZE, wrong="no_id_sum")
        assert (got[0] == -1) == (f["dict_id"] != 0), f["name"]
    # a missing ID treated as -10: a frame without the field decodes without a dictionary
    plain = M.fixtures()["indep_all"]
    assert DM.decode(plain["frame"], 1 << 18, [(77, b"x")]) == \
        (len(plain["content"]), plain["content"])
    assert DM.decode(plain["frame"], 1 << 18, [(77, b"x")], wrong="missing")[0] == -10
    # ... and the fixtures do need theirs
    for f in fx.values():
        if len(f["content"]) >= 100:
            assert DM.decode(f["frame"], 1 << 18, [], flags=DM.ANY_SIZE)[0] == (
                -10 if f["dict_id"] else -4), f["name"]


def test_the_table_rules():
    f = _fx()["four_k_d60k_indep_id4_all"]
    d = _dict(f)
    want = (4000, f["content"])
    assert DM.decode(f["frame"], 4000, [(77, d), (77, None)]) == want          # the first wins
    assert DM.decode(f["frame"], 4000, [(77, None), (77, d)])[0] == -10        # ... unusable too
    assert DM.decode(f["frame"], 4000, [(0, d), (78, d)])[0] == -10
    assert DM.decode(f["frame"], 4000, [(77, b"")])[0] == -4                   # empty: legal
    assert DM.decode(f["frame"], 3999, [(77, d)])[0] == -9
    assert DM.decode(f["frame"], 3999, [])[0] == -10                           # before -9
    assert DM.decode(f["frame"], 4000, [], max_blocks=0)[0] == M.ERANGE        # after ERANGE
    assert DM.decode(f["frame"][:20], 4000, [])[0] == -2


def test_with_an_empty_table_the_model_equals_the_existing_ones():
    frames = [(f["frame"], max(len(f["content"]), 1), 40) for f in M.fixtures().values()] + \
        [(f["frame"], max(len(f["content"]), 1), 40) for f in P.fixtures().values()] + \
        [(c.frame, c.cap, c.max_blocks) for c in M.corruptions()]
    for frame, cap, max_blocks in frames:
        for flags in (0, M.NO_VERIFY, M.NO_LINKED):
            old = M.decode(frame, cap, max_blocks, flags)
            placed = P.decode_placed(frame, cap, max_blocks, flags)
            has_id = DM.header(frame)[2] is not None
            assert DM.decode(frame, cap, [], max_blocks, flags) == ((-10, None) if has_id else old)
            assert DM.decode(frame, cap, [], max_blocks, flags | DM.ANY_SIZE) == (
                (-10, None) if has_id else placed)


def test_the_existing_models_refuse_every_frame_with_an_id():
    for f in _fx().values():
        if f["dict_id"]:
            assert M.decode(f["frame"], 1 << 18)[0] == -3, f["name"]
            assert P.decode_placed(f["frame"], 1 << 18)[0] == -3, f["name"]


# ---------------- the frames the model writes ----------------
def _messages():
    ds = DM.dictionaries()
    d = ds["d60k"]
    own = d[1000:1600] + d[30000:30900] + d[61000:61440] + inputs.make("text", 500, 9)
    return [(b"", d), (b"a", d), (own[:13], d), (own[:1000], ds["d4k"] + own[200:300]),
            (own, d), (own, ds["d70k"] + d[:5000]), (inputs.make("rand", 700, 4), d)]


def test_the_models_frames_decode_under_the_model():
    for k, (msg, d) in enumerate(_messages()):
        for mode in (DM.FAST, DM.HC, DM.HC_OPT):
            for flags, dict_id in ((0, 0), (7, 77), (2, 0x80000001), (5, 0)):
                frame = DM.compress(msg, d, 4096, dict_id, mode, 8, flags)
                assert len(frame) <= DM.compress_bound(len(msg), flags)
                inf = DM.info(frame)
                assert inf[0] == 0 and inf[3] == (1 if msg else 0) and inf[4] == len(frame)
                assert inf[8:] == [int(dict_id != 0), M._i32(dict_id)]
                for dflags in (0, DM.ANY_SIZE):   # (the grid call wants room for its bound)
                    cap = len(msg) if dflags else max(len(msg), inf[5])
                    assert DM.decode(frame, cap, [(dict_id, d)], flags=dflags) == \
                        (len(msg), msg), (k, mode, flags)
                # the frame is a function of the object's window bytes alone
                assert frame == DM.compress(msg, DM.window_bytes(d, 4096, mode), 4096, dict_id,
                                            mode, 8, flags)
    msg, d = _messages()[4]
    used = [DM.compress(msg, d, 4096, 0, mode, 8, 0) for mode in (0, 1, 2)]
    assert all(len(f) < len(msg) // 2 for f in used)
    stored = DM.compress(msg, None, 4096, 77, 0, 0, 7)
    assert len(stored) == DM.compress_bound(len(msg), 7)
    assert DM.decode(stored, len(msg), [(77, None)])[0] == -10
    assert DM.decode(stored, len(msg), [(77, b"")]) == (len(msg), msg)


def _liblz4():
    for name in ("liblz4.so.1", "/usr/lib/x86_64-linux-gnu/liblz4.so.1.9.3"):
        try:
            L = C.CDLL(name)
            break
        except OSError:
            continue
    else:
        return None
    if not hasattr(L, "LZ4F_decompress_usingDict") or not hasattr(L, "LZ4F_createCDict"):
        return None
    L.LZ4F_isError.argtypes = [C.c_size_t]
    L.LZ4F_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]
    L.LZ4F_createDecompressionContext.restype = C.c_size_t
    L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    L.LZ4F_decompress_usingDict.restype = C.c_size_t
    L.LZ4F_decompress_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def _lib_decode(L, frame, dictionary, room):
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    out = C.create_string_buffer(room + 16)
    dst, src = C.c_size_t(room + 16), C.c_size_t(len(frame))
    r = L.LZ4F_decompress_usingDict(ctx, out, C.byref(dst), frame, C.byref(src), dictionary,
                                    len(dictionary), None)
    L.LZ4F_freeDecompressionContext(ctx)
    assert not L.LZ4F_isError(r) and r == 0 and src.value == len(frame), r
    return out.raw[:dst.value]


def test_liblz4_reads_the_models_frames_with_the_original_dictionary():
    L = _liblz4()
    if L is None:
        pytest.skip("the system has no liblz4 with LZ4F_decompress_usingDict")
    import gen_lz4f_dict_golden as G   # (tests/golden, beside inputs.py)
    lib = G.liblz4()
    for msg, d in _messages():
        for mode in (DM.FAST, DM.HC, DM.HC_OPT):
            for flags, dict_id in ((0, 0), (7, 77), (2, 0x80000001)):
                frame = DM.compress(msg, d, 4096, dict_id, mode, 8, flags)
                assert _lib_decode(L, frame, d, len(msg)) == msg, (mode, flags)
                # the header equals liblz4's for the same settings (to which a content size of
                # 0 means "unknown")
                if flags & 4 and not msg:
                    continue
                prefs = G.prefs_of(4, False, False, len(msg) if flags & 4 else 0, dict_id)
                prefs.frameInfo.contentChecksumFlag = flags & 1
                prefs.frameInfo.blockChecksumFlag = (flags >> 1) & 1
                cdict = lib.LZ4F_createCDict(d, len(d))
                theirs = G.make_frame(lib, cdict, msg, None, prefs)
                lib.LZ4F_freeCDict(cdict)
                n = DM.header(frame)[1].size
                assert theirs[:n] == frame[:n], (mode, flags, dict_id)
    # ... and the fixtures, as a check of this harness
    for f in _fx().values():
        assert _lib_decode(L, f["frame"], _dict(f), len(f["content"])) == f["content"], f["name"]
