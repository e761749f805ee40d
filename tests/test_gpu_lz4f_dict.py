"""The calls of include/ape_lz4f_dict.h on the GPU against tests/lz4fdictmodel.py: framed compress
against a prepared dictionary per frame, byte for byte; the framed decode that picks each frame's
dictionary from a table, on liblz4's dictionary frames (tests/golden/lz4f_dict_golden.json), on
the existing fixtures with an empty table beside the existing calls, and on the frames the
compressor wrote; the ten info ints.  No liblz4 here: the fixtures carry its frames."""
import functools

import pytest

import inputs
import lz4fdictmodel as DM
import lz4fmodel as M
import lz4fplacedmodel as P
from gpuutil import CANARY, alloc_out, fetch, ints, pack

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
ERANGE = M.ERANGE
MS = 4096
MODES = (DM.FAST, DM.HC, DM.HC_OPT)
DEPTH = 8
IDS = (0, 77, 0x80000001)          # of the three dictionaries below


def _i32s(cuda, xs):
    return ints(cuda, [M._i32(x & 0xFFFFFFFF) for x in xs])


def _ptrs(cuda, values):
    return cuda.tensor(list(values), dtype=cuda.int64, device="cuda")


def _scratch(cuda, nbytes, fill=0x33):
    assert 0 < nbytes < 1 << 31
    return cuda.full((nbytes,), fill, dtype=cuda.uint8, device="cuda")


# ---------------- compress ----------------
@functools.lru_cache(maxsize=1)
def dicts():
    """100, 4096 and 61440 bytes"""
    ds = DM.dictionaries()
    return [ds["d60k"][-100:], ds["d4k"], ds["d60k"]]


def message(k, n):
    """n bytes that refer to dictionary k: pieces of it, then text of their own"""
    d = dicts()[k]
    own = d[-100:] + d[len(d) // 2:len(d) // 2 + 700] + inputs.make("text", 900, 20 + k) + \
        d[:600] + inputs.make("text", 2000, 30 + k)
    assert len(own) >= MS or k == 0
    return (own * 2)[:n]


class Objects:
    """The three dictionaries prepared in one batch per kind, for max_src, and the bad ones."""

    def __init__(self, cuda, amd, max_src=MS):
        self.keep, dptr, _ = pack(cuda, dicts(), misalign=[3, 0, 9])
        sizes = ints(cuda, map(len, dicts()))
        self.fast = cuda.full((3 * amd.cdict_size(),), 0x5A, dtype=cuda.uint8, device="cuda")
        self.hc = cuda.full((3 * amd.hc_cdict_size(),), 0x5A, dtype=cuda.uint8, device="cuda")
        amd.cdict_prepare_batch(dptr, sizes, max_src, self.fast, amd.cdict_size())
        amd.hc_cdict_prepare_batch(dptr, sizes, max_src, self.hc, amd.hc_cdict_size())
        # never prepared; prepared for other sizes
        self.raw = cuda.full((amd.hc_cdict_size(),), 0x5A, dtype=cuda.uint8, device="cuda")
        self.small = cuda.full((amd.cdict_size(),), 0x5A, dtype=cuda.uint8, device="cuda")
        self.other = cuda.full((amd.hc_cdict_size(),), 0x5A, dtype=cuda.uint8, device="cuda")
        amd.cdict_prepare_batch(dptr[1:2], sizes[1:2], 1000, self.small, amd.cdict_size())
        amd.hc_cdict_prepare_batch(dptr[1:2], sizes[1:2], max_src // 2, self.other,
                                   amd.hc_cdict_size())
        cuda.cuda.synchronize()
        self.amd = amd

    def good(self, mode, k):
        t, size = (self.fast, self.amd.cdict_size()) if mode == DM.FAST else \
            (self.hc, self.amd.hc_cdict_size())
        return t.data_ptr() + k * size

    def bad(self, mode):
        """null, misaligned, of the other kind, never prepared, prepared for another size (hc)"""
        wrong_kind = self.good(DM.HC if mode == DM.FAST else DM.FAST, 1)
        out = [0, self.good(mode, 1) + 8, wrong_kind, self.raw.data_ptr()]
        return out + ([self.other.data_ptr()] if mode != DM.FAST else [])


@pytest.fixture(scope="module")
def objects(cuda, product):
    return Objects(cuda, product)


def compress(cuda, amd, msgs, objs, ids, mode, flags, caps, max_src=MS, sizes=None, depth=DEPTH):
    """(results, the frames, whether each destination is untouched) of one call"""
    n = len(msgs)
    keep, sptr, _ = pack(cuda, msgs, misalign=[(7 * k + 3) % 16 for k in range(n)])
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(5 * k + 1) % 16 for k in range(n)])
    res = ints(cuda, [POISON] * n)
    scr = _scratch(cuda, amd.lz4f_compress_cdicts_scratch_size(n, max_src, mode))
    amd.lz4f_compress_cdicts_batch(
        sptr, ints(cuda, map(len, msgs) if sizes is None else sizes), dptr, ints(cuda, caps), res,
        _ptrs(cuda, objs), None if ids is None else _i32s(cuda, ids), max_src, mode,
        depth if mode else 0, flags, scr)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    outs = [fetch(dst, o, max(r, 0)) for o, r in zip(offs, rs)]
    clean = [fetch(dst, o, max(c, 0)) == bytes([CANARY]) * max(c, 0) for o, c in zip(offs, caps)]
    return rs, outs, clean


def _batch(mode, objects):
    """[(message, object, the dictionary behind it or None, ID)]: every size against the three
    dictionaries in turn, then the bad objects."""
    out = []
    for n in (0, 1, 13, 1000, MS):
        for k in range(3):
            out.append((message(k, n), objects.good(mode, k), dicts()[k], IDS[k]))
    for j, obj in enumerate(objects.bad(mode)):
        out.append((message(1, 1000), obj, None, IDS[j % 3]))
    return out


_made = {}


@pytest.mark.parametrize("mode", MODES)
def test_frames_equal_the_models_byte_for_byte(product, cuda, objects, mode):
    """Capacity exact; then one short: 0 and nothing written.  A message above maxSrcSize, and
    one of negative size, between them."""
    batch = _batch(mode, objects)
    want = [DM.compress(m, d, MS, i, mode, DEPTH, 7) for m, _, d, i in batch]
    msgs = [b[0] for b in batch] + [message(2, MS + 1), message(2, 100)]
    objs = [b[1] for b in batch] + [objects.good(mode, 2)] * 2
    ids = [b[3] for b in batch] + [0, 0]
    sizes = [len(m) for m in msgs[:-1]] + [-5]
    caps = [len(w) for w in want] + [1 << 13, 1 << 13]
    rs, outs, clean = compress(cuda, product, msgs, objs, ids, mode, 7, caps, sizes=sizes)
    assert rs == [len(w) for w in want] + [ERANGE, 0]
    assert outs[:-2] == want
    assert clean[-2] and clean[-1]
    # the bad objects gave valid frames with a stored block, the good ones used their dictionary
    for (m, _, d, i), frame in zip(batch, outs):
        if d is None:
            assert len(frame) == DM.compress_bound(len(m), 7) - (0 if i else 4)
            assert DM.decode(frame, len(m), [(i, b"")], flags=DM.ANY_SIZE) == (len(m), m)
        elif len(m) >= 1000:   # (the 100-byte dictionary is worth little)
            assert len(frame) < (len(m) // 2 if len(d) >= 4096 else len(m))
    _made[mode] = (batch, outs[:-2])
    short = [c - 1 for c in caps[:-2]]
    rs, _, clean = compress(cuda, product, msgs[:-2], objs[:-2], ids[:-2], mode, 7, short)
    assert rs == [0] * len(short) and all(clean)


def test_every_flag_combination_and_no_id_array(product, cuda, objects):
    picks = [(message(k, n), objects.good(DM.FAST, k), dicts()[k], IDS[k])
             for k, n in ((0, 13), (1, 1000), (2, MS), (2, 0))]
    for flags in range(8):
        for with_ids in (True, False):
            want = [DM.compress(m, d, MS, i if with_ids else 0, DM.FAST, 0, flags)
                    for m, _, d, i in picks]
            rs, outs, _ = compress(cuda, product, [p[0] for p in picks], [p[1] for p in picks],
                                   [p[3] for p in picks] if with_ids else None, DM.FAST, flags,
                                   [product.lz4f_compress_cdicts_bound(len(p[0]), flags)
                                    for p in picks])
            assert outs == want and rs == [len(w) for w in want], (flags, with_ids)


def test_the_fast_objects_own_limit_is_erange(product, cuda, objects):
    msgs = [message(1, 1000), message(1, 1001), message(1, 999)]
    want = [DM.compress(m, dicts()[1], 1000, 5, DM.FAST, 0, 1) for m in (msgs[0], msgs[2])]
    rs, outs, clean = compress(cuda, product, msgs, [objects.small.data_ptr()] * 3, [5] * 3,
                               DM.FAST, 1, [1 << 11] * 3)
    assert rs == [len(want[0]), ERANGE, len(want[1])] and clean[1]
    assert [outs[0], outs[2]] == want


@pytest.mark.parametrize("mode", MODES)
def test_max_src_65536_leaves_no_window(product, cuda, mode):
    """D = 0: the frame is that of a message without a dictionary."""
    big = Objects(cuda, product, 65536)
    msgs = [message(2, 3000), message(1, 1), inputs.make("text", 700, 5) * 3]
    want = [DM.compress(m, dicts()[2], 65536, 77, mode, DEPTH, 5) for m in msgs]
    assert want == [DM.compress(m, b"", 65536, 77, mode, DEPTH, 5) for m in msgs]
    rs, outs, _ = compress(cuda, product, msgs, [big.good(mode, 2)] * 3, [77] * 3, mode, 5,
                           [len(w) for w in want], max_src=65536)
    assert outs == want and rs == [len(w) for w in want]


# ---------------- decode ----------------
class Table:
    """[(key, dictionary bytes; or ("null", size) / ("size", n) for an unusable entry)] on the
    device."""

    def __init__(self, cuda, entries):
        blobs = [d if isinstance(d, bytes) else b"" for _, d in entries]
        self.keep, ptrs, _ = pack(cuda, blobs,
                                  misalign=[(3 * k + 5) % 16 for k in range(len(blobs))])
        ptrs, sizes = ptrs.cpu().tolist(), [len(b) for b in blobs]
        for k, (_, d) in enumerate(entries):
            if not isinstance(d, bytes):
                ptrs[k], sizes[k] = (0, d[1]) if d[0] == "null" else (ptrs[k], d[1])
        self.ids = _i32s(cuda, [key for key, _ in entries])
        self.ptrs, self.sizes = _ptrs(cuda, ptrs), ints(cuda, sizes)
        self.model = [(key, d if isinstance(d, bytes) else b"" if d == ("null", 0) else None)
                      for key, d in entries]


def decode(cuda, amd, frames, caps, table, max_blocks, flags, shift=0, old=False):
    """(results, the decoded bytes per frame, whether each destination is untouched); old: the
    existing call of the same placement, which takes no table."""
    n = len(frames)
    keep, sptr, _ = pack(cuda, frames, misalign=[(7 * k + 3) % 16 for k in range(n)])
    dst, dptr, offs = alloc_out(cuda, caps, misalign=[(5 * k + 1 + shift) % 16 for k in range(n)])
    res = ints(cuda, [POISON] * n)
    sizes, capt = ints(cuda, map(len, frames)), ints(cuda, caps)
    if old:
        placed = bool(flags & DM.ANY_SIZE)
        scr = _scratch(cuda, (amd.lz4f_decompress_placed_scratch_size if placed
                              else amd.lz4f_decompress_scratch_size)(n, max_blocks))
        (amd.lz4f_decompress_placed_batch if placed else amd.lz4f_decompress_batch)(
            sptr, sizes, dptr, capt, res, max_blocks, flags & 3, scr)
    else:
        scr = _scratch(cuda, amd.lz4f_decompress_dicts_scratch_size(n, max_blocks, flags))
        amd.lz4f_decompress_dicts_batch(sptr, sizes, dptr, capt, res, max_blocks, table.ids,
                                        table.ptrs, table.sizes, flags, scr)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    outs = [fetch(dst, o, max(r, 0)) for o, r in zip(offs, rs)]
    clean = [fetch(dst, o, max(c, 0)) == bytes([CANARY]) * max(c, 0) for o, c in zip(offs, caps)]
    return rs, outs, clean


def fixture_table(cuda):
    ds = DM.dictionaries()
    return Table(cuda, [(77, ds["d60k"]), (0x80000001, ds["d70k"]), (5, ds["d4k"]),
                        (0, ds["d4k"])])


def _room(frame):
    inf = DM.info(frame)
    return max(inf[5], inf[3] * inf[2], 1)


@functools.lru_cache(maxsize=None)
def _want(name, placed):
    """The model on a fixture, once: at the exact capacity when placed, else at blocks x
    maximum.  (Not verifying gives the same on these intact frames:
    tests/test_lz4f_dict_model.py.)"""
    f = DM.fixtures()[name]
    table = DM.table_for(f)
    if placed:
        return DM.decode(f["frame"], len(f["content"]), table, 4, DM.ANY_SIZE)
    return DM.decode(f["frame"], _room(f["frame"]), table, 4, 0)


@pytest.mark.parametrize("placed", [False, True])
def test_every_fixture_through_the_table(product, cuda, placed):
    fx = list(DM.fixtures().values())
    table = fixture_table(cuda)
    frames = [f["frame"] for f in fx]
    caps = [len(f["content"]) if placed else _room(f["frame"]) for f in fx]
    want = [_want(f["name"], placed) for f in fx]
    assert sum(w[0] >= 0 for w in want) == (23 if placed else 19)
    assert sorted({w[0] for w in want if w[0] < 0}) == ([-3] if placed else [-5])
    for verify in (True, False):
        flags = (DM.ANY_SIZE if placed else 0) | (0 if verify else M.NO_VERIFY)
        rs, outs, clean = decode(cuda, product, frames, caps, table, 4, flags, shift=4 * verify)
        assert rs == [w[0] for w in want], flags
        assert all(o == w[1] for o, w in zip(outs, want) if w[0] >= 0), flags
        # the unsupported linked shape leaves its destination as it was
        assert all(ok for ok, w in zip(clean, want) if w[0] == -3)


def test_an_absent_id_and_an_unusable_entry_are_minus_10(product, cuda):
    ds, fx = DM.dictionaries(), DM.fixtures()
    table = Table(cuda, [(77, ds["d60k"]), (0x80000001, ("null", 70000)), (9, ("size", -1)),
                         (9, ds["d4k"]), (0, ds["d4k"]), (11, ("null", 0))])
    msg = message(1, 1000)
    names = ["four_k_d60k_indep_id4_all", "four_k_d70k_indep_id4_none", "four_k_d4k_indep_id4_none",
             "three_d70k_linked_id4_none", "flush_short_d60k_indep_id4_all"]
    frames = [fx[n]["frame"] for n in names] + \
        [DM.compress(msg, ds["d4k"], MS, i, DM.FAST, 0, 7) for i in (9, 1234, 11)]
    caps = [len(fx[n]["content"]) for n in names] + [1000] * 3
    for flags in (DM.ANY_SIZE, DM.ANY_SIZE | M.NO_VERIFY | M.NO_LINKED):
        want = [DM.decode(f, c, table.model, 4, flags) for f, c in zip(frames, caps)]
        # (a null pointer with size 0 is an empty dictionary; flag 2's -3 comes before -10)
        assert [w[0] for w in want] == [4000, -10, 4000, -10 if flags == DM.ANY_SIZE else -3,
                                        5101, -10, -10, -4]
        rs, outs, clean = decode(cuda, product, frames, caps, table, 4, flags)
        assert rs == [w[0] for w in want]
        assert all(o == w[1] for o, w in zip(outs, want) if w[0] >= 0)
        assert all(ok for ok, w in zip(clean, want) if w[0] < 0)
    # the grid call: -10 comes before -9
    rs, _, clean = decode(cuda, product, frames, [0] * len(frames), table, 4, 0)
    assert rs == [-9, -10, -9, -10, -9, -10, -10, -9] and all(clean)


def test_a_table_of_130_entries(product, cuda):
    """The match at index 0, 64 and 129; of two entries with one key the first counts."""
    ds, fx = DM.dictionaries(), DM.fixtures()
    entries = [(1000 + k, ds["d4k"][:16]) for k in range(130)]
    entries[0] = (77, ds["d60k"])
    entries[64] = (0x80000001, ds["d70k"])
    entries[129] = (0, ds["d4k"])
    entries[100] = (77, ds["d4k"])                     # later: never looked at
    entries[70] = (0x80000001, ("size", -1))
    entries[3] = (1003, ("null", 5))
    table = Table(cuda, entries)
    names = ["four_k_d60k_indep_id4_all", "four_k_d70k_indep_id4_none", "four_k_d4k_indep_id4_none",
             "three_d70k_indep_id4_all", "three_d4k_linked_id4_all"]
    frames = [fx[n]["frame"] for n in names]
    caps = [len(fx[n]["content"]) for n in names]
    rs, outs, _ = decode(cuda, product, frames, caps, table, 4, DM.ANY_SIZE)
    assert rs == caps and outs == [fx[n]["content"] for n in names]
    # ... and the other way round the first still counts
    entries[0], entries[100] = entries[100], entries[0]
    entries[64], entries[70] = entries[70], entries[64]
    table = Table(cuda, entries)
    want = [DM.decode(f, c, table.model, 4, DM.ANY_SIZE) for f, c in zip(frames, caps)]
    assert [w[0] for w in want] == [-4, -10, 4000, -10, caps[4]]
    rs, outs, clean = decode(cuda, product, frames, caps, table, 4, DM.ANY_SIZE)
    assert rs == [w[0] for w in want] and clean[0] and clean[1] and clean[3]


@pytest.mark.parametrize("placed", [False, True])
def test_an_empty_table_is_the_existing_call(product, cuda, placed):
    """Every existing fixture, every corruption and the frames of many blocks: result for result
    and byte for byte what the existing call of the same placement gives on the same batch, but
    -10 where a frame has an ID."""
    import lz4fmany as X
    flag = DM.ANY_SIZE if placed else 0
    empty = Table(cuda, [])
    plain = [f for f in list(M.fixtures().values()) + list(P.fixtures().values())]
    groups = [([f["frame"] for f in plain], [_room(f["frame"]) for f in plain], 40)]
    for max_blocks in sorted({c.max_blocks for c in M.corruptions()}):
        cs = [c for c in M.corruptions() if c.max_blocks == max_blocks]
        groups.append(([c.frame for c in cs], [c.cap for c in cs], max_blocks))
    many = [m[0] for m in X.short_frames()] + [X.one_block()[0], X.unsized_block_70(),
                                               X.flipped_block_100()]
    groups.append((many, [X.bound(f) for f in many], X.SHORT_BLOCKS))
    big = [m[0] for m in X.big_frames()]
    groups.append((big, [X.bound(f) for f in big], X.BIG_BLOCKS))
    with_id = 0
    for frames, caps, max_blocks in groups:
        for flags in (flag, flag | M.NO_VERIFY, flag | M.NO_LINKED):
            if len(frames[0]) > 1 << 20 and flags != flag:
                continue
            new = decode(cuda, product, frames, caps, empty, max_blocks, flags)
            old = decode(cuda, product, frames, caps, empty, max_blocks, flags, old=True)
            for k, frame in enumerate(frames):
                if DM.header(frame)[2] is not None:
                    assert (old[0][k], new[0][k]) == (-3, -10) and new[2][k]
                    with_id += 1
                else:
                    assert (new[0][k], new[1][k]) == (old[0][k], old[1][k]), (max_blocks, flags, k)
    assert with_id == 3
    # ... and on liblz4's dictionary frames: the ones without an ID lack their dictionary
    fx = list(DM.fixtures().values())
    frames, caps = [f["frame"] for f in fx], [_room(f["frame"]) for f in fx]
    new = decode(cuda, product, frames, caps, empty, 4, flag)
    old = decode(cuda, product, frames, caps, empty, 4, flag, old=True)
    for k, f in enumerate(fx):
        if f["dict_id"]:
            assert (old[0][k], new[0][k]) == (-3, -10), f["name"]
        else:
            assert (new[0][k], new[1][k]) == (old[0][k], old[1][k]), f["name"]
            assert new[0][k] == (1 if len(f["content"]) == 1 else -4), f["name"]


@pytest.mark.parametrize("mode", MODES)
def test_round_trip_through_the_gpu_decode(product, cuda, objects, mode):
    """The compressor's frames (written here if that test did not run), bad objects' among
    them, through the table with the ORIGINAL dictionaries: both placements."""
    if mode in _made:
        batch, frames = _made[mode]
    else:
        batch = _batch(mode, objects)
        caps = [product.lz4f_compress_cdicts_bound(len(b[0]), 7) for b in batch]
        _, frames, _ = compress(cuda, product, [b[0] for b in batch], [b[1] for b in batch],
                                [b[3] for b in batch], mode, 7, caps)
    table = Table(cuda, [(i, d) for i, d in zip(IDS, dicts())])
    msgs = [b[0] for b in batch]
    rs, outs, _ = decode(cuda, product, frames, [len(m) for m in msgs], table, 1, DM.ANY_SIZE)
    assert rs == [len(m) for m in msgs] and outs == msgs
    rs, outs, _ = decode(cuda, product, frames, [max(len(m), 65536) for m in msgs], table, 1, 0)
    assert rs == [len(m) for m in msgs] and outs == msgs


def test_the_info_call(product, cuda):
    frames = [f["frame"] for f in DM.fixtures().values()] + [c.frame for c in M.corruptions()] + \
        [f["frame"] for f in M.fixtures().values()]
    n = len(frames)
    keep, sptr, _ = pack(cuda, frames, misalign=[(3 * k + 1) % 16 for k in range(n)])
    sizes = ints(cuda, map(len, frames))
    info, old = ints(cuda, [POISON] * (10 * n)), ints(cuda, [POISON] * (8 * n))
    product.lz4f_info_dict_batch(sptr, sizes, info)
    product.lz4f_info_batch(sptr, sizes, old)
    cuda.cuda.synchronize()
    got, was = info.cpu().tolist(), old.cpu().tolist()
    for k, frame in enumerate(frames):
        assert got[10 * k:10 * k + 10] == DM.info(frame), k
        if not got[10 * k + 8]:
            assert got[10 * k:10 * k + 8] == was[8 * k:8 * k + 8], k
    assert sum(got[8::10]) == sum(1 for f in frames if DM.header(f)[2] is not None) > 10


def test_capture_into_a_graph_and_replay(product, cuda, objects):
    """Compress against the objects, then decode through the table, in one captured graph."""
    batch = _batch(DM.HC, objects)[:12]
    n = len(batch)
    msgs = [b[0] for b in batch]
    keep, sptr, _ = pack(cuda, msgs, misalign=[(k + 1) % 16 for k in range(n)])
    caps = [product.lz4f_compress_cdicts_bound(len(m), 3) for m in msgs]
    mid, mptr, moffs = alloc_out(cuda, caps, misalign=[(3 * k + 2) % 16 for k in range(n)])
    dst, dptr, doffs = alloc_out(cuda, [len(m) for m in msgs])
    sizes, capt, room = ints(cuda, map(len, msgs)), ints(cuda, caps), ints(cuda, map(len, msgs))
    fres, res = ints(cuda, [POISON] * n), ints(cuda, [POISON] * n)
    objs, ids = _ptrs(cuda, [b[1] for b in batch]), _i32s(cuda, [b[3] for b in batch])
    table = Table(cuda, [(i, d) for i, d in zip(IDS, dicts())])
    cscr = _scratch(cuda, product.lz4f_compress_cdicts_scratch_size(n, MS, DM.HC))
    dscr = _scratch(cuda, product.lz4f_decompress_dicts_scratch_size(n, 1, DM.ANY_SIZE))
    st = cuda.cuda.Stream()
    st.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=st):
        product.lz4f_compress_cdicts_batch(sptr, sizes, mptr, capt, fres, objs, ids, MS, DM.HC,
                                           DEPTH, 3, cscr, stream=st)
        product.lz4f_decompress_dicts_batch(mptr, fres, dptr, room, res, 1, table.ids, table.ptrs,
                                            table.sizes, DM.ANY_SIZE, dscr, stream=st)
    for t, v in ((fres, POISON), (res, POISON), (cscr, 0x55), (dscr, 0x55), (mid, CANARY),
                 (dst, CANARY)):
        t.fill_(v)
    g.replay()
    cuda.cuda.synchronize()
    want = [DM.compress(m, d, MS, i, DM.HC, DEPTH, 3) for m, _, d, i in batch]
    assert fres.cpu().tolist() == [len(w) for w in want]
    assert [fetch(mid, o, len(w)) for o, w in zip(moffs, want)] == want
    assert res.cpu().tolist() == [len(m) for m in msgs]
    assert [fetch(dst, o, len(m)) for o, m in zip(doffs, msgs)] == msgs


def test_an_empty_batch_launches_nothing(product, cuda):
    L = product.lib()
    assert L.APE_LZ4_lz4f_info_dict_batch_dev(None, None, None, 0, None) == 0
    assert L.APE_LZ4_lz4f_compress_usingCDicts_batch_dev(None, None, None, None, None, 0, None,
                                                         None, 4096, 2, 8, 7, None, 0, None) == 0
    assert L.APE_LZ4_lz4f_decompress_usingDicts_batch_dev(None, None, None, None, None, 0, 4, None,
                                                          None, None, 0, 7, None, 0, None) == 0
