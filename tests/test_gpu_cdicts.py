"""A prepared dictionary per message on the GPU (include/ape_lz4_cdicts.h):
APE_LZ4_compress_usingCDicts_batch_dev, APE_LZ4_compress_hc_usingCDicts_batch_dev,
APE_LZ4_compress_hc_opt_usingCDicts_batch_dev and the two batched prepares.

The rule under test adds no bytes of its own: message i gets what the single-dictionary call
writes for it against its own object, whatever the other messages name.  So the checker of a mixed
call is one single-dictionary call per group in the same process, every result and output byte
equal; the three CPU models on the messages they can afford; both usingDict decoders with each
message's ORIGINAL dictionary.  tests/cdictscorpus.py is the mixed batch (tests/
test_cdicts_corpus.py shows that it tells the objects apart), destinations are misaligned, and
the canaries behind every destination are checked after each test."""
import functools

import numpy as np
import pytest

import cdictscorpus as K
import encmodel
import hcdictmodel
import hcoptdictmodel
from gpuutil import CANARY, alloc_out, fetch, ints, pack
from test_gpu_cdict import dev_dict
from test_gpu_hc_large import first_difference
from test_gpu_stream import gpu_dict_decode, orc_dict_decode

pytestmark = pytest.mark.gpu

ERANGE = -2147483648
POISON = -7
MS = K.MAX_SRC
FAST, HC, OPT = "fast", "hc", "hc_opt"
ENCODERS = (FAST, HC, OPT)


def sets():
    return {s.name: s for s in K.sets()}


def object_size(amd, enc):
    return amd.cdict_size() if enc == FAST else amd.hc_cdict_size()


def single_prepare(torch, amd, enc, d, max_src=MS, fill=0x5A, odd=True):
    obj = torch.full((object_size(amd, enc),), fill, dtype=torch.uint8, device="cuda")
    prepare = amd.cdict_prepare if enc == FAST else amd.hc_cdict_prepare
    prepare(dev_dict(torch, d, odd), max_src, obj)
    return obj


_objects = {}


def objects(torch, amd, enc, name):
    """The set's four objects, prepared one by one, once per session: they are only read."""
    key = (FAST if enc == FAST else HC, name)
    if key not in _objects:
        _objects[key] = [single_prepare(torch, amd, enc, d) for d in sets()[name].dicts]
    return _objects[key]


def scratch_size(amd, enc, n, max_src=MS):
    return (amd.compress_hc_cdict_scratch_size if enc == HC
            else amd.compress_hc_opt_cdict_scratch_size)(n, max_src)


def new_scratch(torch, amd, enc, n, max_src=MS, fill=0xEE):
    return torch.full((scratch_size(amd, enc, n, max_src),), fill, dtype=torch.uint8, device="cuda")


def ptrs(torch, values):
    return torch.tensor(list(values), dtype=torch.int64, device="cuda")


def launch(torch, amd, enc, objs, msgs, depth=8, sizes=None, caps=None, scratch=None,
           stream=None, max_src=MS):
    """One call: objs is one tensor (the single-dictionary call) or a list with an object
    pointer (an int) per message (the new call).  Returns the device buffers and all they keep
    alive."""
    n = len(msgs)
    src, sptr, _ = pack(torch, msgs, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [amd.compressBound(len(m)) for m in msgs] if caps is None else caps
    sizes = [len(m) for m in msgs] if sizes is None else sizes
    dst, dptr, doffs = alloc_out(torch, caps, misalign=[(3 * i) % 16 for i in range(n)])
    res = ints(torch, [POISON] * n)
    sizes, capt = ints(torch, sizes), ints(torch, caps)
    per = isinstance(objs, list)
    obj = ptrs(torch, objs) if per else objs
    if stream is not None:   # the buffers above were filled on the current stream
        stream.wait_stream(torch.cuda.current_stream())
    if enc == FAST:
        f = amd.compress_cdicts_batch if per else amd.compress_cdict_batch
        f(sptr, sizes, dptr, capt, res, obj, stream=stream)
    else:
        scratch = new_scratch(torch, amd, enc, n, max_src) if scratch is None else scratch
        f = {(HC, True): amd.compress_hc_cdicts_batch, (HC, False): amd.compress_hc_cdict_batch,
             (OPT, True): amd.compress_hc_opt_cdicts_batch,
             (OPT, False): amd.compress_hc_opt_cdict_batch}[enc, per]
        f(sptr, sizes, dptr, capt, res, obj, max_src, depth, scratch, stream=stream)
    return res, dst, doffs, (src, sptr, dptr, sizes, capt, obj, scratch)


def collect(res, dst, doffs):
    rs = res.cpu().tolist()
    host = dst.cpu().numpy()
    return rs, [host[o:o + max(r, 0)].tobytes() for o, r in zip(doffs, rs)]


def encode(torch, amd, enc, objs, msgs, **kw):
    """(results, outputs) of one synchronised call."""
    res, dst, doffs, _ = launch(torch, amd, enc, objs, msgs, **kw)
    torch.cuda.synchronize()
    return collect(res, dst, doffs)


def mixed(torch, amd, enc, name, order=None, **kw):
    """The set in ONE call of the new entry point, message j against its owner's object."""
    s, objs = sets()[name], objects(torch, amd, enc, name)
    order = range(len(s.messages)) if order is None else order
    return encode(torch, amd, enc, [objs[s.owner[j]].data_ptr() for j in order],
                  [s.messages[j] for j in order], **kw)


_twins = {}


def twins(torch, amd, enc, name, depth=8):
    """What the single-dictionary call gives every message of the set: one call per group.
    Computed once per (encoder, set, depth) and shared."""
    key = (enc, name, depth)
    if key not in _twins:
        s, objs = sets()[name], objects(torch, amd, enc, name)
        rs, outs = [None] * len(s.messages), [None] * len(s.messages)
        for k in range(len(s.dicts)):
            idx = s.of(k)
            r, o = encode(torch, amd, enc, objs[k], [s.messages[j] for j in idx], depth=depth)
            for j, rj, oj in zip(idx, r, o):
                rs[j], outs[j] = rj, oj
        assert min(rs) > 0
        _twins[key] = (rs, outs)
    return _twins[key]


# ---- 1. the bytes are the twins' ----
@pytest.mark.parametrize("name", ["content", "size"])
@pytest.mark.parametrize("enc", ENCODERS)
def test_bytes_are_the_single_dictionary_calls(product, cuda, enc, name):
    want = twins(cuda, product, enc, name)
    rs, outs = mixed(cuda, product, enc, name)
    assert outs == want[1], first_difference(outs, want[1])
    assert rs == want[0]


@pytest.mark.parametrize("depth", [1, 0])
@pytest.mark.parametrize("enc", [HC, OPT])
def test_bytes_are_the_single_dictionary_calls_at_other_depths(product, cuda, enc, depth):
    want = twins(cuda, product, enc, "content", depth)
    rs, outs = mixed(cuda, product, enc, "content", depth=depth)
    assert outs == want[1], first_difference(outs, want[1])
    assert rs == want[0]


# ---- 2. the bytes are the models' ----
@functools.lru_cache(maxsize=None)
def model(enc, j):
    s = K.content_set()
    d, m = s.dicts[s.owner[j]], s.messages[j]
    if enc == FAST:
        return encmodel.encode_cdict(m, d, MS)
    return (hcdictmodel if enc == HC else hcoptdictmodel).compress(d, m, MS, 8)


@pytest.mark.parametrize("enc", ENCODERS)
def test_bytes_are_the_models(product, cuda, enc):
    small = K.content_set().small()
    rs, outs = mixed(cuda, product, enc, "content", order=small)
    want = [model(enc, j) for j in small]
    assert outs == want, first_difference(outs, want)
    assert rs == [len(w) for w in want]


# ---- 3. it decodes ----
@pytest.mark.parametrize("name", ["content", "size"])
@pytest.mark.parametrize("enc", ENCODERS)
def test_every_block_decodes_with_its_own_dictionary(oracle, product, cuda, enc, name):
    s = sets()[name]
    rs, outs = mixed(cuda, product, enc, name)
    dicts = [s.dicts[k] for k in s.owner]
    for j, (m, r, c, d) in enumerate(zip(s.messages, rs, outs, dicts)):
        assert r > 0, (j, r)
        assert orc_dict_decode(oracle, c, len(m), d) == (len(m), m), j
    got = gpu_dict_decode(cuda, product, outs, [len(m) for m in s.messages], dicts, adjacent=False)
    assert got == [(len(m), m) for m in s.messages]


# ---- 4. order and company do not matter ----
@pytest.mark.parametrize("enc", ENCODERS)
def test_order_and_company_do_not_matter(product, cuda, enc):
    s = K.content_set()
    want = twins(cuda, product, enc, "content")
    n = len(s.messages)
    order = [(37 * j + 11) % n for j in range(n)]              # a permutation: 37 and 64 coprime
    assert sorted(order) == list(range(n))
    for part in (order, list(range(n // 2 + 3)), list(range(n // 2 + 3, n))):
        rs, outs = mixed(cuda, product, enc, "content", order=part)
        assert outs == [want[1][j] for j in part], part[0]
        assert rs == [want[0][j] for j in part]
    # every message naming ONE object: the single call's bytes for all of them
    objs = objects(cuda, product, enc, "content")
    got = encode(cuda, product, enc, [objs[2].data_ptr()] * n, s.messages)
    assert got == encode(cuda, product, enc, objs[2], s.messages)
    assert [got[1][j] for j in s.of(2)] == [want[1][j] for j in s.of(2)]


# ---- 5. failures are isolated ----
@pytest.mark.parametrize("enc", ENCODERS)
def test_a_bad_object_costs_only_the_messages_that_name_it(product, cuda, enc):
    s = K.content_set()
    objs = objects(cuda, product, enc, "content")
    n = len(s.messages)
    good = mixed(cuda, product, enc, "content")
    zero = cuda.zeros(object_size(product, enc), dtype=cuda.uint8, device="cuda")
    # the other kind's object, in an allocation that would hold either
    other = cuda.zeros(max(product.cdict_size(), product.hc_cdict_size()), dtype=cuda.uint8,
                       device="cuda")
    (product.hc_cdict_prepare if enc == FAST else product.cdict_prepare)(
        dev_dict(cuda, s.dicts[0]), MS, other)
    bad = {5: 0, 14: objs[2].data_ptr() + 8, 23: zero.data_ptr(), 32: other.data_ptr(),
           63: 0, 0: zero.data_ptr()}
    if enc != FAST:     # an object of the right kind, prepared for another maxSrcSize
        bad[41] = single_prepare(cuda, product, enc, s.dicts[1], max_src=2048).data_ptr()
    optr = [bad.get(j, objs[s.owner[j]].data_ptr()) for j in range(n)]
    msgs = list(s.messages)
    long = 31                                    # a 4096-byte message grown to maxSrcSize + 1
    assert len(msgs[long]) == MS and long not in bad
    msgs[long] = msgs[long] + b"x"
    caps = [product.compressBound(MS + 1)] * n
    res, dst, doffs, keep = launch(cuda, product, enc, optr, msgs, caps=caps)
    cuda.cuda.synchronize()
    rs = res.cpu().tolist()
    for j in range(n):
        if j in bad or j == long:
            assert rs[j] == (ERANGE if j == long else 0), (j, rs[j])
            assert fetch(dst, doffs[j], caps[j] + 32) == bytes([CANARY]) * (caps[j] + 32), j
        else:
            assert (rs[j], fetch(dst, doffs[j], rs[j])) == (good[0][j], good[1][j]), j


# ---- 6. passes ----
@pytest.mark.parametrize("enc", [HC, OPT])
def test_scratch_size_and_contents_do_not_matter(product, cuda, enc):
    want = twins(cuda, product, enc, "content")
    for nb, fill in ((1, 0x11), (7, 0xFF), (64, 0x00)):
        got = mixed(cuda, product, enc, "content",
                    scratch=new_scratch(cuda, product, enc, nb, fill=fill))
        assert got == want, (nb, fill)


# ---- 7. batched prepare ----
def batch_prepare(torch, amd, enc, dicts, sizes=None, fill=0x5A, gap=0, odd=(1,), stream=None,
                  max_src=MS):
    """Objects of one prepare_batch call over `fill`; dictionary k of `odd` at an odd address, an
    empty one behind a null pointer.  Returns (the tensor, the stride, what it keeps alive)."""
    size = object_size(amd, enc)
    stride = size + gap
    devs = [dev_dict(torch, d, odd=k in odd) for k, d in enumerate(dicts)]
    dptr = ptrs(torch, [t.data_ptr() if len(d) else 0 for t, d in zip(devs, dicts)])
    dsz = ints(torch, [len(d) for d in dicts] if sizes is None else sizes)
    out = torch.full((len(dicts) * stride,), fill, dtype=torch.uint8, device="cuda")
    f = amd.cdict_prepare_batch if enc == FAST else amd.hc_cdict_prepare_batch
    f(dptr, dsz, max_src, out, stride, stream=stream)
    return out, stride, (devs, dptr, dsz)


@pytest.mark.parametrize("enc", [FAST, HC])
def test_batched_prepare_writes_the_single_prepares_objects(product, cuda, enc):
    """Over 0x00 and over 0xFF (every byte of an object is written), with an empty dictionary
    behind a null pointer, a dictionary at an odd address and one longer than the window; the
    bytes between objects keep their poison."""
    size = object_size(product, enc)
    dicts = list(K.size_set().dicts) + [K.content_set().dicts[1]]
    assert len(dicts[0]) == 0
    singles = [single_prepare(cuda, product, enc, d, fill=0xA5, odd=k != 1).cpu().numpy()
               for k, d in enumerate(dicts)]
    for fill in (0x00, 0xFF):
        out, stride, _ = batch_prepare(cuda, product, enc, dicts, fill=fill, gap=64)
        cuda.cuda.synchronize()
        host = out.cpu().numpy()
        for k, want in enumerate(singles):
            got = host[k * stride:k * stride + size]
            assert np.array_equal(got, want), (fill, k, int(np.nonzero(got != want)[0][0]))
            assert bool((host[k * stride + size:(k + 1) * stride] == fill).all()), (fill, k)


@pytest.mark.parametrize("enc", ENCODERS)
def test_a_bad_entry_of_a_batched_prepare_gets_a_zero_header(product, cuda, enc):
    s = K.content_set()
    size = object_size(product, enc)
    dicts = s.dicts[:3]
    out, stride, keep = batch_prepare(cuda, product, enc, dicts, fill=0xFF, gap=64,
                                      sizes=[len(dicts[0]), -1, len(dicts[2])])
    cuda.cuda.synchronize()
    host = out.cpu().numpy()
    assert not host[stride:stride + 16].any()
    assert bool((host[stride + 16:2 * stride] == 0xFF).all())
    for k in (0, 2):
        want = single_prepare(cuda, product, enc, dicts[k]).cpu().numpy()
        assert np.array_equal(host[k * stride:k * stride + size], want), k
        assert bool((host[k * stride + size:(k + 1) * stride] == 0xFF).all()), k
    # a null pointer with a positive size is the other bad entry
    devs = [dev_dict(cuda, d) for d in dicts]
    f = product.cdict_prepare_batch if enc == FAST else product.hc_cdict_prepare_batch
    out2 = cuda.full((3 * stride,), 0xFF, dtype=cuda.uint8, device="cuda")
    f(ptrs(cuda, [devs[0].data_ptr(), devs[1].data_ptr(), 0]), ints(cuda, [len(d) for d in dicts]),
      MS, out2, stride)
    cuda.cuda.synchronize()
    host2 = out2.cpu().numpy()
    assert not host2[2 * stride:2 * stride + 16].any()
    assert bool((host2[2 * stride + 16:] == 0xFF).all())
    assert np.array_equal(host2[:stride], host[:stride])
    # messages that name object 1 get 0, the others the single calls' bytes
    idx = [j for j in range(len(s.messages)) if s.owner[j] < 3]
    want = twins(cuda, product, enc, "content")
    rs, outs = encode(cuda, product, enc, [out.data_ptr() + s.owner[j] * stride for j in idx],
                      [s.messages[j] for j in idx])
    for j, r, o in zip(idx, rs, outs):
        assert (r, o) == ((0, b"") if s.owner[j] == 1 else (want[0][j], want[1][j])), j


# ---- 8. two streams ----
@pytest.mark.parametrize("enc", ENCODERS)
def test_two_streams_share_the_objects(product, cuda, enc):
    s = K.content_set()
    objs = objects(cuda, product, enc, "content")
    want = twins(cuda, product, enc, "content")
    n = len(s.messages)
    halves = (list(range(0, n, 2)), list(range(1, n, 2)))
    streams = (cuda.cuda.Stream(), cuda.cuda.Stream())
    runs = [launch(cuda, product, enc, [objs[s.owner[j]].data_ptr() for j in part],
                   [s.messages[j] for j in part], stream=st)
            for part, st in zip(halves, streams)]
    cuda.cuda.synchronize()
    for part, run in zip(halves, runs):
        assert collect(*run[:3]) == ([want[0][j] for j in part], [want[1][j] for j in part])


# ---- 9. a captured graph ----
def test_batched_prepare_and_a_two_pass_mixed_call_capture_into_a_graph(product, cuda):
    """One stream, no parallel branches: the batched prepare, then a mixed hc call whose scratch
    holds half the messages."""
    s = K.content_set()
    want = twins(cuda, product, HC, "content")
    n = len(s.messages)
    size = product.hc_cdict_size()
    devs = [dev_dict(cuda, d) for d in s.dicts]
    dptr = ptrs(cuda, [t.data_ptr() for t in devs])
    dsz = ints(cuda, [len(d) for d in s.dicts])
    objs = cuda.full((4 * size,), 0x11, dtype=cuda.uint8, device="cuda")
    optr = ptrs(cuda, [objs.data_ptr() + k * size for k in s.owner])
    src, sptr, _ = pack(cuda, s.messages, misalign=[(5 * i + 1) % 16 for i in range(n)])
    caps = [product.compressBound(len(m)) for m in s.messages]
    dst, dptr_out, doffs = alloc_out(cuda, caps, misalign=[(3 * i) % 16 for i in range(n)])
    sizes, capt, res = ints(cuda, map(len, s.messages)), ints(cuda, caps), ints(cuda, [POISON] * n)
    scratch = new_scratch(cuda, product, HC, n // 2)
    st = cuda.cuda.Stream()
    st.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=st):
        product.hc_cdict_prepare_batch(dptr, dsz, MS, objs, size, stream=st)
        product.compress_hc_cdicts_batch(sptr, sizes, dptr_out, capt, res, optr, MS, 8, scratch,
                                         stream=st)
    res.fill_(POISON)
    objs.fill_(0x22)
    scratch.fill_(0x33)
    g.replay()
    cuda.cuda.synchronize()
    assert collect(res, dst, doffs) == want


# ---- the rest of the interface ----
def test_empty_batches_launch_nothing(product, cuda):
    e = cuda.zeros(0, dtype=cuda.int64, device="cuda")
    z = cuda.zeros(0, dtype=cuda.int32, device="cuda")
    product.compress_cdicts_batch(e, z, e, z, z, e)
    for enc, f in ((HC, product.compress_hc_cdicts_batch),
                   (OPT, product.compress_hc_opt_cdicts_batch)):
        scratch = new_scratch(cuda, product, enc, 1)
        f(e, z, e, z, z, e, MS, 8, scratch)
        cuda.cuda.synchronize()
        assert bool((scratch == 0xEE).all())
    for f, size in ((product.cdict_prepare_batch, product.cdict_size()),
                    (product.hc_cdict_prepare_batch, product.hc_cdict_size())):
        objs = cuda.full((size,), 0x77, dtype=cuda.uint8, device="cuda")
        f(e, z, MS, objs, size)
        cuda.cuda.synchronize()
        assert bool((objs == 0x77).all())


def test_the_bindings_validate_cuda_tensors_too(product, cuda):
    p = cuda.zeros(2, dtype=cuda.int64, device="cuda")
    i = cuda.zeros(2, dtype=cuda.int32, device="cuda")
    for bad in (None, p[:1], p.to(cuda.int32), p.cpu()):
        with pytest.raises(ValueError):
            product.compress_cdicts_batch(p, i, p, i, i, bad)
    size = product.cdict_size()
    objs = cuda.zeros(2 * size, dtype=cuda.uint8, device="cuda")
    for args in ((p, i, MS, objs[:2 * size - 16], size), (p, i, MS, objs, size - 16),
                 (p[:1], i, MS, objs, size), (p, i, MS, objs.cpu(), size)):
        with pytest.raises(ValueError):
            product.cdict_prepare_batch(*args)
