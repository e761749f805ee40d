"""Dictionary training on the GPU: APE_LZ4_dict_train_dev against
tests/dicttrainmodel.py, byte for byte and info word for word, on the shapes of
tests/test_dict_train_model.py (which shows that each of them tells the rule from a wrong
neighbour).  Samples lie at odd addresses, the dictionary lies at an odd address between
canaries (checked after each test), the scratch is filled with 0xEE and info with -7, and each
case synchronises once."""
import pytest

import dicttrainmodel as M
import test_gpu_cdict as fast
import test_gpu_hc_cdict as hc
from gpuutil import alloc_out, ints, pack
from test_dict_train_model import cases, model
from test_gpu_stream import orc_dict_decode

pytestmark = pytest.mark.gpu

POISON = -7


def launch(torch, amd, samples, capacity, segment, max_sample, sizes=None, fill=0xEE,
           stream=None):
    """One dict_train call, not synchronised: (dictionary view, info, what it reads)."""
    n = len(samples)
    sizes = [len(s) for s in samples] if sizes is None else sizes
    src, sptr, _ = pack(torch, samples, misalign=[(2 * i + 1) % 16 for i in range(n)])
    dst, _, offs = alloc_out(torch, [0, capacity], misalign=[0, 5])
    d = dst[offs[1]:offs[1] + capacity]
    assert d.data_ptr() % 2 == 1
    scratch = torch.full((amd.dict_train_scratch_size(n, max_sample, segment),), fill,
                         dtype=torch.uint8, device="cuda")
    info = ints(torch, [POISON] * 4)
    sz = ints(torch, sizes)
    amd.dict_train(sptr, sz, max_sample, d, segment, scratch, info, stream=stream)
    return d, info, (src, sptr, sz, scratch, dst)


def train(torch, amd, case, **more):
    d, info, keep = launch(torch, amd, **case, **more)
    torch.cuda.synchronize()
    return d.cpu().numpy().tobytes(), info.cpu().tolist()


def first_difference(got, want):
    for at, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "byte %d: %d, the model has %d" % (at, g, w)
    return "lengths %d, %d" % (len(got), len(want))


@pytest.mark.parametrize("name", list(cases()))
def test_bytes_and_info_are_the_models(product, cuda, name):
    want, want_info = model(name)
    got, info = train(cuda, product, cases()[name])
    assert info == want_info
    assert got == want, first_difference(got, want)


def test_no_samples_give_zeros(product, cuda):
    got, info = train(cuda, product, dict(samples=[], capacity=1000, segment=16, max_sample=1024))
    assert got == bytes(1000) and info == [0, 0, 0, 0]


def test_nothing_but_ignored_and_empty_samples(product, cuda):
    case = dict(samples=[b"x" * 40] * 5, sizes=[33, -1, 0, 7, 2 ** 31 - 1], capacity=64,
                segment=32, max_sample=32)
    assert train(cuda, product, case) == (bytes(64), [0, 0, 2, 0])
    assert M.train(**case) == (bytes(64), [0, 0, 2, 0])


def test_two_calls_any_scratch_any_stream_give_the_same_bytes(product, cuda):
    case = cases()["quality 64 x 256 B"]
    ref = train(cuda, product, case)
    assert ref == model("quality 64 x 256 B")
    assert train(cuda, product, case) == ref
    assert train(cuda, product, case, fill=0x00) == ref
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    assert train(cuda, product, case, stream=s) == ref


def test_train_and_prepare_capture_into_a_graph(product, cuda):
    case = cases()["quality 64 x 256 B"]
    n = len(case["samples"])
    src, sptr, _ = pack(cuda, case["samples"], misalign=[(2 * i + 1) % 16 for i in range(n)])
    sz = ints(cuda, map(len, case["samples"]))
    d = cuda.full((case["capacity"],), 0x11, dtype=cuda.uint8, device="cuda")
    scratch = cuda.full((product.dict_train_scratch_size(n, 256, 32),), 0x33, dtype=cuda.uint8,
                        device="cuda")
    info = ints(cuda, [POISON] * 4)
    obj = cuda.full((product.cdict_size(),), 0x22, dtype=cuda.uint8, device="cuda")
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        product.dict_train(sptr, sz, 256, d, 32, scratch, info, stream=s)
        product.cdict_prepare(d, 256, obj, stream=s)
    for _ in range(2):
        d.fill_(0x44)
        info.fill_(POISON)
        scratch.fill_(0x55)
        g.replay()
    cuda.cuda.synchronize()
    want, want_info = model("quality 64 x 256 B")
    assert (d.cpu().numpy().tobytes(), info.cpu().tolist()) == (want, want_info)
    assert cuda.equal(obj, fast.prepare(cuda, product, want, 256))


def test_end_to_end_the_trained_dictionary_pays(oracle, product, cuda):
    """256 x 512 B -> 8192 B: train, prepare and compress the 128 held-out messages on one stream.
    The model puts the fast encoder at 2846 bytes against 3763 with the samples' head on the
    first 12 messages, the high-ratio mode at depth 8 at 1456 against 1864 on the first 6."""
    n, L, cap, k = M.QUALITY[1]
    samples, held_out = M.corpus(n, L, 1), M.corpus(128, L, 2)
    d, info, keep = launch(cuda, product, samples, cap, k, L)
    obj = cuda.full((product.cdict_size(),), 0x5A, dtype=cuda.uint8, device="cuda")
    product.cdict_prepare(d, L, obj)
    hobj = cuda.full((product.hc_cdict_size(),), 0x5A, dtype=cuda.uint8, device="cuda")
    product.hc_cdict_prepare(d, L, hobj)
    rs, outs = fast.encode(cuda, product, obj, held_out)
    hrs, houts = hc.encode(cuda, product, hobj, held_out, L, 8)
    trained = d.cpu().numpy().tobytes()
    assert (trained, info.cpu().tolist()) == M.train(samples, cap, k, L)
    for what, r, o in (("fast", rs, outs), ("hc", hrs, houts)):
        for i, m in enumerate(held_out):
            assert r[i] > 0 and orc_dict_decode(oracle, o[i], L, trained) == (L, m), (what, i)
    head = M.naive(samples, cap)
    head_rs, _ = fast.encode(cuda, product, fast.prepare(cuda, product, head, L), held_out)
    head_hrs, _ = hc.encode(cuda, product, hc.prepare(cuda, product, head, L), held_out, L, 8)
    print("256 x 512 B -> 8192 B on 128 held-out messages: compress_usingCDict %d trained, %d "
          "head; compress_hc_usingCDict depth 8 %d trained, %d head"
          % (sum(rs), sum(head_rs), sum(hrs), sum(head_hrs)))
    assert sum(rs) < sum(head_rs)
    assert sum(hrs) < sum(head_hrs)
