"""APE_LZ4_xxh32_batch_dev on the GPU against tests/lz4fmodel.py xxh32: every size around the
kernel's edges (the 16-byte stripe, the 1 KiB round, more than one round, more than one wave),
three seeds, every alignment, batches that mix the longest and the shortest streams."""
import numpy as np
import pytest

import lz4fmodel as M
from gpuutil import ints, pack

pytestmark = pytest.mark.gpu

SIZES = list(range(49)) + [63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65536, (1 << 20) + 3]
SEEDS = (0, 1, 0x9E3779B1)
POISON = 0x5A5A5A5A


def _data(n, salt):
    return np.random.RandomState(1000 + salt).randint(0, 256, n, dtype=np.uint8).tobytes()


def _hash(cuda, product, blobs, seed, misalign=None, sizes=None):
    """The batch's hashes, and the two guard words around them."""
    n = len(blobs)
    keep, ptrs, _ = pack(cuda, blobs, misalign=misalign)
    out = cuda.full((n + 2,), POISON, dtype=cuda.int32, device="cuda")
    product.xxh32_batch(ptrs, ints(cuda, sizes if sizes is not None else map(len, blobs)),
                        out[1:n + 1], seed=seed)
    cuda.cuda.synchronize()
    host = [x & M.M32 for x in out.cpu().tolist()]
    assert host[0] == POISON and host[-1] == POISON, "the words beside d_hash were written"
    return host[1:-1]


@pytest.fixture(scope="module")
def blobs():
    return [_data(n, k) for k, n in enumerate(SIZES)]


@pytest.mark.parametrize("seed", SEEDS)
def test_every_edge_size_and_seed(product, cuda, blobs, seed):
    got = _hash(cuda, product, blobs, seed, misalign=[(7 * k + 1) % 16 for k in range(len(blobs))])
    assert got == [M.xxh32(b, seed) for b in blobs]


def test_known_values_and_a_batch_of_one(product, cuda):
    assert _hash(cuda, product, [b""], 0) == [0x02CC5D05]
    assert _hash(cuda, product, [b"a"], 0) == [0x550D7456]
    one = _data(4097, 77)
    assert _hash(cuda, product, [one], 1) == [M.xxh32(one, 1)]


def test_every_residue_of_16(product, cuda):
    blobs = [_data(200 + r, r) for r in range(16)] + [_data(15, 40 + r) for r in range(16)]
    got = _hash(cuda, product, blobs, 0x9E3779B1, misalign=list(range(16)) * 2)
    assert got == [M.xxh32(b, 0x9E3779B1) for b in blobs]


def test_seventy_streams_mix_the_longest_and_the_shortest(product, cuda, blobs):
    """Five waves; the long streams sit at different places of their waves, next to empty ones."""
    long_ = blobs[-1]
    batch = [long_ if k in (0, 17, 35, 69) else _data(k % 40, k) for k in range(70)]
    got = _hash(cuda, product, batch, 1, misalign=[(3 * k) % 16 for k in range(70)])
    want = {}
    assert got == [want.setdefault(b, M.xxh32(b, 1)) for b in batch]


def test_a_negative_size_hashes_as_empty(product, cuda):
    blobs = [_data(100, 1), _data(100, 2), _data(100, 3)]
    got = _hash(cuda, product, blobs, 0, sizes=[-1, 100, -2 ** 31])
    assert got == [M.xxh32(b""), M.xxh32(blobs[1]), M.xxh32(b"")]


def test_an_empty_batch_launches_nothing(product, cuda):
    empty64 = cuda.zeros(0, dtype=cuda.int64, device="cuda")
    empty32 = cuda.zeros(0, dtype=cuda.int32, device="cuda")
    product.xxh32_batch(empty64, empty32, empty32)
    assert product.lib().APE_LZ4_xxh32_batch_dev(None, None, 0, None, 0, None) == 0
