"""bench.py's own contract: a plain run times exactly --steps steps and nothing else, and
--dump-outputs writes what the last timed step produced, from inputs that depend on the
arguments alone (App. C blocks, seed = block id), as float32 / float64 .npy files."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NB = 65536, 301     # 301 blocks: odd, more than the 64 sampled, several workgroups


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "APE_BENCH_DEVICE"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=300)


def test_bench_rejects_zero_steps():
    r = _bench(["--gpus", "1", "--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout == ""


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(cuda, oracle, tmp_path):
    d = str(tmp_path / "dump")
    r = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--blocks", str(NB),
                "--dump-outputs", d])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value = uncompressed bytes of the job / one timed step (both rounded in the line)
    assert line["value"] == pytest.approx(NB * N / (line["ms_per_step"] * 1e-3) / 2 ** 30, rel=2e-2)
    # nothing but the timed steps ran
    assert line["full"] is False and line["verified"] is None
    assert line["cpu_baseline"] is None and line["config2"] is None and line["config5"] is None

    names = ["block_ids", "comp_sizes", "decode_results", "out_block_sums", "sample_blocks",
             "comp_sample", "out_sample"]
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in names)
    a = {n: np.load(os.path.join(d, n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    assert a["block_ids"].tolist() == list(range(NB))
    assert (a["decode_results"] == N).all()
    assert ((a["comp_sizes"] > 0) & (a["comp_sizes"] < N)).all()      # compressible blocks
    assert line["ratio"] == pytest.approx(NB * N / a["comp_sizes"].sum(dtype=np.float64), abs=1e-4)
    sample = a["sample_blocks"].astype(np.int64)
    assert len(sample) == 64 and len(set(sample.tolist())) == 64
    assert (np.diff(sample) > 0).all() and 0 <= sample[0] and sample[-1] < NB

    # the inputs are the App. C blocks of these ids: rebuild them on the CPU
    buf = C.create_string_buffer(N * NB)
    oracle.synth_blocks(buf, N, C.c_longlong(N), C.c_longlong(0), NB, 1)
    src = np.frombuffer(buf.raw, dtype=np.uint8).reshape(NB, N)
    assert (a["out_block_sums"] == src.sum(axis=1, dtype=np.int64)).all()
    assert (a["out_sample"] == src[sample]).all()
    # and the dumped compressed bytes are the blocks the sizes speak of
    for j, b in enumerate(sample):
        c = int(a["comp_sizes"][b])
        blk = a["comp_sample"][j].astype(np.uint8).tobytes()
        assert not any(blk[c:])
        ob = C.create_string_buffer(N + 64)
        got = oracle.orc_decompress_safe(C.create_string_buffer(blk[:c] + b"\0" * 16, c + 16),
                                         ob, c, N)
        assert got == N and ob.raw[:N] == src[b].tobytes(), ("block", int(b))
