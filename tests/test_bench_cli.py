"""bench.py's launcher logic where no GPU is needed: it must fail loudly, never fall back (`--gpus` was inert)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=300)


def gpus_here():
    import torch
    return torch.cuda.device_count()


def test_more_gpus_than_visible_is_refused():
    n = gpus_here() + 1
    r = run_bench(["--gpus", str(n), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "%d GPUs requested, %d visible" % (n, n - 1) in r.stderr
    assert r.stdout.strip() == ""                   # no JSON line that could be mistaken for a measurement


def test_launcher_rank_count_must_match_the_flag():
    r = run_bench(["--gpus", "1", "--steps", "1", "--warmup", "0"],
                  {"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29999"})
    assert r.returncode != 0 and "--gpus 1 but the launcher started 2 rank(s)" in r.stderr


@pytest.mark.skipif(gpus_here() > 0, reason="needs a box without a GPU")
def test_no_gpu_no_number():
    r = run_bench(["--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and r.stdout.strip() == ""
    assert "visible" in r.stderr or "no HIP device" in r.stderr


@pytest.mark.gpu
def test_two_rank_rehearsal_on_one_gpu():
    """VERDICT r4, task 4 (ii): `bench.py --gpus 2 --control gloo --share-device` - two fresh rank processes on GPU 0, control collectives and
    the gather leg through gloo - exercises what the first real N > 1 run will: the rank spawn, the CPU slices, the barrier / max-over-ranks
    timing, `per_rank`, `imbalance`, `gather_c2` and the ONE JSON line from rank 0, with every stream of both ranks verified"""
    import json
    r = run_bench(["--gpus", "2", "--control", "gloo", "--share-device", "--streams", "48", "--blocks", "12", "--steps", "3", "--warmup", "1",
                   "--full", "--no-extra", "--no-cpu"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["verified_vs_oracle"] is True and j["verified_streams"] == 96
    assert [p["rank"] for p in j["per_rank"]] == [0, 1] and all(p["streams"] == 48 and p["launch_ms"] > 0 for p in j["per_rank"])
    assert j["imbalance"]["samples_max_over_mean"] == 1.0
    assert j["gather_c2"]["bytes_into_rank0"] > 0 and j["gather_c2"]["seconds"] > 0
    assert "rehearsal" in j and "multi_gpu" not in j
    assert j["value"] > 0 and j["scaling"] == "weak"


@pytest.mark.gpu
def test_two_rank_rehearsal_of_the_sharded_corpus():
    """VERDICT r5, task 7: the STRONG-scaling leg - `--workload corpus` sharded over two ranks (longest first by header weight), still on
    one GPU through gloo: the shards differ (imbalance just above 1), every stream of both shards is verified against the oracle,
    the gather leg moves two ragged PCM arenas of different sizes, and the line says which share of the samples the byte-plane
    kernels decode"""
    import json
    r = run_bench(["--gpus", "2", "--control", "gloo", "--share-device", "--workload", "corpus", "--files", "120", "--steps", "3", "--warmup", "1",
                   "--full", "--no-extra", "--no-cpu"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["verified_vs_oracle"] is True and j["verified_streams"] == 120
    assert [p["rank"] for p in j["per_rank"]] == [0, 1] and sum(p["streams"] for p in j["per_rank"]) == 120
    assert 1.0 <= j["imbalance"]["samples_max_over_mean"] <= 1.05                  # ragged shards that longest-first cutting keeps close
    assert all(p["streams"] > 0 and p["launch_ms"] > 0 for p in j["per_rank"])
    assert j["gather_c2"]["bytes_into_rank0"] > 0 and j["gather_c2"]["seconds"] > 0
    ks = j["config"]["kernel_share"]
    assert set(ks["by_level"]) == {"7", "8", "9"} and ks["samples_from_byteplane_form"] > 0.9
    assert "rehearsal" in j


@pytest.mark.gpu
def test_dump_outputs_are_the_decoded_pcm(tmp_path):
    """--dump-outputs DIR: after the timed launches the PCM of the last one lands in DIR as float32 .npy files (64 MB at most); a plain
    run says it did not check against the oracle, the first stream's samples equal the oracle's and --steps is the timed count"""
    import json
    import numpy as np
    import oracle_api as O
    from libacm_amd import synth
    r = run_bench(["--gpus", "1", "--streams", "8", "--blocks", "12", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 7 and j["ms_per_step"] > 0 and j["value"] > 0 and "cpu_baseline" not in j and "sustained" not in j
    assert str(j["verified_vs_oracle"]).startswith("skipped")
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == ["pcm_first_stream.npy", "pcm_last_stream.npy", "pcm_sample.npy"]
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= 64 << 20
    arrs = {n: np.load(str(tmp_path / n)) for n in names}
    assert all(a.dtype == np.float32 for a in arrs.values())
    n = 12 * 16 << 9                                          # one stream: 12 blocks of 16 rows at level 9
    f = synth.generate(seed=synth.BASE_SEED, level=9, rows=16, nblocks=12, channels=1, total_values=n)
    want = O.Oracle.decode_all(f)[0].view(np.int16).astype(np.float32)
    assert np.array_equal(arrs["pcm_first_stream.npy"], want)
    assert np.array_equal(arrs["pcm_sample.npy"][:n], want)  # a batch this small is dumped whole, stream by stream
