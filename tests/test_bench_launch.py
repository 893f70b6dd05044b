"""`python bench.py --gpus N` launches its N ranks itself (the flag used to be parsed and ignored, ranks came
only from RANK / WORLD_SIZE, i.e. from a launcher the driver might not use)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=timeout)
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert len(lines) == 1, "exactly one JSON line (rank 0's)"
    return json.loads(lines[0])


def test_gpus_2_without_a_device_runs_the_launch_path():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a HIP device is present: covered by the gpu test below")
    res = run_bench("--gpus", "2", "--steps", "3", "--warmup", "1")
    assert res["n_gpus"] == 2 and res["config"]["ranks_seen"] == 2
    assert res["valid"] is False and res["value"] == 0.0 and "NO HIP DEVICE" in res["config"]["workload"]


@pytest.mark.gpu
def test_gpus_2_on_a_one_gpu_box_is_labelled_oversubscribed():
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one GPU: a real two-rank run, not the oversubscribed path")
    res = run_bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--seconds", "20", "--cpu-seconds", "0", "--no-secondary")
    assert res["n_gpus"] == 2 and res["value"] > 0
    assert "OVERSUBSCRIBED" in res["config"]["parallelism"]


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["config4", "config5"])
def test_gpus_2_on_a_one_gpu_box_runs_the_sharded_workloads_too(workload):
    """the N > 1 branches of bench_multi.py (shares, agreement over the ranks, the gather or the channel slabs) on one GPU,
    two ranks sharing it over gloo: not a measurement -- the first run of these branches must not be the driver's 8-GPU run"""
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one GPU: a real two-rank run")
    res = run_bench("--gpus", "2", "--workload", workload, "--steps", "2", "--warmup", "1", "--seconds", "20")
    assert res["n_gpus"] == 2 and res["value"] > 0
    if workload == "config4":
        assert res["scaling"] == "strong" and res["config"]["scenes_per_rank"] == 32 and res["parity_gate"]["relerr"] < 1e-8
    else:
        assert res["scaling"] == "weak" and res["config"]["channels"] == 256 and res["config"]["finite"]


def test_dump_outputs_writes_a_fixed_bounded_sample(tmp_path):
    """`--dump-outputs`: a result above the whole-write size becomes its head, its tail and one seeded frame per stretch
    between them -- the same frames on every call, at most 64 MB, in the result's own dtype (CPU tensors: the sampling
    itself, no device)"""
    import numpy as np
    import torch

    import bench

    for n, nch, dt in ((1000, 8, torch.float64), (2_000_000, 8, torch.float64), (40_000_000, 1, torch.float32)):
        out = torch.arange(n * nch, dtype=dt).reshape(nch, n).t()  # [frames x channels], time fastest (bench.py's layout)
        a, b = tmp_path / ("a%d" % n), tmp_path / ("b%d" % n)
        names = bench.dump_outputs(str(a), out)
        assert names == bench.dump_outputs(str(b), out)
        assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 << 20
        got = {k: np.load(a / (k + ".npy")) for k in names}
        for k in names:
            assert got[k].dtype in (np.float32, np.float64) and np.array_equal(got[k], np.load(b / (k + ".npy")))
        want = out.numpy()
        if names == ["output"]:
            assert got["output"].dtype == want.dtype and np.array_equal(got["output"], want)
            continue
        fr = got["output_sample_frames"].astype(np.int64)
        assert np.array_equal(got["output_sample"], want[fr]) and (np.diff(fr) > 0).all()
        assert np.array_equal(got["output_head"], want[:len(got["output_head"])])
        assert np.array_equal(got["output_tail"], want[n - len(got["output_tail"]):])
        assert len(got["output_head"]) <= fr[0] and fr[-1] < n - len(got["output_tail"])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_result(tmp_path):
    """a plain run: exactly --steps timed steps, nothing of --full in its line, and the last timed step's result under
    --dump-outputs -- the same on a second run, and the headline's own values (its head against the CPU oracle)"""
    import numpy as np
    import torch

    from oracle_bridge import oracle_sink, relerr

    import bench
    import sigops_amd as so

    args = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--seconds", "20")
    r = run_bench(*args, "--dump-outputs", str(tmp_path / "a"))
    r2 = run_bench(*args, "--dump-outputs", str(tmp_path / "b"))
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0 and r["dtype"] == "f64"
    assert r["full"] is False and all(r[k] is None for k in ("parity_gate", "parity_full", "cpu_baseline", "config3", "config4"))
    assert "one_shot" not in r
    names = r["dumped_outputs"]
    assert sorted(os.listdir(tmp_path / "a")) == [k + ".npy" for k in names] and names == r2["dumped_outputs"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    for k in names:
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))), k
    head = np.load(tmp_path / "a" / "output_head.npy")
    assert head.dtype == np.float64 and head.shape[1] == 8
    # (bench.py's input: seeded device noise; a prefix of it gives the same first output frames)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1983)
    noise = torch.randn((8, 20 * 44100), dtype=torch.float64, device="cuda:0", generator=gen)
    pre = np.asfortranarray(noise[:, :150_000].t().cpu().numpy())
    want = oracle_sink(bench.tree_ns(so, pre, pre.shape[0]))[:head.shape[0]]
    assert relerr(head, want) < 1e-6


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements_and_checks():
    r = run_bench("--gpus", "1", "--full", "--steps", "3", "--warmup", "1", "--seconds", "20", "--cpu-seconds", "20")
    assert r["full"] is True and r["steps"] == 3 and r["ms_per_step"] > 0
    assert r["parity_gate"]["relerr"] <= 1e-6 and r["parity_full"]["relerr"] <= 1e-6
    assert r["config3"]["ms_per_step"] > 0 and r["cpu_baseline"]["value"] > 0 and "one_shot" in r
