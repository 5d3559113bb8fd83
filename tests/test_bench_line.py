"""bench.py end to end on the GPU: the JSON line the driver parses must come out, with the roofline and host-baseline
objects filled under --full (a changed C-ABI signature that the bench's launch probe does not follow shows up here, not at
round end); a plain run times its steps and nothing else, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_roofline(hip):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--full"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["steps"] == 3 and line["n_gpus"] == 1 and line["value"] > 0
    r = line["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] < 1 and r["achieved"] > 0 and r["peak"] > 0
    c = line["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("port", "reference")
    assert "workload" in line["config"]


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_last_step(hip, tmp_path):
    """The plain invocation: the headline fields, exactly --steps timed steps, none of the --full extras, and
    --dump-outputs: float32 / float64 arrays of the last timed step within 64 MB, the network's outputs among them."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = _last_json(out.stdout)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]      # bs 4 frame pairs per step
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert "other_configs" not in line["config"] and "multirank_path" not in line["config"]
    assert line["config"]["train_stream_split"] is None
    files = {f.name: f for f in tmp_path.iterdir()}
    for name in ("out.loss.npy", "out.translation_preds.npy", "out.rotation_preds.npy", "param_grads.npy",
                 "params_after_step.npy"):
        assert name in files, sorted(files)
    assert sum(f.stat().st_size for f in files.values()) <= 64 << 20
    for f in files.values():
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64) and a.size > 0, f.name
    assert np.isfinite(np.load(files["out.loss.npy"])).all()
    assert float(np.abs(np.load(files["param_grads.npy"])).max()) > 0


def test_dump_outputs_samples_large_arrays_within_the_budget(tmp_path):
    """bench.dump_outputs on the host (a child process: importing bench.py sets HIP environment variables): every array
    as float32 / float64, a large one as the same seeded sample on every call, the whole dump within DUMP_BYTES."""
    code = """if True:
        import sys, numpy as np, torch
        sys.path.insert(0, sys.argv[1])
        import bench
        bench.DUMP_BYTES = 1 << 20
        t = torch.arange(1 << 20, dtype=torch.float32)
        arrays = bench._named_tensors({"a": t, "b": [torch.ones(3, 2, dtype=torch.float64), None],
                                       "c": torch.tensor([1, 0], dtype=torch.bool), "d": 1.5}, "out")
        for d in sys.argv[2:]:
            bench.dump_outputs(d, arrays)
    """
    dirs = [str(tmp_path / "x"), str(tmp_path / "y")]
    out = subprocess.run([sys.executable, "-c", code, ROOT] + dirs, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    x, y = tmp_path / "x", tmp_path / "y"
    assert sorted(f.name for f in x.iterdir()) == ["out.a.npy", "out.b.0.npy", "out.c.npy"]
    a = np.load(x / "out.a.npy")
    assert a.dtype == np.float32 and a.size == (1 << 20) // 8 // 3 and (np.diff(a) > 0).all()
    assert np.array_equal(a, np.load(y / "out.a.npy"))
    b = np.load(x / "out.b.0.npy")
    assert b.dtype == np.float64 and b.shape == (3, 2)
    assert np.load(x / "out.c.npy").tolist() == [1.0, 0.0]
    assert sum(f.stat().st_size - 128 for f in x.iterdir()) <= 1 << 20


def _last_json(stdout):
    return json.loads([ln for ln in stdout.strip().splitlines() if ln.startswith("{")][-1])


def test_bench_gpus_flag_starts_that_many_ranks_by_itself():
    """`python bench.py --gpus 2` with NO launcher around it (the form the driver uses) must start two ranks itself
    (the reference: train_hdf5.py:255 mp.spawn) and report n_gpus 2.  --dry-run: launcher + gloo rendezvous + the
    barrier / max-over-ranks timing protocol on the CPU, no kernels."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--dry-run"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                       # rank 0 alone prints
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["dry_run"] is True
    assert line["ranks"]["world"] == 2 and line["ranks"]["ms_per_step_min"] <= line["ranks"]["ms_per_step_max"]


def test_bench_refuses_a_world_size_that_is_not_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0 and "WORLD_SIZE=2" in (out.stderr + out.stdout)


@pytest.mark.gpu
def test_bench_gpus_2_runs_the_full_two_rank_step(hip):
    """The complete two-rank step (SyncBN statistics exchange, overlapped gradient all-reduce, per-rank prefetch) started
    by `bench.py --gpus 2` itself.  The test boxes have ONE GPU: RSLO_BENCH_ONE_GPU=1 puts both ranks on it over gloo --
    functional, not a performance mode."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["RSLO_BENCH_ONE_GPU"] = "1"
    env["RSLO_PEER_TIMEOUT_MS"] = "20000"          # a peer that does not show up fails the test in seconds, not minutes
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2",
                          "--batch", "1", "--no-cpu-baseline"], capture_output=True, text=True, timeout=400, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = _last_json(out.stdout)
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["rccl"]["ranks"] == 2 and line["rccl"]["ms_per_step_min"] <= line["rccl"]["ms_per_step_max"]
    # SyncBN statistics travelled through the same-stream peer kernel, and after the steps both ranks hold the same bits
    assert "peer kernel" in line["rccl"]["syncbn_exchange"], line["rccl"]
    assert line["rccl"]["replicas_identical"] is True, line["rccl"]
    # diagnostics of an N > 1 run: the exposed part of the gradient exchange, per-rank transport and per-exchange waits
    r = line["rccl"]
    assert r["grad_exchange_exposed_ms_per_step"] is not None and r["grad_exchange_exposed_ms_per_step"] >= 0
    assert len(r["syncbn_transport_per_rank"]) == 2 and len(set(r["syncbn_transport_per_rank"])) == 1
    assert all(w["samples"] > 0 and w["p50_us"] <= w["p99_us"] <= w["max_us"] for w in r["syncbn_wait_us"]), r["syncbn_wait_us"]
    assert "topology_lines" in r          # RCCL's own INIT / GRAPH lines at N > 1 over RCCL (None in the gloo one-GPU mode)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["c2", "c5"])
def test_bench_encoder_configs_print_the_same_schema(hip, cfg):
    """BASELINE configs[1] / configs[4] through the entry point the driver calls: same JSON schema as the C3 line, roofline from
    the launch probe, CPU baseline over the oracle backend."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", cfg, "--steps", "5", "--warmup", "3",
                          "--full"],
                         capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = _last_json(out.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["unit"] == "frame-pairs/s"
    assert line["config"]["workload"].startswith(cfg.upper()) and line["config"]["voxelize_and_plan_on_side_stream"] is True
    r = line["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] < 1 and "k_spconv" in r["kernel"]
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["kind"] == "port"
