"""bench.py's one-line JSON contract (driver-facing): keys, types, and the two extra objects."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_to_run_without_a_device_or_with_wrong_world():
    env = dict(os.environ, WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr     # must be launched through torch.distributed.run


def test_bench_spawns_its_own_ranks_when_started_without_a_launcher():
    """`python bench.py --gpus 2` (no torchrun): the parent starts one child per GPU with RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_* set and returns the worst exit code.  Without a HIP device (this container) every rank
    stops at the device check -- two ranks, two messages, exit code 3; nothing hangs."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("launcher test for machines without a HIP device (on a GPU box ranks would need 2 GPUs)")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 3
    assert r.stderr.count("no HIP device visible") == 2 and r.stdout.strip() == ""


def test_spawned_ranks_get_a_consistent_environment(monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = []

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None):
            seen.append((cmd, env, stdout))

        def wait(self):
            return 0
    monkeypatch.setattr(bench.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--scaling", "strong", "--config", "3"])
    assert bench.spawn_ranks(4) == 0
    assert [e["RANK"] for _, e, _ in seen] == ["0", "1", "2", "3"] and [e["LOCAL_RANK"] for _, e, _ in seen] == ["0", "1", "2", "3"]
    assert {e["WORLD_SIZE"] for _, e, _ in seen} == {"4"} and {e["MASTER_ADDR"] for _, e, _ in seen} == {"127.0.0.1"}
    assert len({e["MASTER_PORT"] for _, e, _ in seen}) == 1 and {e["HSA_ENABLE_IPC_MODE_LEGACY"] for _, e, _ in seen} == {"0"}
    assert all(c[-4:] == ["--scaling", "strong", "--config", "3"] for c, _, _ in seen)
    assert seen[0][2] is None and all(s is not None for _, _, s in seen[1:])     # only rank 0 owns stdout


@pytest.mark.gpu
def test_bench_line_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "8", "--warmup", "3", "--no-extras",
                        "--cpu-seconds", "0.5"], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, "exactly one JSON line on stdout"
    b = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                 ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(b[k], t), k
    assert b["vs_baseline"] is None and b["n_gpus"] == 1 and b["steps"] == 8 and b["warmup"] == 3
    assert b["scaling"] == "weak" and b["higher_is_better"] is True and b["data"] == "synthetic"
    assert "workload" in b["config"] and "model" not in b["config"]
    assert 0.0 <= b["spinup_s"] <= 2.0   # the untimed spin-up before the W warm-up steps is disclosed in the line
    # ... and the figure without it (the same W + K steps, taken first on the device as the process found it) rides along
    assert b["ms_per_step_cold"] > 0 and abs(b["value_cold"] - b["config"]["features_active"] / (b["ms_per_step_cold"] * 1e-3)) <= 1e-6 * b["value_cold"]
    assert b["ms_per_step_cold"] > 0.8 * b["ms_per_step"]
    rf = b["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["achieved"] > 0
    assert rf["traffic"] is None or rf["traffic"] > 0
    cb = b["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert abs(b["value"] - b["config"]["features_active"] / (b["ms_per_step"] * 1e-3)) <= 1e-6 * b["value"]
    assert b["px_err_vs_cpu"] == {"max": 0.0, "p99": 0.0, "status_mismatches": 0}
    assert b["config"]["step_mode"] == "graph"          # the headline is the step a live camera loop can use


@pytest.mark.gpu
def test_bench_forced_collective_reports_the_gather():
    """One rank, the collective forced (PAGK_FORCE_DIST=1): the all-gather goes through the library's communicator,
    is reported on its own, and the line keeps its contract."""
    env = dict(os.environ, PAGK_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "8", "--warmup", "3", "--no-extras",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=280, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"exactly one JSON line on stdout, got {lines[:3]}"
    b = json.loads(lines[0])
    g = b["gather"]
    assert g["gather_ms"] > 0 and g["ranks"] == 1 and "pagk_multi_allgather" in g["via"]
    assert g["ms_per_step_without_gather"] > 0 and b["value"] > 0
    # the line proves itself: RCCL's own rank count beside torch's, and the gathered result against one unsharded launch
    assert g["rccl_ranks"] == 1 and g["torch_world"] == 1
    e = b["px_err_vs_single"]
    assert e["max"] == 0.0 and e["status_mismatches"] == 0 and e["pix_err_mismatches"] == 0 and e["compared"] == 1000


def test_spawned_ranks_of_the_replicas_mode(monkeypatch):
    """`bench.py --mode replicas --config 4 --gpus 8` (BASELINE configs[4]: one camera stream per GPU, no collective):
    eight children with the same environment contract, the mode passed through; `--cameras` is gone."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = []

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None):
            seen.append((cmd, env, stdout))

        def wait(self):
            return 0
    monkeypatch.setattr(bench.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--mode", "replicas", "--config", "4"])
    assert bench.spawn_ranks(8) == 0
    assert [e["LOCAL_RANK"] for _, e, _ in seen] == [str(k) for k in range(8)] and {e["WORLD_SIZE"] for _, e, _ in seen} == {"8"}
    assert all(c[-4:] == ["--mode", "replicas", "--config", "4"] for c, _, _ in seen)
    monkeypatch.undo()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cameras", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "unrecognized arguments" in r.stderr
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "metric_label(w)" in src and '"(21x21, 3-lvl, 30 iter)"' not in src


@pytest.mark.gpu
def test_bench_replicas_mode_on_one_gpu():
    """The replicas form with one rank: configs[4]'s stream shape, graph step, no collective, the mode named in the line."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29534")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--mode", "replicas", "--steps", "6", "--warmup", "2",
                        "--no-extras", "--no-cpu-baseline"], capture_output=True, text=True, timeout=280, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    b = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][0])
    assert b["config"]["mode"] == "replicas" and b["config"]["features_total"] == 4000 and "gather" not in b
    assert b["scaling"] == "weak" and len(b["per_gpu_ms_per_step"]) == 1 and b["config"]["step_mode"] == "graph"
    assert "1280x720" in b["config"]["workload"] and b["metric"].startswith("tracked features/sec (21x21, 3-lvl, 30 iter)")
    c = b["per_stream_check"]["streams"]
    assert len(c) == 1 and c[0]["compared"] == 256 and c[0]["status_mismatches"] == 0 and c[0]["max_px"] == 0.0


def test_the_multi_gpu_line_carries_its_own_proof():
    """VERDICT r3 item 6 (no multi-GPU node in this container): the keys an N > 1 line must carry are assembled in
    bench.py where the run is sharded -- the gathered result against one unsharded launch (px_err_vs_single), RCCL's own
    rank count (gather.rccl_ranks from ncclCommCount) beside torch's world size, and the replicas mode's per-stream check;
    the GPU box exercises them with one rank and the collective forced (tests above)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ('"px_err_vs_single"', '"rccl_ranks"', '"torch_world"', '"per_stream_check"', '"status_mismatches"',
                '"ms_per_step_cold"', '"value_cold"'):
        assert key in src, key
    sys.path.insert(0, ROOT)
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi
    lib = capi.load()
    assert hasattr(lib, "pagk_multi_comm_count")


def _load_bench(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_offers_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_writes_every_field_as_float(tmp_path):
    import numpy as np
    bench = _load_bench("bench_dump")
    n = 37
    rng = np.random.default_rng(3)
    res = {"pt_un": rng.random((n + 5, 2), dtype=np.float32), "pt_dist": rng.random((n + 5, 2), dtype=np.float32),
           "status": (rng.random(n + 5) > 0.3).astype(np.uint8), "pix_err": rng.random(n + 5),
           "dist_pred": rng.random(n + 5), "ncc": rng.random(n + 5, dtype=np.float32),
           "iters": rng.integers(0, 90, n + 5).astype(np.int32)}
    written = bench.dump_outputs(res, n, str(tmp_path / "out"))
    assert sorted(os.path.basename(p) for p in written) == sorted(f"{k}.npy" for k in res)
    for k, v in res.items():
        a = np.load(tmp_path / "out" / f"{k}.npy")
        assert a.dtype == (np.float64 if v.dtype == np.float64 else np.float32), k
        assert a.shape == v[:n].shape and np.array_equal(a, v[:n].astype(a.dtype)), k


def test_dump_outputs_samples_a_fixed_subset_above_the_limit(tmp_path, monkeypatch):
    import numpy as np
    bench = _load_bench("bench_dump_sample")
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    n = 1000
    res = {"pt_un": np.arange(2 * n, dtype=np.float32).reshape(n, 2), "pt_dist": np.zeros((n, 2), np.float32),
           "status": np.ones(n, np.uint8), "pix_err": np.arange(n, dtype=np.float64), "dist_pred": np.zeros(n),
           "ncc": np.zeros(n, np.float32), "iters": np.full(n, 7, np.int32)}
    bench.dump_outputs(res, n, str(tmp_path / "a"))
    bench.dump_outputs(res, n, str(tmp_path / "b"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4096 + 128 * len(os.listdir(tmp_path / "a"))   # (+ the .npy headers)
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert 0 < idx.size < n and np.array_equal(idx, np.load(tmp_path / "b" / "sample_index.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "pix_err.npy"), idx)
    assert np.array_equal(np.load(tmp_path / "a" / "pt_un.npy")[:, 0], 2 * idx.astype(np.float32))


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_and_dumps_the_timed_result(tmp_path):
    """A plain run: one line with the headline keys and nothing measured beside it; --dump-outputs holds the last timed
    step's result, which is the CPU oracle's, field for field."""
    import numpy as np
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "3",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, "exactly one JSON line on stdout"
    b = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("ms_per_step", float), ("higher_is_better", bool),
                 ("dtype", str), ("steps", int), ("warmup", int)):
        assert isinstance(b[k], t), k
    assert b["steps"] == 8 and b["warmup"] == 3 and b["unit"] == "features/s" and b["higher_is_better"] is True
    assert abs(b["value"] - b["config"]["features_active"] / (b["ms_per_step"] * 1e-3)) <= 1e-6 * b["value"]
    for k in ("ms_per_step_cold", "roofline", "cpu_baseline", "px_err_vs_cpu", "configs", "step_modes_ms", "live_step"):
        assert k not in b, k
    sys.path.insert(0, ROOT)
    from oracle import pagk_oracle as orc
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth
    w = synth.config(1, n=1000)
    p = capi.make_params(half_patch=w.half_patch, iterations=w.iterations, pyramids=w.pyramids, has_gyro=w.has_gyro,
                         camera=w.camera)
    ref = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)
    for k in ("pt_un", "pt_dist", "status", "pix_err", "dist_pred", "iters"):
        a = np.load(out_dir / f"{k}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == w.n, k
        assert np.array_equal(a, ref[k][:w.n].astype(a.dtype), equal_nan=True), k
