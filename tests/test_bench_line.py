"""The contract line of bench.py: the driver keeps only the tail of stdout, so the LAST line must be small and carry the keys it parses
(a 23 KB line gave `parsed: null`).  Built here from a recorded full result (profiles/r05_bench_default_f16x3.json) -- no GPU;
the one GPU test runs a plain (lean) bench.py end to end."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

RECORDED = os.path.join(ROOT, "profiles", "r05_bench_default_f16x3.json")


def _recorded():
    d = json.load(open(RECORDED))
    ref = dict(d["cpu_baseline_reference"])
    d["cpu_baseline"] = bench.merge_cpu_baseline(d["cpu_baseline"], ref)
    return d, ref


def test_contract_line_is_small_and_complete():
    d, _ = _recorded()
    line = bench.contract_line(d)
    assert len(line) < 6000 and len(line) <= bench.LINE_BUDGET and "\n" not in line
    p = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in p, k
    assert p["value"] == d["value"] and p["ms_per_step"] == d["ms_per_step"]
    assert "workload" in p["config"] and "model" not in p["config"]
    r = p["roofline"]
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r
    assert 0 < r["frac_on_evaluated_pairs"] < r["frac"]
    c = p["cpu_baseline"]
    assert c["value"] > 0 and c["unit"] == "rays/s" and c["cores"] >= 1 and c["kind"] in ("reference", "port") and c["sample"]
    assert set(p["parity"]) >= {"c1", "c2"} and p["parity"]["c1"]["sign_flips"] == 0


def test_last_stdout_line_is_the_contract_line(tmp_path, monkeypatch):
    d, _ = _recorded()
    monkeypatch.setenv("O2345_BENCH_EXTRA_FILE", str(tmp_path / "bench_extra.json"))
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(d)
    lines = buf.getvalue().strip().split("\n")
    assert len(lines) == 2 and len(lines[-1]) <= bench.LINE_BUDGET
    last = json.loads(lines[-1])
    assert last["roofline"]["frac"] > 0 and last["cpu_baseline"]["value"] > 0
    assert json.loads(lines[0])["dropin"] and json.load(open(tmp_path / "bench_extra.json"))["trained_regime"]
    # the driver's tail window (BENCH_r05.json kept 8.3 KB of stdout): the contract line fits whole
    assert len(lines[-1]) < 8000


def test_cpu_baseline_prefers_the_reference_on_the_same_host_type():
    d, ref = _recorded()
    port = {"value": 390.0, "unit": "rays/s", "cores": 32, "kind": "port", "sample": "x"}
    m = bench.merge_cpu_baseline(port, ref)
    assert m["kind"] == "reference" and m["value"] == ref["value"] and m["port_rays_per_s"] == 390.0 and m["cores"] == ref["torch_threads"] and m["same_host_type"]
    other = dict(ref, same_host_type=False)
    m = bench.merge_cpu_baseline(port, other)
    assert m["kind"] == "port" and m["value"] == 390.0 and m["reference"]["value"] is None and "measured on" in m["reference"]["refused"]
    m = bench.merge_cpu_baseline(port, {"refused": "no file"})
    assert m["kind"] == "port" and m["reference"]["refused"] == "no file"


def test_line_sheds_detail_before_it_exceeds_the_budget():
    d, _ = _recorded()
    d["config"]["workload"] = "x" * 3000                      # truncated to 400
    d["cpu_baseline"]["sample"] = "y" * 1800
    line = bench.contract_line(d)
    assert len(line) <= bench.LINE_BUDGET
    p = json.loads(line)
    assert "dropped_for_size" in p and "roofline" in p and "cpu_baseline" in p


def test_dump_outputs_writes_float_arrays_within_budget(tmp_path):
    """--dump-outputs: per-ray results, mesh and field samples as float32 / float64 .npy, large arrays cut to fixed seeded samples, <= 64 MB."""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(0)
    R, nv, nt = bench.DUMP_RAY_ROWS + 5, bench.DUMP_MESH_ROWS + 7, 1000
    outs = [{"color": torch.rand(R, 3, generator=g), "depth": torch.rand(R, generator=g), "weights_sum": torch.rand(R, generator=g),
             "depth_var": torch.rand(R, generator=g), "color_mask": torch.ones(R, dtype=torch.uint8)}]
    tris = torch.randint(0, nv, (nt, 3), generator=g)
    mesh = (torch.rand(nv, 3, generator=g, dtype=torch.float64), tris, torch.rand(nv, 3, generator=g), torch.rand(40, 40, 40, generator=g))
    vol = {"vol_cl": torch.rand(30, 30, 30, 16, generator=g), "n_voxels": 1234}
    bench.dump_outputs(str(tmp_path / "a"), vol, outs, mesh)
    bench.dump_outputs(str(tmp_path / "b"), vol, outs, mesh)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "color.npy" in files and "mesh_triangles.npy" in files
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f          # same inputs -> same files
        total += a.nbytes
    assert total <= bench.DUMP_BUDGET
    assert np.load(tmp_path / "a" / "color.npy").shape == (bench.DUMP_RAY_ROWS, 3)
    assert np.load(tmp_path / "a" / "mesh_vertices.npy").shape == (bench.DUMP_MESH_ROWS, 3)
    assert np.array_equal(np.load(tmp_path / "a" / "mesh_triangles.npy"), tris.numpy().astype(np.float64))
    assert np.load(tmp_path / "a" / "mesh_counts.npy").tolist() == [nv, nt, 1234]
    assert np.load(tmp_path / "a" / "volume_sample.npy").shape == (30 * 30 * 30 * 16,)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_outputs(tmp_path):
    """A plain run (no --full): --steps timed steps, the contract keys on the last line, nothing beyond the headline figure, the outputs dumped."""
    import subprocess
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["O2345_BENCH_EXTRA_FILE"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--vol", "64", "--ray-scale", "1",
                        "--mesh-res", "96", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    full, p = json.loads(lines[-2]), json.loads(lines[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in p, k
    assert p["steps"] == 3 and p["ms_per_step"] > 0 and abs(p["value"] - 65536 / (p["ms_per_step"] * 1e-3)) < 1e-6 * p["value"]
    assert not {"roofline", "cpu_baseline", "parity", "exhaustive"} & set(p)
    color = np.load(tmp_path / "color.npy")
    assert color.shape == (65536, 3) and color.dtype == np.float32 and np.isfinite(color).all()
    counts = np.load(tmp_path / "mesh_counts.npy")
    assert counts.tolist() == [full["mesh"]["vertices"], full["mesh"]["triangles"], full["kept_voxels"]] and counts[1] > 0
