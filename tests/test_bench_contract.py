"""The bench line's contract, checked on the line committed with the round's profiles (profiles/r04/bench_final.json: what
`python bench.py --steps 20 --warmup 5` printed on an MI355X with the final code, every leg included, as `--full` runs
them now): the keys the driver and the judge read, the roofline block computed from algorithmic bytes over the kernel's
measured launch time, the CPU baseline beside it.
No GPU needed: this guards the SHAPE of the line against edits of bench.py that nobody runs on a GPU box before a round ends."""
import json
from pathlib import Path

import pytest

LINE = Path(__file__).resolve().parent.parent / "profiles" / "r04" / "bench_final.json"


@pytest.fixture(scope="module")
def line():
    if not LINE.exists():
        pytest.skip("no committed bench line")
    return json.loads(LINE.read_text().strip().splitlines()[-1])


def test_bench_line_has_the_contract_keys(line):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["metric"] == "embedded_scf_cycles_per_sec" and line["unit"] == "cycles/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["data"] == "synthetic" and line["vs_baseline"] is None  # (BASELINE.md publishes no number)
    assert line["n_gpus"] == 1 and line["steps"] == 20 and line["warmup"] == 5
    assert "workload" in line["config"] and "model" not in line["config"] and "N_AO=148" in line["config"]["workload"]
    # value = steps / time, whole job
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]


def test_roofline_block_is_algorithmic_bytes_over_measured_launch_time(line):
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["kernel"] == "jk_m8_kernel"
    n = line["config"]["nao"]
    pairs = n * (n + 1) // 2
    # the 8-fold unique integrals, read once per build
    assert r["algorithmic_bytes_per_launch"] == 8 * pairs * (pairs + 1) // 2 == r["bytes_8fold_floor"]
    achieved = r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9
    assert abs(achieved - r["achieved"]) < 1e-6 * achieved and abs(r["frac"] - achieved / r["peak"]) < 1e-9
    assert 0.0 < r["frac"] < 1.0 and r["launches"] >= 1
    assert r["frac"] == r["frac_vs_8fold_floor"] and r["frac_on_4fold_bytes"] > r["frac"]
    # the kernel cannot be slower than the cycle it is part of, and PMC traffic (if measured) is at least the algorithmic bytes
    assert r["avg_launch_ms"] < line["ms_per_step"]
    assert r["traffic"] is None or r["traffic"] >= r["algorithmic_bytes_per_launch"]
    assert r["bytes_read_by_kernel"] >= r["algorithmic_bytes_per_launch"]


def test_cpu_baseline_block(line):
    c = line["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] in ("port", "reference") and c["unit"] == "cycles/s" and c["cores"] >= 1 and c["value"] > 0
    assert line["value"] > c["value"]


def test_secondary_legs_are_present(line):
    for key in ("time_to_solution", "fixed10_cold", "mu_shift", "transform", "n2000_streamed", "n2000_density_fitted_jk",
                "scaling_workload", "small_configs", "breakdown_ms_per_cycle", "check"):
        assert key in line, key
    assert line["fixed10_cold"]["cycles"] == 10
    assert line["mu_shift"]["cycles_per_sec"] > 0 and "cpu_baseline" in line["mu_shift"]
    assert {s["nao"] for s in line["scaling_workload"]} == {256, 384}
    assert line["check"]["one_call_per_cycle"] is True


def _bench_module():
    import sys

    root = str(LINE.parents[2])
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench

    return bench


def test_plain_run_leaves_out_every_secondary_leg(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse_args()
    assert not args.full and args.steps == 7 and args.warmup == 2 and args.dump_outputs is None
    assert all(getattr(args, f"no_{leg}") for leg in bench.SECONDARY_LEGS)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--no-df", "--dump-outputs", "out"])
    args = bench.parse_args()
    assert args.full and args.no_df and args.dump_outputs == "out"
    assert not any(getattr(args, f"no_{leg}") for leg in bench.SECONDARY_LEGS if leg != "df")


def test_dump_outputs_float64_and_bounded(tmp_path):
    import numpy as np

    bench = _bench_module()
    small = np.arange(12, dtype=np.float32).reshape(3, 4)
    big = np.arange(3 * 2048 * 2048, dtype=np.float64).reshape(3, 2048, 2048)  # 96 MB
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"small": small, "big": big})
    got = {f.name: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert set(got) == {"small.npy", "big.npy"}
    assert got["small.npy"].dtype == np.float64 and np.array_equal(got["small.npy"], small)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_LIMIT_BYTES + 4096
    s = got["big.npy"]  # a fixed sample in index order (big holds its own flat indices) and the same one every time
    assert s.ndim == 1 and 0 < s.size < big.size and np.all(np.diff(s) > 0)
    assert np.array_equal(s, big.ravel()[s.astype(np.int64)])
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))


@pytest.mark.gpu
def test_plain_bench_run_and_dumped_outputs(tmp_path):
    """A plain bench run in a child process: exactly --steps timed cycles, the secondary legs null, and the arrays of the
    timed SCF run written by --dump-outputs."""
    import subprocess
    import sys

    import numpy as np

    out_dir = tmp_path / "dump"
    cmd = [sys.executable, str(LINE.parents[2] / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == "embedded_scf_cycles_per_sec" and out["steps"] == 4 and out["warmup"] == 2
    assert out["full"] is False and out["ms_per_step"] > 0 and abs(out["value"] - 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    for key in ("cpu_baseline", "time_to_solution", "fixed10_cold", "mu_shift", "transform", "n2000_streamed",
                "n2000_density_fitted_jk", "real_molecule", "small_configs", "scaling_workload", "multi_gpu"):
        assert out[key] is None, key
    n = out["config"]["nao"]
    shapes = {"mo_coeff": (2, n, n), "mo_energy": (2, n), "dm": (2, n, n), "huzinaga_operator": (2, n, n)}
    for name, shape in shapes.items():
        a = np.load(out_dir / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == shape and np.all(np.isfinite(a)), name
    assert np.all(np.diff(np.load(out_dir / "mo_energy.npy"), axis=1) >= 0)
