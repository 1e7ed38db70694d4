"""CPU-side checks of bench.py: the workload table, the CPU-baseline leg (the oracle timed on a tiny sample), the
line's schema helpers and the output dump -- so a broken baseline leg cannot take the driver's bench run down on the GPU
box.  On the GPU (`-m gpu`): a plain run and its `--dump-outputs`, in fresh child processes."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
bench = importlib.util.module_from_spec(spec)
sys.modules["bench"] = bench          # the worker pool pickles bench._cpu_worker by module name
spec.loader.exec_module(bench)


def test_workloads_name_baseline_configs():
    assert bench.WORKLOADS["pusch273_4rx_filter"] == dict(smoothing="filter", ports=4, slots=8192)      # configs[2], the default
    assert bench.WORKLOADS["pusch273_1rx_none"] == dict(smoothing="none", ports=1, slots=1024)          # configs[1]
    assert bench.WORKLOADS["pusch273_4rx_cnn"]["interp"] == "cnn" and bench.WORKLOADS["pusch273_4rx_denoise"]["denoise"]
    assert bench.HBM_PEAK_GBS == 8000.0 and bench.MFMA_F16_PEAK_TFLOPS == 2500.0
    assert bench.DENOISE_FLOP_PER_PIXEL == 5760


def test_cpu_baseline_leg_runs_on_a_small_sample():
    from srsran_ce_pytorch_amd import synth as S
    case = S.case_spec("tiny", 25, [S.hop_spec([2, 11], 0, 25)], seed=3)
    for flavour, denoise in (("tensorized", False), ("tensorized", True), ("baseline_loop", False), ("cnn", False)):
        items, seconds = bench._cpu_worker((case, 2, 1, 7, flavour, denoise))
        assert items == 2 and seconds > 0
    out = bench.cpu_baseline(case, 2, target_core_seconds=0.2)
    assert out["unit"] == "slots/s" and out["kind"] == "port" and out["value"] > 0 and 1 <= out["cores"] <= 16
    # `value` is the loop-style ce_rule_baseline port (the baseline north_star names); the tensorized port sits next to it
    # (no ordering between the two is asserted: 0.2 core-seconds on a busy host say nothing about speed)
    assert out["flavour"].startswith("ce_rule_baseline") and out["tensorized_value"] > 0 and out["config0_ms"] > 0
    json.dumps(out)
    cnn = bench.cpu_baseline(case, 2, target_core_seconds=0.2, interp="cnn")
    assert cnn["flavour"] == "ce_dl_cnn" and cnn["value"] > 0 and "tensorized_value" not in cnn


DUMPED = ("noise", "rsrp", "epre", "ta", "cfo_hz", "ch_est_sample", "ch_est_sample_items")


def test_dump_outputs_writes_a_fixed_sample_within_the_budget(tmp_path):
    B, R, n_sc, n_sym = 6, 4, 24, 14
    g = torch.Generator().manual_seed(0)
    ch = torch.randn((B, R, n_sc, n_sym, 1), dtype=torch.complex64, generator=g)
    sc = torch.randn((5, B, R), dtype=torch.float64, generator=g)
    out = (ch, sc[0], sc[1], sc[2], sc[3], sc[4])
    budget = 5 * B * R * 8 + 10 * (n_sc * n_sym * 8 + 16) + 3             # room for the scalars and 10 of the 24 items
    first = bench.dump_outputs(out, tmp_path / "a", budget=budget)
    loaded = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(loaded) == sorted(DUMPED)
    assert all(a.dtype in (np.float32, np.float64) for a in loaded.values())
    assert sum(a.nbytes for a in loaded.values()) <= budget
    for k, name in enumerate(("noise", "rsrp", "epre", "ta", "cfo_hz")):
        assert np.array_equal(loaded[name], sc[k].numpy())
    items = loaded["ch_est_sample_items"].astype(int)
    assert items.shape == (10, 2) and len({tuple(i) for i in items}) == 10
    for (s, r), got in zip(items, loaded["ch_est_sample"]):
        assert got.dtype == np.float32 and np.array_equal(got, torch.view_as_real(ch[s, r]).numpy())
    again = bench.dump_outputs(out, tmp_path / "b", budget=budget)       # the same sample every time
    assert all(np.array_equal(first[k], again[k]) for k in DUMPED)
    # the headline (8192 slots x 4 ports, 3276 x 14 x 1 estimates) fits the 64 MB
    assert 5 * 8192 * 4 * 8 + bench.DUMP_MAX_ITEMS * (3276 * 14 * 8 + 16) <= bench.DUMP_BUDGET_BYTES


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path):
    """A plain run times exactly --steps steps and carries nothing of --full's; two runs with the same arguments dump the
    same outputs (seeded inputs, deterministic kernel)."""
    lines, dumps = [], []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--slots", "64", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout
        lines.append(out[0])
        dumps.append({name: np.load(d / f"{name}.npy") for name in DUMPED})
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "slots/s"
        assert line["value"] == pytest.approx(64 * 3 / (line["ms_per_step"] * 3 * 1e-3), rel=1e-6)
        assert "cpu_baseline" not in line and "secondary" not in line
    a, b = dumps
    assert a["ch_est_sample"].shape[0] == 128 and a["rsrp"].shape == (64, 4)                # 64 slots x 4 ports: 128 of 256 items
    assert np.isfinite(a["ch_est_sample"]).all() and np.isfinite(a["rsrp"]).all()
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in DUMPED)
