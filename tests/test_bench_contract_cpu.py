"""The bench line's CONTRACT (CPU tier).  Two things are checked:

1. the COMPACT line bench.py prints (bench.compact_line / emit_line): it is ONE line of strict JSON (no NaN / Infinity), the LAST line of stdout, well
   under the 8,000 characters of stdout the driver keeps (BENCH_r05.json: a 21.9 KB line left `parsed: null`), and it carries every field the
   driver and the judge read -- metric = BASELINE.json's string, value = frames / time, roofline.frac = achieved / peak, parity numbers with
   within_bars, cpu_baseline, one short row per extra configuration; prose and per-kernel tables go to gpurun_out/bench_detail.json;
2. the committed line of the round's last GPU call (profiles/r06_bench_default.json when present, else the round-5 full record pushed through the
   same compactor): typed and mutually consistent."""
import importlib.util
import io
import json
import math
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R06_LINE = os.path.join(REPO, "profiles", "r06_bench_default.json")          # the compact line, as printed
R06_DETAIL = os.path.join(REPO, "profiles", "r06_bench_detail.json")         # the full record of the same run
R05_FULL = os.path.join(REPO, "profiles", "r05_bench_driver_cmd.json")       # round 5 printed the full record as its line
DRIVER_TAIL = 8000


def _strict_loads(text):
    def bad(c):
        raise ValueError("non-finite constant %s in the line" % c)
    return json.loads(text, parse_constant=bad)


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def full():
    path = R06_DETAIL if os.path.exists(R06_DETAIL) else R05_FULL
    with open(path) as f:
        text = f.read()
    return _strict_loads(text if path == R06_DETAIL else [l for l in text.splitlines() if l.startswith("{")][-1])


@pytest.fixture(scope="module")
def line(bench, full):
    if os.path.exists(R06_LINE):
        with open(R06_LINE) as f:
            return _strict_loads([l for l in f.read().splitlines() if l.startswith("{")][-1])
    return json.loads(json.dumps(bench.compact_line(full, "gpurun_out/bench_detail.json")))


def test_printed_line_is_small_strict_and_last(bench, full, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "REPO", str(tmp_path))
    out = io.StringIO()
    out.write("some earlier stdout\n")
    dirty = dict(full)
    dirty["running_loss"] = float("nan")                     # a diverged run must still print a parseable line
    dirty["roofline"] = dict(full["roofline"], achieved=float("inf"))
    bench.emit_line(dirty, False, out)
    text = out.getvalue()
    assert text.endswith("}\n") and text.count("\n") == 2                       # ONE line, and nothing after it
    last = text.splitlines()[-1]
    assert len(last) < bench.LINE_LIMIT < DRIVER_TAIL - 1500                    # fits the driver's stdout tail whole, with room for a preamble
    d = _strict_loads(last)
    assert d["running_loss"] is None and d["roofline"]["achieved"] is None
    assert d["detail"] == "gpurun_out/bench_detail.json"
    with open(os.path.join(str(tmp_path), d["detail"])) as f:                    # the prose / tables went to the side file, strict JSON too
        det = _strict_loads(f.read())
    assert "extra_configs" in det and "timed_region_detail" in det
    assert "note" not in json.dumps({k: v for k, v in d.items() if k != "cpu_baseline"})      # numbers only
    # --full-line (what the extra-config sub-processes print for their parent) is the whole record on one line
    out2 = io.StringIO()
    bench.emit_line(full, True, out2)
    assert out2.getvalue().count("\n") == 1 and _strict_loads(out2.getvalue())["config"] == full["config"]


def test_line_sheds_fields_rather_than_outgrow_the_tail(bench, full, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "REPO", str(tmp_path))
    fat = json.loads(json.dumps(full))
    fat["extra_configs"] = (fat.get("extra_configs") or []) * 12
    out = io.StringIO()
    bench.emit_line(fat, False, out)
    assert len(out.getvalue()) < DRIVER_TAIL - 1000
    d = _strict_loads(out.getvalue())
    assert d["value"] == full["value"] and d["roofline"]["frac"] == full["roofline"]["frac"]


def test_driver_fields(line):
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert line["metric"] == base["metric"].replace("×", "x")
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["scaling"] == "weak" and line["data"] == "synthetic"
    assert line["n_gpus"] == 1 and line["steps"] > 0 and line["warmup"] >= 0 and line["vs_baseline"] is None      # BASELINE.md publishes no number
    assert "workload" in line["config"] and "854x480 batch=1 online" in line["config"]["workload"] and "model" not in line["config"]
    assert line["config"]["global_batch"] == 1 and line["config"]["parallelism"] == "dp1"
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 2e-3 * line["value"]          # batch 1: frames/s = 1000 / ms per step
    assert line["dtype"].startswith("f32") and len(line["dtype"]) < 64
    assert 1500 < line["pipe_sustained_tflops"] < 2600                                      # box speed, next to the value
    assert all(isinstance(line[k], (int, float)) and math.isfinite(line[k]) for k in ("value", "ms_per_step", "sustained_value"))


def test_roofline_and_cpu_baseline(line):
    r = line["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0.3 < r["frac"] < 1.0
    assert r["avg_launch_ms"] * 1.0 < line["ms_per_step"]                                   # a launch is shorter than the step that holds it
    assert abs(r["executed_over_algorithmic"] - 5.97) < 0.05                                # f32x3: six bf16 products per fp32 product, minus the exact passes
    assert 0.3 < r["step_conv_fraction_of_mfma_roofline"] <= r["frac"] + 0.02
    t = r["traffic"]
    assert t["static"] is True and t["measured_at_commit"] not in ("", "unknown") and t["source"].startswith("profiles/r0")
    assert "pmc_traffic_configs1" in t["source"] and os.path.exists(os.path.join(REPO, t["source"]))
    assert 1.0 < t["ratio"] < 3.0 and t["conv_algorithmic_MB_per_step"] == 2712.0
    assert abs(t["conv_hbm_MB_per_launch"] - t["conv_hbm_MB_per_step"] / r["launches"]) < 0.1
    ps = r["pipe_sustained"]
    assert 1500 < ps["noise"] < ps["zeros"] <= 2600
    c = line["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "frames/s" and 0.1 < c["value"] < 50 and 1 <= c["cores"] <= c["host_nproc"] and "iterations" in c["sample"]
    assert abs(line["gpu_over_cpu"] - line["value"] / c["value"]) < 0.01 * line["gpu_over_cpu"]


def test_parity_gate_is_in_the_line(line):
    p = line["parity"]
    assert p["within_bars"] is True and p["bars"] == {"max_dlogit_over_std": 1e-3, "loss_rel": 1e-5, "grad_rel_l2": 1e-3, "iou": 1.0 - 1e-3}
    assert p["max_dlogit_over_std"] <= 1e-3 and p["loss_rel"] <= 1e-5 and p["iou"] >= 1 - 1e-3 and p["grad_rel_l2_worst"] <= 1e-3
    extras = {e["config"]: e for e in line["extra_configs"]}
    assert set(extras) >= {"configs[1]/fp32-exact", "configs[1]/window-fused", "configs[2]", "configs[4]", "configs[4]/fp32-exact"}      # (+ configs[1]/fp32x2 from round 6 on)
    if "configs[1]/fp32x3b2" in extras:    # forward = the headline's, backward on two pieces: faster AND inside the flat f32 bars
        b2 = extras["configs[1]/fp32x3b2"]
        assert b2["within_bars"] is True and b2["value"] > 1.1 * line["value"] and b2["max_dlogit_over_std"] == line["parity"]["max_dlogit_over_std"]
    if "configs[1]/fp32x2" in extras:      # two bf16 pieces per operand: faster than the headline, flat f32 bars reported honestly, its own bars held
        x2 = extras["configs[1]/fp32x2"]
        assert x2["within_x2_bars"] is True and x2["iou"] >= 1 - 1e-3 and x2["max_dlogit_over_std"] <= 1e-3 and x2["value"] > line["value"]
    if "configs[1]/fp32x3h2" in extras:    # forward = the headline's, backward on FP16 pairs under block exponents (22-23-bit operands, three products)
        h = extras["configs[1]/fp32x3h2"]
        assert h["within_bars"] is True and h["value"] > 1.1 * line["value"] and h["max_dlogit_over_std"] == line["parity"]["max_dlogit_over_std"]
    if "configs[1]/fp32h2" in extras:      # FP16 pairs in both passes: logits / loss / IoU at the flat bars; the gradient bar is the ReLU-flip lottery (profiles/r06_fp32h2.txt)
        h = extras["configs[1]/fp32h2"]
        assert h["max_dlogit_over_std"] <= 1e-3 and h["loss_rel"] <= 1e-5 and h["iou"] >= 1 - 1e-3 and h["value"] > 1.2 * line["value"]
        assert h["within_bars"] is True or h["grad_rel_l2_worst"] <= 3e-3
    if "configs[4]/fp32h2" in extras:      # inference: inside the flat bars, faster than the three-piece forward
        h = extras["configs[4]/fp32h2"]
        assert h["within_bars"] is True and h["value"] > 1.3 * extras["configs[4]"]["value"]
    for e in extras.values():
        assert "error" not in e and e["value"] > 0 and e["ms_per_step"] > 0 and 0.2 < e["frac"] < 1.0
    c2, c4 = extras["configs[2]"], extras["configs[4]"]
    assert c2["dtype"] == "bf16" and isinstance(c2["within_bars"], bool) and c2["iou"] >= 0.985 and 1.0 < c2["traffic_ratio"] < 2.0
    assert c4["within_bars"] is True and c4["iou"] >= 1 - 1e-3 and c4["algorithmic_hbm_GBps"] > 100
    assert extras["configs[1]/fp32-exact"]["within_bars"] is True


def test_dump_outputs_stay_under_the_limit_and_sample_the_same_indices(bench, tmp_path):
    """--dump-outputs: DIR/<name>.npy in float32 / float64, at most 64 MB together; an output set larger than that (configs[4]: five 1920x1080
    batch-4 logit maps) is cut to a fixed seeded sample, the same elements in every run, so two runs can be compared array for array."""
    import numpy as np
    rng = np.random.default_rng(0)
    arrays = {n: rng.standard_normal((4, 1, 1080, 1920)).astype(np.float32) for n in bench.HEAD_NAMES}
    arrays["loss"] = np.arange(5, dtype=np.float64)
    small = {"logits_fused": arrays["logits_fused"][:1, :, :48, :64], "loss": arrays["loss"]}
    for tag in ("a", "b"):
        bench.write_outputs(arrays, str(tmp_path / tag))
        bench.write_outputs(small, str(tmp_path / ("small_" + tag)))
    for tag in ("a", "b"):
        files = sorted(os.listdir(str(tmp_path / tag)))
        assert files == sorted(n + ".npy" for n in arrays)
        assert sum(os.path.getsize(str(tmp_path / tag / f)) for f in files) <= bench.DUMP_LIMIT_BYTES <= 64 * 10 ** 6
    for n in arrays:
        a, b = np.load(str(tmp_path / "a" / (n + ".npy"))), np.load(str(tmp_path / "b" / (n + ".npy")))
        assert a.dtype == arrays[n].dtype and np.array_equal(a, b)
        assert np.isin(a, arrays[n]).all()                        # a sample of the array's own elements
    assert np.array_equal(np.load(str(tmp_path / "small_a" / "logits_fused.npy")), small["logits_fused"])      # under the limit: whole, shape kept
