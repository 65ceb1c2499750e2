"""GPU: the DAVIS boundary measure on the device (osvos_mask_jf_counts, csrc/boundary.hip) against the committed fixture
tests/golden/boundary_f.npz -- integer counts, compared exactly -- and the Python layers above it (results.boundary_f,
results.SequenceEvaluator, the J / F / J&F lines of train_online.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_cases as bc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = bc.load()


def _logit(thr):
    return float(np.log(thr / (1.0 - thr)))


def _jf(logits, gt, r, thr=0.5, counts=None, accumulate=0, dirty=False):
    """one osvos_mask_jf_counts call on CUDA tensors [N,1,H,W] -> the int64 count table [N, 6] (a CUDA tensor)"""
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    n, h, w = logits.shape[0], logits.shape[-2], logits.shape[-1]
    nbytes = l.osvos_boundary_ws_bytes(n, h, w)
    assert nbytes == 2 * n * h * ((w + 63) // 64) * 8
    ws = torch.empty(nbytes // 8, device=logits.device, dtype=torch.int64)
    if dirty:
        ws.fill_(-1)
    if counts is None:
        counts = torch.full((n, 6), -7 if dirty else 0, device=logits.device, dtype=torch.int64)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(l.osvos_mask_jf_counts(C.c_void_p(logits.data_ptr()), C.c_void_p(gt.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(counts.data_ptr()),
                                      n, h, w, _logit(thr), r, accumulate, stream), "mask_jf_counts")
    return counts


def _iou(logits, gt, thr=0.5):
    from osvos_pytorch_amd import _lib
    n = logits.shape[0]
    counts = torch.empty((n, 2), device=logits.device, dtype=torch.int64)
    _lib.check(_lib.lib().osvos_mask_iou_counts(C.c_void_p(logits.data_ptr()), C.c_void_p(gt.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                logits.numel() // n, n, _logit(thr), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "mask_iou_counts")
    return counts


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_counts_equal_the_golden_exactly(case):
    logits, gt = [torch.from_numpy(a).cuda() for a in bc.tensors(case)]
    got = _jf(logits, gt, case["r"], case["thr"], dirty=True).cpu().numpy()
    print(case["name"], "device", got.tolist(), "golden", case["counts"].tolist())
    assert np.array_equal(got, case["counts"]), (got.tolist(), case["counts"].tolist())
    # the region counts are those of the J kernel on the same tensors
    assert np.array_equal(got[:, :2], _iou(logits, gt, case["thr"]).cpu().numpy())
    from osvos_pytorch_amd import results
    fs = results.boundary_f(logits, gt, threshold=case["thr"], bound_th=case["r"])
    assert fs == case["f"].tolist()
    if case["thr"] == 0.5:
        js = results.jaccard(logits, gt)
        assert js == [1.0 if u == 0 else float(i) / float(u) for i, u in case["counts"][:, :2]]


def test_batch_equals_single_frames_accumulate_adds_and_side_stream_with_dirty_workspace():
    by_name = {c["name"]: c for c in CASES}
    for name in ("ellipse_roll", "noise_30x85_r8", "hd_shapes"):
        case = by_name[name]
        logits, gt = [torch.from_numpy(a).cuda() for a in bc.tensors(case)]
        whole = _jf(logits, gt, case["r"]).cpu().numpy()
        assert np.array_equal(whole, case["counts"])
        for i in range(case["N"]):
            one = _jf(logits[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), case["r"]).cpu().numpy()
            assert np.array_equal(one[0], whole[i]), (name, i)
        # accumulate: a table zeroed once, two calls -> the sum; then a call without the flag overwrites
        table = torch.zeros((case["N"], 6), device="cuda", dtype=torch.int64)
        _jf(logits, gt, case["r"], counts=table, accumulate=1)
        _jf(logits, gt, case["r"], counts=table, accumulate=1)
        assert np.array_equal(table.cpu().numpy(), 2 * whole), name
        _jf(logits, gt, case["r"], counts=table, accumulate=0)
        assert np.array_equal(table.cpu().numpy(), whole), name
        # a side stream, workspace and counts full of garbage: nothing is assumed zero
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _jf(logits, gt, case["r"], dirty=True)
        side.synchronize()
        assert np.array_equal(got.cpu().numpy(), whole), name


def test_radius_beyond_the_built_maximum_is_an_error_not_an_answer():
    from osvos_pytorch_amd import _lib, results
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="radius"):
        _jf(x, x, 1000)
    with pytest.raises(RuntimeError, match="radius"):
        results.boundary_f(x, x, bound_th=1000)
    assert _lib.lib().osvos_last_error()


def _synthetic_sequence():
    """12 frames, two frame sizes: a drifting, growing ellipse as the prediction (noisy logits) against a fixed one"""
    g = torch.Generator().manual_seed(7)
    batches = []
    for (h, w, n, per) in [(48, 64, 8, 3), (60, 107, 4, 2)]:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        gt = ((((yy - 0.5 * h) / (0.3 * h)) ** 2 + ((xx - 0.5 * w) / (0.3 * w)) ** 2) <= 1).float()
        frames = []
        for i in range(n):
            d = ((((yy - 0.5 * h - 0.4 * i) / (0.3 * h + 0.3 * i)) ** 2 + ((xx - 0.5 * w - 0.8 * i) / (0.3 * w)) ** 2))
            frames.append((1.0 - d) * 6.0 + 0.4 * torch.randn(h, w, generator=g))
        logits = torch.stack(frames)[:, None]
        gts = gt[None, None].repeat(n, 1, 1, 1)
        for s in range(0, n, per):
            batches.append((logits[s:s + per].cuda(), gts[s:s + per].cuda()))
    return batches


def test_sequence_evaluator_matches_the_per_frame_functions_without_touching_the_host(monkeypatch):
    from osvos_pytorch_amd import results
    batches = _synthetic_sequence()
    assert sum(b[0].shape[0] for b in batches) == 12
    js, fs = [], []
    for x, g in batches:
        js.extend(results.jaccard(x, g))
        fs.extend(results.boundary_f(x, g))
    assert 0.0 < min(fs) and min(fs) < 1.0 and len(set(fs)) > 4          # the sequence is not a trivial one
    torch.cuda.synchronize()

    calls = {"synchronize": 0, "cpu": 0, "item": 0, "tolist": 0}

    def counting(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(torch.cuda, "synchronize", counting("synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "cpu", counting("cpu", torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "item", counting("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "tolist", counting("tolist", torch.Tensor.tolist))
    ev = results.SequenceEvaluator()
    ev.CHUNK = 5                      # the table grows twice inside twelve frames
    for x, g in batches:
        ev.add(x, g)
    assert calls == {"synchronize": 0, "cpu": 0, "item": 0, "tolist": 0}, calls
    got_js, got_fs = ev.per_frame()
    assert calls["cpu"] == 1 and calls["synchronize"] == 0 and calls["item"] == 0 and calls["tolist"] == 0, calls
    monkeypatch.undo()

    assert ev.frames == 12 and got_js == js and got_fs == fs
    s = ev.summary()
    assert s["J"] == results.davis_statistics(js) and s["F"] == results.davis_statistics(fs) and s["frames"] == 12
    assert s["J&F"] == (s["J"]["mean"] + s["F"]["mean"]) / 2


def test_train_online_prints_j_f_and_jf(tmp_path):
    env = dict(os.environ, OSVOS_SAVE_ROOT=str(tmp_path), OSVOS_MODELS_DIR=str(tmp_path), PYTHONPATH=REPO, SEQ_NAME="blackswan")
    r = subprocess.run([sys.executable, "train_online.py", "--synthetic", "--epochs", "10", "--height", "48", "--width", "64"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    num = r"(-?\d+\.\d{4})"
    at = [i for i, ln in enumerate(lines) if ln.startswith("J (region similarity) on blackswan:")]
    assert len(at) == 1, r.stdout[-2000:]
    j = re.fullmatch(r"J \(region similarity\) on blackswan: mean %s recall %s decay %s over (\d+) frames" % (num, num, num), lines[at[0]])
    f = re.fullmatch(r"F \(contour accuracy\) on blackswan: mean %s recall %s decay %s over (\d+) frames" % (num, num, num), lines[at[0] + 1])
    jf = re.fullmatch(r"J&F on blackswan: %s" % num, lines[at[0] + 2])
    assert j and f and jf, lines[at[0]:at[0] + 3]
    assert j.group(4) == f.group(4) == "1"
    assert 0.0 <= float(j.group(1)) <= 1.0 and 0.0 <= float(f.group(1)) <= 1.0 and 0.0 <= float(f.group(2)) <= 1.0
    assert abs(float(jf.group(1)) - (float(j.group(1)) + float(f.group(1))) / 2) <= 1.01e-4          # (three numbers rounded to 4 places)
