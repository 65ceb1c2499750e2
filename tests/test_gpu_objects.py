"""GPU: the multi-object (DAVIS 2017) results path on the device -- osvos_merge_objects and osvos_labels_jf_counts (csrc/objects.hip) against
the committed fixture tests/golden/objects.npz, every comparison exact (bytes and integers); the per-object rows against the single-object
entry point osvos_mask_jf_counts on the object's two binary maps; results.MultiObjectEvaluator; train_online.py --multi-object."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import object_cases as oc
import script_runner

pytestmark = pytest.mark.gpu
CASES = oc.load()
IDS = [c["name"] for c in CASES]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _merge(x, thr=0.5, dirty=True):
    """one osvos_merge_objects call on a CUDA tensor [K,N,H,W] -> uint8 CUDA tensor [N,H,W]"""
    from osvos_pytorch_amd import _lib
    k, n, h, w = x.shape
    out = torch.full((n, h, w), 201 if dirty else 0, device=x.device, dtype=torch.uint8)
    _lib.check(_lib.lib().osvos_merge_objects(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), n, k, h, w, float(oc.logit_threshold(thr)),
                                              _stream()), "merge_objects")
    return out


def _counts(pred, gt, k, r, counts=None, accumulate=0, dirty=False):
    """one osvos_labels_jf_counts call on uint8 CUDA tensors [N,H,W] -> the int64 count table [N, K, 6] (a CUDA tensor)"""
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    n, h, w = pred.shape
    nbytes = l.osvos_labels_jf_ws_bytes(n, k, h, w)
    assert nbytes == 2 * n * k * h * ((w + 63) // 64) * 8
    ws = torch.empty(nbytes // 8, device=pred.device, dtype=torch.int64)
    if dirty:
        ws.fill_(-1)
    if counts is None:
        counts = torch.full((n, k, 6), -7 if dirty else 0, device=pred.device, dtype=torch.int64)
    _lib.check(l.osvos_labels_jf_counts(C.c_void_p(pred.data_ptr()), C.c_void_p(gt.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(counts.data_ptr()),
                                        n, k, h, w, r, accumulate, _stream()), "labels_jf_counts")
    return counts


def _mask_jf(p, g, r):
    """the single-object entry point on two bool maps [N,H,W] fed as floats (logit threshold 0: P = x > 0) -> int64 [N, 6]"""
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    n, h, w = p.shape
    x, y = p.float().contiguous() * 2 - 1, g.float().contiguous()
    ws = torch.empty(l.osvos_boundary_ws_bytes(n, h, w) // 8, device=p.device, dtype=torch.int64)
    counts = torch.empty((n, 6), device=p.device, dtype=torch.int64)
    _lib.check(l.osvos_mask_jf_counts(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(counts.data_ptr()),
                                      n, h, w, 0.0, r, 0, _stream()), "mask_jf_counts")
    return counts


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_merge_equals_the_fixture_label_maps(case):
    from osvos_pytorch_amd import results
    x = torch.from_numpy(oc.logits(case)).cuda()
    got = _merge(x, case["thr"]).cpu().numpy()
    bad = np.argwhere(got != case["pred"])
    print(case["name"], "pixels that differ:", len(bad), bad[:5].tolist())
    assert np.array_equal(got, case["pred"])
    # a batch equals its single frames (a single frame of an odd size takes the one-pixel-per-lane form)
    for n in range(case["N"]):
        one = _merge(x[:, n:n + 1].contiguous(), case["thr"]).cpu().numpy()
        assert np.array_equal(one[0], case["pred"][n]), (case["name"], n)
    # a side stream, and the Python layer (also with the channel axis a network output carries)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = _merge(x, case["thr"])
    side.synchronize()
    assert np.array_equal(s.cpu().numpy(), case["pred"])
    lab = results.merge_objects(x, threshold=case["thr"])
    assert lab.dtype == torch.uint8 and lab.is_cuda and np.array_equal(lab.cpu().numpy(), case["pred"])
    assert np.array_equal(results.merge_objects(x[:, :, None], threshold=case["thr"]).cpu().numpy(), case["pred"])


def test_merge_on_unaligned_planes_and_a_pointer_off_the_16_byte_grid():
    """plane strides that are not multiples of four floats, and a logits pointer 4 bytes past a 16-byte boundary"""
    case = [c for c in CASES if c["name"] == "k3_30x85_r8"][0]
    x = oc.logits(case)[:, :1]                                    # 30 x 85 = 2550 floats per plane
    assert x[0].size % 4 != 0
    assert np.array_equal(_merge(torch.from_numpy(np.ascontiguousarray(x)).cuda(), case["thr"]).cpu().numpy(), case["pred"][:1])
    full = oc.logits(case)                                        # 5100 floats per plane: vector form when aligned
    flat = torch.empty(full.size + 1, device="cuda", dtype=torch.float32)
    flat[1:].copy_(torch.from_numpy(full).reshape(-1))
    assert flat[1:].data_ptr() % 16 == 4
    assert np.array_equal(_merge(flat[1:].view(*full.shape), case["thr"]).cpu().numpy(), case["pred"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_equal_the_fixture_and_the_single_object_entry_point(case):
    pred, gt = torch.from_numpy(case["pred"]).cuda(), torch.from_numpy(case["gt"]).cuda()
    k, r = case["K"], case["r"]
    got = _counts(pred, gt, k, r, dirty=True).cpu().numpy()
    print(case["name"], "device", got.tolist(), "golden", case["counts"].tolist())
    assert np.array_equal(got, case["counts"])
    # every object's row is osvos_mask_jf_counts on that object's two binary maps
    for j in range(1, k + 1):
        ref = _mask_jf(pred == j, gt == j, r).cpu().numpy()
        assert np.array_equal(got[:, j - 1], ref), (case["name"], j, got[:, j - 1].tolist(), ref.tolist())
    # a batch equals its single frames
    for n in range(case["N"]):
        one = _counts(pred[n:n + 1].contiguous(), gt[n:n + 1].contiguous(), k, r).cpu().numpy()
        assert np.array_equal(one[0], case["counts"][n]), (case["name"], n)
    # accumulate: a table zeroed once, two calls -> the sum; then a call without the flag overwrites
    table = torch.zeros((case["N"], k, 6), device="cuda", dtype=torch.int64)
    _counts(pred, gt, k, r, counts=table, accumulate=1)
    _counts(pred, gt, k, r, counts=table, accumulate=1)
    assert np.array_equal(table.cpu().numpy(), 2 * case["counts"])
    _counts(pred, gt, k, r, counts=table, accumulate=0)
    assert np.array_equal(table.cpu().numpy(), case["counts"])
    # a side stream, workspace and counts full of garbage: nothing is assumed zero
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = _counts(pred, gt, k, r, dirty=True)
    side.synchronize()
    assert np.array_equal(s.cpu().numpy(), case["counts"])


def test_a_larger_k_only_appends_rows():
    """ids above K belong to no object: counting the K = 3 maps with K = 5 gives the same three rows and two rows of an absent object"""
    case = [c for c in CASES if c["name"] == "k3_30x85_r8"][0]
    pred, gt = torch.from_numpy(case["pred"]).cuda(), torch.from_numpy(case["gt"]).cuda()
    got = _counts(pred, gt, 5, case["r"], dirty=True).cpu().numpy()
    assert np.array_equal(got[:, :3], case["counts"]) and not got[:, 3:].any()
    got2 = _counts(pred, gt, 2, case["r"], dirty=True).cpu().numpy()
    assert np.array_equal(got2, case["counts"][:, :2])


def test_argument_errors_are_errors_not_answers():
    from osvos_pytorch_amd import _lib, results
    l = _lib.lib()
    p = torch.zeros(1, 8, 8, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="radius"):
        _counts(p, p, 1, 0)
    with pytest.raises(RuntimeError, match="radius"):
        _counts(p, p, 1, 65)
    # K above the built maximum, N * K above 65535, unaligned ws / counts: called directly (the helper's size query answers 0 for such K)
    ws = torch.empty(64, device="cuda", dtype=torch.int64)
    counts = torch.empty(17 * 6 + 1, device="cuda", dtype=torch.int64)
    vp = C.c_void_p

    def call(k, n=1, ws_off=0, c_off=0):
        return l.osvos_labels_jf_counts(vp(p.data_ptr()), vp(p.data_ptr()), vp(ws.data_ptr() + ws_off), vp(counts.data_ptr() + c_off), n, k, 8, 8, 1, 0,
                                        _stream())
    assert call(17) < 0 and b"K 17 objects" in l.osvos_last_error()
    assert call(0) < 0 and b"K 0 objects" in l.osvos_last_error()
    assert call(16, n=4096) < 0 and b"65535" in l.osvos_last_error()          # (checked before anything is read)
    assert call(1, ws_off=4) < 0 and b"aligned" in l.osvos_last_error()
    assert call(1, c_off=4) < 0 and b"aligned" in l.osvos_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(call(17), "labels_jf_counts")
    x = torch.zeros(17, 1, 8, 8, device="cuda")
    out = torch.empty(1, 8, 8, device="cuda", dtype=torch.uint8)
    assert l.osvos_merge_objects(vp(x.data_ptr()), vp(out.data_ptr()), 1, 17, 8, 8, 0.0, _stream()) < 0 and b"K 17 objects" in l.osvos_last_error()
    assert l.osvos_merge_objects(vp(x.data_ptr()), vp(out.data_ptr()), 1, 0, 8, 8, 0.0, _stream()) < 0
    with pytest.raises(ValueError):
        results.merge_objects(x)
    with pytest.raises(RuntimeError):
        results.merge_objects(x.cpu()[:2])
    torch.cuda.synchronize()


def _label_sequence():
    """12 frames, two frame sizes, three objects: drifting ellipses as the prediction against fixed ones, in batches"""
    batches = []
    for (h, w, n, per) in [(48, 64, 8, 3), (60, 107, 4, 2)]:
        gt = oc.raster([(oc.ELLIPSE, 0.5 * h, 0.3 * w, 0.3 * h, 0.15 * w, 0, 1), (oc.ELLIPSE, 0.5 * h, 0.7 * w, 0.25 * h, 0.2 * w, 0, 2),
                        (oc.RECT, 0, 0.2 * h, 0, 0.5 * w, 0, 3)], h, w)
        preds = [oc.raster([(oc.ELLIPSE, 0.5 * h + 0.4 * i, 0.3 * w + 0.8 * i, 0.3 * h, 0.15 * w + 0.3 * i, 0, 1),
                            (oc.ELLIPSE, 0.5 * h, 0.7 * w - 0.5 * i, 0.25 * h + 0.4 * i, 0.2 * w, 0, 2),
                            (oc.RECT, 0, 0.2 * h + (i % 3), 0, 0.5 * w - i, 0, 3)], h, w) for i in range(n)]
        p, g = torch.from_numpy(np.stack(preds)), torch.from_numpy(np.stack([gt] * n))
        for s in range(0, n, per):
            batches.append((p[s:s + per].cuda(), g[s:s + per].cuda()))
    return batches


def test_multi_object_evaluator_matches_the_single_object_functions_without_touching_the_host(monkeypatch):
    from osvos_pytorch_amd import results
    batches = _label_sequence()
    assert sum(b[0].shape[0] for b in batches) == 12
    want = []
    for k in (1, 2, 3):
        js, fs = [], []
        for p, g in batches:
            x, y = ((p == k).float() * 2 - 1)[:, None], (g == k).float()[:, None]
            js.extend(results.jaccard(x, y))
            fs.extend(results.boundary_f(x, y))
        want.append((js, fs))
    assert all(0.0 < min(fs) < 1.0 and len(set(fs)) > 4 for _, fs in want)          # the sequence is not a trivial one
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
    ev = results.MultiObjectEvaluator(3)
    ev.CHUNK = 5                      # the table grows twice inside twelve frames
    for p, g in batches:
        ev.add(p, g)
    assert calls == {"synchronize": 0, "cpu": 0, "item": 0, "tolist": 0}, calls
    got = ev.per_object()
    assert calls["cpu"] == 1 and calls["synchronize"] == 0 and calls["item"] == 0 and calls["tolist"] == 0, calls
    s = ev.summary()
    e = ev.summary(exclude_ends=True)
    assert calls["cpu"] == 1, calls                                                  # (the read-back is kept)
    monkeypatch.undo()

    assert ev.frames == 12 and got == want
    assert s["frames"] == 12 and e["frames"] == 10
    for k in range(3):
        assert s["objects"][k]["J"] == results.davis_statistics(want[k][0]) and s["objects"][k]["F"] == results.davis_statistics(want[k][1])
        assert e["objects"][k]["J"] == results.davis_statistics(want[k][0][1:-1])
    assert s["J"] == pytest.approx(np.mean([np.mean(w[0]) for w in want]), abs=1e-12)
    assert s["J&F"] == 0.5 * (s["J"] + s["F"])


def test_train_online_multi_object(tmp_path):
    from PIL import Image
    r = script_runner.train_online(tmp_path, "--multi-object", epochs=10, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    num = r"(-?\d+\.\d{4})"
    objs = [re.fullmatch(r"J&F on blackswan object (\d+): J %s F %s" % (num, num), ln) for ln in lines]
    objs = [m for m in objs if m]
    assert [m.group(1) for m in objs] == ["1", "2"], r.stdout[-2000:]
    seq = [re.fullmatch(r"J&F on blackswan \(2 objects\): %s" % num, ln) for ln in lines]
    seq = [m for m in seq if m]
    assert len(seq) == 1, r.stdout[-2000:]
    assert any(ln.startswith("Testing time multi-object: ") for ln in lines)
    js, fs = [float(m.group(2)) for m in objs], [float(m.group(3)) for m in objs]
    assert all(0.0 <= v <= 1.0 for v in js + fs)
    assert abs(float(seq[0].group(1)) - (sum(js) + sum(fs)) / 4) <= 1.01e-4          # (the mean of four numbers rounded to 4 places, itself rounded)
    with Image.open(os.path.join(str(tmp_path), "Results", "blackswan", "00000.png")) as im:
        assert im.mode == "P" and im.size == (64, 48)
        assert set(np.unique(np.asarray(im)).tolist()) <= {0, 1, 2}
