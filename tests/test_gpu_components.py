"""GPU: connected-component labelling and selection on the device -- osvos_mask_components and osvos_components_select (csrc/components.hip)
against the committed fixture tests/golden/components.npz, every comparison exact (integers and bytes); results.components,
results.filter_components, results.ComponentTracker; train_online.py --track-components."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import component_cases as cc
import script_runner

pytestmark = pytest.mark.gpu
CASES = cc.load()
BY_NAME = {c["name"]: c for c in CASES}
LOGITS = {c["name"]: cc.logits(c) for c in CASES}          # made once, shared, never written to
IDS = [c["name"] for c in CASES]
vp = C.c_void_p


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _ws(n, h, w):
    from osvos_pytorch_amd import _lib
    nbytes = _lib.lib().osvos_components_ws_bytes(n, h, w)
    assert nbytes == 16 * n + (4 * n * h * w + 7) // 8 * 8 + 8 * n * h * ((w + 63) // 64)
    return torch.full(((nbytes + 7) // 8,), -3, device="cuda", dtype=torch.int64)         # garbage: nothing is assumed zero


def _label(x, thr, conn, want_area=True, want_stats=True):
    """one osvos_mask_components call on a CUDA tensor [N,H,W], outputs and workspace pre-filled with garbage -> CUDA tensors"""
    from osvos_pytorch_amd import _lib
    n, h, w = x.shape
    labels = torch.full((n, h, w), -77, device="cuda", dtype=torch.int32)
    area = torch.full((n, h, w), 123456, device="cuda", dtype=torch.int32)
    stats = torch.full((n, 4), -9, device="cuda", dtype=torch.int64)
    ws = _ws(n, h, w)
    _lib.check(_lib.lib().osvos_mask_components(vp(x.data_ptr()), vp(labels.data_ptr()), vp(area.data_ptr()) if want_area else None,
                                                vp(stats.data_ptr()) if want_stats else None, vp(ws.data_ptr()), n, h, w,
                                                float(cc.logit_threshold(thr)), conn, _stream()), "mask_components")
    return labels, area, stats


def _same(name, what, got, want):
    bad = np.argwhere(got != want)
    print(name, what, "entries that differ:", len(bad), [(b.tolist(), got[tuple(b)].item(), want[tuple(b)].item()) for b in bad[:5]])
    return np.array_equal(got, want)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_labels_area_and_stats_equal_the_fixture(case, conn):
    x = torch.from_numpy(LOGITS[case["name"]]).cuda()
    labels, area, stats = _label(x, case["thr"], conn)
    ok = _same(case["name"], "labels", labels.cpu().numpy(), case["labels"][conn])
    ok &= _same(case["name"], "area", area.cpu().numpy(), case["area"][conn])
    ok &= _same(case["name"], "stats", stats.cpu().numpy(), case["stats"][conn])
    assert ok
    # area and stats are optional
    only, _, _ = _label(x, case["thr"], conn, want_area=False, want_stats=False)
    assert np.array_equal(only.cpu().numpy(), case["labels"][conn])
    _, _, st = _label(x, case["thr"], conn, want_area=False)
    assert np.array_equal(st.cpu().numpy(), case["stats"][conn])


@pytest.mark.parametrize("name", ["empty_full_30x85", "two_frames_37x53", "track"])
def test_a_batch_equals_its_single_frames_also_on_a_side_stream_and_through_the_python_layer(name):
    from osvos_pytorch_amd import results
    case, conn = BY_NAME[name], 8
    x = torch.from_numpy(LOGITS[name]).cuda()
    for n in range(case["N"]):
        labels, area, stats = _label(x[n:n + 1].contiguous(), case["thr"], conn)
        assert np.array_equal(labels.cpu().numpy()[0], case["labels"][conn][n]), (name, n)
        assert np.array_equal(area.cpu().numpy()[0], case["area"][conn][n]) and np.array_equal(stats.cpu().numpy()[0], case["stats"][conn][n])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        labels, area, stats = _label(x, case["thr"], conn)
    side.synchronize()
    assert np.array_equal(labels.cpu().numpy(), case["labels"][conn]) and np.array_equal(stats.cpu().numpy(), case["stats"][conn])
    for inp in (x, x[:, None]):                                  # also with the channel axis a network output carries
        labels, area, stats = results.components(inp, threshold=case["thr"], connectivity=conn)
        assert labels.dtype == torch.int32 and area.dtype == torch.int32 and stats.dtype == torch.int64 and labels.is_cuda
        assert tuple(labels.shape) == tuple(x.shape) and tuple(stats.shape) == (case["N"], 4)
        assert np.array_equal(labels.cpu().numpy(), case["labels"][conn]) and np.array_equal(area.cpu().numpy(), case["area"][conn])
        assert np.array_equal(stats.cpu().numpy(), case["stats"][conn])


def test_a_logits_pointer_off_the_16_byte_grid_with_an_odd_plane_size():
    case = BY_NAME["two_frames_37x53"]                           # 37 x 53 = 1961 floats per plane
    full = LOGITS[case["name"]]
    assert full[0].size % 2 == 1
    flat = torch.empty(full.size + 1, device="cuda", dtype=torch.float32)
    flat[1:].copy_(torch.from_numpy(full).reshape(-1))
    assert flat[1:].data_ptr() % 16 == 4
    for conn in (4, 8):
        labels, area, stats = _label(flat[1:].view(*full.shape), case["thr"], conn)
        assert np.array_equal(labels.cpu().numpy(), case["labels"][conn]) and np.array_equal(area.cpu().numpy(), case["area"][conn])
        assert np.array_equal(stats.cpu().numpy(), case["stats"][conn])


@pytest.mark.parametrize("name", ["serpentine_150x300", "noise_64x128", "noise_60x107_thr03"])
def test_three_consecutive_calls_give_the_same_bytes(name):
    case = BY_NAME[name]
    x = torch.from_numpy(LOGITS[name]).cuda()
    for conn in (4, 8):
        runs = [[t.cpu().numpy().tobytes() for t in _label(x, case["thr"], conn)] for _ in range(3)]
        assert runs[0] == runs[1] == runs[2], (name, conn)
        assert runs[0][0] == case["labels"][conn].tobytes()


def _select(x, case, s, n0=0, n1=None, seed=None, alias=False, conn=None):
    """labelling + one osvos_components_select call on frames n0..n1 of CUDA logits x -> (out, kept) as numpy"""
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    n1 = case["N"] if n1 is None else n1
    xs = x[n0:n1].contiguous().clone()
    n, h, w = xs.shape
    labels, area, stats = _label(xs, case["thr"], s["conn"])
    if seed is None:
        seed = torch.from_numpy(s["seed"][:1] if s["chain"] else s["seed"][n0:n1]).to(torch.uint8).cuda() * 255      # non-zero means seed
    out = xs if alias else torch.full_like(xs, 55.0)
    kept = torch.full((n, h, w), 9, device="cuda", dtype=torch.uint8)
    ws = _ws(n, h, w)
    _lib.check(l.osvos_components_select(vp(xs.data_ptr()), vp(labels.data_ptr()), vp(area.data_ptr()), vp(stats.data_ptr()), vp(seed.data_ptr()),
                                         s["chain"], s["radius"], s["min_area"], s["keep_largest"], s["fill"], vp(out.data_ptr()), vp(kept.data_ptr()),
                                         vp(ws.data_ptr()), n, h, w, float(cc.logit_threshold(case["thr"])), _stream()), "components_select")
    return out.cpu().numpy(), kept.cpu().numpy()


@pytest.mark.parametrize("setting", ["chain_r3", "chain_r0", "frames_r3", "keep_largest", "min_area5"])
def test_selection_equals_the_fixture(setting):
    case = BY_NAME["track"]
    s = case["settings"][setting]
    x = torch.from_numpy(LOGITS["track"]).cuda()
    want_out, want_kept = cc.expected_out(s, LOGITS["track"]), s["kept"].astype(np.uint8)
    for alias in (False, True):
        out, kept = _select(x, case, s, alias=alias)
        print(setting, "alias", alias, "kept pixels per frame", kept.reshape(case["N"], -1).sum(1).tolist(), "want",
              want_kept.reshape(case["N"], -1).sum(1).tolist())
        assert np.array_equal(kept, want_kept)
        assert np.array_equal(out, want_out, equal_nan=True)
    if s["chain"]:
        # two chained calls of four frames, kept[3] handed back as the seed, equal one call of eight
        out_a, kept_a = _select(x, case, s, 0, 4)
        out_b, kept_b = _select(x, case, s, 4, 8, seed=torch.from_numpy(kept_a[3:4]).cuda())
        assert np.array_equal(np.concatenate([kept_a, kept_b]), want_kept)
        assert np.array_equal(np.concatenate([out_a, out_b]), want_out, equal_nan=True)


def test_filter_components_and_dropped_pixels_are_background_in_the_merge():
    from osvos_pytorch_amd import results
    case = BY_NAME["track"]
    x = torch.from_numpy(LOGITS["track"]).cuda()
    for name, s in case["settings"].items():
        seed = torch.from_numpy(s["seed"]).cuda()                                        # a bool tensor
        for inp in (x, x[:, None]):
            out, kept = results.filter_components(inp, threshold=case["thr"], connectivity=s["conn"], min_area=s["min_area"],
                                                  keep_largest=bool(s["keep_largest"]), seed=seed, seed_radius=s["radius"], chain=bool(s["chain"]),
                                                  fill=s["fill"])
            assert out.shape == inp.shape and kept.dtype == torch.uint8 and tuple(kept.shape) == tuple(x.shape)
            assert np.array_equal(kept.cpu().numpy(), s["kept"].astype(np.uint8)), name
            assert np.array_equal(out.reshape(x.shape).cpu().numpy(), cc.expected_out(s, LOGITS["track"]), equal_nan=True), name
    # no seed, no other rule: everything is kept and the logits pass unchanged; a float seed counts non-zero pixels
    out, kept = results.filter_components(x)
    assert np.array_equal(kept.cpu().numpy(), case["mask"].astype(np.uint8)) and np.array_equal(out.cpu().numpy(), LOGITS["track"], equal_nan=True)
    s = case["settings"]["frames_r3"]
    out, kept = results.filter_components(x, seed=torch.from_numpy(s["seed"]).cuda().float() * 0.25, seed_radius=3)
    assert np.array_equal(kept.cpu().numpy(), s["kept"].astype(np.uint8))
    # fill = -inf can never win a merge: with a second object that is background everywhere, the label map is the kept map
    other = torch.full_like(x, -50.0)
    lab = results.merge_objects(torch.stack([out, other]), threshold=case["thr"])
    assert np.array_equal(lab.cpu().numpy(), s["kept"].astype(np.uint8))
    lab = results.merge_objects(torch.stack([other, out]), threshold=case["thr"])
    assert np.array_equal(lab.cpu().numpy(), 2 * s["kept"].astype(np.uint8))


def test_kept_as_a_prediction_gives_the_j_counts_of_numpy():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    case = BY_NAME["track"]
    s = case["settings"]["chain_r3"]
    x = torch.from_numpy(LOGITS["track"]).cuda()
    _, kept = _select(x, case, s)
    gt = case["settings"]["frames_r3"]["seed"]                                           # the object of every frame
    n, h, w = kept.shape
    p, g = torch.from_numpy(kept).cuda().float() * 2 - 1, torch.from_numpy(gt).cuda().float()
    ws = torch.empty(l.osvos_boundary_ws_bytes(n, h, w) // 8, device="cuda", dtype=torch.int64)
    counts = torch.empty((n, 6), device="cuda", dtype=torch.int64)
    _lib.check(l.osvos_mask_jf_counts(vp(p.data_ptr()), vp(g.data_ptr()), vp(ws.data_ptr()), vp(counts.data_ptr()), n, h, w, 0.0, 3, 0, _stream()),
               "mask_jf_counts")
    got = counts.cpu().numpy()[:, :2]
    k = s["kept"]
    want = np.stack([(k & gt).reshape(n, -1).sum(1), (k | gt).reshape(n, -1).sum(1)], axis=1)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


def test_component_tracker_enqueues_only_and_its_totals_equal_the_fixture(monkeypatch):
    from osvos_pytorch_amd import results
    case = BY_NAME["track"]
    s = case["settings"]["chain_r3"]
    x = torch.from_numpy(LOGITS["track"]).cuda()
    first = torch.from_numpy(s["seed"]).cuda()                                           # [1,H,W] bool
    want_out = cc.expected_out(s, LOGITS["track"])
    lab = case["labels"][8]
    want = {"seen": int(case["stats"][8][:, 0].sum()), "kept": sum(len(np.unique(lab[n][s["kept"][n]])) for n in range(case["N"])),
            "frames": case["N"]}
    assert 0 < want["kept"] < want["seen"]
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
    tr = results.ComponentTracker(first, s["radius"], threshold=case["thr"], connectivity=8)
    outs = [tr(x[0:3]), tr(x[3:4, None]), tr(x[4:8])]                                    # batches of consecutive frames, one with a channel axis
    assert calls == {"synchronize": 0, "cpu": 0, "item": 0, "tolist": 0}, calls
    got = tr.summary()
    assert calls["cpu"] == 1 and calls["synchronize"] == 0 and calls["item"] == 0 and calls["tolist"] == 0, calls
    assert tr.summary() == got and calls["cpu"] == 1, calls                              # (the read-back is kept)
    monkeypatch.undo()

    assert got == want, (got, want)
    assert outs[1].shape == (1, 1, case["H"], case["W"])
    out = torch.cat([outs[0], outs[1][:, 0], outs[2]]).cpu().numpy()
    assert np.array_equal(out, want_out, equal_nan=True)
    with pytest.raises(ValueError, match="first mask"):
        tr(torch.zeros(1, 40, 64, device="cuda"))
    # min_area reaches the kernel
    s5 = case["settings"]["min_area5"]
    tr5 = results.ComponentTracker(first[0], 3, min_area=5)
    assert np.array_equal(tr5(x).cpu().numpy(), cc.expected_out(s5, LOGITS["track"]), equal_nan=True)


def test_argument_errors_are_errors_not_answers():
    from osvos_pytorch_amd import _lib, results
    l = _lib.lib()
    x = torch.zeros(1, 8, 8, device="cuda")
    labels = torch.zeros(1, 8, 8, device="cuda", dtype=torch.int32)
    area = torch.zeros(1, 8, 8, device="cuda", dtype=torch.int32)
    stats = torch.zeros(1, 4, device="cuda", dtype=torch.int64)
    seed = torch.zeros(1, 8, 8, device="cuda", dtype=torch.uint8)
    kept = torch.zeros(1, 8, 8, device="cuda", dtype=torch.uint8)
    out = torch.zeros(1, 8, 8, device="cuda")
    ws = torch.zeros(256, device="cuda", dtype=torch.int64)

    def label(n=1, conn=8, ws_off=0, st_off=0):
        return l.osvos_mask_components(vp(x.data_ptr()), vp(labels.data_ptr()), vp(area.data_ptr()), vp(stats.data_ptr() + st_off), vp(ws.data_ptr() + ws_off),
                                       n, 8, 8, 0.0, conn, _stream())

    def select(radius=0, fill=-1.0, out_p=out.data_ptr(), kept_p=kept.data_ptr(), chain=0, n=1):
        return l.osvos_components_select(vp(x.data_ptr()), vp(labels.data_ptr()), vp(area.data_ptr()), vp(stats.data_ptr()), vp(seed.data_ptr()), chain,
                                         radius, 0, 0, fill, vp(out_p) if out_p else None, vp(kept_p) if kept_p else None, vp(ws.data_ptr()), n, 8, 8,
                                         0.0, _stream())
    assert label() == 0 and select() == 0 and select(fill=0.0) == 0 and select(fill=float("-inf")) == 0 and select(out_p=0) == 0
    assert label(conn=6) < 0 and b"connectivity 6" in l.osvos_last_error()
    assert label(n=0) < 0 and b"N 0" in l.osvos_last_error()
    assert label(n=65536) < 0 and b"N 65536" in l.osvos_last_error()
    assert label(ws_off=4) < 0 and b"aligned" in l.osvos_last_error()
    assert label(st_off=4) < 0 and b"aligned" in l.osvos_last_error()
    assert select(n=0) < 0 and b"N 0" in l.osvos_last_error()
    assert select(radius=65) < 0 and b"radius 65" in l.osvos_last_error()
    assert select(radius=-1) < 0 and b"radius" in l.osvos_last_error()
    assert select(fill=0.5) < 0 and b"fill" in l.osvos_last_error()
    assert select(fill=float("nan")) < 0 and b"fill" in l.osvos_last_error()
    assert select(out_p=0, kept_p=0) < 0 and b"both outputs" in l.osvos_last_error()
    assert select(chain=1, kept_p=0) < 0 and b"chain" in l.osvos_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(label(conn=6), "mask_components")
    with pytest.raises(ValueError, match="connectivity"):
        results.components(x, connectivity=6)
    with pytest.raises(ValueError):
        results.components(torch.zeros(0, 8, 8, device="cuda"))
    with pytest.raises(ValueError, match="seed_radius"):
        results.filter_components(x, seed=seed, seed_radius=65)
    with pytest.raises(ValueError, match="fill"):
        results.filter_components(x, fill=0.5)
    with pytest.raises(ValueError, match="fill"):
        results.filter_components(x, fill=float("nan"))
    with pytest.raises(ValueError, match="chain"):
        results.filter_components(x, chain=True)
    with pytest.raises(ValueError, match="seed"):
        results.filter_components(x, seed=seed[:, :4])
    with pytest.raises(ValueError, match="seed_radius"):
        results.ComponentTracker(seed, 65)
    torch.cuda.synchronize()


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi_object"])
def test_train_online_track_components(tmp_path, multi):
    r = script_runner.train_online(tmp_path, "--track-components", "8", *(["--multi-object"] if multi else []), epochs=10, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    if multi:
        assert sum(1 for ln in lines if re.fullmatch(r"J&F on blackswan object \d+: J -?\d+\.\d{4} F -?\d+\.\d{4}", ln)) == 2, r.stdout[-2000:]
        assert any(re.fullmatch(r"J&F on blackswan \(2 objects\): -?\d+\.\d{4}", ln) for ln in lines)
        got = [re.fullmatch(r"Components kept on blackswan object (\d+): (\d+) of (\d+) over (\d+) frames", ln) for ln in lines]
        got = [m for m in got if m]
        assert [m.group(1) for m in got] == ["1", "2"], r.stdout[-2000:]
    else:
        assert any(ln.startswith("J (region similarity) on blackswan: mean ") for ln in lines), r.stdout[-2000:]
        assert any(ln.startswith("F (contour accuracy) on blackswan: mean ") for ln in lines)
        assert any(re.fullmatch(r"J&F on blackswan: -?\d+\.\d{4}", ln) for ln in lines)
        got = [re.fullmatch(r"Components kept on blackswan(): (\d+) of (\d+) over (\d+) frames", ln) for ln in lines]
        got = [m for m in got if m]
        assert len(got) == 1, r.stdout[-2000:]
    for m in got:
        kept, seen, frames = int(m.group(2)), int(m.group(3)), int(m.group(4))
        assert 0 <= kept <= seen and frames == 1, m.group(0)
    jf = [i for i, ln in enumerate(lines) if ln.startswith("J&F on blackswan")]
    assert max(jf) < min(i for i, ln in enumerate(lines) if ln.startswith("Components kept on"))      # after the existing J&F lines
