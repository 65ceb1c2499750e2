"""GPU: appearance matching on the device -- osvos_match_quantize, osvos_match_cell_labels and osvos_match_nearest (csrc/match.hip) against the
numpy restatement of the rule in tests/match_cases.py, bit for bit (integer dot products and single fp32 operations: every comparison is an
equality, there is no tolerance), OSVOS.forward_features, the wrappers of osvos_pytorch_amd.match, AppearanceMatcher, the two-frame scenario,
and train_online.py --match-gain.  Outputs and workspaces are pre-filled with garbage before every call; a guard band after ws is checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import match_cases as mc
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE_BYTE = 0xa5
GARBAGE_INT = 0x5a5a5a5a
GUARD = 256


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t.contiguous()).view(np.uint32)


def _quantize(feat, fmt):
    """feat: float32 numpy [P, C] (already bf16-representable when fmt is 1) -> (q, rinv) numpy from one device call"""
    from osvos_pytorch_amd import _lib
    p, c = feat.shape
    f = _dev(feat)
    if fmt == 1:
        f = f.to(torch.bfloat16)
    q = torch.full((p, c), 0x5a, device="cuda", dtype=torch.int8)
    rinv = torch.full((p,), float("nan"), device="cuda", dtype=torch.float32)
    vp = C.c_void_p
    _lib.check(_lib.lib().osvos_match_quantize(vp(f.data_ptr()), fmt, vp(q.data_ptr()), vp(rinv.data_ptr()), p, c, _stream()), "match_quantize")
    return _np(q), _np(rinv)


@pytest.mark.parametrize("fmt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", mc.FEATURE_KINDS)
@pytest.mark.parametrize("c", mc.QUANT_C)
def test_quantize_bit_for_bit(c, kind, fmt):
    for p in mc.QUANT_P:
        f = mc.features(kind, p, c)
        if fmt == 1:
            f = mc.bf16_round(f)
        want_q, want_r = mc.quantize(f)
        q, rinv = _quantize(f, fmt)
        print("quantize %s C %d P %d: %d of %d bytes and %d of %d words differ" % (kind, c, p, int((q != want_q).sum()), q.size,
                                                                                  int((rinv.view(np.uint32) != want_r.view(np.uint32)).sum()), p))
        assert np.array_equal(q, want_q)
        assert np.array_equal(rinv.view(np.uint32), want_r.view(np.uint32))


def _cell_labels_rc(mask, h, w, stride, label=None):
    from osvos_pytorch_amd import _lib
    n, H, W = (int(v) for v in mask.shape)
    if label is None:
        label = torch.full((n, max(h, 1), max(w, 1)), 7, device="cuda", dtype=torch.uint8)
    vp = C.c_void_p
    return _lib.lib().osvos_match_cell_labels(vp(mask.data_ptr()), vp(label.data_ptr()), n, H, W, h, w, stride, _stream()), label


@pytest.mark.parametrize("c", mc.LABEL_CASES, ids=str)
def test_cell_labels_bit_for_bit(c):
    from osvos_pytorch_amd import _lib
    H, W, S = c
    m = mc.masks(H, W, 2)
    h, w = mc.grid_shape(H, W, S)
    rc, label = _cell_labels_rc(_dev(m), h, w, S)
    _lib.check(rc, "match_cell_labels")
    assert np.array_equal(_np(label), mc.cell_labels(m, S))


def _nearest_rc(p, with_idx=True, ws=None, outs=None):
    """one osvos_match_nearest call on the arrays of a match_cases.nearest_problem -> (rc, sim, idx or None, ws buffer, ws bytes)"""
    from osvos_pytorch_amd import _lib
    n, pq, c = p["Q"].shape
    nr, pr = p["label"].shape
    t = {k: _dev(p[k]) for k in ("Q", "rinv_q", "R", "rinv_r", "label")}
    if outs is None:
        sim = torch.full((n, 2, pq), float("nan"), device="cuda", dtype=torch.float32)
        idx = torch.full((n, 2, pq), GARBAGE_INT, device="cuda", dtype=torch.int32) if with_idx else None
    else:
        sim, idx = outs
    if ws is None:
        need = int(_lib.lib().osvos_match_ws_bytes(n, pq, pr, c))
        assert need >= n * 2 * pq * 8
        ws = (torch.full((need + GUARD,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8), need)
    buf, need = ws
    vp = C.c_void_p
    rc = _lib.lib().osvos_match_nearest(vp(t["Q"].data_ptr()), vp(t["rinv_q"].data_ptr()), vp(t["R"].data_ptr()), vp(t["rinv_r"].data_ptr()),
                                        vp(t["label"].data_ptr()), vp(sim.data_ptr()), vp(idx.data_ptr()) if idx is not None else None,
                                        vp(buf.data_ptr()), n, nr, pq, pr, c, _stream())
    return rc, sim, idx, buf, need


def _nearest(p, with_idx=True):
    from osvos_pytorch_amd import _lib
    rc, sim, idx, buf, need = _nearest_rc(p, with_idx)
    _lib.check(rc, "match_nearest")
    assert bool((buf[need:] == GARBAGE_BYTE).all()), "the call wrote past osvos_match_ws_bytes"
    return sim, idx


def _check_nearest(p, what):
    sim, idx = _nearest(p)
    bad_s, bad_i = int((_bits(sim) != p["sim"].view(np.uint32)).sum()), int((_np(idx) != p["idx"]).sum())
    print("nearest %s: %d of %d sim words and %d idx differ" % (what, bad_s, p["sim"].size, bad_i))
    assert np.array_equal(_bits(sim), p["sim"].view(np.uint32))
    assert np.array_equal(_np(idx), p["idx"])
    return sim, idx


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("nr", [1, 2])
@pytest.mark.parametrize("c", mc.NEAREST_CASES, ids=str)
def test_nearest_bit_for_bit(c, nr, kind):
    """one K step and many, ragged row and column tiles, one slice and several; labels all foreground, all background, mixed with void, void
    only; duplicated reference rows (index ties), queries that are reference rows, +-127 everywhere at C = 1024"""
    p = mc.nearest_problem(*c, n=2, nr=nr, kind=kind)
    if c[2] == 1024 and kind == "mixed":
        assert float(np.abs(p["Q"][0, 33].astype(np.int64) @ p["R"][0, 30].astype(np.int64))) == 127 * 127 * 1024
    _check_nearest(p, "%s NR %d %s" % (c, nr, kind))


def test_nearest_on_a_davis_sized_grid():
    """conv4_3 of an 854 x 480 frame against itself: 6420 x 6420 x 512, several reference tiles per slice"""
    p = mc.nearest_problem(*mc.DAVIS_CASE, n=1, nr=1, kind="mixed")
    _check_nearest(p, "%s" % (mc.DAVIS_CASE,))


def test_nearest_without_idx_batches_and_repeats():
    p = mc.nearest_problem(130, 257, 128, n=2, nr=2)
    sim, idx = _nearest(p)
    sim2, none = _nearest(p, with_idx=False)
    assert none is None and np.array_equal(_bits(sim), _bits(sim2))
    sim3, idx3 = _nearest(p)                                                 # a call repeats
    assert np.array_equal(_bits(sim), _bits(sim3)) and np.array_equal(_np(idx), _np(idx3))
    # frame 1 alone gives frame 1's rows of the batch
    one = {k: np.ascontiguousarray(v[1:2]) for k, v in p.items()}
    s1, i1 = _nearest(one)
    assert np.array_equal(_bits(s1)[0], _bits(sim)[1]) and np.array_equal(_np(i1)[0], _np(idx)[1])
    # and changing frame 0's queries leaves frame 1 alone
    other = dict(p)
    other["Q"] = np.ascontiguousarray(p["Q"][::-1])
    other["rinv_q"] = np.ascontiguousarray(p["rinv_q"][::-1])
    s2, _ = _nearest(other)
    want, _ = mc.nearest(other["Q"], other["rinv_q"], p["R"], p["rinv_r"], p["label"])
    assert np.array_equal(_bits(s2), want.view(np.uint32))


def test_bad_arguments_return_an_error_and_write_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    p = mc.nearest_problem(37, 33, 64, n=2, nr=1)
    vp = C.c_void_p
    for what, kw in [("Pq", dict(pq=0)), ("Pr", dict(pr=(1 << 20) + 1)), ("C", dict(c=96)), ("NR", dict(nr=3)), ("N", dict(n=0))]:
        t = {k: _dev(p[k]) for k in ("Q", "rinv_q", "R", "rinv_r", "label")}
        sim = torch.full((2, 2, 37), float("nan"), device="cuda", dtype=torch.float32)
        idx = torch.full((2, 2, 37), GARBAGE_INT, device="cuda", dtype=torch.int32)
        ws = torch.full((1 << 16,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
        a = dict(n=2, nr=1, pq=37, pr=33, c=64)
        a.update(kw)
        rc = l.osvos_match_nearest(vp(t["Q"].data_ptr()), vp(t["rinv_q"].data_ptr()), vp(t["R"].data_ptr()), vp(t["rinv_r"].data_ptr()),
                                   vp(t["label"].data_ptr()), vp(sim.data_ptr()), vp(idx.data_ptr()), vp(ws.data_ptr()), a["n"], a["nr"], a["pq"], a["pr"],
                                   a["c"], _stream())
        assert rc < 0 and what.encode() + b" " in l.osvos_last_error(), (what, l.osvos_last_error())
        torch.cuda.synchronize()
        assert bool(torch.isnan(sim).all()) and bool((idx == GARBAGE_INT).all()) and bool((ws == GARBAGE_BYTE).all())
    # aliasing: sim inside Q
    t = {k: _dev(p[k]) for k in ("Q", "rinv_q", "R", "rinv_r", "label")}
    ws = torch.full((1 << 16,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
    before = t["Q"].clone()
    rc = l.osvos_match_nearest(vp(t["Q"].data_ptr()), vp(t["rinv_q"].data_ptr()), vp(t["R"].data_ptr()), vp(t["rinv_r"].data_ptr()),
                               vp(t["label"].data_ptr()), vp(t["Q"].data_ptr() + 64), None, vp(ws.data_ptr()), 2, 1, 37, 33, 64, _stream())
    assert rc < 0 and b"aliasing" in l.osvos_last_error()
    assert torch.equal(before, t["Q"]) and bool((ws == GARBAGE_BYTE).all())
    # quantize and cell_labels
    f = torch.zeros((4, 64), device="cuda")
    q = torch.full((4, 64), 0x5a, device="cuda", dtype=torch.int8)
    rinv = torch.full((4,), float("nan"), device="cuda")
    assert l.osvos_match_quantize(vp(f.data_ptr()), 0, vp(q.data_ptr()), vp(rinv.data_ptr()), 4, 100, _stream()) < 0 and b"C 100 " in l.osvos_last_error()
    assert l.osvos_match_quantize(vp(f.data_ptr()), 3, vp(q.data_ptr()), vp(rinv.data_ptr()), 4, 64, _stream()) < 0 and b"format 3" in l.osvos_last_error()
    assert bool((q == 0x5a).all()) and bool(torch.isnan(rinv).all())
    m = torch.ones((1, 45, 70), device="cuda", dtype=torch.uint8)
    rc, label = _cell_labels_rc(m, 5, 8, 8)
    assert rc < 0 and b"grid h 5 w 8" in l.osvos_last_error() and bool((label == 7).all())
    rc, label = _cell_labels_rc(m, 6, 9, 6)
    assert rc < 0 and b"stride 6 " in l.osvos_last_error() and bool((label == 7).all())


# ------------------------------------------------------------------------------------------------------------------ the network side


def _net(precision, n=2, h=48, w=64, seed=5):
    import networks.vgg_osvos as vo
    from oracle import synth
    wts, x, _ = synth.calibrated_problem(n, h, w, seed=seed)
    net = vo.OSVOS(pretrained=0)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in wts.items()})
    net = net.cuda()
    net.set_precision(precision)
    return net, torch.from_numpy(x).cuda()


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_forward_features(precision):
    from osvos_pytorch_amd import _lib
    net, x = _net(precision)
    n, h, w = 2, 48, 64
    with torch.no_grad():
        plain = net.forward(x)
    graph = net.forward(x.clone().requires_grad_())
    ws = graph[0].grad_fn.saved_tensors[0]
    lib, dt = _lib.lib(), net._runtime.dtype
    for layer, channels, stride in ((3, 128, 2), (6, 256, 4), (9, 512, 8), (12, 512, 16)):
        outs, feat, fmt = net.forward_features(x, layer)
        assert len(outs) == 5 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(outs, plain))
        assert tuple(feat.shape) == (n, h // stride, w // stride, channels) and fmt == lib.osvos_net_ws_format(dt, layer)
        assert feat.dtype == (torch.bfloat16 if fmt == 1 else torch.float32)
        off, el, ch, hh, ww = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(lib.osvos_net_ws_query(n, h, w, dt, layer, C.byref(off), C.byref(el), C.byref(ch), C.byref(hh), C.byref(ww)))
        size = 2 if fmt == 1 else 4
        want = ws[off.value:off.value + size * el.value].view(feat.dtype).view(n, hh.value, ww.value, ch.value)
        assert torch.equal(feat.view(torch.int16 if fmt == 1 else torch.int32), want.view(torch.int16 if fmt == 1 else torch.int32))
        assert float(feat.float().abs().max()) > 0
    for bad in (5, 0, 13, True, 9.0):
        with pytest.raises(ValueError):
            net.forward_features(x, bad)


def test_wrappers_match_the_direct_calls():
    from osvos_pytorch_amd import match
    f = mc.features("relu", 63, 192)
    q, rinv = match.quantize(_dev(f).view(7, 9, 192))
    want_q, want_r = mc.quantize(f)
    assert tuple(q.shape) == (7, 9, 192) and tuple(rinv.shape) == (7, 9)
    assert np.array_equal(_np(q).reshape(63, 192), want_q) and np.array_equal(_bits(rinv).reshape(63), want_r.view(np.uint32))
    qb, rb = match.quantize(_dev(mc.bf16_round(f)).to(torch.bfloat16))
    want_q, want_r = mc.quantize(mc.bf16_round(f))
    assert np.array_equal(_np(qb), want_q) and np.array_equal(_bits(rb), want_r.view(np.uint32))
    m = mc.masks(45, 70, 2)
    assert np.array_equal(_np(match.cell_labels(_dev(m), 8)), mc.cell_labels(m, 8))
    assert np.array_equal(_np(match.cell_labels(_dev(m != 0)[:, None], 8)), mc.cell_labels(m, 8))      # bool [N,1,H,W]
    assert np.array_equal(_np(match.cell_labels(_dev(m[0]), 4)), mc.cell_labels(m[:1], 4))            # [H,W]
    p = mc.nearest_problem(129, 1000, 512, n=2, nr=1)
    t = [_dev(p[k]) for k in ("Q", "rinv_q", "R", "rinv_r", "label")]
    sim, idx = match.nearest(*t, with_idx=True)
    assert np.array_equal(_bits(sim), p["sim"].view(np.uint32)) and np.array_equal(_np(idx), p["idx"])
    ws = match.nearest_workspace(2, 129, 1000, 512, sim.device)
    assert np.array_equal(_bits(match.nearest(*t, ws=ws)), p["sim"].view(np.uint32))
    with pytest.raises(ValueError):
        match.quantize(_dev(f[:, :100]))
    with pytest.raises(ValueError):
        match.quantize(_dev(f).double())
    with pytest.raises(ValueError):
        match.cell_labels(_dev(m).float(), 8)
    with pytest.raises(ValueError):
        match.cell_labels(_dev(m), 6)
    with pytest.raises(ValueError):
        match.nearest(t[0], t[1], t[2], t[3], t[4][:, :999])
    with pytest.raises(ValueError):
        match.nearest(t[0].to(torch.uint8), t[1], t[2], t[3], t[4])
    with pytest.raises(ValueError):
        match.nearest(t[0], t[1], torch.cat([t[2]] * 3), torch.cat([t[3]] * 3), torch.cat([t[4]] * 3))      # NR = 3 for N = 2


def _restated_map(net, layer, x0, mask0, x, prev=None):
    """the restatement's map [N,h,w] for frames x against the first frame (x0, mask0 numpy [1,H,W]); prev = (x_prev, mask_prev numpy [N,H,W]):
    also against that bank, per-class maximum"""
    stride = {3: 2, 6: 4, 9: 8, 12: 16}[layer]

    def banks(xx):
        feat = net.forward_features(xx, layer)[1]
        n, h, w, c = feat.shape
        qs, rs = zip(*(mc.quantize(_np(feat[b].float()).reshape(h * w, c)) for b in range(n)))
        return np.stack(qs), np.stack(rs), (h, w)
    R, rinv_r, _ = banks(x0)
    Q, rinv_q, (h, w) = banks(x)
    sim, _ = mc.nearest(Q, rinv_q, R, rinv_r, mc.cell_labels(mask0, stride).reshape(1, -1))
    if prev is not None:
        P, rinv_p, _ = banks(prev[0])
        sim2, _ = mc.nearest(Q, rinv_q, P, rinv_p, mc.cell_labels(prev[1], stride).reshape(len(P), -1))
        sim = np.maximum(sim, sim2)
    return mc.match_map(sim).reshape(-1, h, w)


def _half_mask(n=1, h=48, w=64):
    m = np.zeros((n, h, w), np.uint8)
    m[:, :, :w // 2 + 3] = 255                                              # whole object cells, one void column of cells, background cells
    return m


@pytest.mark.parametrize("precision,layer", [("fp32x3", 9), ("bf16", 6)])
def test_appearance_matcher(precision, layer, capfd):
    from osvos_pytorch_amd import match, tta
    net, x = _net(precision, n=3)
    x0, x1 = x[:1], x[1:]
    mask0 = _half_mask()
    with torch.no_grad():
        plain = net.forward(x1)
    # gain 0: the forward's bits, whether or not a reference was set
    off = match.AppearanceMatcher(net, layer, 0.0)
    assert off.has_reference
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(off(x1), plain))
    # gain > 0: fused + gain * map as tta.fuse_views computes it from the restatement's map; the side heads untouched
    m = match.AppearanceMatcher(net, layer, 2.5)
    with pytest.raises(RuntimeError):
        m(x1)
    assert m.set_reference(x0, _dev(mask0)) is m and not m.inert and m.has_reference
    got = m(x1)
    mp = _restated_map(net, layer, x0, mask0, x1)
    assert np.abs(mp).max() > 0
    want = tta.fuse_views([plain[-1], _dev(mp)], [False, False], (48, 64), weights=[1.0, 2.5])
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[:4], plain[:4]))
    assert np.array_equal(_bits(got[-1]), _bits(want)) and not np.array_equal(_bits(got[-1]), _bits(plain[-1]))
    assert np.array_equal(_bits(m(x1)[-1]), _bits(want))                     # repeats
    # a reference without foreground: inert, says so once, returns the forward's bits
    capfd.readouterr()
    inert = match.AppearanceMatcher(net, layer, 2.5).set_reference(x0, _dev(np.zeros((1, 48, 64), np.uint8)))
    assert inert.inert and "no matching" in capfd.readouterr().err
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(inert(x1), plain))
    assert capfd.readouterr().err == ""


def test_appearance_matcher_with_the_previous_frame():
    from osvos_pytorch_amd import match, tta
    net, x = _net("fp32x3", n=3)
    x0, xa, xb = x[:1], x[1:2], x[2:3]
    mask0 = _half_mask()
    prev_mask = np.zeros((1, 48, 64), np.uint8)
    prev_mask[:, 8:40, 16:48] = 1
    m = match.AppearanceMatcher(net, 9, 1.5, previous=True).set_reference(x0, _dev(mask0))
    with torch.no_grad():
        plain_a, plain_b = net.forward(xa)[-1], net.forward(xb)[-1]
    first = m(xa, None)                                                      # nothing to look back at: the first-frame bank alone
    want_a = tta.fuse_views([plain_a, _dev(_restated_map(net, 9, x0, mask0, xa))], [False, False], (48, 64), weights=[1.0, 1.5])
    assert np.array_equal(_bits(first[-1]), _bits(want_a))
    second = m(xb, _dev(prev_mask)[:, None] != 0)
    mp = _restated_map(net, 9, x0, mask0, xb, prev=(xa, prev_mask))
    alone = _restated_map(net, 9, x0, mask0, xb)
    assert not np.array_equal(mp, alone)                                     # the second bank changes the map
    want_b = tta.fuse_views([plain_b, _dev(mp)], [False, False], (48, 64), weights=[1.0, 1.5])
    assert np.array_equal(_bits(second[-1]), _bits(want_b))


def test_scenario_on_the_device():
    """tests/test_match_cpu.py pins the scenario on the restatement (IoU 0.5 -> 1.0); here the product computes the banks, the search and the
    map and gives the restatement's bytes, hence -- through tta.fuse_views -- its IoUs"""
    from osvos_pytorch_amd import match, tta
    s, sc = mc.scenario(), mc.SCENE
    h, w, c = s["h"], s["w"], sc["C"]
    r, rinv_r = match.quantize(_dev(s["f0"]).view(1, h * w, c))
    q, rinv_q = match.quantize(_dev(s["f1"]).view(1, h * w, c))
    label = match.cell_labels(_dev(s["mask0"]), sc["stride"]).view(1, h * w)
    assert np.array_equal(_np(r)[0], s["R"]) and np.array_equal(_np(q)[0], s["Q"]) and np.array_equal(_np(label), s["label"])
    assert np.array_equal(_bits(rinv_r)[0], s["rinv_r"].view(np.uint32)) and np.array_equal(_bits(rinv_q)[0], s["rinv_q"].view(np.uint32))
    sim, idx = match.nearest(q, rinv_q, r, rinv_r, label, with_idx=True)
    assert np.array_equal(_bits(sim), s["sim"].view(np.uint32)) and np.array_equal(_np(idx), s["idx"])
    mp = (sim[:, 0] - sim[:, 1]).view(1, h, w)
    assert np.array_equal(_bits(mp), s["map"].view(np.uint32))
    logits = _dev(s["logits1"])[None, None]
    fused = tta.fuse_views([logits, mp], [False, False], (sc["H"], sc["W"]), weights=[1.0, sc["gain"]])
    plain, matched = mc.iou(_np(logits)[0, 0] > 0, s["truth1"]), mc.iou(_np(fused)[0, 0] > 0, s["truth1"])
    print("matching scenario on the device: IoU %.4f -> %.4f" % (plain, matched))
    assert plain == mc.SCENE_IOU_PLAIN <= 0.90 and matched == mc.SCENE_IOU_MATCHED >= 0.99
    assert np.array_equal(_np(fused)[0, 0] > 0, s["fused"][0] > 0)


# ------------------------------------------------------------------------------------------------------------------ the script


def _run_script(tmp, *args):
    return script_runner.train_online(tmp, *args).stdout


def _train_online(tmp, *extra):
    r = script_runner.train_online(tmp, "--device-augment", "--synthetic-frames", "3", *extra, frames=3)
    return r.stdout, r.masks


def test_train_online_with_matching(tmp_path):
    """the option on (with the previous-frame bank); and --match-gain 0 against the command without the option, byte for byte.  (The two
    compared commands run without --track-components for the reason tests/test_gpu_flow.py gives.)"""
    out, _ = _train_online(tmp_path / "on", "--match-gain", "2", "--match-previous")
    assert "Online training time" in out and "J&F on blackswan:" in out, out[-2000:]
    _, off = _train_online(tmp_path / "off", "--match-gain", "0")
    _, plain = _train_online(tmp_path / "plain")
    assert off == plain


def test_train_online_matching_under_online_adaptation(tmp_path):
    """--adapt-steps sees the matched output: both of the adapter's forwards go through the matcher"""
    out, _ = _train_online(tmp_path / "on", "--match-gain", "2", "--adapt-steps", "2", "--adapt-mix", "2")
    assert "Online adaptation on blackswan: 2 frames seen" in out and "J&F on blackswan:" in out, out[-2000:]


def test_train_online_multi_object_with_matching(tmp_path):
    """one matcher per object's network"""
    out = _run_script(tmp_path / "on", "--multi-object", "--match-gain", "2", "--match-layer", "6")
    assert "J&F on blackswan (2 objects):" in out and "J&F on blackswan object 2:" in out, out[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path / "on"), "Results", "blackswan", "00000.png"))
