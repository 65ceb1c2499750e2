"""GPU: top-K averaging and the local window of appearance matching -- osvos_match_topk and osvos_match_local (csrc/match_ext.hip) against the
numpy restatement in tests/match_ext_cases.py, bit for bit (integer dot products and single fp32 operations: every comparison is an equality),
against the unchanged osvos_match_nearest on the device where the rules coincide, the wrappers of osvos_pytorch_amd.match, AppearanceMatcher
with topk and the local view, the two scenarios, and train_online.py --match-topk / --match-local.  Outputs and workspaces are pre-filled
with garbage before every call; a guard band after ws is checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import match_cases as mc
import match_ext_cases as me
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE_BYTE = 0xa5
GARBAGE_INT = 0x5a5a5a5a
GUARD = 256
OPERANDS = ("Q", "rinv_q", "R", "rinv_r", "label")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t.contiguous()).view(np.uint32)


def _ptrs(t):
    return [C.c_void_p(t[k].data_ptr()) for k in OPERANDS]


def _topk_rc(p, k, ws=None, fill=GARBAGE_BYTE):
    """one osvos_match_topk call on the arrays of a nearest_problem -> (rc, sim, ws buffer, ws bytes)"""
    from osvos_pytorch_amd import _lib
    n, pq, c = p["Q"].shape
    nr, pr = p["label"].shape
    t = {key: _dev(p[key]) for key in OPERANDS}
    sim = torch.full((n, 2, pq), float("nan"), device="cuda", dtype=torch.float32)
    need = int(_lib.lib().osvos_match_topk_ws_bytes(n, pq, pr, c, k))
    assert need >= n * 2 * pq * 4 * k
    if ws is None:
        ws = torch.full((need + GUARD,), fill, device="cuda", dtype=torch.uint8)
    assert ws.numel() >= need + GUARD
    rc = _lib.lib().osvos_match_topk(*_ptrs(t), C.c_void_p(sim.data_ptr()), C.c_void_p(ws.data_ptr()), n, nr, pq, pr, c, k, _stream())
    return rc, sim, ws, need


def _topk(p, k, ws=None, fill=GARBAGE_BYTE):
    from osvos_pytorch_amd import _lib
    rc, sim, buf, need = _topk_rc(p, k, ws, fill)
    _lib.check(rc, "match_topk")
    if ws is None:
        assert bool((buf[need:] == fill).all()), "the call wrote past osvos_match_topk_ws_bytes"
    return sim


def _nearest(p):
    """the unchanged osvos_match_nearest on the device -> (sim, idx)"""
    from osvos_pytorch_amd import match
    return match.nearest(*(_dev(p[key]) for key in OPERANDS), with_idx=True)


def _local(p, h, w, radius, with_idx=True):
    from osvos_pytorch_amd import _lib
    n, pq, c = p["Q"].shape
    nr = p["label"].shape[0]
    t = {key: _dev(p[key]) for key in OPERANDS}
    sim = torch.full((n, 2, pq), float("nan"), device="cuda", dtype=torch.float32)
    idx = torch.full((n, 2, pq), GARBAGE_INT, device="cuda", dtype=torch.int32) if with_idx else None
    rc = _lib.lib().osvos_match_local(*_ptrs(t), C.c_void_p(sim.data_ptr()), C.c_void_p(idx.data_ptr()) if with_idx else None, n, nr, h, w, c, radius,
                                      _stream())
    _lib.check(rc, "match_local")
    return sim, idx


# ------------------------------------------------------------------------------------------------------------------ top-K


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("nr", [1, 2])
@pytest.mark.parametrize("c", me.TOPK_CASES, ids=str)
def test_topk_bit_for_bit(c, nr, kind):
    """every list length (K = 1, 3, 4 in four slots, 8, 16), a class with fewer rows than K, ragged query and reference tiles, one slice and
    several, every label kind, duplicated rows, +-127 everywhere at C = 1024"""
    from osvos_pytorch_amd import _lib
    pq, pr, ch, k = c
    p = me.topk_problem(*c, n=2, nr=nr, kind=kind)
    if c == (37, 33, 64, 4) and kind == "mixed" and nr == 2:
        assert 0 < int((p["label"][0] == 1).sum()) < k                       # fewer foreground rows than K: the mean of all of them
    if c == (129, 1000, 512, 8):
        assert int(_lib.lib().osvos_match_topk_ws_bytes(2, pq, pr, ch, k)) // (2 * 2 * pq * 4 * k) > 1      # several slices
    sim = _topk(p, k)
    bad = int((_bits(sim) != p["topk"].view(np.uint32)).sum())
    print("topk %s NR %d %s: %d of %d sim words differ" % (c, nr, kind, bad, p["topk"].size))
    assert np.array_equal(_bits(sim), p["topk"].view(np.uint32))


def test_topk_with_fewer_rows_than_k_in_a_class():
    p = me.topk_problem(37, 33, 64, 16, n=2, nr=1, kind="mixed")
    n_fg, n_bg = int((p["label"][0] == 1).sum()), int((p["label"][0] == 0).sum())
    assert 0 < n_fg < 16 and 0 < n_bg                                        # the mean of ALL rows of the class
    assert np.array_equal(_bits(_topk(p, 16)), p["topk"].view(np.uint32))


def test_topk_on_a_davis_sized_grid():
    """conv4_3 of an 854 x 480 frame against itself: 6420 x 6420 x 512, several reference tiles per slice, K = 4"""
    p = me.topk_problem(*me.TOPK_DAVIS_CASE, n=1, nr=1, kind="mixed")
    sim = _topk(p, me.TOPK_DAVIS_CASE[3])
    print("topk %s: %d of %d sim words differ" % (me.TOPK_DAVIS_CASE, int((_bits(sim) != p["topk"].view(np.uint32)).sum()), p["topk"].size))
    assert np.array_equal(_bits(sim), p["topk"].view(np.uint32))


@pytest.mark.parametrize("c", mc.NEAREST_CASES, ids=str)
def test_topk_of_one_is_the_device_nearest(c):
    p = mc.nearest_problem(*c, n=2, nr=2, kind="mixed")
    sim, _ = _nearest(p)
    assert np.array_equal(_bits(_topk(p, 1)), _bits(sim)) and np.array_equal(_bits(sim), p["sim"].view(np.uint32))


def test_topk_repeats_on_a_reused_workspace_full_of_ones():
    """nothing in ws is read before it is written: a workspace of 0xff bytes (NaNs), then the same buffer again with what the first call and a
    call of another shape and K left in it"""
    big, small = me.topk_problem(129, 1000, 512, 8, n=2, nr=1), me.topk_problem(130, 257, 128, 3, n=2, nr=2)
    from osvos_pytorch_amd import _lib
    need = int(_lib.lib().osvos_match_topk_ws_bytes(2, 129, 1000, 512, 8))
    ws = torch.full((need + GUARD,), 0xff, device="cuda", dtype=torch.uint8)
    for p, k in ((big, 8), (big, 8), (small, 3), (big, 8), (small, 3)):
        assert np.array_equal(_bits(_topk(p, k, ws=ws)), p["topk"].view(np.uint32))
    assert bool((ws[need:] == 0xff).all())


# ------------------------------------------------------------------------------------------------------------------ the local window


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("nr", [1, 2])
@pytest.mark.parametrize("c", me.LOCAL_CASES, ids=str)
def test_local_bit_for_bit(c, nr, kind):
    """one cell, grids that are no multiple of the 4 x 8 tile, one tile and many, windows cut by every border, a window that covers the grid,
    1 to 8 pieces per lane, every label kind, duplicated rows (index ties)"""
    h, w, ch, radius = c
    p = me.local_problem(*c, n=2, nr=nr, kind=kind)
    sim, idx = _local(p, h, w, radius)
    bad_s, bad_i = int((_bits(sim) != p["lsim"].view(np.uint32)).sum()), int((_np(idx) != p["lidx"]).sum())
    print("local %s NR %d %s: %d of %d sim words and %d idx differ" % (c, nr, kind, bad_s, p["lsim"].size, bad_i))
    assert np.array_equal(_bits(sim), p["lsim"].view(np.uint32))
    assert np.array_equal(_np(idx), p["lidx"])
    if radius >= max(h, w) - 1:                                              # the window covers the grid: the device's nearest
        nsim, nidx = _nearest(p)
        assert np.array_equal(_bits(sim), _bits(nsim)) and np.array_equal(_np(idx), _np(nidx))


def test_local_on_a_davis_sized_grid():
    h, w, ch, radius = me.LOCAL_DAVIS_CASE
    p = me.local_problem(*me.LOCAL_DAVIS_CASE, n=1, nr=1, kind="mixed")
    sim, idx = _local(p, h, w, radius)
    print("local %s: %d sim words and %d idx differ" % (me.LOCAL_DAVIS_CASE, int((_bits(sim) != p["lsim"].view(np.uint32)).sum()),
                                                          int((_np(idx) != p["lidx"]).sum())))
    assert np.array_equal(_bits(sim), p["lsim"].view(np.uint32)) and np.array_equal(_np(idx), p["lidx"])


def test_local_without_idx_and_repeats():
    h, w, ch, radius = 33, 41, 64, 3
    p = me.local_problem(h, w, ch, radius, n=2, nr=2)
    sim, none = _local(p, h, w, radius, with_idx=False)
    assert none is None and np.array_equal(_bits(sim), p["lsim"].view(np.uint32))
    sim2, idx2 = _local(p, h, w, radius)
    assert np.array_equal(_bits(sim2), _bits(sim)) and np.array_equal(_np(idx2), p["lidx"])


# ------------------------------------------------------------------------------------------------------------------ arguments and wrappers


def test_bad_arguments_return_an_error_and_write_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    p = mc.nearest_problem(35, 35, 64, n=2, nr=1)
    vp = C.c_void_p

    def buffers():
        t = {k: _dev(p[k]) for k in OPERANDS}
        sim = torch.full((2, 2, 35), float("nan"), device="cuda", dtype=torch.float32)
        idx = torch.full((2, 2, 35), GARBAGE_INT, device="cuda", dtype=torch.int32)
        ws = torch.full((1 << 16,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
        return t, sim, idx, ws

    def untouched(sim, idx, ws):
        torch.cuda.synchronize()
        return bool(torch.isnan(sim).all()) and bool((idx == GARBAGE_INT).all()) and bool((ws == GARBAGE_BYTE).all())

    for what, kw in [("K", dict(k=0)), ("K", dict(k=17)), ("Pq", dict(pq=0)), ("Pr", dict(pr=(1 << 20) + 1)), ("C", dict(c=96)), ("NR", dict(nr=3)),
                     ("N", dict(n=0))]:
        t, sim, idx, ws = buffers()
        a = dict(n=2, nr=1, pq=35, pr=35, c=64, k=4)
        a.update(kw)
        rc = l.osvos_match_topk(*_ptrs(t), vp(sim.data_ptr()), vp(ws.data_ptr()), a["n"], a["nr"], a["pq"], a["pr"], a["c"], a["k"], _stream())
        assert rc < 0 and what.encode() + b" " in l.osvos_last_error(), (what, l.osvos_last_error())
        assert untouched(sim, idx, ws)
    for what, kw in [("radius", dict(radius=16)), ("radius", dict(radius=-1)), ("grid h", dict(h=0)), ("C", dict(c=96)), ("NR", dict(nr=3)), ("N", dict(n=0))]:
        t, sim, idx, ws = buffers()
        a = dict(n=2, nr=1, h=5, w=7, c=64, radius=2)
        a.update(kw)
        rc = l.osvos_match_local(*_ptrs(t), vp(sim.data_ptr()), vp(idx.data_ptr()), a["n"], a["nr"], a["h"], a["w"], a["c"], a["radius"], _stream())
        assert rc < 0 and what.encode() + b" " in l.osvos_last_error(), (what, l.osvos_last_error())
        assert untouched(sim, idx, ws)
    # aliasing: sim inside Q
    t, sim, idx, ws = buffers()
    before = t["Q"].clone()
    rc = l.osvos_match_topk(*_ptrs(t), vp(t["Q"].data_ptr() + 64), vp(ws.data_ptr()), 2, 1, 35, 35, 64, 4, _stream())
    assert rc < 0 and b"aliasing" in l.osvos_last_error()
    rc = l.osvos_match_local(*_ptrs(t), vp(t["Q"].data_ptr() + 64), None, 2, 1, 5, 7, 64, 2, _stream())
    assert rc < 0 and b"aliasing" in l.osvos_last_error()
    torch.cuda.synchronize()
    assert torch.equal(before, t["Q"]) and bool((ws == GARBAGE_BYTE).all())


def test_wrappers_match_the_direct_calls():
    from osvos_pytorch_amd import match
    p = me.topk_problem(129, 1000, 512, 8, n=2, nr=1)
    t = [_dev(p[k]) for k in OPERANDS]
    assert np.array_equal(_bits(match.topk(*t, 8)), p["topk"].view(np.uint32))
    ws = match.topk_workspace(2, 129, 1000, 512, 8, t[0].device)
    assert ws.numel() == match.lib().osvos_match_topk_ws_bytes(2, 129, 1000, 512, 8)
    assert np.array_equal(_bits(match.topk(*t, 8, ws=ws)), p["topk"].view(np.uint32))
    assert np.array_equal(_bits(match.topk(*t, 1)), p["sim"].view(np.uint32))
    q = me.local_problem(12, 67, 512, 4, n=2, nr=2)
    t = [_dev(q[k]) for k in OPERANDS]
    sim, idx = match.local(*t, grid=(12, 67), radius=4, with_idx=True)
    assert np.array_equal(_bits(sim), q["lsim"].view(np.uint32)) and np.array_equal(_np(idx), q["lidx"])
    assert np.array_equal(_bits(match.local(*t, grid=(12, 67), radius=4)), q["lsim"].view(np.uint32))
    assert np.array_equal(_bits(match.local_map(sim)), me.local_map(q["lsim"]).view(np.uint32))
    with pytest.raises(ValueError):
        match.local(*t, grid=(12, 66), radius=4)                             # not the operands' rows
    with pytest.raises(ValueError):
        match.local(*t, grid=(12, 67), radius=16)
    with pytest.raises(ValueError):
        match.topk(*t, 17)
    with pytest.raises(ValueError):
        match.topk(t[0], t[1], t[2], t[3], t[4][:, :800], 4)


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


def _banks(net, layer, xx):
    feat = net.forward_features(xx, layer)[1]
    n, h, w, c = feat.shape
    qs, rs = zip(*(mc.quantize(_np(feat[b].float()).reshape(h * w, c)) for b in range(n)))
    return np.stack(qs), np.stack(rs), (int(h), int(w))


def _masks():
    mask0 = np.zeros((1, 48, 64), np.uint8)
    mask0[:, :, :64 // 2 + 3] = 255                                         # whole object cells, one void column of cells, background cells
    prev_mask = np.zeros((1, 48, 64), np.uint8)
    prev_mask[:, 8:24, 8:24] = 1                                            # 2 x 2 cells of layer 9: far corners see none of them within 3 cells
    return mask0, prev_mask


def test_appearance_matcher_with_topk_and_the_local_view():
    """the matcher's output equals tta.fuse_views of a map restated from its own features: top-K over the first-frame bank (and, with
    previous=True, over the previous frame's), plus the local view as a third view once there is a previous frame"""
    from osvos_pytorch_amd import match, tta
    net, x = _net("fp32x3", n=3)
    x0, xa, xb = x[:1], x[1:2], x[2:3]
    mask0, prev_mask = _masks()
    K, RADIUS, GAIN, LOCAL_GAIN = 4, 3, 1.5, 2.0
    with torch.no_grad():
        plain_a, plain_b = net.forward(xa)[-1], net.forward(xb)[-1]
    R, rinv_r, _ = _banks(net, 9, x0)
    label0 = mc.cell_labels(mask0, 8).reshape(1, -1)
    assert min(int((label0 == 1).sum()), int((label0 == 0).sum())) > K
    Qa, rinv_qa, (h, w) = _banks(net, 9, xa)
    Qb, rinv_qb, _ = _banks(net, 9, xb)
    plabel = mc.cell_labels(prev_mask, 8).reshape(1, -1)
    map_a = mc.match_map(me.topk(Qa, rinv_qa, R, rinv_r, label0, K)).reshape(1, h, w)
    sim_b = me.topk(Qb, rinv_qb, R, rinv_r, label0, K)
    lsim, _ = me.local(Qb, rinv_qb, Qa, rinv_qa, plabel, h, w, RADIUS)
    lmap = me.local_map(lsim).reshape(1, h, w)
    assert (lsim == -2).any() and (lsim > -2).any()                          # some windows hold no object cell
    want_a = tta.fuse_views([plain_a, _dev(map_a)], [False, False], (48, 64), weights=[1.0, GAIN])
    for previous in (False, True):
        m = match.AppearanceMatcher(net, 9, GAIN, previous=previous, topk=K, local_radius=RADIUS, local_gain=LOCAL_GAIN).set_reference(x0, _dev(mask0))
        assert m.needs_previous
        first = m(xa, None)                                                  # the first matched frame: no local view
        assert np.array_equal(_bits(first[-1]), _bits(want_a))
        second = m(xb, _dev(prev_mask)[:, None] != 0)
        sim = np.maximum(sim_b, me.topk(Qb, rinv_qb, Qa, rinv_qa, plabel, K)) if previous else sim_b
        map_b = mc.match_map(sim).reshape(1, h, w)
        want_b = tta.fuse_views([plain_b, _dev(map_b), _dev(lmap)], [False] * 3, (48, 64), weights=[1.0, GAIN, LOCAL_GAIN])
        assert np.array_equal(_bits(second[-1]), _bits(want_b))
        without = tta.fuse_views([plain_b, _dev(map_b)], [False, False], (48, 64), weights=[1.0, GAIN])
        assert not np.array_equal(_bits(second[-1]), _bits(without))         # the third view changes the output
        third = m(xb, None)                                                  # no previous mask: no local view, the first-frame bank alone
        want_c = tta.fuse_views([plain_b, _dev(mc.match_map(sim_b).reshape(1, h, w))], [False, False], (48, 64), weights=[1.0, GAIN])
        assert np.array_equal(_bits(third[-1]), _bits(want_c))


def test_the_default_options_are_the_matcher_as_it_was():
    from osvos_pytorch_amd import match
    net, x = _net("fp32x3", n=3)
    x0, xa, xb = x[:1], x[1:2], x[2:3]
    mask0, prev_mask = _masks()
    pm = _dev(prev_mask)[:, None] != 0
    for previous in (False, True):
        a = match.AppearanceMatcher(net, 9, 2.5, previous).set_reference(x0, _dev(mask0))
        b = match.AppearanceMatcher(net, 9, 2.5, previous, topk=1, local_radius=0, local_gain=0.0).set_reference(x0, _dev(mask0))
        assert b.needs_previous == previous
        for xx, prev in ((xa, None), (xb, pm)):
            assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a(xx, prev), b(xx, prev)))
        assert (b._last is not None) == previous


def test_the_scenarios_on_the_device():
    """tests/test_match_ext_cpu.py pins both scenarios on the restatement; here the product computes the banks, the searches and the maps and
    gives the restatement's bytes, hence -- through tta.fuse_views -- its IoUs"""
    from osvos_pytorch_amd import match, tta

    def operands(s, c, stride):
        h, w = s["h"], s["w"]
        r, rinv_r = match.quantize(_dev(s["f0"]).view(1, h * w, c))
        q, rinv_q = match.quantize(_dev(s["f1"]).view(1, h * w, c))
        label = match.cell_labels(_dev(s["mask0"]), stride).view(1, h * w)
        assert np.array_equal(_np(r)[0], s["R"]) and np.array_equal(_np(q)[0], s["Q"]) and np.array_equal(_np(label), s["label"])
        return q, rinv_q, r, rinv_r, label

    def iou_of(views, weights, s, size):
        fused = tta.fuse_views(views, [False] * len(views), size, weights=weights)
        return mc.iou(_np(fused)[0, 0] > 0, s["truth1"])

    s, sc = me.bleed_scenario(), me.BLEED
    ops = operands(s, sc["C"], sc["stride"])
    logits = _dev(s["logits1"])[None, None]
    ious = {}
    for k in (1, sc["K"]):
        sim = match.topk(*ops, k)
        assert np.array_equal(_bits(sim), s["sim%d" % k].view(np.uint32))
        ious[k] = iou_of([logits, (sim[:, 0] - sim[:, 1]).view(1, s["h"], s["w"])], [1.0, sc["gain"]], s, (sc["H"], sc["W"]))
    plain = mc.iou(_np(logits)[0, 0] > 0, s["truth1"])
    print("bleed scenario on the device: IoU %.4f plain, %.4f at K = 1, %.4f at K = %d" % (plain, ious[1], ious[sc["K"]], sc["K"]))
    assert (plain, ious[1], ious[sc["K"]]) == (me.BLEED_IOU_PLAIN, me.BLEED_IOU_K1, me.BLEED_IOU_K4)

    s, sc = me.twin_scenario(), me.TWIN
    ops = operands(s, sc["C"], sc["stride"])
    logits = _dev(s["logits1"])[None, None]
    sim = match.nearest(*ops)
    lsim, lidx = match.local(*ops, grid=(s["h"], s["w"]), radius=sc["radius"], with_idx=True)
    assert np.array_equal(_bits(sim), s["sim"].view(np.uint32))
    assert np.array_equal(_bits(lsim), s["lsim"].view(np.uint32)) and np.array_equal(_np(lidx), s["lidx"])
    mp, lmp = (sim[:, 0] - sim[:, 1]).view(1, s["h"], s["w"]), match.local_map(lsim).view(1, s["h"], s["w"])
    assert np.array_equal(_bits(lmp), s["lmap"].view(np.uint32))
    plain = mc.iou(_np(logits)[0, 0] > 0, s["truth1"])
    first = iou_of([logits, mp], [1.0, sc["gain"]], s, (sc["H"], sc["W"]))
    both = iou_of([logits, mp, lmp], [1.0, sc["gain"], sc["local_gain"]], s, (sc["H"], sc["W"]))
    print("twin scenario on the device: IoU %.4f plain, %.4f first-frame matching, %.4f with the local view" % (plain, first, both))
    assert (plain, first) == (me.TWIN_IOU_PLAIN, me.TWIN_IOU_FIRST) and both >= me.TWIN_IOU_LOCAL_AT_LEAST and both == s["iou_local"]


# ------------------------------------------------------------------------------------------------------------------ the script


def test_train_online_multi_object_with_topk_and_the_local_view(tmp_path):
    out = script_runner.train_online(tmp_path / "on", "--multi-object", "--match-gain", "2", "--match-topk", "4", "--match-local", "3,2").stdout
    assert "J&F on blackswan (2 objects):" in out and "J&F on blackswan object 2:" in out, out[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path / "on"), "Results", "blackswan", "00000.png"))


def test_train_online_topk_of_one_changes_no_byte(tmp_path):
    """--match-topk 1 builds the matcher of --match-gain alone: the PNGs are byte-identical.  (Without --track-components, for the reason
    tests/test_gpu_flow.py gives.)  Both runs start from the SAME seeded parent checkpoint, written into their directories: without one
    train_online.py --synthetic fine-tunes a randomly initialised network, another one in every process, and with the matcher on -- its map
    is made from that network's features -- two runs of one and the same command then write different masks."""
    import networks.vgg_osvos as vo
    torch.manual_seed(0)
    parent = vo.OSVOS(pretrained=0).state_dict()

    def run(name, *extra):
        os.makedirs(str(tmp_path / name))
        torch.save(parent, str(tmp_path / name / "parent_epoch-239.pth"))
        return script_runner.train_online(tmp_path / name, "--device-augment", "--synthetic-frames", "3", "--match-gain", "2", *extra, frames=3).masks
    assert run("one", "--match-topk", "1") == run("plain")
