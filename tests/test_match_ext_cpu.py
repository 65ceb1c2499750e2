"""CPU: top-K averaging and the local window of appearance matching as tests/match_ext_cases.py restates the rules of include/osvos_hip.h -- the
naive loops against the vectorised forms, K = 1 and the grid-covering window against match_cases.nearest, short and empty classes, planted
duplicates, radius 0, the two pinned scenarios -- and what runs without a GPU of osvos_match_topk / osvos_match_local, of their wrappers in
osvos_pytorch_amd.match and of train_online.py --match-topk / --match-local.  The GPU tests compare the kernels against this restatement."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_cases as mc
import match_ext_cases as me

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("osvos_match_topk_ws_bytes", "osvos_match_topk", "osvos_match_local")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ops(p):
    return p["Q"], p["rinv_q"], p["R"], p["rinv_r"], p["label"]


# ------------------------------------------------------------------------------------------------------------------ the restatement


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("c", [(1, 1, 64, 1), (7, 9, 64, 4), (12, 40, 128, 3), (5, 21, 64, 16)], ids=str)
@pytest.mark.parametrize("nr", [1, 2])
def test_naive_loop_equals_the_vectorised_topk(c, nr, kind):
    p = me.topk_problem(*c, n=2, nr=nr, kind=kind)
    assert p["topk"].dtype == np.float32 and p["topk"].shape == (2, 2, c[0])
    assert np.array_equal(_bits(me.topk_naive(*_ops(p), c[3])), _bits(p["topk"]))


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("c", [(1, 1, 64, 0), (3, 4, 64, 1), (5, 7, 64, 2), (4, 9, 128, 15)], ids=str)
@pytest.mark.parametrize("nr", [1, 2])
def test_naive_loop_equals_the_vectorised_local(c, nr, kind):
    h, w, ch, radius = c
    p = me.local_problem(*c, n=2, nr=nr, kind=kind)
    sim, idx = me.local_naive(*_ops(p), h, w, radius)
    assert p["lsim"].dtype == np.float32 and p["lidx"].dtype == np.int32
    assert np.array_equal(_bits(sim), _bits(p["lsim"])) and np.array_equal(idx, p["lidx"])


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("c", mc.NEAREST_CASES, ids=str)
def test_topk_of_one_is_nearest_bit_for_bit(c, kind):
    p = mc.nearest_problem(*c, n=2, nr=1, kind=kind)
    assert np.array_equal(_bits(me.topk(*_ops(p), 1)), _bits(p["sim"]))


@pytest.mark.parametrize("c", [(1, 1, 64), (5, 7, 64), (9, 13, 128)], ids=str)
def test_a_window_that_covers_the_grid_is_nearest(c):
    h, w, ch = c
    p = mc.nearest_problem(h * w, h * w, ch, n=2, nr=2)
    sim, idx = me.local(*_ops(p), h, w, max(h, w) - 1)
    assert np.array_equal(_bits(sim), _bits(p["sim"])) and np.array_equal(idx, p["idx"])


def test_short_and_empty_classes_and_planted_duplicates():
    p = mc.nearest_problem(37, 33, 64, n=2, nr=1, kind="mixed")
    lab = p["label"][0]
    n_fg, n_bg = int((lab == 1).sum()), int((lab == 0).sum())
    assert 0 < n_fg < 16 <= n_bg                                             # the foreground is shorter than K = 16, the background is not
    all_fg = me.topk(*_ops(p), 16)[:, 0]
    assert np.array_equal(_bits(all_fg), _bits(me.topk(*_ops(p), n_fg)[:, 0]))      # k = min(K, n): the mean of every row of the class
    assert not np.array_equal(_bits(all_fg), _bits(me.topk(*_ops(p), n_fg - 1)[:, 0]))
    # the mean of the k best never exceeds the best, and falls (weakly) with K
    sims = [me.topk(*_ops(p), k) for k in (1, 2, 4, 16)]
    for a, b in zip(sims, sims[1:]):
        assert (b <= a + 1e-6).all()
    # empty classes
    for kind, empty in (("fg", 1), ("bg", 0), ("void", None)):
        q = mc.nearest_problem(37, 33, 64, n=2, nr=1, kind=kind)
        s = me.topk(*_ops(q), 4)
        for row in (0, 1):
            assert ((s[:, row] == -2).all()) == (empty is None or row == empty)
    # a duplicated row is a separate member: query 5's own row is in the bank twice (rows 5 and 9), so with K = 2 the mean is that row's score
    d = mc.nearest_problem(37, 33, 64, n=1, nr=1, kind="fg")
    R, rinv_r = d["R"], d["rinv_r"]
    assert np.array_equal(R[0, 5], R[0, 9])
    Q, rinv_q = np.ascontiguousarray(R[:, 5:6]), np.ascontiguousarray(rinv_r[:, 5:6])
    one, two = me.topk(Q, rinv_q, R, rinv_r, d["label"], 1), me.topk(Q, rinv_q, R, rinv_r, d["label"], 2)
    t = mc.scores(Q[0], R[0], rinv_r[0])[0]
    assert t[5] == t[9] == t.max() and np.array_equal(_bits(one), _bits(two))      # (v + v) / 2 = v exactly


def test_radius_zero_looks_at_the_same_cell_only():
    p = me.local_problem(5, 7, 64, 0, n=2, nr=2)
    sim, idx = p["lsim"], p["lidx"]
    rows = np.arange(35)
    for b in range(2):
        for row, cls in ((0, 1), (1, 0)):
            own = p["label"][b] == cls
            assert np.array_equal(idx[b, row], np.where(own, rows, -1))
            t = mc.scores(p["Q"][b], p["R"][b], p["rinv_r"][b])[rows, rows]
            assert np.array_equal(_bits(sim[b, row]), _bits(np.where(own, (t * p["rinv_q"][b]).astype(np.float32), np.float32(-2))))
    assert np.array_equal(_bits(me.local_map(sim)), _bits(np.maximum(sim[:, 0], np.float32(-1)) - np.maximum(sim[:, 1], np.float32(-1))))
    assert me.local_map(np.full((1, 2, 3), -2, np.float32)).tolist() == [[0.0, 0.0, 0.0]]


def test_the_scenarios_are_pinned():
    b = me.bleed_scenario()
    assert (b["iou_plain"], b["iou1"], b["iou%d" % me.BLEED["K"]]) == (me.BLEED_IOU_PLAIN, me.BLEED_IOU_K1, me.BLEED_IOU_K4) == (0.5, 0.5, 1.0)
    assert b["margin%d" % me.BLEED["K"]] >= 0.25                             # no fused logit near its threshold: a last-bit change flips nothing
    cell = me.BLEED["cell"][0] * b["w"] + me.BLEED["cell"][1]
    assert b["label"][0, cell] == 1 and int((b["label"] == 1).sum()) == 17   # the 16 object cells and the bleed
    t = me.twin_scenario()
    assert (t["iou_plain"], t["iou_first"]) == (me.TWIN_IOU_PLAIN, me.TWIN_IOU_FIRST) == (0.5, 0.5)
    assert t["iou_local"] >= me.TWIN_IOU_LOCAL_AT_LEAST == 0.99
    tw = (slice(me.TWIN["twin"][0], me.TWIN["twin"][0] + 4), slice(me.TWIN["twin"][1], me.TWIN["twin"][1] + 4))
    assert (t["lsim"].reshape(2, t["h"], t["w"])[0][tw] == -2).all()         # no object cell in the twin's window a frame ago
    assert (t["map"][0][tw] > 0).all() and (t["lmap"][0][tw] < -1).all()     # first-frame matching confirms the twin; the local view denies it


# ------------------------------------------------------------------------------------------------------------------ the library, no device


def test_the_symbols_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(l, name)
        assert re.search(r" T %s$" % name, nm, re.M)
    got = {k: int(v) for k, v in re.findall(r"#define OSVOS_MATCH_MAX_(K|RADIUS)\s+(\d+)", hdr)}
    assert got == {"K": _lib.MATCH_MAX_K, "RADIUS": _lib.MATCH_MAX_RADIUS} == {"K": me.MAX_K, "RADIUS": me.MAX_RADIUS} == {"K": 16, "RADIUS": 15}


def test_the_workspace_size_needs_no_device_and_grows_with_k():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for n, pq, pr, c in [(1, 1, 1, 64), (2, 129, 1000, 512), (1, 6420, 6420, 512), (3, 1 << 20, 1 << 20, 64)]:
        sizes = [l.osvos_match_topk_ws_bytes(n, pq, pr, c, k) for k in range(1, 17)]
        assert sizes[0] >= n * 2 * pq * 4 and all(s == k * sizes[0] for k, s in enumerate(sizes, 1))      # K floats per slice, class and query
        assert sizes[0] // (n * 2 * pq * 4) == l.osvos_match_ws_bytes(n, pq, pr, c) // (n * 2 * pq * 8)    # nearest's slices
    assert l.osvos_match_topk_ws_bytes(2, 129, 1000, 512, 8) // (2 * 2 * 129 * 4 * 8) > 1                  # several slices
    for bad in [(0, 8, 8, 64, 1), (65536, 8, 8, 64, 1), (1, 0, 8, 64, 1), (1, 8, 0, 64, 1), (1, (1 << 20) + 1, 8, 64, 1), (1, 8, (1 << 20) + 1, 64, 1),
                (1, 8, 8, 96, 1), (1, 8, 8, 1088, 1), (1, 8, 8, 64, 0), (1, 8, 8, 64, 17), (1, 8, 8, 64, -1)]:
        assert l.osvos_match_topk_ws_bytes(*bad) == 0, bad


def _err(l, rc, *words):
    msg = l.osvos_last_error()
    assert rc < 0 and all(w in msg for w in words), (rc, msg)


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    vp = C.c_void_p
    A, B, D, E, F, G, H_ = (vp(k << 20) for k in range(1, 8))
    # topk: Q, rinv_q, R, rinv_r, label_r, sim, ws, N, NR, Pq, Pr, C, K, stream
    ok = [A, B, D, E, F, G, H_, 2, 1, 37, 33, 64, 4, None]
    for k in range(7):
        a = list(ok)
        a[k] = None
        _err(l, l.osvos_match_topk(*a), b"match_topk", b"null")
    for k, name, bad in [(7, b"N", (0, 65536)), (8, b"NR", (0, 3)), (9, b"Pq", (0, (1 << 20) + 1)), (10, b"Pr", (0, -5, (1 << 20) + 1)),
                         (11, b"C", (0, 32, 96, 1088)), (12, b"K", (0, 17, -1))]:
        for v in bad:
            a = list(ok)
            a[k] = v
            _err(l, l.osvos_match_topk(*a), b"match_topk", name + b" %d " % v)
    for k, word in [(0, b"Q and R"), (2, b"Q and R"), (6, b"ws"), (1, b"rinv_q"), (5, b"sim")]:
        a = list(ok)
        a[k] = vp(a[k].value + (8 if k in (0, 2) else 4 if k == 6 else 2))
        _err(l, l.osvos_match_topk(*a), b"misaligned", word)
    for out_k in (5, 6):
        for in_k in range(5):
            a = list(ok)
            a[out_k] = vp(a[in_k].value + 16)
            _err(l, l.osvos_match_topk(*a), b"aliasing")
    a = list(ok)
    a[6] = vp(a[5].value + 64)
    _err(l, l.osvos_match_topk(*a), b"aliasing", b"two buffers")
    # local: Q, rinv_q, R, rinv_r, label_r, sim, idx, N, NR, h, w, C, radius, stream
    ok = [A, B, D, E, F, G, H_, 2, 1, 5, 7, 64, 2, None]
    for k in range(6):                                                       # every pointer but idx
        a = list(ok)
        a[k] = None
        _err(l, l.osvos_match_local(*a), b"match_local", b"null")
    for k, name, bad in [(7, b"N", (0, 65536)), (8, b"NR", (0, 3)), (11, b"C", (0, 32, 96, 1088)), (12, b"radius", (-1, 16))]:
        for v in bad:
            a = list(ok)
            a[k] = v
            _err(l, l.osvos_match_local(*a), b"match_local", name + b" %d " % v)
    for hh, ww in ((0, 7), (5, 0), (-1, 7), (1 << 11, 1 << 10), ((1 << 20) + 1, 1), (1 << 16, 1 << 16)):
        a = list(ok)
        a[9], a[10] = hh, ww
        _err(l, l.osvos_match_local(*a), b"grid h %d w %d " % (hh, ww))
    for k, word in [(0, b"Q and R"), (2, b"Q and R"), (1, b"rinv_q"), (5, b"sim"), (6, b"idx")]:
        a = list(ok)
        a[k] = vp(a[k].value + (8 if k in (0, 2) else 2))
        _err(l, l.osvos_match_local(*a), b"misaligned", word)
    for out_k in (5, 6):
        for in_k in range(5):
            a = list(ok)
            a[out_k] = vp(a[in_k].value + 16)
            _err(l, l.osvos_match_local(*a), b"aliasing")
    a = list(ok)
    a[6] = vp(a[5].value + 64)
    _err(l, l.osvos_match_local(*a), b"aliasing", b"two buffers")


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from osvos_pytorch_amd import match
    ops = (torch.zeros(1, 4, 64, dtype=torch.int8), torch.zeros(1, 4), torch.zeros(1, 4, 64, dtype=torch.int8), torch.zeros(1, 4),
           torch.zeros(1, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match.topk(*ops, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match.local(*ops, grid=(2, 2), radius=1)
    for k in (0, 17, 2.0, True, "4"):
        with pytest.raises(ValueError, match="k"):
            match.topk(*ops, k)
        with pytest.raises(ValueError, match="k"):
            match.topk_workspace(1, 4, 4, 64, k, torch.device("cpu"))
    for radius in (-1, 16, 1.0, True):
        with pytest.raises(ValueError, match="radius"):
            match.local(*ops, grid=(2, 2), radius=radius)
    for grid in ((2,), 4, (0, 4), (2, 2.0), None):
        with pytest.raises(ValueError, match="grid"):
            match.local(*ops, grid=grid, radius=1)
    sim = torch.tensor([[[0.5, -2.0, -2.0], [0.25, 0.5, -2.0]]])
    assert match.local_map(sim).tolist() == [[0.25, -1.5, 0.0]]
    for kw in (dict(topk=0), dict(topk=17), dict(topk=2.0), dict(local_radius=16), dict(local_radius=-1), dict(local_gain=-1.0),
               dict(local_gain=float("nan"))):
        with pytest.raises(ValueError, match="topk|local_radius|local_gain"):
            match.AppearanceMatcher(None, **kw)
    m = match.AppearanceMatcher(None, 9, 2.0)
    assert (m.topk, m.local_radius, m.local_gain, m.needs_previous) == (1, 0, 0.0, False)
    assert match.AppearanceMatcher(None, 9, 2.0, local_radius=3, local_gain=1.0).needs_previous
    assert match.AppearanceMatcher(None, 9, 2.0, previous=True).needs_previous


def test_frame_forward_remembers_the_mask_for_the_local_view():
    from osvos_pytorch_amd import match, sequence
    logits = torch.tensor([[[[1.0, -1.0]]]])
    f = sequence.FrameForward(None, matcher=match.AppearanceMatcher(None, 9, 2.0, local_radius=3, local_gain=1.0))
    f.remember(logits)
    assert f.match_prev.tolist() == [[[[True, False]]]]
    f = sequence.FrameForward(None, matcher=match.AppearanceMatcher(None, 9, 2.0, topk=4))
    f.remember(logits)
    assert f.match_prev is None


def _train_online(*args):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "train_online.py"] + list(args), cwd=REPO, env=env, capture_output=True, text=True, timeout=600)


def test_train_online_refuses_bad_topk_and_local_arguments_before_any_gpu_work():
    base = ("--synthetic", "--device-augment")
    for extra in (("--match-topk", "4"), ("--match-local", "3,2")):
        r = _train_online(*base, *extra)
        assert r.returncode != 0 and "need --match-gain" in r.stderr, r.stderr[-2000:]
    for extra, word in ((("--match-topk", "17"), "topk"), (("--match-local", "16"), "local_radius"), (("--match-local", "3,-1"), "local_gain"),
                        (("--match-local", "3,2,1"), "--match-local")):
        r = _train_online(*base, "--match-gain", "2", *extra)
        assert r.returncode != 0 and "--match-*" in r.stderr and word in r.stderr, r.stderr[-2000:]
    r = _train_online(*base, "--match-gain", "2", "--match-local", "3,2", "--adapt-steps", "2")
    assert r.returncode != 0 and "--match-local is not run together with --adapt-steps" in r.stderr, r.stderr[-2000:]
    r = _train_online(*base, "--match-gain", "2", "--match-topk", "4", "--tta-flip")
    assert r.returncode != 0 and "--tta-scales / --tta-flip" in r.stderr, r.stderr[-2000:]
