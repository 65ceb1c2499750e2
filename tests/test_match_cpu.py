"""CPU: appearance matching as tests/match_cases.py restates the rule of include/osvos_hip.h -- the restatement's own properties (the naive loops
against the vectorised form, the range of sim, identical rows, channel permutations, the empty-class and void rules, the pinned scenario), and what
runs without a GPU of the four osvos_match_* entry points, of osvos_pytorch_amd.match and of train_online.py --match-gain.  The GPU tests compare
the kernels against this restatement bit for bit."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_cases as mc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("osvos_match_quantize", "osvos_match_cell_labels", "osvos_match_ws_bytes", "osvos_match_nearest")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the restatement


@pytest.mark.parametrize("kind", mc.FEATURE_KINDS)
def test_quantize_obeys_its_rule(kind):
    f = mc.features(kind, 63, 192)
    q, rinv = mc.quantize(f)
    assert q.dtype == np.int8 and rinv.dtype == np.float32 and q.shape == f.shape and rinv.shape == (63,)
    assert q.min() >= -127                                                   # -128 never appears
    dead = [1, 2, 3]                                                         # all zero, an inf, a NaN
    assert not q[dead].any() and not rinv[dead].any()
    live = np.setdiff1d(np.arange(63), dead)
    assert (np.abs(q[live].astype(int)).max(axis=1) == 127).all()            # the largest channel lands on +-127
    assert (np.abs(q[4]) == 127).all() and rinv[4] == np.float32(1.0) / np.sqrt(np.float32(127 * 127 * 192))
    assert np.array_equal(q[5], q[6]) and rinv[5] == rinv[6]
    assert set(np.unique(q[7])) <= {-127, 0, 127} and q[7, 1] == 127         # the scale overflowed: zeros stay zero, the rest saturates
    n = (q.astype(np.int64) ** 2).sum(axis=1)
    assert np.array_equal(_bits(rinv[live]), _bits((1.0 / np.sqrt(n[live].astype(np.float64).astype(np.float32))).astype(np.float32)))
    if kind == "halves":                                                     # s = 1: the products are the values, ties go to even
        rows = np.setdiff1d(live, [4, 7])                                    # (the planted pixels are not of this kind)
        want = np.clip(np.rint(f[rows].astype(np.float64)), -127, 127)
        assert np.array_equal(q[rows], want.astype(np.int8)) and (f[rows] % 1 == 0.5).any()


def test_bf16_rounding_helper_is_torch_s():
    f = mc.features("signed", 63, 64)
    want = torch.from_numpy(f).to(torch.bfloat16).to(torch.float32).numpy()
    got = mc.bf16_round(f)
    keep = ~np.isnan(f)
    assert np.array_equal(_bits(got)[keep], _bits(want)[keep]) and np.isnan(got[~keep]).all()


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("c", [(1, 1, 64), (7, 9, 64), (12, 40, 128)])
@pytest.mark.parametrize("nr", [1, 2])
def test_naive_loop_equals_the_vectorised_nearest(c, nr, kind):
    p = mc.nearest_problem(*c, n=2, nr=nr, kind=kind)
    sim, idx = mc.nearest_naive(p["Q"], p["rinv_q"], p["R"], p["rinv_r"], p["label"])
    assert p["sim"].dtype == np.float32 and p["idx"].dtype == np.int32 and p["sim"].shape == (2, 2, c[0])
    assert np.array_equal(_bits(sim), _bits(p["sim"])) and np.array_equal(idx, p["idx"])


@pytest.mark.parametrize("c", mc.NEAREST_CASES, ids=str)
def test_sim_is_a_cosine_or_minus_two_and_ties_take_the_smaller_index(c):
    pq, pr, ch = c
    p = mc.nearest_problem(pq, pr, ch, n=2, nr=1)
    sim, idx = p["sim"], p["idx"]
    assert (((sim >= -1 - 1e-6) & (sim <= 1 + 1e-6)) | (sim == -2)).all()
    assert ((sim == -2) == (idx == -1)).all()
    lab = p["label"][0]
    for row, cls in ((0, 1), (1, 0)):
        if not (lab == cls).any():
            assert (idx[:, row] == -1).all()
            continue
        assert (lab[idx[:, row]] == cls).all()
        # no earlier row of the class reaches the winner's score
        t = mc.scores(p["Q"][0], p["R"][0], p["rinv_r"][0])
        win = t[np.arange(pq), idx[0, row]]
        for a in range(0, pq, max(pq // 16, 1)):
            cols = np.flatnonzero(lab == cls)
            assert (t[a, cols] <= win[a]).all() and (t[a, cols[cols < idx[0, row, a]]] < win[a]).all()
    # the planted duplicates never win over their originals
    for src, dst in ((5, 9), (11, 139), (20, pr - 1)):
        if dst < pr and src < dst and src != pr // 2 and dst != pr // 2:
            assert not (idx == dst).any()


def test_a_query_identical_to_a_reference_row_gives_n_rinv_rinv():
    p = mc.nearest_problem(37, 33, 64, n=2, nr=1, kind="fg")
    for a in range(8, 24):
        b = (a * 37) % 33
        assert np.array_equal(p["Q"][0, a], p["R"][0, b])
        n = int((p["R"][0, b].astype(np.int64) ** 2).sum())
        want = np.float32(np.float32(np.float32(n) * p["rinv_r"][0, b]) * p["rinv_q"][0, a])
        if n:                                                                # (Cauchy-Schwarz: nothing beats the row itself)
            assert _bits(p["sim"][0, 0, a]) == _bits(want) and abs(float(want) - 1) < 1e-6
        else:
            assert p["sim"][0, 0, a] == 0


def test_sim_is_invariant_under_a_channel_permutation():
    p = mc.nearest_problem(130, 257, 128, n=2, nr=2)
    perm = np.random.default_rng(3).permutation(128)
    sim, idx = mc.nearest(p["Q"][..., perm], p["rinv_q"], p["R"][..., perm], p["rinv_r"], p["label"])
    assert np.array_equal(_bits(sim), _bits(p["sim"])) and np.array_equal(idx, p["idx"])
    # and a permutation of the reference rows maps idx accordingly wherever the winner is unique
    rp = np.random.default_rng(4).permutation(257)
    sim2, idx2 = mc.nearest(p["Q"], p["rinv_q"], p["R"][:, rp], p["rinv_r"][:, rp], p["label"][:, rp])
    assert np.array_equal(_bits(sim2), _bits(p["sim"]))
    t = mc.scores(p["Q"][0], p["R"][0], p["rinv_r"][0])
    for row, cls in ((0, 1), (1, 0)):
        cols = np.flatnonzero(p["label"][0] == cls)
        unique = (t[:, cols] == t[np.arange(130), p["idx"][0, row]][:, None]).sum(axis=1) == 1
        assert unique.any() and np.array_equal(rp[idx2[0, row]][unique], p["idx"][0, row][unique])


@pytest.mark.parametrize("kind,want", [("fg", (False, True)), ("bg", (True, False)), ("void", (True, True)), ("mixed", (False, False))])
def test_the_empty_class_rule(kind, want):
    p = mc.nearest_problem(37, 33, 64, n=2, nr=1, kind=kind)
    for row in (0, 1):
        empty = (p["sim"][:, row] == -2).all() and (p["idx"][:, row] == -1).all()
        assert empty == want[row]
        if not want[row]:
            assert (p["idx"][:, row] >= 0).all() and (p["sim"][:, row] > -2).all()


@pytest.mark.parametrize("c", mc.LABEL_CASES, ids=str)
def test_cell_labels_and_the_void_rule_at_ragged_borders(c):
    H, W, S = c
    m = mc.masks(H, W, 2)
    lab = mc.cell_labels(m, S)
    assert lab.shape == (2,) + mc.grid_shape(H, W, S) and lab.dtype == np.uint8
    assert np.array_equal(lab, mc.cell_labels_naive(m, S))
    assert set(np.unique(lab)) <= {0, 1, 255}
    if lab[0].size > 4:
        assert set(np.unique(lab)) == {0, 1, 255}                            # object, background and void cells all occur


def test_cell_label_thresholds_are_exact():
    """a 4 x 4 cell with k object pixels: object from 12, background up to 4; a ragged 4 x 3 cell (12 pixels): from 9, up to 3"""
    for k in range(17):
        m = np.zeros((1, 4, 4), np.uint8)
        m.reshape(-1)[:k] = 200
        assert mc.cell_labels(m, 4)[0, 0, 0] == (1 if k >= 12 else 0 if k <= 4 else 255)
    for k in range(13):
        m = np.zeros((1, 4, 7), np.uint8)
        cell = np.zeros(12, np.uint8)
        cell[:k] = 1
        m[0, :, 4:] = cell.reshape(4, 3)
        assert mc.cell_labels(m, 4)[0, 0, 1] == (1 if k >= 9 else 0 if k <= 3 else 255)


def test_the_scenario_is_pinned():
    s = mc.scenario()
    assert s["iou_plain"] <= 0.90 and s["iou_matched"] >= 0.99
    assert s["iou_plain"] == mc.SCENE_IOU_PLAIN and s["iou_matched"] == mc.SCENE_IOU_MATCHED
    assert s["margin"] > 0.25                                                # no fused logit is near its threshold: a last-bit change flips nothing
    assert set(np.unique(s["label"])) == {0, 1}
    obj = s["truth1"][::8, ::8] != 0
    assert (s["map"][0][obj] > 0.4).all() and (s["map"][0][~obj] < -0.4).all()


# ------------------------------------------------------------------------------------------------------------------ the library, no device


def test_the_four_symbols_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(l, name)
        assert re.search(r" T %s$" % name, nm, re.M)


def test_size_queries_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for n, pq, pr, c in [(1, 1, 1, 64), (2, 300, 2049, 1024), (1, 6420, 6420, 512), (1, 25680, 25680, 256), (3, 1 << 20, 1 << 20, 64)]:
        need = l.osvos_match_ws_bytes(n, pq, pr, c)
        assert need >= n * 2 * pq * 8 and need % (n * 2 * pq * 8) == 0        # a (value, index) pair per slice, class and query
        assert need // (n * 2 * pq * 8) <= -(-pr // 128)                      # never more slices than reference tiles
    assert l.osvos_match_ws_bytes(1, 1, 1, 64) == 16
    assert l.osvos_match_ws_bytes(1, 6420, 6420, 512) > 16 * 6420             # DAVIS size: the reference rows are split over several slices
    for bad in [(0, 8, 8, 64), (65536, 8, 8, 64), (1, 0, 8, 64), (1, 8, 0, 64), (1, (1 << 20) + 1, 8, 64), (1, 8, (1 << 20) + 1, 64), (1, 8, 8, 0),
                (1, 8, 8, 32), (1, 8, 8, 96), (1, 8, 8, 1088), (1, 8, 8, -64)]:
        assert l.osvos_match_ws_bytes(*bad) == 0, bad


def _err(l, rc, *words):
    msg = l.osvos_last_error()
    assert rc < 0 and all(w in msg for w in words), (rc, msg)


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    vp = C.c_void_p
    A, B, D, E, F, G, H_, I = (vp(1 << 20), vp(2 << 20), vp(3 << 20), vp(4 << 20), vp(5 << 20), vp(6 << 20), vp(7 << 20), vp(8 << 20))
    # quantize
    _err(l, l.osvos_match_quantize(None, 0, B, D, 4, 64, None), b"match_quantize", b"null")
    _err(l, l.osvos_match_quantize(A, 0, None, D, 4, 64, None), b"match_quantize", b"null")
    _err(l, l.osvos_match_quantize(A, 0, B, None, 4, 64, None), b"match_quantize", b"null")
    _err(l, l.osvos_match_quantize(A, 2, B, D, 4, 64, None), b"format 2")
    for p in (0, -1, (1 << 30) + 1):
        _err(l, l.osvos_match_quantize(A, 0, B, D, p, 64, None), b"P %d " % p)
    for c in (0, 32, 96, 1088, -64):
        _err(l, l.osvos_match_quantize(A, 0, B, D, 4, c, None), b"C %d " % c)
    _err(l, l.osvos_match_quantize(A, 0, vp((2 << 20) + 8), D, 4, 64, None), b"misaligned", b"q by 16")
    _err(l, l.osvos_match_quantize(vp((1 << 20) + 2), 0, B, D, 4, 64, None), b"misaligned")
    _err(l, l.osvos_match_quantize(vp((1 << 20) + 1), 1, B, D, 4, 64, None), b"misaligned")
    _err(l, l.osvos_match_quantize(A, 0, B, vp((3 << 20) + 2), 4, 64, None), b"misaligned")
    _err(l, l.osvos_match_quantize(A, 0, vp((1 << 20) + 512), D, 4, 64, None), b"aliasing")
    _err(l, l.osvos_match_quantize(A, 0, B, vp((2 << 20) + 128), 4, 64, None), b"aliasing")
    # cell_labels
    _err(l, l.osvos_match_cell_labels(None, B, 1, 48, 64, 6, 8, 8, None), b"match_cell_labels", b"null")
    _err(l, l.osvos_match_cell_labels(A, None, 1, 48, 64, 6, 8, 8, None), b"match_cell_labels", b"null")
    for n in (0, 65536):
        _err(l, l.osvos_match_cell_labels(A, B, n, 48, 64, 6, 8, 8, None), b"N %d " % n)
    for hh, ww in ((0, 64), (48, 0), (16385, 64), (48, 16385)):
        _err(l, l.osvos_match_cell_labels(A, B, 1, hh, ww, 6, 8, 8, None), b"bad size")
    for s in (0, 3, 128, -8):
        _err(l, l.osvos_match_cell_labels(A, B, 1, 48, 64, 6, 8, s, None), b"stride %d " % s)
    _err(l, l.osvos_match_cell_labels(A, B, 1, 45, 70, 5, 9, 8, None), b"grid h 5 w 9", b"6 x 9")      # ceil, not floor
    _err(l, l.osvos_match_cell_labels(A, vp((1 << 20) + 100), 1, 48, 64, 6, 8, 8, None), b"aliasing")
    # nearest
    ok = [A, B, D, E, F, G, H_, I, 2, 1, 37, 33, 64, None]
    for k in (0, 1, 2, 3, 4, 5, 7):                                          # every pointer but idx
        a = list(ok)
        a[k] = None
        _err(l, l.osvos_match_nearest(*a), b"match_nearest", b"null")
    for k, name, bad in [(8, b"N", (0, 65536)), (9, b"NR", (0, 3)), (10, b"Pq", (0, (1 << 20) + 1)), (11, b"Pr", (0, -5, (1 << 20) + 1)),
                         (12, b"C", (0, 32, 96, 1088))]:
        for v in bad:
            a = list(ok)
            a[k] = v
            _err(l, l.osvos_match_nearest(*a), name + b" %d " % v)
    for k, word in [(0, b"Q and R"), (2, b"Q and R"), (7, b"ws"), (1, b"rinv_q"), (5, b"sim"), (6, b"idx")]:
        a = list(ok)
        a[k] = vp(a[k].value + (8 if k in (0, 2) else 4 if k == 7 else 2))
        _err(l, l.osvos_match_nearest(*a), b"misaligned", word)
    for out_k in (5, 6, 7):
        for in_k in (0, 1, 2, 3, 4):
            a = list(ok)
            a[out_k] = vp(a[in_k].value + 16)
            _err(l, l.osvos_match_nearest(*a), b"aliasing")
    a = list(ok)
    a[6] = vp(a[5].value + 64)
    _err(l, l.osvos_match_nearest(*a), b"aliasing", b"three buffers")
    with pytest.raises(RuntimeError, match="match_nearest"):
        _lib.check(l.osvos_match_nearest(*([None] * 8 + [1, 1, 1, 1, 64, None])), "match_nearest")


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from osvos_pytorch_amd import match
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match.quantize(torch.zeros(4, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match.cell_labels(torch.zeros(1, 8, 8, dtype=torch.uint8), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match.nearest(torch.zeros(1, 4, 64, dtype=torch.int8), torch.zeros(1, 4), torch.zeros(1, 4, 64, dtype=torch.int8), torch.zeros(1, 4),
                      torch.zeros(1, 4, dtype=torch.uint8))
    for layer in (5, 0, 13, "9"):
        with pytest.raises(ValueError, match="layer"):
            match.check_match(layer, 1.0)
    for gain in (float("nan"), float("inf"), -1.0, "2"):
        with pytest.raises(ValueError, match="gain"):
            match.check_match(9, gain)
    assert match.stride_of(3) == 2 and match.stride_of(6) == 4 and match.stride_of(9) == 8 and match.stride_of(12) == 16


def _train_online(*args):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "train_online.py"] + list(args), cwd=REPO, env=env, capture_output=True, text=True, timeout=600)


def test_train_online_refuses_match_gain_with_test_time_augmentation():
    r = _train_online("--synthetic", "--device-augment", "--match-gain", "1", "--tta-flip")
    assert r.returncode != 0 and "--match-gain" in r.stderr and "--tta-scales / --tta-flip" in r.stderr, r.stderr[-2000:]
    r = _train_online("--match-gain", "1", "--tta-flip")
    assert r.returncode != 0


def test_train_online_refuses_bad_match_arguments_before_any_gpu_work():
    r = _train_online("--match-gain", "1")
    assert r.returncode != 0 and "--match-gain needs --device-augment" in r.stderr, r.stderr[-2000:]
    r = _train_online("--synthetic", "--device-augment", "--match-gain", "1", "--match-layer", "5")
    assert r.returncode != 0 and "--match-*" in r.stderr and "layer" in r.stderr, r.stderr[-2000:]
    r = _train_online("--synthetic", "--device-augment", "--match-gain", "-1")
    assert r.returncode != 0 and "--match-*" in r.stderr and "gain" in r.stderr, r.stderr[-2000:]
