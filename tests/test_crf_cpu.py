"""CPU: the host side of the mask refinement -- the two ABI symbols of csrc/crf.hip and their argument checks (which run before any device
call), the numpy restatement of the rule (tests/crf_cases.py) against a plain per-pixel loop and a torch float64 F.unfold formulation, the
coefficients of osvos_pytorch_amd.refine, the decision cap of test_gpu_crf.py on the reference alone, and the argument checks of
train_online.py --crf-*."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osvos_crf_ws_bytes", "osvos_crf_refine")


def test_the_two_symbols_and_the_limits_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    declared = set(re.findall(r"\b(osvos_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (osvos_[a-z0-9_]+)$", nm, re.M))
    for s in SYMBOLS:
        assert s in declared and s in _lib.PROTOTYPES and s in exported and hasattr(l, s), s
    for name, value, mirror in (("OSVOS_CRF_MAX_RADIUS", 7, _lib.CRF_MAX_RADIUS), ("OSVOS_CRF_MAX_REACH", 16, _lib.CRF_MAX_REACH),
                                ("OSVOS_CRF_MAX_ITERS", 64, _lib.CRF_MAX_ITERS)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == value == mirror, name
    assert l.osvos_crf_ws_bytes(2, 37, 53, 5) == 2 * 37 * 53 * 4 and l.osvos_crf_ws_bytes(2, 37, 53, 2) == 2 * 37 * 53 * 4
    assert l.osvos_crf_ws_bytes(2, 37, 53, 1) == 0 and l.osvos_crf_ws_bytes(2, 37, 53, 0) == 0          # one step goes straight to out
    assert l.osvos_crf_ws_bytes(1, 16384, 16384, 64) == 4 * 16384 * 16384
    for bad in [(0, 8, 8, 5), (1, 0, 8, 5), (1, 8, 16385, 5), (1, 8, 8, 65), (1, 8, 8, -1)]:
        assert l.osvos_crf_ws_bytes(*bad) == 0, bad


def _call(l, **kw):
    """osvos_crf_refine on fake, aligned, non-null 'device' pointers: the checks under test return before anything is dereferenced"""
    a = dict(unary=4096, init=None, bgr=8192, out=16384, ws=32768, N=1, H=8, W=8, iters=5, radius=2, dilation=2, w_a=1.0, w_s=1.0, a_s=0.1,
             a_c=0.01, g_s=0.2)
    a.update(kw)
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return l.osvos_crf_refine(p(a["unary"]), p(a["init"]), p(a["bgr"]), p(a["out"]), p(a["ws"]), a["N"], a["H"], a["W"], a["iters"], a["radius"],
                              a["dilation"], a["w_a"], a["w_s"], a["a_s"], a["a_c"], a["g_s"], None)


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    refused = [
        (dict(unary=None), b"null pointer"), (dict(bgr=None), b"null pointer"), (dict(out=None), b"null pointer"),
        (dict(ws=None), b"ws is a null pointer with iters 5"), (dict(ws=None, iters=2), b"ws is a null pointer with iters 2"),
        (dict(unary=4098), b"4-byte aligned"), (dict(init=4099), b"4-byte aligned"), (dict(out=16385), b"4-byte aligned"),
        (dict(ws=32770), b"4-byte aligned"),
        (dict(out=4096), b"out must not be unary or init"), (dict(init=16384), b"out must not be unary or init"),
        (dict(ws=4096), b"ws must not be unary, init or out"), (dict(ws=16384), b"ws must not be unary, init or out"),
        (dict(N=0), b"N 0 images"), (dict(N=-3), b"N -3 images"),
        (dict(H=0), b"bad size H 0 W 8"), (dict(W=0), b"bad size H 8 W 0"), (dict(H=16385), b"bad size"), (dict(W=16385), b"bad size"),
        (dict(iters=-1), b"iters -1 (0..64)"), (dict(iters=65), b"iters 65 (0..64)"),
        (dict(radius=-1), b"radius -1 (0..7)"), (dict(radius=8, dilation=1), b"radius 8 (0..7)"),
        (dict(dilation=0), b"dilation 0 (>= 1)"), (dict(dilation=-2), b"dilation -2 (>= 1)"),
        (dict(radius=5, dilation=4), b"reaches 20 pixels (at most 16)"), (dict(radius=1, dilation=17), b"reaches 17 pixels (at most 16)"),
        (dict(radius=7, dilation=2 ** 30), b"at most 16"),
    ]
    for name in ("w_a", "w_s", "a_s", "a_c", "g_s"):
        for v in (-1.0, float("nan"), float("inf"), -float("inf")):
            refused.append(({name: v}, b"must be finite and >= 0"))
    for kw, msg in refused:
        assert _call(l, **kw) < 0, kw
        assert msg in l.osvos_last_error(), (kw, l.osvos_last_error())
    with pytest.raises(RuntimeError, match="crf_refine"):
        _lib.check(_call(l, N=0), "crf_refine")


def _pixel_loop(u, frames, T, R, D, coeffs, init=None):
    """the rule, pixel by pixel and neighbour by neighbour, in Python floats"""
    w_a, w_s, a_s, a_c, g_s = [float(np.float32(c)) for c in coeffs]
    N, H, W = u.shape
    z = [[[float((u if init is None else init)[n, y, x]) for x in range(W)] for y in range(H)] for n in range(N)]
    for _ in range(T):
        new = [[[0.0] * W for _ in range(H)] for _ in range(N)]
        for n in range(N):
            for y in range(H):
                for x in range(W):
                    total = 0.0
                    for oy, ox in cc.offsets(R, D):
                        yy, xx = y + oy, x + ox
                        if not (0 <= yy < H and 0 <= xx < W):
                            continue
                        dc = sum((int(frames[n, y, x, c]) - int(frames[n, yy, xx, c])) ** 2 for c in range(3))
                        ds = oy * oy + ox * ox
                        k = w_a * math.exp(-(a_s * ds + a_c * dc)) + w_s * math.exp(-g_s * ds)
                        total += k * (2.0 / (1.0 + math.exp(-z[n][yy][xx])) - 1.0)
                    new[n][y][x] = float(u[n, y, x]) + total
        z = new
    return np.array(z)


@pytest.mark.parametrize("h,w,n", cc.SIZES[:3], ids=["%dx%dx%d" % s for s in cc.SIZES[:3]])
def test_reference_agrees_with_a_plain_per_pixel_loop(h, w, n):
    u, fr = cc.scene(h, w, n)
    for (R, D), ws, T in [((5, 1), "strong", 1), ((3, 2), "contractive", 2), ((2, 4), "strong", 2), ((1, 16), "strong", 1)]:
        coeffs = cc.coefficients(R, D, *cc.WEIGHTS[ws])
        mine, loop = cc.reference(u, fr, T, R, D, coeffs), _pixel_loop(u, fr, T, R, D, coeffs)
        assert mine.shape == loop.shape == (n, h, w) and mine.dtype == np.float64
        assert np.abs(mine - loop).max() <= 1e-12 * max(1.0, np.abs(loop).max()), (R, D, ws)
    init = u[:, ::-1].copy()
    coeffs = cc.coefficients(2, 2, *cc.WEIGHTS["strong"])
    assert np.abs(cc.reference(u, fr, 2, 2, 2, coeffs, init) - _pixel_loop(u, fr, 2, 2, 2, coeffs, init)).max() <= 1e-12 * np.abs(u).max()
    assert np.array_equal(cc.reference(u, fr, 0, 2, 2, coeffs, init), init.astype(np.float64))


def _unfold_form(u, frames, T, R, D, coeffs):
    """torch float64: F.unfold gathers the dilated window of s and of the three colour planes (zero padding: s = 0 outside the image)"""
    F = torch.nn.functional
    w_a, w_s, a_s, a_c, g_s = [float(np.float32(c)) for c in coeffs]
    N, H, W = u.shape
    K = 2 * R + 1
    ut = torch.from_numpy(np.asarray(u, dtype=np.float64))[:, None]
    col = torch.from_numpy(np.asarray(frames).astype(np.float64)).permute(0, 3, 1, 2)
    kw = dict(kernel_size=K, dilation=D, padding=R * D)
    nb = F.unfold(col, **kw).view(N, 3, K * K, H * W)
    dc = ((nb - col.reshape(N, 3, 1, H * W)) ** 2).sum(1)
    r = torch.arange(-R, R + 1, dtype=torch.float64) * D
    ds = (r[:, None] ** 2 + r[None, :] ** 2).reshape(1, K * K, 1)
    k = w_a * torch.exp(-(a_s * ds + a_c * dc)) + w_s * torch.exp(-g_s * ds)
    k[:, K * K // 2] = 0.0
    z = ut.clone()
    for _ in range(T):
        s = F.unfold(2.0 * torch.sigmoid(z) - 1.0, **kw)
        z = ut + (k * s).sum(1).view(N, 1, H, W)
    return z[:, 0].numpy()


def test_reference_agrees_with_a_torch_float64_unfold_formulation():
    h, w, n = 30, 85, 1
    u, fr = cc.scene(h, w, n)
    for (R, D) in cc.WINDOWS + cc.LIMIT_WINDOWS:
        for ws in cc.WEIGHTS:
            coeffs = cc.coefficients(R, D, *cc.WEIGHTS[ws])
            mine, other = cc.reference(u, fr, 3, R, D, coeffs), _unfold_form(u, fr, 3, R, D, coeffs)
            assert np.abs(mine - other).max() <= 1e-12 * np.abs(other).max(), (R, D, ws)


def test_crf_coefficients():
    from osvos_pytorch_amd import refine
    for (R, D) in cc.WINDOWS + cc.LIMIT_WINDOWS + [(5, 3)]:
        for ws in cc.WEIGHTS.values():
            got = refine.crf_coefficients(R, D, ws[0], ws[1], 4.0 * D, cc.THETA_BETA, 1.5 * D)
            assert got == cc.coefficients(R, D, *ws) and all(float(np.float32(c)) == c for c in got)
            w_a, w_s, a_s, a_c, g_s = got
            assert (a_s, a_c, g_s) == tuple(float(np.float32(1.0 / (2.0 * t * t))) for t in (4.0 * D, 13.0, 1.5 * D))
            # the normalised masses: each kernel's weights over the full window sum to the weight asked for
            ds = np.array([oy * oy + ox * ox for oy, ox in cc.offsets(R, D)], dtype=np.float64)
            assert abs(w_a * np.exp(-a_s * ds).sum() - ws[0]) <= 1e-6 * ws[0] and abs(w_s * np.exp(-g_s * ds).sum() - ws[1]) <= 1e-6 * ws[1]
            assert abs(cc.ksum(R, D, got) - (ws[0] + ws[1])) <= 1e-6 * (ws[0] + ws[1])
            raw = refine.crf_coefficients(R, D, ws[0], ws[1], 4.0 * D, cc.THETA_BETA, 1.5 * D, normalize=False)
            assert raw[:2] == (float(np.float32(ws[0])), float(np.float32(ws[1]))) and raw[2:] == got[2:]
    assert refine.crf_coefficients(5, 3, 4.0, 1.0, 8.0, 13.0, 3.0)[2:] == tuple(float(np.float32(v)) for v in (1 / 128.0, 1 / 338.0, 1 / 18.0))
    assert refine.crf_coefficients(0, 1, 4.0, 1.0, 8.0, 13.0, 3.0)[:2] == (4.0, 1.0)          # no window: nothing to normalise by
    for bad in [dict(radius=8), dict(radius=-1), dict(dilation=0), dict(radius=5, dilation=4), dict(w_appearance=-1.0), dict(w_smooth=float("nan")),
                dict(theta_alpha=0.0), dict(theta_beta=-2.0), dict(theta_gamma=float("inf")), dict(radius=2.5), dict(theta_gamma=1e-3, dilation=3)]:
        kw = dict(radius=5, dilation=3, w_appearance=4.0, w_smooth=1.0, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            refine.crf_coefficients(**kw)


def test_normalised_weights_bound_the_change_and_an_empty_kernel_changes_nothing():
    from osvos_pytorch_amd import refine
    h, w, n = 30, 85, 1
    u, fr = cc.scene(h, w, n)
    for (R, D) in cc.WINDOWS + cc.LIMIT_WINDOWS:
        for w_a, w_s in [(1.5, 0.5), (6.0, 2.0), (0.0, 3.0), (5.0, 0.0)]:
            coeffs = refine.crf_coefficients(R, D, w_a, w_s, 4.0 * D, cc.THETA_BETA, 1.5 * D)
            z = cc.reference(u, fr, 4, R, D, coeffs)
            assert np.abs(z - u).max() <= (w_a + w_s) * (1 + 1e-6), (R, D, w_a, w_s)
            assert np.abs(z - u).max() > 0.05 * (w_a + w_s)          # ... and real messages flow
        assert np.array_equal(cc.reference(u, fr, 3, R, D, refine.crf_coefficients(R, D, 0.0, 0.0, 4.0 * D, 13.0, 1.5 * D)), u.astype(np.float64))
    assert np.array_equal(cc.reference(u, fr, 3, 0, 1, refine.crf_coefficients(0, 1, 4.0, 1.0, 8.0, 13.0, 3.0)), u.astype(np.float64))
    assert np.array_equal(cc.reference(u, fr, 3, 0, 5, refine.crf_coefficients(0, 5, 4.0, 1.0, 8.0, 13.0, 3.0), init=-u), u.astype(np.float64))


@pytest.mark.parametrize("c", cc.ONE_STEP_CASES + cc.FIVE_STEP_CASES + [cc.LARGE_CASE], ids=cc.case_id)
def test_reference_alone_meets_the_decision_cap(c):
    """the share of a case's pixels whose reference lies within the case's bound of the threshold -- the pixels test_gpu_crf.py excludes from
    its decision comparison -- is at most 0.5 %; and the scenes exercise real messages: refinement changes decisions"""
    k = cc.case(*c)
    near = float((np.abs(k["ref"]) <= k["bound"]).mean())
    changed = float(((k["ref"] > 0) != (k["u"] > 0)).mean())
    print("%s: bound %.2e, %.4f %% of the pixels within it, %.1f %% of the decisions changed by refinement" % (cc.case_id(c), k["bound"], 100 * near, 100 * changed))
    assert near <= cc.DECISION_CAP
    assert 1e-6 <= k["bound"] <= 2e-3
    if c[0] * c[1] >= 1024:          # (a 16 x 16 frame holds few neighbours of a window that reaches 8 pixels)
        assert changed >= 0.005


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from osvos_pytorch_amd import refine
    u, fr = torch.zeros(1, 1, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.crf_refine(u, fr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.CrfRefiner()(u, fr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.refine_raw(u, fr, (1.0, 1.0, 0.1, 0.1, 0.1), 1, 1, 1)
    # parameters are refused before the tensors are looked at
    for bad in [dict(iters=-1), dict(iters=65), dict(radius=8), dict(dilation=0), dict(radius=5, dilation=4), dict(w_appearance=-1.0),
                dict(theta_beta=0.0), dict(iters=2.5)]:
        with pytest.raises(ValueError):
            refine.crf_refine(u, fr, **bad)
        with pytest.raises(ValueError):
            refine.CrfRefiner(**bad)
    with pytest.raises(ValueError):
        refine.refine_raw(u, fr, (1.0, -1.0, 0.1, 0.1, 0.1), 1, 1, 1)
    with pytest.raises(ValueError):
        refine.refine_raw(u, fr, (1.0, 1.0, 0.1, 0.1), 1, 1, 1)
    assert refine.parse_pair("4, 1", 2, "w") == (4.0, 1.0) and refine.parse_pair("8,13,3", 3, "t") == (8.0, 13.0, 3.0)
    for text, n in [("x", 2), ("1", 2), ("1,2,3", 2), ("1,nan", 2), ("", 3), ("1,,2", 3)]:
        with pytest.raises(ValueError):
            refine.parse_pair(text, n, "w")


def _train_online(*args):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "train_online.py"] + list(args), cwd=REPO, env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("args,message", [
    (("--crf-iters", "3"), "--crf-iters needs --device-augment"),
    (("--synthetic", "--device-augment", "--crf-iters", "-1"), "--crf-iters takes an iteration count >= 0"),
    (("--synthetic", "--device-augment", "--crf-iters", "3", "--crf-radius", "8"), "radius 8 (0..7)"),
    (("--synthetic", "--device-augment", "--crf-iters", "3", "--crf-radius", "5", "--crf-dilation", "4"), "reaches 20 pixels (at most 16)"),
    (("--synthetic", "--device-augment", "--crf-iters", "3", "--crf-weights", "x"), "--crf-weights WA,WS takes 2 comma-separated numbers"),
], ids=["no-device-augment", "iters-1", "radius-8", "reach-20", "weights-x"])
def test_train_online_refuses_bad_crf_arguments_before_any_gpu_work(args, message):
    r = _train_online(*args)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
