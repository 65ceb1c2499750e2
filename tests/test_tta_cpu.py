"""CPU: the host side of test-time augmentation -- the two ABI symbols of csrc/tta.hip and their argument checks (which run before any device
call), the numpy restatement of the sampling rule (tests/tta_cases.py) against torch's float64 F.interpolate, the view plan of
osvos_pytorch_amd.tta, and the argument checks of train_online.py --tta-scales / --tta-flip."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tta_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osvos_tta_view", "osvos_tta_fuse")


def test_the_two_symbols_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    declared = set(re.findall(r"\b(osvos_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (osvos_[a-z0-9_]+)$", nm, re.M))
    for s in SYMBOLS:
        assert s in declared and s in _lib.PROTOTYPES and s in exported and hasattr(l, s), s
    m = re.search(r"#define\s+OSVOS_TTA_MAX_VIEWS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 16 == _lib.TTA_MAX_VIEWS


def _fuse_args(V, n=16):
    """host arrays of n entries and fake, aligned, non-null 'device' pointers: the checks under test return before anything is dereferenced"""
    ia = C.c_int * n
    views = (C.c_void_p * n)(*[C.c_void_p(4096)] * n)
    return [views, ia(*[8] * n), ia(*[8] * n), ia(*[0] * n), None, V, C.c_void_p(8192)]


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    mean = (C.c_float * 3)(*tc.MEANVAL)
    assert l.osvos_tta_view(None, None, None, 1, 8, 8, 8, 8, 0, None) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_tta_view(C.c_void_p(4096), None, C.c_void_p(8192), 1, 8, 8, 8, 8, 0, None) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_tta_fuse(None, None, None, None, None, 1, None, 1, 8, 8, None) < 0 and b"null" in l.osvos_last_error()
    for V in (0, 17, -1):
        assert l.osvos_tta_fuse(*(_fuse_args(V, 17) + [1, 8, 8, None])) < 0
        assert b"views (1..16)" in l.osvos_last_error() and (b"V %d " % V) in l.osvos_last_error()
    # sizes below 1 or above 16384, on either side of either call
    for (h, w, hv, wv) in [(0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0), (16385, 8, 8, 8), (8, 16385, 8, 8), (8, 8, 16385, 8), (8, 8, 8, 16385)]:
        assert l.osvos_tta_view(C.c_void_p(4096), mean, C.c_void_p(8192), 1, h, w, hv, wv, 0, None) < 0 and b"bad size" in l.osvos_last_error()
    assert l.osvos_tta_view(C.c_void_p(4096), mean, C.c_void_p(8192), 0, 8, 8, 8, 8, 0, None) < 0 and b"N 0" in l.osvos_last_error()
    for (h, w) in [(0, 8), (8, 0), (16385, 8), (8, 16385)]:
        assert l.osvos_tta_fuse(*(_fuse_args(2) + [1, h, w, None])) < 0 and b"bad size" in l.osvos_last_error()
    a = _fuse_args(2)
    a[1][1] = 16385
    assert l.osvos_tta_fuse(*(a + [1, 8, 8, None])) < 0 and b"view 1 has bad size" in l.osvos_last_error()
    a = _fuse_args(2)
    a[0][1] = None
    assert l.osvos_tta_fuse(*(a + [1, 8, 8, None])) < 0 and b"view 1 is a null" in l.osvos_last_error()
    # misaligned float pointers
    a = _fuse_args(2)
    a[0][1] = C.c_void_p(4098)
    assert l.osvos_tta_fuse(*(a + [1, 8, 8, None])) < 0 and b"view 1 must be 4-byte aligned" in l.osvos_last_error()
    a = _fuse_args(2)
    a[6] = C.c_void_p(8193)
    assert l.osvos_tta_fuse(*(a + [1, 8, 8, None])) < 0 and b"out must be 4-byte aligned" in l.osvos_last_error()
    assert l.osvos_tta_view(C.c_void_p(4096), mean, C.c_void_p(8194), 1, 8, 8, 8, 8, 0, None) < 0 and b"out must be 4-byte aligned" in l.osvos_last_error()


@pytest.mark.parametrize("h,w", [(16, 16), (30, 85), (37, 53), (48, 64), (480, 854)])
def test_numpy_reference_agrees_with_torch_float64_interpolate(h, w):
    """at most 1e-9 absolute on 0..255 data (observed 3e-11); exact at scale 1; resizing a mirrored source agrees with mirroring the resized
    one to 1e-12 (observed 9e-14)"""
    rng = np.random.default_rng(h * 1000 + w)
    a = rng.integers(0, 256, size=(2, 3, h, w)).astype(np.float64)
    worst = worst_flip = 0.0
    for s in tc.SCALES:
        hv, wv = tc.view_size(h, w, s)
        mine = tc.resize(a, hv, wv)
        ref = torch.nn.functional.interpolate(torch.from_numpy(a), size=(hv, wv), mode="bilinear", align_corners=False).numpy()
        assert mine.shape == ref.shape == (2, 3, hv, wv) and mine.dtype == np.float64
        worst = max(worst, float(np.abs(mine - ref).max()))
        worst_flip = max(worst_flip, float(np.abs(tc.resize(a[..., ::-1], hv, wv) - mine[..., ::-1]).max()))
        if s == 1.0:
            assert np.array_equal(mine, a)
    print("%dx%d: numpy rule vs torch float64 %.1e, mirror commutes to %.1e" % (h, w, worst, worst_flip))
    assert worst <= 1e-9 and worst_flip <= 1e-12


def test_reference_passes_a_same_size_source_through_with_inf_and_nan():
    a = np.array([[1.0, np.inf, -np.inf], [np.nan, 2.0, 3.0]])
    assert np.array_equal(tc.resize(a, 2, 3), a, equal_nan=True)
    fr = tc.frames(5, 7, 2)
    assert np.array_equal(tc.view_reference(fr, 5, 7, True), tc.view_reference(fr, 5, 7)[..., ::-1])
    x = tc.logits(2, 5, 7)
    assert np.allclose(tc.fuse_reference([x, x], [False, True], (5, 7)), 0.5 * x.astype(np.float64) + 0.5 * x[..., ::-1], rtol=0, atol=1e-13)
    i0, i1, f = tc.taps(4, 2)          # centres at 0.25 steps of a 2-sample source: -0.25 (clamped), 0.25, 0.75, 1.25 (clamped)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and f.tolist() == [0.0, 0.25, 0.75, 0.25]


def test_view_size_and_plan():
    from osvos_pytorch_amd import tta
    assert tta.view_size(480, 854, 0.5) == (240, 427)
    assert tta.view_size(480, 854, 0.75) == (360, 641)
    assert tta.view_size(480, 854, 1.25) == (600, 1068)
    assert tta.view_size(480, 854, 1.0) == (480, 854)
    assert tta.view_size(3, 5, 0.01) == (1, 1) and tta.view_size(1, 1, 0.3) == (1, 1)          # the 1-pixel floor
    for h, w, _ in tc.FRAME_SIZES:
        for s in tc.SCALES + (2.5, 0.01):
            assert tta.view_size(h, w, s) == tc.view_size(h, w, s)
    assert tta.plan(480, 854, (1.0,), False) == [(480, 854, False)]
    assert tta.plan(480, 854, (1.25, 0.5), True) == [(600, 1068, False), (600, 1068, True), (240, 427, False), (240, 427, True)]
    assert tta.plan(480, 854, (0.75, 1, 1.25), False) == [(360, 641, False), (480, 854, False), (600, 1068, False)]
    assert len(tta.plan(480, 854, [0.5 + 0.1 * i for i in range(16)], False)) == 16
    assert len(tta.plan(480, 854, [0.5 + 0.1 * i for i in range(8)], True)) == 16
    for bad in [(), (0.0,), (-1.0,), (float("nan"),), (float("inf"),), (1.0, 1.0), (1.0, 1.0004)]:
        with pytest.raises(ValueError):
            tta.plan(480, 854, bad, False)
    with pytest.raises(ValueError, match="at most 16"):
        tta.plan(480, 854, [0.5 + 0.1 * i for i in range(17)], False)
    with pytest.raises(ValueError, match="at most 16"):
        tta.plan(480, 854, [0.5 + 0.1 * i for i in range(9)], True)
    with pytest.raises(ValueError, match="same view size"):
        tta.plan(4, 4, (0.2, 0.3), False)                       # both floor to 1 x 1
    with pytest.raises(ValueError, match="at most 16384"):
        tta.plan(480, 854, (40.0,), False)
    assert tta.parse_scales("0.75, 1,1.25") == (0.75, 1.0, 1.25) and tta.parse_scales("") == ()
    for bad in ("a", "1,,x", "0", "-2"):
        with pytest.raises(ValueError):
            tta.parse_scales(bad)
    with pytest.raises(ValueError):
        tta.TestTimeAugment(lambda x: [x], ())
    with pytest.raises(ValueError):
        tta.TestTimeAugment(lambda x: [x], (1.0, 0.5), True, weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        tta.TestTimeAugment(lambda x: [x], [0.5 + 0.1 * i for i in range(9)], True)


def test_wrappers_refuse_cpu_tensors_loudly():
    from osvos_pytorch_amd import tta
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tta.make_view(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tta.fuse_views([torch.zeros(1, 4, 4)], [False], (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tta.TestTimeAugment(lambda x: [x])(torch.zeros(4, 4, 3, dtype=torch.uint8))


def _train_online(*args):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "train_online.py"] + list(args), cwd=REPO, env=env, capture_output=True, text=True, timeout=600)


def test_train_online_tta_needs_the_decoded_frame_on_the_device():
    r = _train_online("--tta-flip")
    assert r.returncode != 0
    assert "--tta-scales / --tta-flip need --device-augment" in r.stderr, r.stderr[-2000:]


def test_train_online_refuses_bad_tta_scales_before_any_gpu_work():
    r = _train_online("--synthetic", "--device-augment", "--tta-scales", "0.75,0")
    assert r.returncode != 0 and "--tta-scales: a test-time augmentation scale must be a positive number" in r.stderr, r.stderr[-2000:]
    r = _train_online("--synthetic", "--device-augment", "--tta-scales", "1,1.0004")
    assert r.returncode != 0 and "--tta-scales: scales" in r.stderr and "same view size" in r.stderr, r.stderr[-2000:]
