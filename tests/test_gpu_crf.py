"""GPU: mask refinement on the device -- osvos_crf_refine (csrc/crf.hip) against the float64 restatement of the rule in tests/crf_cases.py,
its exact properties bit for bit (no iterations, no messages, composition through `init`, batch independence, repeatability), the wrappers of
osvos_pytorch_amd.refine, and train_online.py --crf-iters.

Bounds (tests/crf_cases.py, derived there).  One step: |diff| <= 2^-24 (2 umax + (2 M + 28) ksum) with M the window's neighbours and ksum the
upper bound on a pixel's summed kernel weights -- 9e-6 .. 1.3e-4 for the cases here.  T steps: that times sum_{t<T} max(1, ksum / 2)^t.
Decisions: out > 0 equals reference > 0 wherever |reference| exceeds the bound used, and the pixels excluded that way are at most 0.5 % of a
case (test_crf_cpu.py shows the reference alone meets that cap).  Outputs and workspaces are pre-filled with garbage."""
import ctypes as C

import numpy as np
import pytest
import torch

import crf_cases as cc
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE = 7.25e33


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _refine(u, fr, coeffs, T, R, D, init=None, ws_fill=GARBAGE):
    """one osvos_crf_refine call through _lib on CUDA tensors u [N,H,W] float32, fr [N,H,W,3] uint8 -> out [N,H,W]"""
    from osvos_pytorch_amd import _lib
    n, h, w = u.shape
    out = torch.full((n, h, w), GARBAGE, device="cuda", dtype=torch.float32)
    ws = torch.full((n, h, w), ws_fill, device="cuda", dtype=torch.float32) if T >= 2 else None
    assert ws is None or _lib.lib().osvos_crf_ws_bytes(n, h, w, T) == ws.numel() * 4
    vp = C.c_void_p
    _lib.check(_lib.lib().osvos_crf_refine(vp(u.data_ptr()), vp(init.data_ptr()) if init is not None else None, vp(fr.data_ptr()), vp(out.data_ptr()),
                                           vp(ws.data_ptr()) if ws is not None else None, n, h, w, T, R, D, *[float(c) for c in coeffs], _stream()),
               "crf_refine")
    return out


def _dev(k):
    return torch.from_numpy(k["u"].copy()).cuda(), torch.from_numpy(k["frames"].copy()).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _against_reference(c):
    """runs case c, prints the figures, asserts the bound and the decisions"""
    k = cc.case(*c)
    h, w, n, R, D, _, T = c
    u, fr = _dev(k)
    got = _refine(u, fr, k["coeffs"], T, R, D).cpu().numpy().astype(np.float64)
    diff = float(np.abs(got - k["ref"]).max())
    sure = np.abs(k["ref"]) > k["bound"]
    excluded = 1.0 - float(sure.mean())
    wrong = int(((got > 0) != (k["ref"] > 0))[sure].sum())
    print("%s: |diff| %.2e of %.2e allowed; %d wrong decisions, %.4f %% of the pixels excluded" % (cc.case_id(c), diff, k["bound"], wrong, 100 * excluded))
    assert diff <= k["bound"], diff
    assert wrong == 0 and excluded <= cc.DECISION_CAP


@pytest.mark.parametrize("c", cc.ONE_STEP_CASES, ids=cc.case_id)
def test_one_step_against_the_float64_rule(c):
    _against_reference(c)


@pytest.mark.parametrize("c", cc.FIVE_STEP_CASES, ids=cc.case_id)
def test_five_steps_against_the_float64_rule(c):
    _against_reference(c)


def test_five_steps_on_a_davis_sized_frame():
    _against_reference(cc.LARGE_CASE)


@pytest.mark.parametrize("h,w,n", cc.SIZES[:-1], ids=["%dx%dx%d" % s for s in cc.SIZES[:-1]])
def test_one_call_is_its_steps_chained_through_init(h, w, n):
    """strong weights, five steps: the ping-pong through the workspace and the last iteration's write to `out`, without a loose bound"""
    u_h, fr_h = cc.scene(h, w, n)
    u, fr = torch.from_numpy(u_h).cuda(), torch.from_numpy(fr_h).cuda()
    for R, D in cc.WINDOWS[:2] + cc.LIMIT_WINDOWS[:1]:
        coeffs = cc.coefficients(R, D, *cc.WEIGHTS["strong"])
        whole = _refine(u, fr, coeffs, 5, R, D)
        z = None
        for _ in range(5):
            z = _refine(u, fr, coeffs, 1, R, D, init=z)
        assert _same_bits(whole, z), (R, D)
        # ... and an even count, which starts the ping-pong on the other buffer; a start state that is not the unary
        z = _refine(u, fr, coeffs, 1, R, D, init=_refine(u, fr, coeffs, 1, R, D, init=-u))
        assert _same_bits(_refine(u, fr, coeffs, 2, R, D, init=-u), z), (R, D)
        if h * w > 1:
            assert not _same_bits(whole, u)


@pytest.mark.parametrize("h,w,n", cc.SIZES[:-1], ids=["%dx%dx%d" % s for s in cc.SIZES[:-1]])
def test_cases_that_must_return_their_input_bit_for_bit(h, w, n):
    u_h, fr_h = cc.scene(h, w, n)
    u_h = u_h.copy()
    u_h[0, 0, 0] = -0.0
    u, fr = torch.from_numpy(u_h).cuda(), torch.from_numpy(fr_h).cuda()
    other = torch.from_numpy(cc.scene(h, w, n, seed=1)[0]).cuda()
    strong = cc.coefficients(5, 1, *cc.WEIGHTS["strong"])
    # no iterations: the start state, with and without init
    assert _same_bits(_refine(u, fr, strong, 0, 5, 1), u) and _same_bits(_refine(u, fr, strong, 0, 5, 1, init=other), other)
    # zero weights, and no window: the unary, whatever the start state
    for T in (1, 3):
        assert _same_bits(_refine(u, fr, (0.0, 0.0) + strong[2:], T, 5, 1), u) and _same_bits(_refine(u, fr, (0.0, 0.0) + strong[2:], T, 5, 1, init=other), u)
        assert _same_bits(_refine(u, fr, strong, T, 0, 1), u) and _same_bits(_refine(u, fr, strong, T, 0, 9, init=other), u)
    if (h, w) == (1, 1):          # a frame of one pixel has no neighbour inside the image
        for R, D in cc.WINDOWS + cc.LIMIT_WINDOWS:
            assert _same_bits(_refine(u, fr, cc.coefficients(R, D, *cc.WEIGHTS["strong"]), 5, R, D, init=other), u)


@pytest.mark.parametrize("R,D", cc.WINDOWS + cc.LIMIT_WINDOWS, ids=["R%dD%d" % p for p in cc.WINDOWS + cc.LIMIT_WINDOWS])
def test_images_of_a_batch_are_independent_and_calls_repeat(R, D):
    h, w, n = 37, 53, 2
    u_h, fr_h = cc.scene(h, w, n)
    u, fr = torch.from_numpy(u_h).cuda(), torch.from_numpy(fr_h).cuda()
    coeffs = cc.coefficients(R, D, *cc.WEIGHTS["strong"])
    both = _refine(u, fr, coeffs, 3, R, D)
    assert _same_bits(both, _refine(u, fr, coeffs, 3, R, D))
    for i in range(n):
        assert _same_bits(both[i:i + 1], _refine(u[i:i + 1].contiguous(), fr[i:i + 1].contiguous(), coeffs, 3, R, D)), i
    assert not _same_bits(both[0], both[1])


@pytest.mark.parametrize("h,w,n", [(30, 85, 1), (37, 53, 2)], ids=["30x85x1", "37x53x2"])
def test_a_mirrored_input_gives_the_mirrored_output(h, w, n):
    for R, D in cc.WINDOWS:
        for ws in cc.WEIGHTS:
            k = cc.case(h, w, n, R, D, ws, 1)
            u, fr = _dev(k)
            plain = _refine(u, fr, k["coeffs"], 1, R, D)
            for axis in (1, 2):
                mirrored = _refine(u.flip(axis).contiguous(), fr.flip(axis).contiguous(), k["coeffs"], 1, R, D).flip(axis)
                diff = float((mirrored - plain).abs().max())
                print("mirror %dx%d R%dD%d %s axis %d: |diff| %.2e of %.2e allowed" % (h, w, R, D, ws, axis, diff, k["bound"]))
                assert diff <= k["bound"], (R, D, ws, axis, diff)


def test_appearance_kernel_on_a_constant_frame_is_the_smoothness_kernel():
    """dc = 0 everywhere: w_a exp(-a_s ds) alone must act as w_s exp(-g_s ds) with g_s = a_s, on any frame"""
    h, w, n = 37, 53, 2
    u_h, fr_h = cc.scene(h, w, n)
    u, fr = torch.from_numpy(u_h).cuda(), torch.from_numpy(fr_h).cuda()
    flat = torch.full_like(fr, 77)
    for R, D in cc.WINDOWS + cc.LIMIT_WINDOWS:
        w_a, _, a_s, a_c, _ = cc.coefficients(R, D, 3.0, 0.0)
        app = _refine(u, flat, (w_a, 0.0, a_s, a_c, 0.5), 1, R, D)
        smooth = _refine(u, fr, (0.0, w_a, 0.25, a_c, a_s), 1, R, D)
        bound = cc.step_bound(float(np.abs(u_h).max()), (2 * R + 1) ** 2 - 1, cc.ksum(R, D, (w_a, 0.0, a_s, a_c, 0.5)))
        diff = float((app - smooth).abs().max())
        print("constant frame R%dD%d: |diff| %.2e of %.2e allowed" % (R, D, diff, bound))
        assert diff <= bound, (R, D, diff)
        ref = cc.reference(u_h, fr_h, 1, R, D, (0.0, w_a, 0.25, a_c, a_s))
        assert float(np.abs(smooth.cpu().numpy().astype(np.float64) - ref).max()) <= bound


def test_the_workspace_needs_no_zeroing():
    h, w, n = 37, 53, 2
    u_h, fr_h = cc.scene(h, w, n)
    u, fr = torch.from_numpy(u_h).cuda(), torch.from_numpy(fr_h).cuda()
    for R, D in [(5, 1), (1, 16)]:
        coeffs = cc.coefficients(R, D, *cc.WEIGHTS["strong"])
        for T in (2, 5):
            poisoned = _refine(u, fr, coeffs, T, R, D, ws_fill=float("nan"))
            assert not bool(torch.isnan(poisoned).any()) and _same_bits(poisoned, _refine(u, fr, coeffs, T, R, D))


def test_wrappers_match_the_direct_call():
    from osvos_pytorch_amd import refine
    h, w, n = 37, 53, 2
    u_h, fr_h = cc.scene(h, w, n)
    u, fr = torch.from_numpy(u_h).cuda(), torch.from_numpy(fr_h).cuda()
    kw = dict(radius=3, dilation=2, w_appearance=6.0, w_smooth=2.0, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0)
    coeffs = cc.coefficients(3, 2, 6.0, 2.0)
    assert refine.crf_coefficients(**kw) == coeffs
    want = _refine(u, fr, coeffs, 5, 3, 2)
    got = refine.crf_refine(u, fr, iters=5, **kw)
    assert tuple(got.shape) == (n, h, w) and _same_bits(got, want)
    got4 = refine.crf_refine(u[:, None], fr, iters=5, **kw)                              # [N,1,H,W] in, [N,1,H,W] out
    assert tuple(got4.shape) == (n, 1, h, w) and _same_bits(got4[:, 0], want)
    out = torch.full((n, 1, h, w), GARBAGE, device="cuda")
    assert refine.crf_refine(u[:, None], fr, iters=5, out=out, **kw) is out and _same_bits(out[:, 0], want)
    one = refine.crf_refine(u[:1], fr[0], iters=5, **kw)                                # [H,W,3] for one image
    assert _same_bits(one, want[:1])
    r = refine.CrfRefiner(iters=5, **kw)
    assert _same_bits(r(u, fr), want) and _same_bits(r(u[:, None], fr)[:, 0], want) and _same_bits(r(u, fr), want)
    assert len(r._ws) == 1
    assert _same_bits(r(u[:1], fr[:1]), want[:1]) and len(r._ws) == 2                   # one workspace per size
    assert r(u, fr, out=out[:, 0]) is not None and _same_bits(out[:, 0], want)
    start = torch.from_numpy(cc.scene(h, w, n, seed=1)[0]).cuda()
    assert _same_bits(r(u, fr, init=start), _refine(u, fr, coeffs, 5, 3, 2, init=start))
    assert _same_bits(refine.CrfRefiner(iters=0)(u, fr), u) and _same_bits(refine.crf_refine(u, fr, iters=1, **kw), _refine(u, fr, coeffs, 1, 3, 2))
    with pytest.raises(ValueError):
        refine.crf_refine(u, fr[:1])                                                    # one frame for two maps
    with pytest.raises(ValueError):
        refine.crf_refine(u.double(), fr)
    with pytest.raises(ValueError):
        refine.crf_refine(u, fr.float())
    with pytest.raises(ValueError):
        refine.crf_refine(u, fr, out=u)
    with pytest.raises(ValueError):
        refine.crf_refine(u, fr, init=u[:1])


def _train_online(tmp, *extra):
    r = script_runner.train_online(tmp, *extra, frames=1)
    return r.stdout, r.masks[0]


def test_train_online_with_refinement(tmp_path):
    out, refined = _train_online(tmp_path / "on", "--device-augment", "--crf-iters", "3")
    assert "Online training time" in out and "J&F on blackswan:" in out, out[-2000:]
    # --crf-iters 0 is the loop without the option: the same bytes on disk
    _, off = _train_online(tmp_path / "off", "--device-augment", "--crf-iters", "0")
    _, plain = _train_online(tmp_path / "plain", "--device-augment")
    assert off == plain


def test_train_online_multi_object_with_refinement(tmp_path):
    """every object's logit stack refined against the stacked frames before the merge.  (No byte comparison of --crf-iters 0 against a run
    without the option here: two runs of the --multi-object loop WITHOUT any --crf option do not write the same label map -- measured on an
    MI355X, one label byte apart after five epochs -- so such a comparison would test that loop's repeatability, not this option.)"""
    out, _ = _train_online(tmp_path / "on", "--multi-object", "--crf-iters", "3")
    assert "J&F on blackswan (2 objects):" in out and "J&F on blackswan object 2:" in out, out[-2000:]
