"""TEST INFRASTRUCTURE: the CPU reference of the mask refinement (csrc/crf.hip), shared by test_crf_cpu.py and test_gpu_crf.py.  It
restates the rule of include/osvos_hip.h in numpy float64 -- the mean field of a two-label Potts CRF over a dilated window, in logit form --
with the seeded scenes, the windows, the weight sets and the error bounds the tests use.  The reference has no counterpart of this step, so
this restatement is the yardstick; test_crf_cpu.py pins it against two independent formulations."""
import functools

import numpy as np

SIZES = [(1, 1, 1), (3, 40, 1), (16, 16, 1), (30, 85, 1), (37, 53, 2), (48, 64, 1), (480, 854, 1)]          # (H, W, N)
WINDOWS = [(5, 1), (3, 2), (2, 4)]                   # (radius, dilation)
LIMIT_WINDOWS = [(7, 2), (1, 16)]                    # the largest radius, the largest reach
WEIGHTS = {"contractive": (1.5, 0.5), "strong": (6.0, 2.0)}          # (w_appearance, w_smooth), normalised
THETA_BETA = 13.0
DECISION_CAP = 0.005                                 # share of a case's pixels that may lie within the bound of the threshold


def offsets(R, D):
    """the (2R+1)^2 - 1 window offsets (oy, ox) in pixels, row by row"""
    return [(dy * D, dx * D) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dy, dx) != (0, 0)]


def coefficients(R, D, w_appearance, w_smooth, theta_alpha=None, theta_beta=THETA_BETA, theta_gamma=None, normalize=True):
    """(w_a, w_s, a_s, a_c, g_s) as fp32 values: the tests' theta_alpha = 4 D, theta_gamma = 1.5 D unless given.  An independent restatement of
    osvos_pytorch_amd.refine.crf_coefficients (test_crf_cpu.py compares the two)."""
    ta = 4.0 * D if theta_alpha is None else theta_alpha
    tg = 1.5 * D if theta_gamma is None else theta_gamma
    a_s, a_c, g_s = [float(np.float32(1.0 / (2.0 * t * t))) for t in (ta, theta_beta, tg)]
    w_a, w_s = float(w_appearance), float(w_smooth)
    if normalize and R > 0:
        ds = np.array([oy * oy + ox * ox for oy, ox in offsets(R, D)], dtype=np.float64)
        w_a, w_s = w_a / np.exp(-a_s * ds).sum(), w_s / np.exp(-g_s * ds).sum()
    return tuple(float(np.float32(v)) for v in (w_a, w_s, a_s, a_c, g_s))


def ksum(R, D, coeffs):
    """w_a sum_d exp(-a_s ds) + w_s sum_d exp(-g_s ds): the exact upper bound on sum_j k(i, j) (dc = 0, every neighbour inside)"""
    w_a, w_s, a_s, _, g_s = [float(c) for c in coeffs]
    ds = np.array([oy * oy + ox * ox for oy, ox in offsets(R, D)], dtype=np.float64)
    return float(w_a * np.exp(-a_s * ds).sum() + w_s * np.exp(-g_s * ds).sum()) if ds.size else 0.0


def reference(u, frames, T, R, D, coeffs, init=None):
    """u [N,H,W] logits, frames [N,H,W,3] uint8, coeffs the five fp32 values (widened to float64) -> z^T float64 [N,H,W].  Vectorised per
    offset: a neighbour outside the image is simply not in the overlap of the shifted slices."""
    u = np.asarray(u, dtype=np.float64)
    w_a, w_s, a_s, a_c, g_s = [float(np.float32(c)) for c in coeffs]
    col = np.asarray(frames).astype(np.int64)
    N, H, W = u.shape
    assert col.shape == (N, H, W, 3)
    z = u.copy() if init is None else np.asarray(init, dtype=np.float64).reshape(u.shape).copy()
    for _ in range(T):
        s = 2.0 / (1.0 + np.exp(-z)) - 1.0
        acc = np.zeros_like(u)
        for oy, ox in offsets(R, D):
            y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            here = (slice(None), slice(y0, y1), slice(x0, x1))
            there = (slice(None), slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            dc = ((col[here] - col[there]) ** 2).sum(-1).astype(np.float64)
            ds = float(oy * oy + ox * ox)
            acc[here] += (w_a * np.exp(-(a_s * ds + a_c * dc)) + w_s * np.exp(-g_s * ds)) * s[there]
        z = u + acc
    return z


def step_bound(umax, M, ks):
    """|kernel - reference| after ONE step from the same state, in units of eps = 2^-24 (half an fp32 ulp of a value in [1, 2)):

        2^-24 (2 umax + (2 M + 28) ksum),   M = (2R+1)^2 - 1 neighbours, ksum >= sum_j k(i, j)

    Per neighbour, k carries at most 8 eps of relative error: the exponent argument two roundings, the exp, the scale by the spatial factor
    and the addition of the smoothness term.  (csrc/crf.hip evaluates exp2(c2 dc) with the hardware exponential, 1 ulp, on an argument whose
    two roundings cost a RELATIVE error of 2 x eps at x = a_c dc; on a term of size A e^-x that is at most 2 x e^-x <= 0.74 eps of A, and
    the A sum to at most ksum -- inside the 8 eps ksum allotted, so the constant is NOT widened.)  s = 2 sigmoid(z) - 1, |s| <= 1, carries at
    most 4 eps (exp, two additions, division), the product k s one more: 13 eps ksum over the sum.  Each of the M accumulations rounds a
    partial sum of magnitude <= ksum: M eps ksum.  The final u + sum rounds a value of magnitude <= umax + ksum.  That is
    eps (umax + (M + 14) ksum); the bound is twice it."""
    return 2.0 ** -24 * (2.0 * umax + (2.0 * M + 28.0) * ks)


def steps_bound(umax, M, ks, T):
    """T steps: step_bound sum_{t<T} G^t with G = max(1, ksum / 2) -- an error e in z becomes at most e / 2 in s (|ds/dz| <= 1/2) and so at
    most e ksum / 2 in the next z, on top of that step's own error"""
    G = max(1.0, ks / 2.0)
    return step_bound(umax, M, ks) * sum(G ** t for t in range(T))


def scene(h, w, n, seed=0):
    """seeded (logits float32 [n,h,w], frames uint8 [n,h,w,3]): +-2 inside / outside an ellipse plus N(0, 3) noise; two distinct BGR colours
    inside / outside plus uniform noise of +-20, clipped.  (The seed base is a choice made on the REFERENCE alone: in a 120-pixel case one
    pixel is 0.83 % of the case, so a draw that puts one refined logit within 1e-4 of zero -- base 4000 did, at 3x40 -- cannot meet the 0.5 %
    decision cap whatever the kernel does; test_crf_cpu.py checks the cap on every case.)"""
    rng = np.random.default_rng(5000 + seed + 131 * h + w)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u = np.empty((n, h, w), np.float32)
    fr = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        cy, cx = 0.5 * (h - 1) + 0.1 * h * i, 0.45 * (w - 1)
        inside = ((yy - cy) / max(0.3 * h, 0.6)) ** 2 + ((xx - cx) / max(0.3 * w, 0.6)) ** 2 <= 1.0
        u[i] = (np.where(inside, 2.0, -2.0) + rng.normal(0.0, 3.0, size=(h, w))).astype(np.float32)
        base = np.where(inside[..., None], np.array([40, 160, 220]), np.array([200, 90, 30]))
        fr[i] = np.clip(base + rng.integers(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)
    return u, fr


@functools.lru_cache(maxsize=None)
def case(h, w, n, R, D, weights, T):
    """one seeded case with its reference, computed once per process and shared (treat the arrays as read-only):
    dict(u, frames, coeffs, ref, bound, M, ksum)"""
    u, fr = scene(h, w, n)
    coeffs = coefficients(R, D, *WEIGHTS[weights])
    ks, M = ksum(R, D, coeffs), (2 * R + 1) ** 2 - 1
    ref = reference(u, fr, T, R, D, coeffs)
    for a in (u, fr, ref):
        a.setflags(write=False)
    return dict(u=u, frames=fr, coeffs=coeffs, ref=ref, M=M, ksum=ks, bound=steps_bound(float(np.abs(u).max()), M, ks, T))


ONE_STEP_CASES = [(h, w, n, R, D, ws, 1) for (h, w, n) in SIZES for (R, D) in WINDOWS for ws in ("contractive", "strong")]
FIVE_STEP_CASES = ([(h, w, n, R, D, "contractive", 5) for (h, w, n) in SIZES[:-1] for (R, D) in WINDOWS[:1]]
                   + [(37, 53, 2, R, D, "contractive", 5) for (R, D) in WINDOWS[1:] + LIMIT_WINDOWS])
LARGE_CASE = (480, 854, 1, 5, 3, "contractive", 5)


def case_id(c):
    return "%dx%dx%d-R%dD%d-%s-T%d" % c
