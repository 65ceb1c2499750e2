"""TEST INFRASTRUCTURE: the CPU reference of the test-time augmentation kernels (csrc/tta.hip), shared by test_tta_cpu.py and
test_gpu_tta.py.  It restates the sampling rule of include/osvos_hip.h in numpy float64 -- integer taps, x pass then y pass, a tap of weight
zero selected away -- and the two calls built on it."""
import numpy as np

MEANVAL = (104.00699, 116.66877, 122.67892)
FRAME_SIZES = [(16, 16, 1), (30, 85, 1), (37, 53, 2), (48, 64, 1), (480, 854, 1)]          # (H, W, N)
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5)
VIEW_BOUND = 16 * 2.0 ** -24 * 256          # osvos_tta_view against view_reference (values below 256, at most eight fp32 roundings, doubled)


def fuse_bound(n_views, largest):
    """osvos_tta_fuse against fuse_reference: at most 8 roundings per sample and 2 per accumulated view of magnitude <= largest, doubled"""
    return (8 + 2 * n_views) * 2.0 ** -23 * largest


def taps(n_dst, n_src):
    """(i0, i1, f) for every destination index: f is the weight of i1"""
    i = np.arange(n_dst, dtype=np.int64)
    num = np.maximum((2 * i + 1) * n_src - n_dst, 0)
    den = 2 * n_dst
    i0 = np.minimum(num // den, n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, (num % den).astype(np.float64) / float(den)


def _lerp(a, b, f):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(f == 0, a, (1.0 - f) * a + f * b)


def resize(a, h, w):
    """a [..., hs, ws] -> float64 [..., h, w]"""
    a = np.asarray(a, dtype=np.float64)
    x0, x1, fx = taps(w, a.shape[-1])
    r = _lerp(a[..., x0], a[..., x1], fx)
    y0, y1, fy = taps(h, a.shape[-2])
    return _lerp(r[..., y0, :], r[..., y1, :], fy[:, None])


def view_reference(frames_u8, hv, wv, flip=False, meanval=MEANVAL):
    """uint8 [N,H,W,3] -> float64 [N,3,hv,wv] (the mean as the fp32 values the C ABI receives)"""
    a = np.asarray(frames_u8).transpose(0, 3, 1, 2)
    mean = np.asarray(meanval, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    r = resize(a, hv, wv) - mean
    return r[..., ::-1].copy() if flip else r


def fuse_reference(views, flips, size, weights=None):
    """views: V arrays [N,hv,wv]; -> float64 [N,H,W]"""
    h, w = size
    if weights is None:
        weights = [1.0 / len(views)] * len(views)
    out = 0.0
    for v, f, wt in zip(views, flips, weights):
        v = np.asarray(v, dtype=np.float64)
        out = out + float(wt) * resize(v[..., ::-1] if f else v, h, w)
    return out


def frames(h, w, n, seed=0):
    """seeded random uint8 frames [n,h,w,3]"""
    return np.random.default_rng(7000 + seed + 131 * h + w).integers(0, 256, size=(n, h, w, 3)).astype(np.uint8)


def logits(n, h, w, seed=0):
    """seeded float32 logits in [-20, 20], [n,h,w]"""
    return np.random.default_rng(9000 + seed + 131 * h + w).uniform(-20.0, 20.0, size=(n, h, w)).astype(np.float32)


def view_size(h, w, s):
    return max(1, int(np.floor(h * s + 0.5))), max(1, int(np.floor(w * s + 0.5)))
