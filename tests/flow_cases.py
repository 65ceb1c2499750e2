"""Numpy restatement of the motion-compensation rule of include/osvos_hip.h (luma, block matcher, median passes, integer warp), the cases
the CPU and the GPU tests share, and seeded scenes.  Everything is integer arithmetic: the tests compare with np.array_equal.

The matcher follows the rule literally, not the kernel: both luma planes are edge-padded once (clamp(p) and clamp(p + d) depend on the
absolute coordinate alone), every candidate gets ONE absolute-difference image over the span of all blocks, the block sums come from its
prefix sums (an integral image taken separably: along x, read at the blocks' left and right edges, then along y, read at their top and
bottom edges), and the candidates are visited in the order (dx^2 + dy^2, dy, dx) with a strict `<`, so the first of equal costs wins.
"""
import numpy as np

# (H, W, N, block, step, search, penalty, median)
MATCH_CASES = [
    (37, 53, 2, 8, 4, 5, 0, 0),
    (45, 70, 1, 16, 4, 9, 3, 1),
    (16, 16, 1, 16, 8, 3, 0, 2),
    (5, 3, 1, 8, 4, 2, 1, 1),            # the frame is smaller than the block
    (1, 1, 1, 4, 1, 2, 0, 0),
    (33, 65, 1, 7, 5, 6, 2, 1),          # odd block, odd step
    (24, 40, 1, 32, 32, 48, 0, 0),       # every limit reached, the search exceeds the frame
    (40, 64, 3, 4, 1, 3, 0, 0),          # step 1
]
LARGE_CASE = (480, 854, 1, 16, 4, 24, 4, 1)
SCENES = ("noise", "constant", "periodic", "gradient")
DEFAULTS = dict(search=24, block=16, step=4, penalty=4, median=1)


def case_id(c):
    return "%dx%dx%d_B%d_S%d_R%d_P%d_M%d" % tuple(c)


def grid_shape(h, w, step):
    return -(-h // step), -(-w // step)


def luma(bgr):
    """uint8 [...,3] BGR -> uint8 [...]"""
    c = bgr.astype(np.int32)
    return ((29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8).astype(np.uint8)


def candidates(search):
    """the (dx, dy) of the search window in the order (dx^2 + dy^2, dy, dx)"""
    r = range(-search, search + 1)
    return sorted(((dx, dy) for dy in r for dx in r), key=lambda d: (d[0] * d[0] + d[1] * d[1], d[1], d[0]))


def _match_one(yp, yc, block, step, search, penalty):
    h, w = yc.shape
    gh, gw = grid_shape(h, w, step)
    off = (step - block) // 2
    y0, x0 = min(off, 0), min(off, 0)                                        # the span of all block pixels, frame included
    y1, x1 = max(h, (gh - 1) * step + off + block), max(w, (gw - 1) * step + off + block)
    cur = np.pad(yc, ((-y0, y1 - h), (-x0, x1 - w)), mode="edge").astype(np.int16)
    prev = np.pad(yp, ((search - y0, y1 - h + search), (search - x0, x1 - w + search)), mode="edge").astype(np.int16)
    top = np.arange(gh) * step + off - y0                                    # block corners in span coordinates
    left = np.arange(gw) * step + off - x0
    eh, ew = y1 - y0, x1 - x0
    best = np.full((gh, gw), np.iinfo(np.int64).max, dtype=np.int64)
    vec = np.zeros((gh, gw, 2), dtype=np.int32)
    rows = np.zeros((eh + 1, gw), dtype=np.int32)
    for dx, dy in candidates(search):
        ad = np.abs(cur - prev[search + dy:search + dy + eh, search + dx:search + dx + ew])
        px = np.zeros((eh, ew + 1), dtype=np.int32)
        np.cumsum(ad, axis=1, dtype=np.int32, out=px[:, 1:])
        np.cumsum(px[:, left + block] - px[:, left], axis=0, out=rows[1:])
        c = (rows[top + block] - rows[top]).astype(np.int64) + penalty * (abs(dx) + abs(dy))
        better = c < best
        best[better] = c[better]
        vec[better] = (dx, dy)
    return vec, best.astype(np.int32)


def median_pass(vec):
    """one pass over [..., GH, GW, 2]: each component's median over the 3 x 3 grid neighbourhood, indices clamped"""
    gh, gw = vec.shape[-3], vec.shape[-2]
    pad = [(0, 0)] * (vec.ndim - 3) + [(1, 1), (1, 1), (0, 0)]
    p = np.pad(vec, pad, mode="edge")
    stack = np.stack([p[..., a:a + gh, b:b + gw, :] for a in range(3) for b in range(3)])
    return np.sort(stack, axis=0)[4].astype(np.int32)


def block_match(prev_bgr, cur_bgr, search=24, block=16, step=4, penalty=4, median=1):
    """uint8 [N,H,W,3] twice -> (vec int32 [N,GH,GW,2] = (dx, dy), cost int32 [N,GH,GW])"""
    yp, yc = luma(prev_bgr), luma(cur_bgr)
    out = [_match_one(yp[n], yc[n], block, step, search, penalty) for n in range(yc.shape[0])]
    vec, cost = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    for _ in range(median):
        vec = median_pass(vec)
    return vec, cost


def block_match_naive(prev_bgr, cur_bgr, search, block, step, penalty):
    """the rule as loops over cells, candidates and pixels (tiny frames only); no median"""
    yp, yc = luma(prev_bgr).astype(int), luma(cur_bgr).astype(int)
    n, h, w = yc.shape
    gh, gw = grid_shape(h, w, step)
    off = (step - block) // 2
    vec, cost = np.zeros((n, gh, gw, 2), np.int32), np.zeros((n, gh, gw), np.int32)
    cl = lambda v, hi: min(max(v, 0), hi - 1)
    for f in range(n):
        for i in range(gh):
            for j in range(gw):
                best = None
                for dy in range(-search, search + 1):
                    for dx in range(-search, search + 1):
                        c = penalty * (abs(dx) + abs(dy))
                        for y in range(i * step + off, i * step + off + block):
                            for x in range(j * step + off, j * step + off + block):
                                c += abs(yc[f, cl(y, h), cl(x, w)] - yp[f, cl(y + dy, h), cl(x + dx, w)])
                        key = (c, dx * dx + dy * dy, dy, dx)
                        if best is None or key < best:
                            best = key
                vec[f, i, j], cost[f, i, j] = (best[3], best[2]), best[0]
    return vec, cost


def warp(src, vec, step, fill=0):
    """src [N,H,W] of any dtype, vec int [N,GH,GW,2] -> out(n, y, x) = src(n, y + dy, x + dx) of the pixel's cell, fill outside the frame.
    float32 goes through its bits."""
    if src.dtype == np.float32:
        return warp(src.view(np.uint32), vec, step, np.float32(fill).view(np.uint32)).view(np.float32)
    n, h, w = src.shape
    gh, gw = vec.shape[1:3]
    ci, cj = np.minimum(np.arange(h) // step, gh - 1), np.minimum(np.arange(w) // step, gw - 1)
    d = vec[:, ci][:, :, cj].astype(np.int64)                                 # [N,H,W,2]
    sx, sy = np.arange(w)[None, None, :] + d[..., 0], np.arange(h)[None, :, None] + d[..., 1]
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.full(src.shape, fill, dtype=src.dtype)
    nn = np.broadcast_to(np.arange(n)[:, None, None], src.shape)
    out[inside] = src[nn[inside], sy[inside], sx[inside]]
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

def shift_of(search):
    """the displacement of the 'noise' and 'gradient' scenes of a case: inside the search window, not on an axis when it can be helped"""
    return min(search, 5), -min(search, 2)


def pair(kind, h, w, n, search, seed=0):
    """-> (prev, cur) uint8 [N,H,W,3].  'noise': crops of one larger noise image, cur(p) = prev(p + shift_of(search)) wherever p + shift is
    inside the frame; 'constant': one colour; 'periodic': a texture of period 2 x 2 (below every search range from 3 on) against itself;
    'gradient': a smooth ramp and the same ramp displaced -- many near-ties"""
    rng = np.random.default_rng([seed, h, w, n, search, SCENES.index(kind)])
    dx, dy = shift_of(search)
    m = max(abs(dx), abs(dy))
    if kind == "noise":
        big = rng.integers(0, 256, size=(n, h + 2 * m, w + 2 * m, 3), dtype=np.uint8)
        return big[:, m:m + h, m:m + w].copy(), big[:, m + dy:m + dy + h, m + dx:m + dx + w].copy()
    if kind == "constant":
        f = np.empty((n, h, w, 3), np.uint8)
        f[...] = rng.integers(0, 256, size=(n, 1, 1, 3), dtype=np.uint8)
        return f, f.copy()
    yy, xx = np.meshgrid(np.arange(h + 2 * m), np.arange(w + 2 * m), indexing="ij")
    if kind == "periodic":
        tile = rng.integers(0, 256, size=(n, 2, 2, 3), dtype=np.uint8)
        f = tile[:, yy[:h, :w] % 2, xx[:h, :w] % 2]
        return f.copy(), f.copy()
    if kind == "gradient":
        ramp = np.stack([(3 * xx + 2 * yy) // 4 % 256, (xx + 5 * yy) // 3 % 256, (2 * xx + yy) // 5 % 256], axis=-1).astype(np.uint8)
        big = np.broadcast_to(ramp, (n,) + ramp.shape)
        return big[:, m:m + h, m:m + w].copy(), big[:, m + dy:m + dy + h, m + dx:m + dx + w].copy()
    raise ValueError(kind)


_cache = {}


def reference(kind, c):
    """-> dict(prev, cur, vec, cost) of scene `kind` under case c; computed once per process, never modified"""
    key = (kind,) + tuple(c)
    if key not in _cache:
        h, w, n, block, step, search, penalty, median = c
        prev, cur = pair(kind, h, w, n, search)
        vec, cost = block_match(prev, cur, search, block, step, penalty, median)
        for a in (prev, cur, vec, cost):
            a.setflags(write=False)
        _cache[key] = dict(prev=prev, cur=cur, vec=vec, cost=cost)
    return _cache[key]


def border_field(h, w, step, n=1):
    """a hand-made vector grid that pushes sources out of every border, by little and by much, next to cells that stay inside"""
    gh, gw = grid_shape(h, w, step)
    vec = np.zeros((n, gh, gw, 2), np.int32)
    vec[:, 0, :, 1] = -3                     # top row of cells reads above the frame
    vec[:, -1, :, 1] = 2 * h                 # bottom row far below
    vec[:, :, 0, 0] = -w - 7                 # left column far left
    vec[:, :, -1, 0] = 1                     # right column one pixel out at the last column only
    if gh > 2 and gw > 2:
        vec[:, 1:-1, 1:-1, 0] = (np.arange(gw - 2) % 5 - 2)[None, None, :]
        vec[:, 1:-1, 1:-1, 1] = (np.arange(gh - 2) % 3 - 1)[None, :, None]
    return vec


# ---- the tracking scenario ------------------------------------------------------------------------------------------------------------

TRACK = dict(h=72, w=200, frames=5, size=24, speed=32, x0=6, y0=10, radius=2, search=40, block=16, step=4, penalty=4, median=1,
             distractor=(52, 150, 12))       # its top, left and side: static, far from the object's path


def tracking_scene(seed=3):
    """-> (frames uint8 [T,H,W,3], object masks bool [T,H,W], distractor mask bool [H,W]): a textured square that moves TRACK['speed']
    pixels per frame over a static textured background, and a static blob the network is imagined to mistake for the object"""
    t = TRACK
    rng = np.random.default_rng(seed)
    back = rng.integers(0, 256, size=(t["h"], t["w"], 3), dtype=np.uint8)
    obj = rng.integers(0, 256, size=(t["size"], t["size"], 3), dtype=np.uint8)
    frames = np.repeat(back[None], t["frames"], axis=0)
    masks = np.zeros((t["frames"], t["h"], t["w"]), bool)
    for f in range(t["frames"]):
        x = t["x0"] + f * t["speed"]
        frames[f, t["y0"]:t["y0"] + t["size"], x:x + t["size"]] = obj
        masks[f, t["y0"]:t["y0"] + t["size"], x:x + t["size"]] = True
    top, left, side = t["distractor"]
    blob = np.zeros((t["h"], t["w"]), bool)
    blob[top:top + side, left:left + side] = True
    return frames, masks, blob


def tracking_logits(masks, blob):
    """float32 [T,1,H,W]: +5 on the object and on the distractor, -5 elsewhere"""
    return np.where(masks | blob[None], 5.0, -5.0).astype(np.float32)[:, None]


def dilate(mask, radius):
    """bool [H,W] grown by a disk of `radius` pixels"""
    h, w = mask.shape
    out = np.zeros_like(mask)
    p = np.pad(mask, radius)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dx * dx + dy * dy <= radius * radius:
                out |= p[radius + dy:radius + dy + h, radius + dx:radius + dx + w]
    return out
