"""The memory bank of appearance matching (osvos_match_bank_update, csrc/match_bank.hip; the rule: include/osvos_hip.h) restated in numpy -- a plain
per-row loop and a vectorised form -- with the case list and the seeded operands shared by tests/test_match_bank_cpu.py and
tests/test_gpu_match_bank.py.  The rows are made as tests/match_cases.py makes its own: awkward float features through the quantiser.

The rule is integer arithmetic, copies and single float32 comparisons (one float32 subtraction for the margin): the device is compared bit
for bit."""
import functools

import numpy as np

import match_cases as mc

F32 = np.float32
VOID = 255
MAX_P = 1 << 20

# ---------------------------------------------------------------------------------------------------------------- the restatement


def select(rinv_q, label_q, sim, tau, margin):
    """rinv_q float32 [P], label_q uint8 [P], sim float32 [2, P] (foreground first) -> bool [P]: the label is 0 or 1, rinv_q > 0, own < tau and
    fl32(own - other) >= margin.  Comparisons with a NaN are false"""
    fg = np.asarray(label_q) == 1
    sim = np.asarray(sim, F32)
    own, other = np.where(fg, sim[0], sim[1]), np.where(fg, sim[1], sim[0])
    with np.errstate(invalid="ignore"):
        gap = (own - other).astype(F32)
        return (np.asarray(label_q) <= 1) & (np.asarray(rinv_q, F32) > 0) & (own < F32(tau)) & (gap >= F32(margin))


def subsample(n, m):
    """-> (kept bool [n], j int64 [n]): rank r is kept iff floor((r + 1) m / n) > floor(r m / n), as kept row j = floor(r m / n)"""
    r = np.arange(n, dtype=np.int64)
    if n == 0:
        return np.zeros(0, bool), r
    j = r * m // n
    return (r + 1) * m // n > j, j


def update(q, rinv_q, label_q, sim, R, rinv_r, label_r, state, protected, max_new, tau, margin):
    """ONE bank (no leading N): -> new (R, rinv_r, label_r, state); the inputs are left alone.  Vectorised"""
    R, rinv_r, label_r, state = np.array(R), np.array(rinv_r), np.array(label_r), np.array(state, np.int32)
    cap = R.shape[0]
    ring = cap - protected
    rows = np.flatnonzero(select(rinv_q, label_q, sim, tau, margin))
    n = rows.size
    m = min(n, max_new, ring)
    cursor, filled, calls, _ = (int(v) for v in state)
    if m > 0:
        kept, j = subsample(n, m)
        slots = protected + (cursor + j[kept]) % ring
        assert np.unique(slots).size == m
        R[slots], rinv_r[slots], label_r[slots] = q[rows[kept]], rinv_q[rows[kept]], label_q[rows[kept]]
        cursor, filled = (cursor + m) % ring, min(filled + m, ring)
    return R, rinv_r, label_r, np.array([cursor, filled, calls + 1, m], np.int32)


def update_loop(q, rinv_q, label_q, sim, R, rinv_r, label_r, state, protected, max_new, tau, margin):
    """the same as the rule reads: one row at a time, Python integers, numpy float32 scalars"""
    R, rinv_r, label_r = np.array(R), np.array(rinv_r), np.array(label_r)
    cap, P = R.shape[0], q.shape[0]
    ring = cap - protected
    chosen = []
    for a in range(P):
        l = int(label_q[a])
        if l not in (0, 1):
            continue
        own, other = (F32(sim[0][a]), F32(sim[1][a])) if l == 1 else (F32(sim[1][a]), F32(sim[0][a]))
        with np.errstate(invalid="ignore"):
            if F32(rinv_q[a]) > F32(0) and own < F32(tau) and F32(own - other) >= F32(margin):
                chosen.append(a)
    n = len(chosen)
    m = min(n, max_new, ring)
    cursor, filled, calls, _ = (int(v) for v in state)
    for r, a in enumerate(chosen):
        if m > 0 and ((r + 1) * m) // n > (r * m) // n:
            slot = protected + (cursor + (r * m) // n) % ring
            R[slot], rinv_r[slot], label_r[slot] = q[a], rinv_q[a], label_q[a]
    if m > 0:
        cursor, filled = (cursor + m) % ring, min(filled + m, ring)
    return R, rinv_r, label_r, np.array([cursor, filled, calls + 1, m], np.int32)


def bound_rows(protected, ring, max_new, calls):
    """the host's bound on the rows written after `calls` updates (osvos_pytorch_amd.match.MemoryBank.rows)"""
    return protected + min(ring, calls * min(max_new, ring))


# ---------------------------------------------------------------------------------------------------------------- the operands


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def frame(p, c, seed=0, awkward=True, every=False):
    """the rows of one searched frame: q int8 [p, c] and rinv_q [p] from match_cases' awkward features (rows with rinv_q = 0 among them when p
    allows), label_q of every kind, and a sim [2, p] of cosines in [-1, 1] with, when `awkward`, -2 for an empty class and NaNs planted.
    `every`: a frame of which tau = 2, margin = -4 select EVERY row (n = P: every ballot is full) -- seeded int8 rows with a nonzero
    component, so rinv_q > 0 by the quantiser's rule, every label 0 or 1, every sim finite"""
    rng = np.random.default_rng([p, c, seed, 77])
    if every:
        q = rng.integers(-127, 128, size=(p, c)).astype(np.int8)
        q[:, seed % c] = 127
        n = (q.astype(np.int32) ** 2).sum(axis=1, dtype=np.int32)
        rinv_q = (F32(1.0) / np.sqrt(n.astype(F32))).astype(F32)
        label_q = rng.integers(0, 2, size=p).astype(np.uint8)
        return _freeze(dict(q=q, rinv_q=rinv_q, label_q=label_q, sim=rng.uniform(-1, 1, size=(2, p)).astype(F32)))
    q, rinv_q = mc.quantize(mc.features("relu" if seed % 2 == 0 else "signed", p, c, seed))
    label_q = rng.choice(np.array([1, 0, VOID, 7], np.uint8), size=p, p=[0.35, 0.4, 0.2, 0.05])
    sim = rng.uniform(-1, 1, size=(2, p)).astype(F32)
    if awkward:
        sim[0, rng.random(p) < 0.05] = F32(-2.0)
        sim[1, rng.random(p) < 0.05] = F32(-2.0)
        sim[0, rng.random(p) < 0.03] = np.nan
        sim[1, rng.random(p) < 0.03] = np.nan
        sim[:, rng.random(p) < 0.02] = np.nan
    return _freeze(dict(q=q, rinv_q=rinv_q, label_q=label_q, sim=sim))


@functools.lru_cache(maxsize=None)
def bank(cap, c, protected, seed=0, calls=3):
    """a bank full of a known pattern (so that "no other byte changes" can be seen) with a valid, non-zero state"""
    rng = np.random.default_rng([cap, c, protected, seed, 78])
    ring = cap - protected
    R = rng.integers(-127, 128, size=(cap, c)).astype(np.int8)
    rinv_r = rng.uniform(0.001, 0.1, size=cap).astype(F32)
    label_r = rng.choice(np.array([1, 0, VOID], np.uint8), size=cap)
    cursor = int(rng.integers(0, ring)) if ring else 0
    state = np.array([cursor, min(ring, cursor + 2), calls, 1], np.int32)
    return _freeze(dict(R=R, rinv_r=rinv_r, label_r=label_r, state=state))


# name -> dict(P, C, cap, protected, max_new, tau, margin[, every]); max_new "n" / "n-1" / "n+1": relative to the rows the restatement selects;
# every: frame(every=True), so that with ALL n = P
ALL = dict(tau=2.0, margin=-4.0)          # every labelled row with rinv_q > 0 and no NaN is selected
CASES = {
    "every_row_of_one": dict(P=1, C=64, cap=8, protected=3, max_new=4, every=True, **ALL),
    "every_row_of_a_wave": dict(P=64, C=128, cap=200, protected=40, max_new="n", every=True, **ALL),
    "every_row_of_a_workgroup": dict(P=256, C=64, cap=400, protected=40, max_new=300, every=True, **ALL),
    "every_row_with_a_tail": dict(P=4099, C=64, cap=9000, protected=100, max_new=1 << 20, every=True, **ALL),
    "every_row_subsampled": dict(P=4099, C=128, cap=6000, protected=4099, max_new=1000, every=True, **ALL),
    "one_row": dict(P=1, C=64, cap=8, protected=3, max_new=4, **ALL),
    "partial_wave": dict(P=63, C=64, cap=200, protected=40, max_new="n-1", **ALL),
    "one_wave": dict(P=64, C=128, cap=200, protected=40, max_new="n", **ALL),
    "wave_and_one": dict(P=65, C=64, cap=200, protected=40, max_new="n+1", **ALL),
    "several_workgroups": dict(P=1000, C=128, cap=1500, protected=1000, max_new=137, tau=0.3, margin=-0.5),
    "tail": dict(P=4099, C=64, cap=6000, protected=4099, max_new=512, tau=0.5, margin=0.0),
    "tail_all_rows": dict(P=4099, C=64, cap=9000, protected=100, max_new=1 << 20, **ALL),
    "most_channels": dict(P=300, C=1024, cap=400, protected=150, max_new=100, tau=0.9, margin=-0.25),
    "nothing_novel": dict(P=1000, C=64, cap=1500, protected=500, max_new=512, tau=-3.0, margin=-4.0),
    "max_new_zero": dict(P=1000, C=64, cap=1500, protected=500, max_new=0, **ALL),
    "ring_smaller_than_m": dict(P=1000, C=64, cap=505, protected=500, max_new=512, **ALL),
    "ring_of_one": dict(P=65, C=64, cap=41, protected=40, max_new=3, **ALL),
    "no_ring": dict(P=1000, C=64, cap=500, protected=500, max_new=512, **ALL),
    "nothing_protected": dict(P=1000, C=128, cap=700, protected=0, max_new=300, tau=0.6, margin=-1.0),
}


@functools.lru_cache(maxsize=None)
def problem(name, seed=0):
    """the operands of case `name` with the restatement's answer, computed once and read-only -> dict(q, rinv_q, label_q, sim, R, rinv_r,
    label_r, state, n, and the arguments with max_new resolved, out = (R, rinv_r, label_r, state) after the call)"""
    c = dict(CASES[name])
    f = frame(c["P"], c["C"], seed, every=c.pop("every", False))
    b = bank(c["cap"], c["C"], c["protected"], seed)
    n = int(select(f["rinv_q"], f["label_q"], f["sim"], c["tau"], c["margin"]).sum())
    if isinstance(c["max_new"], str):
        c["max_new"] = max(n + {"n": 0, "n-1": -1, "n+1": 1}[c["max_new"]], 0)
    out = update(f["q"], f["rinv_q"], f["label_q"], f["sim"], b["R"], b["rinv_r"], b["label_r"], b["state"], c["protected"], c["max_new"], c["tau"],
                 c["margin"])
    for v in out:
        v.setflags(write=False)
    return dict(f, **b, n=n, args=c, out=out)


# the chain: five frames into a ring of 100 rows, 50 rows at a time -- the cursor passes the end of the ring twice
CHAIN = dict(P=300, C=64, cap=130, protected=30, max_new=50, frames=5, **ALL)


# ---------------------------------------------------------------------------------------------------------------- the matcher's sequence

SEQ = dict(H=48, W=64, stride=8, C=64, frames=4, gain=1.5, memory=40, memory_new=12, tau=0.97, margin=-0.05, seed=11)


@functools.lru_cache(maxsize=None)
def sequence():
    """What a stand-in network plants: per frame the five logit maps [1, 1, H, W] and the features [1, h, w, C] of a slowly changing scene (a
    frame's features are the previous frame's plus noise, so some rows are novel and some are not), the annotation of frame 0 and the masks
    handed over after frames 1 and 2.  With it the restatement's banks, sims and maps for the matcher with memory: before frame t >= 2 is
    searched, the bank takes frame t - 1 in."""
    s = SEQ
    H, W, S, C = s["H"], s["W"], s["stride"], s["C"]
    h, w = mc.grid_shape(H, W, S)
    p = h * w
    rng = np.random.default_rng(s["seed"])
    feats = [np.maximum(rng.standard_normal((h, w, C)), 0).astype(F32)]
    for _ in range(1, s["frames"]):
        feats.append(np.maximum(feats[-1] + 0.45 * rng.standard_normal((h, w, C)), 0).astype(F32))
    outs = [[rng.standard_normal((1, 1, H, W)).astype(F32) for _ in range(5)] for _ in range(s["frames"])]
    masks = []
    for t in range(s["frames"]):
        m = np.zeros((1, H, W), np.uint8)
        m[:, :, :W // 2 + 3 + 8 * (t % 2)] = 1                               # whole object cells, one void column of cells, background cells
        masks.append(m)
    Q, rinv = zip(*(mc.quantize(f.reshape(p, C)) for f in feats))
    labels = [mc.cell_labels(m, S).reshape(p) for m in masks]
    cap = p + s["memory"]
    R = np.zeros((cap, C), np.int8)
    rinv_r = np.zeros(cap, F32)
    label_r = np.full(cap, VOID, np.uint8)
    R[:p], rinv_r[:p], label_r[:p] = Q[0], rinv[0], labels[0]
    state = np.zeros(4, np.int32)
    sims, sims_first, maps, added = [None], [None], [None], [0]
    for t in range(1, s["frames"]):
        if t >= 2:                                                           # the mask of frame t - 1 arrives with frame t
            R, rinv_r, label_r, state = update(Q[t - 1], rinv[t - 1], labels[t - 1], sims[t - 1][0], R, rinv_r, label_r, state, p, s["memory_new"],
                                               s["tau"], s["margin"])
            added.append(int(state[3]))
        else:
            added.append(0)
        sim, _ = mc.nearest(Q[t][None], rinv[t][None], R[None], rinv_r[None], label_r[None])
        first, _ = mc.nearest(Q[t][None], rinv[t][None], R[None, :p], rinv_r[None, :p], label_r[None, :p])
        sims.append(sim)
        sims_first.append(first)
        maps.append(mc.match_map(sim).reshape(1, h, w))
    return _freeze(dict(h=h, w=w, p=p, feats=feats, outs=outs, masks=masks, labels=labels, Q=Q, rinv=rinv, sims=sims, sims_first=sims_first, maps=maps,
                        added=added, bank=(R, rinv_r, label_r, state)))
