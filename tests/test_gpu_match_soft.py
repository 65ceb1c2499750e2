"""GPU: the softmax readout of appearance matching -- osvos_match_soft (csrc/match_soft.hip) against the numpy restatement in
tests/match_soft_cases.py: lse within the restatement's ``bar`` (the hardware exponential and float32 sums are allowed), -2 and ``best`` bit for
bit, ``best`` also against the unchanged osvos_match_nearest on the device; the probes that make one bank row matter; repeatability; the
argument errors; the wrappers of osvos_pytorch_amd.match; AppearanceMatcher with soft_beta (off: today's bytes; the wide-bleed scenario; the
union with the previous frame's bank; the memory bank that must evolve as without it; soft_balance) and train_online.py --match-soft.
Outputs and workspaces are pre-filled with garbage before every call; a guard band after ws is checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import match_bank_cases as mb
import match_cases as mc
import match_soft_cases as ms
import script_runner
import tta_cases

pytestmark = pytest.mark.gpu
GARBAGE_BYTE = 0xa5
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


def _soft(p, beta, with_best=True, ws=None, fill=GARBAGE_BYTE):
    """one osvos_match_soft call on the arrays of a problem -> (lse, best or None); outputs start as NaN, ws as ``fill`` with a guard band"""
    from osvos_pytorch_amd import _lib
    n, pq, c = p["Q"].shape
    nr, pr = p["label"].shape
    t = {key: _dev(p[key]) for key in OPERANDS}
    lse = torch.full((n, 2, pq), float("nan"), device="cuda", dtype=torch.float32)
    best = torch.full((n, 2, pq), float("nan"), device="cuda", dtype=torch.float32) if with_best else None
    need = int(_lib.lib().osvos_match_soft_ws_bytes(n, pq, pr, c))
    assert need >= n * 4 * pq * 4
    own = ws is None
    if own:
        ws = torch.full((need + GUARD,), fill, device="cuda", dtype=torch.uint8)
    assert ws.numel() >= need + GUARD
    rc = _lib.lib().osvos_match_soft(*_ptrs(t), C.c_void_p(lse.data_ptr()), C.c_void_p(best.data_ptr()) if with_best else None,
                                     C.c_void_p(ws.data_ptr()), n, nr, pq, pr, c, beta, _stream())
    _lib.check(rc, "match_soft")
    if own:
        assert bool((ws[need:] == fill).all()), "the call wrote past osvos_match_soft_ws_bytes"
    return lse, best


def _check(p, beta, what, nearest=True):
    """both forms of the call against the restatement of problem ``p``; -> the largest |lse - ref| / bar"""
    from osvos_pytorch_amd import match
    bar = ms.bar_of(p, beta)
    empty = p["lse"] == -2
    worst = 0.0
    for with_best in (True, False):
        lse, best = _soft(p, beta, with_best)
        got = _np(lse)
        assert not np.isnan(got).any()
        assert np.array_equal(_bits(lse)[empty], p["lse"].view(np.uint32)[empty]) and np.array_equal(got == -2, empty)
        ratio = np.where(empty, 0.0, np.abs(got.astype(np.float64) - p["lse"]) / bar)
        worst = max(worst, float(ratio.max()))
        print("soft %s beta %g best %d: |lse - ref| at most %.3f of the bar (largest difference %.3e)"
              % (what, beta, with_best, ratio.max(), np.where(empty, 0.0, np.abs(got.astype(np.float64) - p["lse"])).max()))
        assert (ratio <= 1.0).all()
        if with_best:
            assert np.array_equal(_bits(best), p["best"].view(np.uint32))
            if nearest:
                assert np.array_equal(_bits(best), _bits(match.nearest(*(_dev(p[key]) for key in OPERANDS))))
    return worst


# ------------------------------------------------------------------------------------------------------------------ the C ABI


@pytest.mark.parametrize("beta", ms.SOFT_BETAS)
@pytest.mark.parametrize("nr", [1, 2])
@pytest.mark.parametrize("c", ms.SOFT_CASES, ids=str)
def test_soft_against_the_restatement(c, nr, beta):
    """one row, ragged query and reference tiles, one slice, 8 slices of one tile, 9 slices of two tiles with a last tile of one row, dead
    queries (rinv_q = 0), duplicated rows, +-127 everywhere at C = 1024, a bank per frame and one for both"""
    from osvos_pytorch_amd import _lib
    pq, pr, ch = c
    p = ms.soft_problem(*c, beta, n=2, nr=nr, kind="mixed")
    if c == (129, 1000, 512):
        assert int(_lib.lib().osvos_match_soft_ws_bytes(2, pq, pr, ch)) // (2 * 4 * pq * 4) == 8
    if c == (300, 2049, 1024):
        assert int(_lib.lib().osvos_match_soft_ws_bytes(2, pq, pr, ch)) // (2 * 4 * pq * 4) == 9
    _check(p, beta, "%s NR %d" % (c, nr))


@pytest.mark.parametrize("kind", ["fg", "bg", "void"])
def test_soft_with_an_empty_class(kind):
    """a class without a row gives -2.0f exactly, in lse and in best"""
    for c in ((37, 33, 64), (130, 257, 128)):
        p = ms.soft_problem(*c, 10.0, n=2, nr=1, kind=kind)
        assert (p["lse"] == -2).any() and ((p["lse"] == -2) == (p["best"] == -2)).all()
        _check(p, 10.0, "%s %s" % (c, kind))


def test_soft_on_a_davis_sized_grid():
    """conv4_3 of an 854 x 480 frame against itself: 6420 x 6420 x 512, several reference tiles per slice"""
    p = ms.soft_problem(*ms.SOFT_DAVIS_CASE, ms.SOFT_DAVIS_BETA, n=1, nr=1, kind="mixed")
    _check(p, ms.SOFT_DAVIS_BETA, str(ms.SOFT_DAVIS_CASE))


@pytest.mark.parametrize("pr", ms.UNIFORM_PR)
def test_every_row_of_a_uniform_bank_counts(pr):
    """lse = cos + ln(n_c) / beta: a dropped or doubled row would move it by 15 bars or more (tests/test_match_soft_cpu.py)"""
    _check(ms.uniform_probe(pr), 1.0, "uniform bank of %d rows" % pr)


def test_one_hot_row_decides_wherever_it_sits():
    """the first and last row of a tile, the last row of the bank (alone in a ragged tile), the first row of the second slice; under the
    void label it must contribute nothing"""
    for b in ms.hot_rows():
        for void in (False, True):
            p = ms.hot_probe(b, void=void)
            lse, _ = _soft(p, 40.0)
            hot = 0 if b % 2 == 0 else 1
            assert (float(lse[0, hot, 0]) > 0.99) == (not void)
            _check(p, 40.0, "hot row %d%s" % (b, " (void)" if void else ""))


def test_soft_repeats_whatever_the_workspace_held():
    """nothing in ws is read before it is written: the same call into workspaces of 0xa5, of 0xff (NaNs) and into what a call of another
    shape left gives the same bytes; N = 2 with one bank is two calls with N = 1"""
    from osvos_pytorch_amd import _lib
    big, small = ms.soft_problem(129, 1000, 512, 10.0, n=2, nr=1), ms.soft_problem(130, 257, 128, 10.0, n=2, nr=2)
    lse0, best0 = _soft(big, 10.0)
    need = int(_lib.lib().osvos_match_soft_ws_bytes(2, 129, 1000, 512))
    ws = torch.full((need + GUARD,), 0xff, device="cuda", dtype=torch.uint8)
    for p, ref in ((big, (lse0, best0)), (small, None), (big, (lse0, best0)), (big, (lse0, best0))):
        lse, best = _soft(p, 10.0, ws=ws)
        if ref is not None:
            assert np.array_equal(_bits(lse), _bits(ref[0])) and np.array_equal(_bits(best), _bits(ref[1]))
    lse_nb, _ = _soft(big, 10.0, with_best=False, ws=ws)
    assert np.array_equal(_bits(lse_nb), _bits(lse0))
    assert bool((ws[need:] == 0xff).all())
    p = ms.soft_problem(300, 2049, 1024, 10.0, n=2, nr=1)
    both, both_best = _soft(p, 10.0)
    for b in range(2):
        one = dict(p, Q=p["Q"][b:b + 1], rinv_q=p["rinv_q"][b:b + 1])
        lse, best = _soft(one, 10.0)
        assert np.array_equal(_bits(lse)[0], _bits(both)[b]) and np.array_equal(_bits(best)[0], _bits(both_best)[b])


def test_bad_arguments_return_an_error_and_write_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    p = mc.nearest_problem(35, 35, 64, n=2, nr=1)
    vp = C.c_void_p

    def buffers():
        t = {k: _dev(p[k]) for k in OPERANDS}
        out = torch.full((2, 2, 2, 35), float("nan"), device="cuda", dtype=torch.float32)      # lse and best
        ws = torch.full((1 << 16,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
        return t, out, ws

    def call(t, out, ws, lse=True, best=True, wsp=True, n=2, nr=1, pq=35, pr=35, c=64, beta=10.0, q_off=0):
        ptrs = _ptrs(t)
        ptrs[0] = vp(t["Q"].data_ptr() + q_off)
        return l.osvos_match_soft(*ptrs, lse if lse is not True else vp(out[0].data_ptr()), best if best is not True else vp(out[1].data_ptr()),
                                  wsp if wsp is not True else vp(ws.data_ptr()), n, nr, pq, pr, c, beta, _stream())

    def untouched(out, ws):
        torch.cuda.synchronize()
        return bool(torch.isnan(out).all()) and bool((ws == GARBAGE_BYTE).all())

    cases = [("beta", dict(beta=0.0)), ("beta", dict(beta=41.0)), ("beta", dict(beta=float("nan"))), ("null", dict(lse=None)), ("null", dict(wsp=None)),
             ("misaligned", dict(q_off=8)), ("NR", dict(n=2, nr=3)), ("NR", dict(nr=0)), ("Pq", dict(pq=0)), ("Pr", dict(pr=(1 << 20) + 1)), ("C", dict(c=96)),
             ("N", dict(n=0))]
    for what, kw in cases:
        t, out, ws = buffers()
        rc = call(t, out, ws, **kw)
        assert rc < 0 and what.encode() in l.osvos_last_error(), (what, l.osvos_last_error())
        assert untouched(out, ws), what
    for key in ("rinv_q", "R", "rinv_r", "label"):                            # a null input
        t, out, ws = buffers()
        ptrs = _ptrs(t)
        ptrs[OPERANDS.index(key)] = None
        rc = l.osvos_match_soft(*ptrs, vp(out[0].data_ptr()), vp(out[1].data_ptr()), vp(ws.data_ptr()), 2, 1, 35, 35, 64, 10.0, _stream())
        assert rc < 0 and b"null" in l.osvos_last_error() and untouched(out, ws)
    # overlapping lse and ws; lse inside Q
    t, out, ws = buffers()
    before = t["Q"].clone()
    assert call(t, out, ws, wsp=vp(out[0].data_ptr() + 64)) < 0 and b"aliasing" in l.osvos_last_error()
    assert call(t, out, ws, lse=vp(ws.data_ptr() + 128)) < 0 and b"aliasing" in l.osvos_last_error()
    assert call(t, out, ws, best=vp(out[0].data_ptr() + 16)) < 0 and b"aliasing" in l.osvos_last_error()
    assert call(t, out, ws, lse=vp(t["Q"].data_ptr() + 64)) < 0 and b"aliasing" in l.osvos_last_error()
    assert untouched(out, ws) and torch.equal(before, t["Q"])


def test_wrapper_shapes_and_refusals():
    from osvos_pytorch_amd import match
    p = ms.soft_problem(129, 1000, 512, 10.0, n=2, nr=1)
    t = [_dev(p[k]) for k in OPERANDS]
    bar = ms.bar_of(p, 10.0)
    lse = match.soft(*t, 10.0)
    assert isinstance(lse, torch.Tensor) and lse.dtype == torch.float32 and tuple(lse.shape) == (2, 2, 129)
    ws = match.soft_workspace(2, 129, 1000, 512, t[0].device)
    assert ws.dtype == torch.uint8 and ws.numel() == match.lib().osvos_match_soft_ws_bytes(2, 129, 1000, 512)
    lse2, best = match.soft(*t, 10.0, ws=ws, with_best=True)
    assert best.dtype == torch.float32 and tuple(best.shape) == (2, 2, 129) and np.array_equal(_bits(lse2), _bits(lse))
    assert np.array_equal(_bits(best), p["best"].view(np.uint32)) and (np.abs(_np(lse).astype(np.float64) - p["lse"]) <= bar).all()
    with pytest.raises(ValueError):
        match.soft(*t, 41.0)
    with pytest.raises(ValueError):
        match.soft(*t, 0.0)
    with pytest.raises(ValueError):
        match.soft(t[0], t[1], t[2], t[3], t[4][:, :800], 10.0)


# ------------------------------------------------------------------------------------------------------------------ the matcher


class _Planted(object):
    """stands in for the network, as in tests/test_gpu_match_bank.py: ``forward_features`` returns the planted logit maps and features of the
    frame whose number x carries"""

    def __init__(self, outs, feats):
        self.outs = [[_dev(o) for o in frame] for frame in outs]
        self.feats = [_dev(f[None]) for f in feats]

    def forward_features(self, x, layer):
        t = int(x[0, 0, 0, 0].item())
        return self.outs[t], self.feats[t], None


def _frame_input(t, H, W):
    return torch.full((1, 3, H, W), float(t), device="cuda")


def _sequence_net():
    s = mb.sequence()
    return s, _Planted(s["outs"], s["feats"])


def _run(matcher, s):
    """tests/test_gpu_match_bank.py's run: the annotated frame 0, then frames 1 .. with the mask of the frame before from frame 2 on"""
    q = mb.SEQ
    matcher.set_reference(_frame_input(0, q["H"], q["W"]), _dev(s["masks"][0]))
    return [matcher(_frame_input(t, q["H"], q["W"]), None if t == 1 else _dev(s["masks"][t - 1]))[-1] for t in range(1, q["frames"])]


def test_the_matcher_with_the_option_off_is_the_matcher_as_it_was(monkeypatch):
    from osvos_pytorch_amd import match
    s, net = _sequence_net()
    g = mb.SEQ["gain"]

    def never(*a, **k):
        raise AssertionError("soft_beta = 0 must not call match.soft")
    monkeypatch.setattr(match, "soft", never)
    for kw in (dict(), dict(previous=True), dict(memory=mb.SEQ["memory"], memory_tau=mb.SEQ["tau"], memory_new=mb.SEQ["memory_new"])):
        a = _run(match.AppearanceMatcher(net, 9, g, **kw), s)
        b = _run(match.AppearanceMatcher(net, 9, g, soft_beta=0.0, soft_balance=False, **kw), s)
        assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def test_the_matcher_on_the_wide_bleed_scenario():
    """four mislabelled rows are as many as topk = 4 averages: the distractor stays (IoU 0.5 at the bleed scenario's gain, less at gain 8);
    the soft readout outvotes them (IoU 1.0), and its fused logits are the float64 fusion of the restated map within gain * 2 * bar (two lse
    per map value) plus fuse_views' own bound"""
    from osvos_pytorch_amd import match
    s, sc = ms.wide_bleed_scenario(), ms.WIDE
    H, W = sc["H"], sc["W"]
    zeros = np.zeros((1, 1, H, W), np.float32)
    frames = [[zeros] * 5, [zeros] * 4 + [s["logits1"][None, None]]]
    net = _Planted(frames, [s["f0"], s["f1"]])

    def run(gain, **kw):
        m = match.AppearanceMatcher(net, 9, gain, **kw).set_reference(_frame_input(0, H, W), _dev(s["mask0"]))
        assert np.array_equal(_np(m._bank[0])[0], s["R"]) and np.array_equal(_np(m._bank[2]), s["label"])
        return _np(m(_frame_input(1, H, W))[-1])[0, 0]

    iou_k4 = mc.iou(run(sc["topk_gain"], topk=sc["K"]) > 0, s["truth1"])
    iou_k4_8 = mc.iou(run(sc["gain"], topk=sc["K"]) > 0, s["truth1"])
    fused = run(sc["gain"], soft_beta=sc["beta"])
    iou_soft = mc.iou(fused > 0, s["truth1"])
    rows = ms.class_rows(s["label"])[0]
    bar = float(ms.bar(rows[:, None], sc["beta"], s["lse"][0]).max())
    big = max(float(np.abs(s["logits1"]).max()), sc["gain"] * float(np.abs(s["map_soft"]).max()))
    bound = sc["gain"] * 2 * bar + tta_cases.fuse_bound(2, big)
    diff = float(np.abs(fused.astype(np.float64) - s["fused_soft"][0]).max())
    print("wide bleed on the device: IoU %.4f topk 4 at gain %g, %.4f topk 4 at gain %g, %.4f soft beta %g; |fused - ref| %.3e of %.3e allowed; margin %.3f"
          % (iou_k4, sc["topk_gain"], iou_k4_8, sc["gain"], iou_soft, sc["beta"], diff, bound, float(np.abs(fused).min())))
    assert (iou_k4, iou_k4_8, iou_soft) == (ms.WIDE_IOU_K4, ms.WIDE_IOU_K4_AT_SOFT_GAIN, ms.WIDE_IOU_SOFT) and iou_k4 == 0.5 and iou_soft == 1.0
    assert diff <= bound


GLUE = 16 * 2.0 ** -24     # the matcher's torch glue on a map: at most sixteen float32 roundings of values below 1 (beta * lse is below 16, divided by beta = 10 again)


def _soft_map_bound(Q, rinv_q, R, rinv_r, label, beta, balance=False):
    """the restated map (float64) of one bank [1, Pr] for queries [1, Pq] and the bound on a device map's distance from it: a bar per lse,
    and the glue"""
    lse, _ = ms.soft(Q, rinv_q, R, rinv_r, label, beta)
    rows = ms.class_rows(label)[0]
    assert (rows > 0).all()
    bar = ms.bar(rows[:, None], beta, lse[0])
    lse = lse.astype(np.float64)
    if balance:
        lse = lse - np.log(rows)[None, :, None] / beta
    return lse[0, 0] - lse[0, 1], float((bar[0] + bar[1]).max()) + GLUE


def _fused_distance(got, logits, want_map, grid, gain, map_bound):
    """-> (the largest |fused - float64 fusion of the planted logits and the restated map|, what the map's bound and fuse_views' allow)"""
    size = tuple(int(v) for v in got.shape[2:])
    host = _np(logits)[0].astype(np.float64)
    ref = tta_cases.fuse_reference([host, want_map.reshape((1,) + grid)], [False, False], size, [1.0, gain])
    big = max(float(np.abs(host).max()), gain * float(np.abs(want_map).max()))
    return float(np.abs(_np(got)[0].astype(np.float64) - ref).max()), gain * map_bound + tta_cases.fuse_bound(2, big)


def test_previous_is_the_soft_readout_of_the_two_banks_together_and_balance_subtracts_the_class_sizes():
    """frame 2 of the planted sequence with previous=True: the map is the soft readout of the first frame's rows and frame 1's rows under
    its mask in ONE bank, within the bar; with soft_balance it is that minus ln(n_c) / beta, n_c the rows of both banks; without a previous
    frame soft_balance subtracts the first bank's ln(n_c) / beta"""
    from osvos_pytorch_amd import match
    s, net = _sequence_net()
    q, beta = mb.SEQ, 10.0
    h, w, p = s["h"], s["w"], s["p"]
    first = (s["Q"][0][None], s["rinv"][0][None], s["labels"][0][None])
    both = (np.concatenate([s["Q"][0], s["Q"][1]])[None], np.concatenate([s["rinv"][0], s["rinv"][1]])[None],
            np.concatenate([s["labels"][0], s["labels"][1]])[None])                       # frame 1's rows under the mask handed over with frame 2
    runs = {}
    for balance in (False, True):
        got = runs[balance] = _run(match.AppearanceMatcher(net, 9, q["gain"], previous=True, soft_beta=beta, soft_balance=balance), s)
        for t, bank in ((1, first), (2, both)):
            want, map_bound = _soft_map_bound(s["Q"][t][None], s["rinv"][t][None], *bank, beta, balance)
            diff, allowed = _fused_distance(got[t - 1], net.outs[t][-1], want, (h, w), q["gain"], map_bound)
            print("previous=True balance %d frame %d: |fused - ref| %.3e of %.3e allowed" % (balance, t, diff, allowed))
            assert diff <= allowed
    rows = ms.class_rows(first[2])[0]
    assert rows[0] != rows[1] and not np.array_equal(_bits(runs[False][0]), _bits(runs[True][0]))      # uneven classes: the balance moves the map


def test_the_memory_bank_evolves_as_without_the_soft_readout():
    """over the three searched frames of the planted sequence the bank's bytes and state equal those of the run with soft_beta = 0 (and the
    restatement's): MemoryBank.update is fed nearest's sim, which the soft search returns from the same pass"""
    from osvos_pytorch_amd import match
    s, net = _sequence_net()
    q = mb.SEQ
    kw = dict(memory=q["memory"], memory_tau=q["tau"], memory_new=q["memory_new"], memory_margin=q["margin"])
    plain = match.AppearanceMatcher(net, 9, q["gain"], **kw)
    soft = match.AppearanceMatcher(net, 9, q["gain"], soft_beta=10.0, **kw)
    fused_plain, fused_soft = _run(plain, s), _run(soft, s)
    for name, want in zip(("r", "rinv_r", "label_r", "state"), s["bank"]):
        a, b = _np(getattr(plain._memory, name)), _np(getattr(soft._memory, name))
        assert a.tobytes() == b.tobytes() == want[None].tobytes(), name
    assert _np(soft._memory.state)[0, 3] == s["added"][-1] > 0
    assert np.array_equal(_bits(soft._last[2]), _bits(plain._last[2]))       # the sim kept for the next update is nearest's
    assert not np.array_equal(_bits(fused_soft[-1]), _bits(fused_plain[-1])) # while the map itself is the soft one
    t = q["frames"] - 1
    R, rinv_r, label_r, _ = s["bank"]                                        # (the bank after its last update is the bank frame t searched)
    want, map_bound = _soft_map_bound(s["Q"][t][None], s["rinv"][t][None], R[None], rinv_r[None], label_r[None], 10.0)
    diff, allowed = _fused_distance(fused_soft[-1], net.outs[t][-1], want, (s["h"], s["w"]), q["gain"], map_bound)
    print("memory and soft, frame %d: |fused - ref| %.3e of %.3e allowed" % (t, diff, allowed))
    assert diff <= allowed


# ------------------------------------------------------------------------------------------------------------------ the script


def test_train_online_multi_object_with_the_soft_readout(tmp_path):
    out = script_runner.train_online(tmp_path / "on", "--multi-object", "--match-gain", "2", "--match-soft", "10").stdout
    assert "J&F on blackswan (2 objects):" in out and "J&F on blackswan object 2:" in out, out[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path / "on"), "Results", "blackswan", "00000.png"))
