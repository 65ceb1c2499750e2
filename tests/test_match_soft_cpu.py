"""CPU: the softmax readout of appearance matching as tests/match_soft_cases.py restates the rule of include/osvos_hip.h -- the naive loop
against the vectorised form, ``best`` against match_cases.nearest bit for bit, the bounds max cos <= lse <= max cos + ln(n_c) / beta, the
limit of a high temperature, the probes that make one bank row matter, the pinned wide-bleed scenario -- and what runs without a GPU of
osvos_match_soft, of its wrappers in osvos_pytorch_amd.match and of train_online.py --match-soft.  The GPU tests compare the kernel against
this restatement."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_cases as mc
import match_soft_cases as ms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("osvos_match_soft_ws_bytes", "osvos_match_soft")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ops(p):
    return p["Q"], p["rinv_q"], p["R"], p["rinv_r"], p["label"]


# ------------------------------------------------------------------------------------------------------------------ the restatement


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("beta", [0.0625, 1.0, 10.0, 40.0])
@pytest.mark.parametrize("c", [(1, 1, 64), (7, 9, 64), (12, 40, 128)], ids=str)
@pytest.mark.parametrize("nr", [1, 2])
def test_naive_loop_equals_the_vectorised_soft(c, nr, beta, kind):
    """the loop sums in another order, in float64: the two agree to the last bit or the one next to it, far inside the bar"""
    p = ms.soft_problem(*c, beta, n=2, nr=nr, kind=kind)
    lse, best = ms.soft_naive(*_ops(p), beta)
    assert p["lse"].dtype == np.float32 and p["lse"].shape == (2, 2, c[0]) == p["best"].shape
    assert np.array_equal(_bits(best), _bits(p["best"]))
    assert np.array_equal(lse == -2, p["lse"] == -2)
    assert (np.abs(lse.astype(np.float64) - p["lse"]) <= 2.0 ** -23 * np.maximum(1, np.abs(p["lse"]))).all()


@pytest.mark.parametrize("kind", mc.LABEL_KINDS)
@pytest.mark.parametrize("c", ms.SOFT_CASES, ids=str)
def test_best_is_nearest_bit_for_bit_and_bounds_lse(c, kind):
    """best is match_cases.nearest's sim; max cos <= lse <= max cos + ln(n_c) / beta within the bar (a dead query, rinv_q = 0, sits on the
    upper bound: every cosine is 0); at beta 40 lse is within ln(n_c) / 40 of nearest"""
    near = mc.nearest_problem(*c, n=2, nr=1, kind=kind)
    rows = ms.class_rows(near["label"])[0]
    for beta in ms.SOFT_BETAS:
        p = ms.soft_problem(*c, beta, n=2, nr=1, kind=kind)
        assert np.array_equal(_bits(p["best"]), _bits(near["sim"]))
        bar = ms.bar_of(p, beta)
        for row in (0, 1):
            lse, best = p["lse"][:, row].astype(np.float64), p["best"][:, row].astype(np.float64)
            if rows[row] == 0:
                assert (_bits(p["lse"][:, row]) == _bits(np.float32(-2))).all() and (_bits(p["best"][:, row]) == _bits(np.float32(-2))).all()
                continue
            assert (lse != -2).all()
            assert (lse >= best - bar[:, row]).all() and (lse <= best + math.log(rows[row]) / beta + bar[:, row]).all()
            if c[0] > 1:                                                     # pixel 1 of every frame is all zero: rinv_q = 0
                assert (near["rinv_q"][:, 1] == 0).all()
                assert (np.abs(lse[:, 1] - math.log(rows[row]) / beta) <= bar[:, row, 1]).all()
            if beta == 40.0:
                assert (np.abs(lse - best) <= math.log(rows[row]) / 40.0 + bar[:, row]).all()


def test_the_uniform_bank_makes_every_row_count():
    """all weights of a query are equal, so lse = cos + ln(n_c) / beta, and one row more or less moves it by ln(1 +- 1 / n_c) / beta.  Up to
    257 rows that is hundreds of times the bar.  At 2049 rows it is 2^24 / n_c^2 = 16 times the bar's sum term alone and 15.6 times the whole
    bar (the exponential's 2^-21 and the final rounding add 2 percent to it): asserted as 15.5, the figure the bar's own formula gives."""
    for pr in ms.UNIFORM_PR:
        p = ms.uniform_probe(pr)
        rows = ms.class_rows(p["label"])[0]
        assert tuple(rows) == ((pr + 1) // 2, pr // 2)
        bar = ms.bar_of(p, 1.0)[0]
        for row in (0, 1):
            lse, cos = p["lse"][0, row].astype(np.float64), p["best"][0, row].astype(np.float64)
            assert (np.abs(lse - (cos + math.log(rows[row]))) <= bar[row]).all()
            moved = min(-math.log1p(-1.0 / rows[row]), math.log1p(1.0 / rows[row]))
            margin = moved / bar[row].max()
            print("uniform bank of %d rows, class %d (%d rows): one row moves lse by %.3e, %.1f times the bar %.3e" % (pr, 1 - row, rows[row], moved, margin,
                                                                                                              bar[row].max()))
            assert margin >= (16 if pr <= 257 else 15.5)
    assert p["best"][0, 0, 0] == 1.0 or abs(p["best"][0, 0, 0] - 1.0) < 1e-6     # query 0 is the bank's vector


def test_the_hot_row_decides_its_class_wherever_it_sits():
    rows = ms.hot_rows()
    tps, slices = ms.slicing(1, 3, ms.PROBE_PR)
    assert (tps, slices) == (2, 9) and rows == (0, 127, 128, ms.PROBE_PR - 1, 256)
    cold = math.log(ms.PROBE_PR // 2) / 40.0 - 1.0                           # a class of rows at cosine -1
    for b in rows:
        p = ms.hot_probe(b)
        hot, other = (0, 1) if b % 2 == 0 else (1, 0)                        # even rows are foreground
        lse = p["lse"][0, :, 0].astype(np.float64)
        assert abs(lse[hot] - 1.0) < 1e-6 and abs(lse[other] - cold) < 1e-3
        assert lse[hot] - lse[other] > 1.8 > 1e4 * ms.bar_of(p, 40.0).max()  # dropping the hot row moves lse by 1.8: no bar hides it
        v = ms.hot_probe(b, void=True)
        assert (np.abs(v["lse"][0, :, 0].astype(np.float64) - cold) < 1e-3).all() and (v["best"][0, :, 0] < -0.999).all()


def test_the_wide_bleed_scenario_is_pinned():
    s = ms.wide_bleed_scenario()
    assert (s["iou_plain"], s["iou_k1"], s["iou_k4"], s["iou_soft"]) == (ms.WIDE_IOU_PLAIN, ms.WIDE_IOU_K1, ms.WIDE_IOU_K4, ms.WIDE_IOU_SOFT) \
        == (0.5, 0.5, 0.5, 1.0)
    assert s["iou_k1_at_soft_gain"] == ms.WIDE_IOU_K1_AT_SOFT_GAIN and s["iou_k4_at_soft_gain"] == ms.WIDE_IOU_K4_AT_SOFT_GAIN < 0.5
    assert abs(s["margin_soft"] - ms.WIDE_MARGIN_SOFT) < 5e-4
    cells = [i * s["w"] + j for i, j in ms.WIDE["cells"]]
    assert (s["label"][0, cells] == 1).all() and int((s["label"] == 1).sum()) == 20      # the 16 object cells and the 2 x 2 bleed
    rows = ms.class_rows(s["label"])[0]
    bar = ms.bar(rows[:, None], ms.WIDE["beta"], s["lse"][0]).max()
    assert s["margin_soft"] > 1e4 * ms.WIDE["gain"] * 2 * bar                # no fused logit near its threshold: the bar flips nothing


# ------------------------------------------------------------------------------------------------------------------ the library, no device


def test_the_symbols_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(l, name)
        assert re.search(r" T %s$" % name, nm, re.M)
    got = {k: float(v) for k, v in re.findall(r"#define OSVOS_MATCH_(MIN|MAX)_BETA\s+([0-9.]+)f", hdr)}
    assert got == {"MIN": _lib.MATCH_MIN_BETA, "MAX": _lib.MATCH_MAX_BETA} == {"MIN": ms.MIN_BETA, "MAX": ms.MAX_BETA} == {"MIN": 0.0625, "MAX": 40.0}


def test_the_workspace_size_needs_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for n, pq, pr, c in [(1, 1, 1, 64), (2, 129, 1000, 512), (2, 300, 2049, 1024), (1, 3, 2049, 64), (1, 6420, 6420, 512), (3, 1 << 20, 1 << 20, 64)]:
        slices = ms.slicing(n, pq, pr)[1]
        assert l.osvos_match_soft_ws_bytes(n, pq, pr, c) == n * slices * 4 * pq * 4      # two sums and two maxima per slice and query
        assert slices == l.osvos_match_ws_bytes(n, pq, pr, c) // (n * 2 * pq * 8)        # nearest's slices
    assert ms.slicing(2, 129, 1000) == (1, 8) and ms.slicing(2, 300, 2049) == (2, 9)
    for bad in [(0, 8, 8, 64), (65536, 8, 8, 64), (1, 0, 8, 64), (1, 8, 0, 64), (1, (1 << 20) + 1, 8, 64), (1, 8, (1 << 20) + 1, 64), (1, 8, 8, 96),
                (1, 8, 8, 1088)]:
        assert l.osvos_match_soft_ws_bytes(*bad) == 0, bad


def _err(l, rc, *words):
    msg = l.osvos_last_error()
    assert rc < 0 and all(w in msg for w in words), (rc, msg)


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    vp = C.c_void_p
    A, B, D, E, F, G, H_, I = (vp(k << 20) for k in range(1, 9))
    # Q, rinv_q, R, rinv_r, label_r, lse, best, ws, N, NR, Pq, Pr, C, beta, stream
    ok = [A, B, D, E, F, G, H_, I, 2, 1, 37, 33, 64, 10.0, None]
    for k in (0, 1, 2, 3, 4, 5, 7):                                          # every pointer but best
        a = list(ok)
        a[k] = None
        _err(l, l.osvos_match_soft(*a), b"match_soft", b"null")
    for k, name, bad in [(8, b"N", (0, 65536)), (9, b"NR", (0, 3)), (10, b"Pq", (0, (1 << 20) + 1)), (11, b"Pr", (0, -5, (1 << 20) + 1)),
                         (12, b"C", (0, 32, 96, 1088))]:
        for v in bad:
            a = list(ok)
            a[k] = v
            _err(l, l.osvos_match_soft(*a), b"match_soft", name + b" %d " % v)
    for beta in (0.0, 0.06, 40.5, 41.0, -1.0, float("nan"), float("inf"), -float("inf")):
        a = list(ok)
        a[13] = beta
        _err(l, l.osvos_match_soft(*a), b"match_soft", b"beta ")
    for k, word in [(0, b"Q and R"), (2, b"Q and R"), (7, b"ws"), (1, b"rinv_q"), (5, b"lse"), (6, b"best")]:
        a = list(ok)
        a[k] = vp(a[k].value + (8 if k in (0, 2) else 4 if k == 7 else 2))
        _err(l, l.osvos_match_soft(*a), b"misaligned", word)
    for out_k in (5, 6, 7):
        for in_k in range(5):
            a = list(ok)
            a[out_k] = vp(a[in_k].value + 16)
            _err(l, l.osvos_match_soft(*a), b"aliasing")
    for out_k, other in ((6, 5), (7, 5), (7, 6)):
        a = list(ok)
        a[out_k] = vp(a[other].value + 64)
        _err(l, l.osvos_match_soft(*a), b"aliasing", b"three buffers")


def test_check_soft_and_the_wrappers_refuse_bad_arguments():
    from osvos_pytorch_amd import match
    for beta, balance in ((0, False), (0.0, True), (0.0625, False), (10, True), (40.0, False), (np.float32(2.5), False)):
        match.check_soft(beta, balance)
    for beta in (-1, 0.01, 0.06, 40.5, float("nan"), float("inf"), "10", True, None):
        with pytest.raises(ValueError, match="soft_beta"):
            match.check_soft(beta, False)
    for balance in (1, 0, "balance", None):
        with pytest.raises(ValueError, match="soft_balance"):
            match.check_soft(10.0, balance)
    ops = (torch.zeros(1, 4, 64, dtype=torch.int8), torch.zeros(1, 4), torch.zeros(1, 4, 64, dtype=torch.int8), torch.zeros(1, 4),
           torch.zeros(1, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match.soft(*ops, 10.0)
    for beta in (0, 0.0, 41, float("nan"), "10"):
        with pytest.raises(ValueError, match="soft"):
            match.soft(*ops, beta)
    with pytest.raises(ValueError, match="workspace"):
        match.soft_workspace(1, 4, 4, 96, torch.device("cpu"))


def test_the_torch_glue_of_the_soft_readout():
    """soft_union is the softmax over both banks' rows, with -2 as "no row"; soft_balanced subtracts ln(rows) / beta and leaves an empty class"""
    from osvos_pytorch_amd import match
    a = torch.tensor([[[0.5, -2.0, -2.0, 0.25], [0.1, 0.3, -2.0, -0.5]]])
    b = torch.tensor([[[0.25, 0.75, -2.0, -2.0], [0.1, -2.0, -2.0, 0.0]]])
    u = match.soft_union(a, b, 10.0).numpy().astype(np.float64)
    want = np.array([[[math.log(math.exp(5.0) + math.exp(2.5)) / 10, 0.75, -2.0, 0.25], [0.1 + math.log(2) / 10, 0.3, -2.0, math.log(math.exp(-5.0) + 1) / 10]]])
    assert np.abs(u - want).max() < 1e-6 and (u[0, :, 2] == -2).all()
    label = torch.tensor([[1, 0, 0, 255, 0, 7]], dtype=torch.uint8)
    rows = match.soft_rows(label)
    assert rows.shape == (1, 2, 1) and rows.flatten().tolist() == [1.0, 3.0]
    bal = match.soft_balanced(a, rows, 10.0).numpy().astype(np.float64)
    assert np.abs(bal[0, 0] - a[0, 0].numpy()).max() == 0 and np.abs(bal[0, 1] - (a[0, 1].numpy() - math.log(3) / 10)).max() < 1e-6
    empty = match.soft_balanced(torch.full((1, 2, 3), -2.0), match.soft_rows(torch.full((1, 5), 255, dtype=torch.uint8)), 10.0)
    assert (empty == -2).all()


def test_the_matcher_takes_the_soft_options_and_refuses_topk_with_them():
    from osvos_pytorch_amd import match
    with pytest.raises(ValueError, match="soft_beta.*topk"):
        match.AppearanceMatcher(None, soft_beta=10, topk=4)
    for kw in (dict(soft_beta=-1.0), dict(soft_beta=41), dict(soft_beta=0.01), dict(soft_beta=float("nan")), dict(soft_beta=10.0, soft_balance=1)):
        with pytest.raises(ValueError, match="soft_beta|soft_balance"):
            match.AppearanceMatcher(None, **kw)
    m = match.AppearanceMatcher(None, 9, 2.0)
    assert (m.soft_beta, m.soft_balance, m.needs_previous) == (0.0, False, False)
    m = match.AppearanceMatcher(None, 9, 2.0, soft_beta=10, soft_balance=True, topk=1)
    assert (m.soft_beta, m.soft_balance, m.needs_previous) == (10.0, True, False)     # the soft readout alone keeps no state between frames


def _train_online(*args):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "train_online.py"] + list(args), cwd=REPO, env=env, capture_output=True, text=True, timeout=600)


class _Args(object):
    def __init__(self, **kw):
        self.__dict__.update(dict(match_layer=9, match_gain=2.0, match_previous=False, match_topk=1, match_local="", match_memory="", match_soft="",
                                  tta=None, adapt_steps=0, device_augment=True, multi_object=False, synthetic=True), **kw)


def test_check_match_args_accepts_and_refuses_match_soft():
    """in process, as far as the flag's own rules go; the refusals are SystemExit before any GPU work"""
    import train_online
    for text, want in (("", {}), ("0", {}), ("10", dict(soft_beta=10.0, soft_balance=False)), ("2.5,balance", dict(soft_beta=2.5, soft_balance=True)),
                       ("40,BALANCE", dict(soft_beta=40.0, soft_balance=True))):
        args = _Args(match_soft=text)
        train_online.check_match_args(args)
        assert {k: v for k, v in args.match.items() if k.startswith("soft")} == want
        assert set(args.match) - set(want) == {"layer", "gain", "previous"}
    args = _Args(match_soft="10", adapt_steps=2)                             # no state between frames: runs with --adapt-steps
    train_online.check_match_args(args)
    assert args.match["soft_beta"] == 10.0
    for text, word in (("41", "soft_beta"), ("0.01", "soft_beta"), ("nan", "--match-soft"), ("ten", "--match-soft"), ("10,yes", "--match-soft"),
                       ("10,balance,1", "--match-soft"), ("-3", "soft_beta")):
        with pytest.raises(SystemExit, match=r"--match-\*.*%s" % word):
            train_online.check_match_args(_Args(match_soft=text))
    with pytest.raises(SystemExit, match="--match-topk above 1"):
        train_online.check_match_args(_Args(match_soft="10", match_topk=4))
    with pytest.raises(SystemExit, match="--match-soft needs --match-gain"):
        train_online.check_match_args(_Args(match_soft="10", match_gain=0.0))
    args = _Args(match_soft="0", match_gain=0.0)
    train_online.check_match_args(args)
    assert args.match is None


def test_train_online_refuses_bad_match_soft_before_any_gpu_work():
    base = ("--synthetic", "--device-augment")
    r = _train_online(*base, "--match-soft", "10")
    assert r.returncode != 0 and "--match-soft needs --match-gain" in r.stderr, r.stderr[-2000:]
    r = _train_online(*base, "--match-gain", "2", "--match-soft", "10", "--match-topk", "4")
    assert r.returncode != 0 and "--match-*" in r.stderr and "--match-topk above 1" in r.stderr, r.stderr[-2000:]
    r = _train_online("--help")
    assert r.returncode == 0 and "--match-soft BETA[,balance]" in r.stdout
