"""CPU: the memory bank of appearance matching as tests/match_bank_cases.py restates the rule of include/osvos_hip.h -- the per-row loop against
the vectorised form, the even subsample -- and what runs without a GPU of osvos_match_bank_ws_bytes / osvos_match_bank_update, of
osvos_pytorch_amd.match.MemoryBank / bank_update / AppearanceMatcher(memory=..) and of train_online.py --match-memory.  The GPU tests compare
the kernels against this restatement."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_bank_cases as mb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("osvos_match_bank_ws_bytes", "osvos_match_bank_update")


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ the restatement


@pytest.mark.parametrize("name", sorted(mb.CASES))
def test_the_loop_equals_the_vectorised_restatement(name):
    p = mb.problem(name)
    c = p["args"]
    loop = mb.update_loop(p["q"], p["rinv_q"], p["label_q"], p["sim"], p["R"], p["rinv_r"], p["label_r"], p["state"], c["protected"], c["max_new"],
                          c["tau"], c["margin"])
    assert _same(loop, p["out"])
    ring = c["cap"] - c["protected"]
    m = min(p["n"], c["max_new"], ring)
    cursor, filled, calls, _ = (int(v) for v in p["state"])
    want = [(cursor + m) % ring if ring else cursor, min(filled + m, ring) if m else filled, calls + 1, m]
    assert p["out"][3].tolist() == want
    changed = np.flatnonzero((p["out"][0] != p["R"]).any(axis=1) | (p["out"][1].view(np.uint32) != p["rinv_r"].view(np.uint32))
                             | (p["out"][2] != p["label_r"]))
    assert changed.size <= m and (changed >= c["protected"]).all()          # the first frame's rows are never written


def test_the_cases_cover_what_they_are_named_for():
    n = {k: mb.problem(k)["n"] for k in mb.CASES}
    a = {k: mb.problem(k)["args"] for k in mb.CASES}
    assert n["nothing_novel"] == 0 and n["tail_all_rows"] > 2048 and n["one_row"] <= 1
    for k in ("every_row_of_one", "every_row_of_a_wave", "every_row_of_a_workgroup", "every_row_with_a_tail", "every_row_subsampled"):
        assert n[k] == a[k]["P"], (k, n[k])                                  # n == P: every ballot is full, every workgroup counts 256 (or its tail)
    assert [int(mb.problem(k)["out"][3][3]) for k in ("every_row_of_one", "every_row_of_a_wave", "every_row_of_a_workgroup", "every_row_with_a_tail",
                                                      "every_row_subsampled")] == [1, 64, 256, 4099, 1000]
    assert a["partial_wave"]["max_new"] == n["partial_wave"] - 1 and a["one_wave"]["max_new"] == n["one_wave"] > 8
    assert a["wave_and_one"]["max_new"] == n["wave_and_one"] + 1
    for k in ("several_workgroups", "tail", "most_channels", "nothing_protected"):
        assert 0 < a[k]["max_new"] < n[k] < a[k]["P"], (k, n[k])            # a real selection, really subsampled
    assert n["ring_smaller_than_m"] > 5 and mb.problem("ring_smaller_than_m")["out"][3][3] == 5
    assert mb.problem("no_ring")["out"][3].tolist()[3] == 0 and mb.problem("max_new_zero")["out"][3].tolist()[3] == 0
    f = mb.frame(1000, 64, 0)
    assert np.isnan(f["sim"]).any() and (f["sim"] == -2).any() and (f["rinv_q"] == 0).any() and (f["label_q"] == 7).any()
    sel = mb.select(f["rinv_q"], f["label_q"], f["sim"], 2.0, -4.0)
    assert not sel[np.isnan(f["sim"]).any(axis=0)].any() and not sel[f["rinv_q"] == 0].any() and not sel[f["label_q"] > 1].any()
    # NaN thresholds never select; the margin is ONE float32 subtraction
    assert not mb.select(f["rinv_q"], f["label_q"], f["sim"], np.nan, -4.0).any()
    one = np.ones(1, np.float32)
    sim = np.array([[1.0], [2.0 ** -25]], np.float32)                       # 1 - 2^-25 rounds to 1 in float32 (half to even): the margin 1 is met
    assert 1.0 - 2.0 ** -25 < 1.0 and mb.select(one, np.ones(1, np.uint8), sim, 2.0, 1.0).all()
    assert mb.select(one, np.zeros(1, np.uint8), np.array([[0.5], [0.25]], np.float32), 2.0, -0.25).all()      # background: own is row 1
    assert not mb.select(one, np.zeros(1, np.uint8), np.array([[0.5], [0.25]], np.float32), 2.0, -0.2).any()


def test_the_subsample_keeps_m_rows_with_distinct_j():
    for n in range(1, 71):
        for m in range(0, n + 1):
            kept, j = mb.subsample(n, m)
            assert int(kept.sum()) == m and sorted(j[kept].tolist()) == list(range(m)), (n, m)
    kept, _ = mb.subsample(10, 5)
    assert kept.tolist() == [False, True] * 5                               # even
    big = 1 << 20
    kept, j = mb.subsample(big, big - 1)                                    # (r + 1) m passes 2^31: 64-bit integers
    assert int(kept.sum()) == big - 1 and j[kept][-1] == big - 2


def test_the_chain_wraps_twice():
    c = mb.CHAIN
    b = mb.bank(c["cap"], c["C"], c["protected"], 5)
    cur = (b["R"], b["rinv_r"], b["label_r"], np.array([90, 10, 0, 0], np.int32))
    ring, wraps = c["cap"] - c["protected"], 0
    for t in range(c["frames"]):
        f = mb.frame(c["P"], c["C"], 20 + t)
        new = mb.update(f["q"], f["rinv_q"], f["label_q"], f["sim"], *cur, c["protected"], c["max_new"], c["tau"], c["margin"])
        assert new[3][3] == c["max_new"] and _same(new, mb.update_loop(f["q"], f["rinv_q"], f["label_q"], f["sim"], *cur, c["protected"],
                                                                        c["max_new"], c["tau"], c["margin"]))
        wraps += int(new[3][0] < cur[3][0])
        cur = new
    assert wraps >= 2 and cur[3].tolist() == [(90 + 250) % ring, ring, 5, 50]
    assert mb.bound_rows(30, 100, 50, 0) == 30 and mb.bound_rows(30, 100, 50, 1) == 80 and mb.bound_rows(30, 100, 50, 9) == 130
    assert mb.bound_rows(30, 5, 50, 1) == 35 and mb.bound_rows(30, 100, 0, 7) == 30


def test_the_matcher_sequence_admits_rows():
    s = mb.sequence()
    assert s["added"][:2] == [0, 0] and all(0 < a <= mb.SEQ["memory_new"] for a in s["added"][2:])
    # the memory changes what the last frame sees
    assert not np.array_equal(s["sims"][-1].view(np.uint32), s["sims_first"][-1].view(np.uint32))
    assert np.array_equal(s["sims"][1].view(np.uint32), s["sims_first"][1].view(np.uint32))
    assert all((l == 1).any() and (l == 0).any() and (l == 255).any() for l in s["labels"])


# ------------------------------------------------------------------------------------------------------------------ the library, no device


def test_the_symbols_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(l, name)
        assert re.search(r" T %s$" % name, nm, re.M)
    assert len(_lib.PROTOTYPES["osvos_match_bank_update"][1]) == 18
    assert "match_bank.hip" in open(os.path.join(REPO, "osvos-pytorch_amd", "csrc", "Makefile")).read()


def test_the_workspace_size_needs_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for n, p in [(1, 1), (1, 64), (2, 4099), (1, 6420), (3, 1 << 20)]:
        need = l.osvos_match_bank_ws_bytes(n, p)
        assert need >= n * (p + 16) and need <= n * (2 * p + 64) + 16 and need % 8 == 0, (n, p, need)
    assert l.osvos_match_bank_ws_bytes(2, 4099) > l.osvos_match_bank_ws_bytes(1, 4099)
    for bad in [(0, 8), (65536, 8), (1, 0), (1, -1), (1, (1 << 20) + 1)]:
        assert l.osvos_match_bank_ws_bytes(*bad) == 0, bad


def _err(l, rc, *words):
    msg = l.osvos_last_error()
    assert rc < 0 and all(w in msg for w in words), (rc, msg)


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    vp = C.c_void_p
    # q, rinv_q, label_q, sim, R, rinv_r, label_r, state, ws, N, P, C, cap, protected_rows, max_new, tau, margin, stream
    ok = [vp(k << 24) for k in range(1, 10)] + [2, 37, 64, 60, 33, 8, 0.9, 0.0, None]
    for k in range(9):
        a = list(ok)
        a[k] = None
        _err(l, l.osvos_match_bank_update(*a), b"match_bank_update", b"null")
    for k, name, bad in [(9, b"N", (0, 65536)), (10, b"P", (0, -3, (1 << 20) + 1)), (11, b"C", (0, 32, 96, 1088)), (12, b"cap", (0, -1, (1 << 20) + 1)),
                         (13, b"protected_rows", (-1, 61)), (14, b"max_new", (-1, -512))]:
        for v in bad:
            a = list(ok)
            a[k] = v
            _err(l, l.osvos_match_bank_update(*a), b"match_bank_update", name + b" %d " % v)
    for k, name in ((15, b"tau"), (16, b"margin")):
        for v in (float("nan"), float("inf"), -float("inf")):
            a = list(ok)
            a[k] = v
            _err(l, l.osvos_match_bank_update(*a), b"match_bank_update", name + b" ")
    for k, word in [(0, b"q and R"), (4, b"q and R"), (8, b"ws"), (1, b"rinv_q"), (3, b"sim"), (5, b"rinv_r"), (7, b"state")]:
        a = list(ok)
        a[k] = vp(a[k].value + (8 if k in (0, 4) else 4 if k == 8 else 2))
        _err(l, l.osvos_match_bank_update(*a), b"misaligned", word)
    for out_k in range(4, 9):                                               # the bank, state and ws: inside a frame array, and inside each other
        for in_k in range(9):
            if in_k != out_k:
                a = list(ok)
                a[out_k] = vp(a[in_k].value + 16)
                _err(l, l.osvos_match_bank_update(*a), b"aliasing")


def _cpu_frame(p=4, c=64, cap=10):
    return dict(q=torch.zeros(1, p, c, dtype=torch.int8), rinv_q=torch.zeros(1, p), label_q=torch.zeros(1, p, dtype=torch.uint8),
                sim=torch.zeros(1, 2, p), r=torch.zeros(1, cap, c, dtype=torch.int8), rinv_r=torch.zeros(1, cap),
                label_r=torch.zeros(1, cap, dtype=torch.uint8), state=torch.zeros(1, 4, dtype=torch.int32))


def test_wrappers_refuse_cpu_tensors_and_bad_values():
    from osvos_pytorch_amd import match
    t = _cpu_frame()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match.bank_update(*t.values(), max_new=4, tau=0.9, margin=0.0, protected=4)
    bank = match.MemoryBank(6)
    assert (bank.capacity_rows, bank.tau, bank.max_new, bank.margin, bank.rows, bank.ring) == (6, 0.9, 512, 0.0, 0, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.seed(t["r"][:, :4], t["rinv_r"][:, :4], t["label_r"][:, :4])
    with pytest.raises(RuntimeError, match="seed"):
        bank.update(t["q"], t["rinv_q"], t["label_q"], t["sim"])
    for args in ((0,), (-1,), (1 << 20,), (2.0,), (True,), ("8",), (8, float("nan")), (8, float("inf")), (8, "0.9"), (8, 0.9, -1), (8, 0.9, 2.5),
                 (8, 0.9, 4, float("nan")), (8, 0.9, 4, None)):
        with pytest.raises(ValueError, match="memory|MemoryBank"):
            match.MemoryBank(*args)
    match.check_memory(0)
    match.check_memory(1024, -3.0, 0, -4.0)
    for args in ((-1,), (1 << 20,), (1.5,), (8, float("inf")), (8, 0.9, -2), (8, 0.9, 4, float("nan"))):
        with pytest.raises(ValueError, match="memory"):
            match.check_memory(*args)
    for kw in (dict(memory=-1), dict(memory=1 << 20), dict(memory=2.0), dict(memory=8, memory_tau=float("nan")), dict(memory=8, memory_new=-1),
               dict(memory=8, memory_margin=float("inf"))):
        with pytest.raises(ValueError, match="memory"):
            match.AppearanceMatcher(None, **kw)
    m = match.AppearanceMatcher(None, 9, 2.0)
    assert (m.memory, m.memory_tau, m.memory_new, m.memory_margin, m.needs_previous) == (0, 0.9, 512, 0.0, False)
    # the host-side bound: protected + min(ring, calls * min(max_new, ring))
    bank = match.MemoryBank(100, max_new=50)
    bank.protected = 30
    for calls, rows in ((0, 30), (1, 80), (2, 130), (9, 130)):
        bank.host_calls = calls
        assert bank.rows == rows == mb.bound_rows(30, 100, 50, calls)


def test_a_matcher_with_memory_needs_the_previous_mask_and_frame_forward_remembers_it():
    from osvos_pytorch_amd import match, sequence
    assert match.AppearanceMatcher(None, memory=64).needs_previous
    assert not match.AppearanceMatcher(None, memory=0).needs_previous

    class Recorder(object):
        """stands in for a matcher: FrameForward asks it for needs_previous alone"""
        def __init__(self, matcher):
            self.needs_previous, self.previous = matcher.needs_previous, matcher.previous

    logits = torch.tensor([[[[1.0, -1.0]]]])
    f = sequence.FrameForward(None, matcher=Recorder(match.AppearanceMatcher(None, 9, 2.0, memory=64)))
    f.remember(logits)
    assert f.match_prev.tolist() == [[[[True, False]]]]
    f = sequence.FrameForward(None, matcher=match.AppearanceMatcher(None, 9, 2.0, memory=64))
    f.remember(logits)
    assert f.match_prev.tolist() == [[[[True, False]]]]
    f = sequence.FrameForward(None, matcher=Recorder(match.AppearanceMatcher(None, 9, 2.0)))
    f.remember(logits)
    assert f.match_prev is None


def _train_online(*args):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "train_online.py"] + list(args), cwd=REPO, env=env, capture_output=True, text=True, timeout=600)


def test_train_online_refuses_bad_memory_arguments_before_any_gpu_work():
    base = ("--synthetic", "--device-augment")
    r = _train_online(*base, "--match-memory", "256")
    assert r.returncode != 0 and "--match-memory needs --match-gain" in r.stderr, r.stderr[-2000:]
    for value, word in (("-1", "memory"), ("1048576", "memory"), ("256,nan", "finite"), ("256,0.9,-1", "memory_new"), ("256,0.9,1.5", "--match-memory"),
                        ("256,0.9,64,0,1", "--match-memory")):
        r = _train_online(*base, "--match-gain", "2", "--match-memory", value)
        assert r.returncode != 0 and "--match-*" in r.stderr and word in r.stderr, (value, r.stderr[-2000:])
    r = _train_online(*base, "--match-gain", "2", "--match-memory", "256", "--adapt-steps", "2")
    assert r.returncode != 0 and "--match-memory is not run together with --adapt-steps" in r.stderr and "twice" in r.stderr, r.stderr[-2000:]
    r = _train_online(*base, "--match-gain", "2", "--match-memory", "256,0.8,128,0.1", "--tta-flip")
    assert r.returncode != 0 and "--tta-scales / --tta-flip" in r.stderr, r.stderr[-2000:]
    r = _train_online("--help")
    assert r.returncode == 0 and "--match-memory ROWS[,TAU[,NEW[,MARGIN]]]" in r.stdout
    own = " ".join(r.stdout.split("--match-memory ROWS[,TAU[,NEW[,MARGIN]]]")[-1].split("--lucid")[0].split())
    assert "starting values, not tuned on DAVIS" in own and "Not with --adapt" in own, own      # (argparse breaks lines at hyphens)
