"""CPU: the host side of the connected-component clean-up -- the fixture tests/golden/components.npz against scipy.ndimage.label and plain
numpy counts, the consistency of its stored selection outputs, the three ABI symbols of csrc/components.hip, and the argument handling of
results.components / results.filter_components, which needs no device."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

import component_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osvos_components_ws_bytes", "osvos_mask_components", "osvos_components_select")
CASES = cc.load()


def _renumbered(lab):
    """labels replaced by the rank of their value: canonical labels sort in the order of first appearance in raster order"""
    ids = np.unique(lab[lab > 0])
    out = np.zeros_like(lab)
    out[lab > 0] = np.searchsorted(ids, lab[lab > 0]) + 1
    return out


def test_fixture_loads_and_covers_what_it_must():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names)) == 11
    assert os.path.getsize(cc.GOLDEN) < 200 * 1024
    assert any(c["W"] % 64 for c in CASES) and any(c["N"] > 1 for c in CASES) and any(c["thr"] != 0.5 for c in CASES)
    assert any(c["H"] > 64 and c["W"] > 128 for c in CASES)                                 # several tiles in both directions
    kinds = set(int(k) for c in CASES for k in c["special"][:, 3])
    assert kinds == {cc.THR_EQ, cc.NAN}
    d = [c for c in CASES if c["name"] == "diagonal_checker_16x16"][0]
    assert d["stats"][4][:, 0].tolist() == [16, 128] and d["stats"][8][:, 0].tolist() == [1, 1]
    s = [c for c in CASES if c["name"] == "serpentine_150x300"][0]
    assert s["stats"][8].tolist() == [[1, 22575, 22575, 1]]
    ties = 0
    for c in CASES:
        x = cc.logits(c)
        assert x.dtype == np.float32 and x.shape == c["mask"].shape
        with np.errstate(invalid="ignore"):
            assert np.array_equal(x > cc.logit_threshold(c["thr"]), c["mask"]), c["name"]
        for n, y, xx, kind in c["special"]:
            assert not c["mask"][n, y, xx]
            assert np.isnan(x[n, y, xx]) if kind == cc.NAN else x[n, y, xx] == cc.logit_threshold(c["thr"])
        if c["name"].startswith("noise"):
            for conn in (4, 8):
                a = c["area"][conn][c["area"][conn] > 0]
                ties += int((a == a.max()).sum() > 1)
    assert ties >= 1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_stored_labels_equal_scipy_and_area_and_stats_equal_numpy_counts(case):
    for conn in (4, 8):
        lab, area, stats = case["labels"][conn], case["area"][conn], case["stats"][conn]
        assert lab.dtype == np.int32 and area.dtype == np.int32 and stats.dtype == np.int64
        assert lab.shape == area.shape == case["mask"].shape and stats.shape == (case["N"], 4)
        for n in range(case["N"]):
            m = case["mask"][n]
            ref, count = ndimage.label(m, structure=np.ones((3, 3)) if conn == 8 else None)
            assert np.array_equal((lab[n] > 0), m)
            assert np.array_equal(_renumbered(lab[n]), ref), (case["name"], conn, n)        # scipy numbers by first appearance in raster order
            counts = np.bincount(lab[n].reshape(-1), minlength=m.size + 1)
            counts[0] = 0
            ids = np.nonzero(counts)[0]
            # a label is 1 + the flat index of the first pixel that carries it
            flat = lab[n].reshape(-1)
            assert all(flat[i - 1] == i and not (flat[:i - 1] == i).any() for i in ids[:50])
            assert np.array_equal(area[n].reshape(-1), counts[1:])
            best = int(counts.max())
            want = [len(ids), int(m.sum()), best, int(np.nonzero(counts == best)[0].min()) if len(ids) else 0]
            assert len(ids) == count and stats[n].tolist() == want, (case["name"], conn, n)


def test_stored_selection_outputs_are_consistent():
    case = [c for c in CASES if c["name"] == "track"][0]
    x = cc.logits(case)
    assert sorted(case["settings"]) == ["chain_r0", "chain_r3", "frames_r3", "keep_largest", "min_area5"]
    kepts = []
    for name, s in case["settings"].items():
        lab = case["labels"][s["conn"]]
        kept, out = s["kept"], cc.expected_out(s, x)
        assert not (kept & ~case["mask"]).any()                                             # kept is a subset of the foreground
        same = kept | ~case["mask"]
        assert np.array_equal(out[same], x[same], equal_nan=True)                           # untouched where kept or background
        assert (out[~same] == np.float32(s["fill"])).all()
        assert s["fill"] <= cc.logit_threshold(case["thr"])
        for n in range(case["N"]):                                                          # whole components are kept or dropped
            for i in np.unique(lab[n][lab[n] > 0]):
                assert len(set(kept[n][lab[n] == i].tolist())) == 1
        assert s["seed"].shape[0] == (1 if s["chain"] else case["N"])
        kepts.append(kept)
    for i in range(len(kepts)):
        for j in range(i + 1, len(kepts)):
            assert not np.array_equal(kepts[i], kepts[j])
    k = case["settings"]["chain_r3"]["kept"]
    assert not k[4].any() and np.array_equal(k[5], case["mask"][5])


def test_the_three_symbols_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    declared = set(re.findall(r"\b(osvos_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (osvos_[a-z0-9_]+)$", nm, re.M))
    for s in SYMBOLS:
        assert s in declared and s in _lib.PROTOTYPES and s in exported and hasattr(l, s), s
    assert l.osvos_version() == 1
    m = re.search(r"#define\s+OSVOS_BOUNDARY_MAX_RADIUS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.BOUNDARY_MAX_RADIUS
    # the size query is host arithmetic: 16 bytes per frame, a flag word per pixel, a seed bit per pixel in rows padded to 64-pixel words
    assert l.osvos_components_ws_bytes(3, 480, 854) == 16 * 3 + 4 * 3 * 480 * 854 + 8 * 3 * 480 * 14
    assert l.osvos_components_ws_bytes(1, 3, 3) == 16 + 40 + 24
    assert l.osvos_components_ws_bytes(0, 8, 8) == 0 and l.osvos_components_ws_bytes(65536, 8, 8) == 0
    assert l.osvos_components_ws_bytes(1, 46341, 46341) == 0                                # H W >= 2^31 - 1


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    assert l.osvos_mask_components(None, None, None, None, None, 1, 8, 8, 0.0, 8, None) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_components_select(None, None, None, None, None, 0, 0, 0, 0, 0.0, None, None, None, 1, 8, 8, 0.0, None) < 0
    assert b"null" in l.osvos_last_error()


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from osvos_pytorch_amd import results
    x = torch.zeros(1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        results.components(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        results.filter_components(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        results.ComponentTracker(torch.zeros(8, 8), 3)
    # the value checks need no device behind the tensor: a stand-in that says it is a CUDA tensor reaches them
    class Fake(object):
        is_cuda = True
    for fn in (results.components, results.filter_components):
        for bad in (0.0, 1.0, -0.5, 1.5):
            with pytest.raises(ValueError, match="threshold"):
                fn(Fake(), threshold=bad)
        with pytest.raises(ValueError, match="connectivity"):
            fn(Fake(), connectivity=6)
