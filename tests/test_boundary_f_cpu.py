"""CPU: the fixture of the DAVIS boundary measure (tests/golden/boundary_f.npz) is pinned by a second, independent numpy restatement of the
boundary rule and the matching rule (and by the generator's scipy recipe where scipy imports), the host-side functions of
osvos_pytorch_amd.results follow the published definition, and the two C entry points exist and refuse bad arguments."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import boundary_cases as bc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _boundary(m):
    """rule 1 by comparisons of slices"""
    b = np.zeros(m.shape, dtype=bool)
    b[:-1, :-1] = (m[:-1, :-1] != m[:-1, 1:]) | (m[:-1, :-1] != m[1:, :-1]) | (m[:-1, :-1] != m[1:, 1:])
    b[-1, :-1] = m[-1, :-1] != m[-1, 1:]
    b[:-1, -1] = m[:-1, -1] != m[1:, -1]
    return b


def _nearest_in_row(b):
    """per pixel the horizontal distance to the nearest set pixel of its row (a large number when the row is empty)"""
    h, w = b.shape
    big = 1 << 30
    xs = np.arange(w)[None, :]
    left = np.maximum.accumulate(np.where(b, xs, -big), axis=1)                    # nearest set column at or left of x
    right = np.minimum.accumulate(np.where(b, xs, big)[:, ::-1], axis=1)[:, ::-1]  # ... at or right of x
    return np.minimum(xs - left, right - xs)


def _matched(a, b, r):
    """rule 3 in its distance form: pixels of a with a pixel of b at dy*dy + dx*dx <= r*r"""
    h, w = a.shape
    near = _nearest_in_row(b)
    hit = np.zeros((h, w), dtype=bool)
    for dy in range(-r, r + 1):
        half = math.isqrt(r * r - dy * dy)
        lo, hi = max(0, -dy), min(h, h - dy)              # rows y with 0 <= y + dy < h
        if lo < hi:
            hit[lo:hi] |= near[lo + dy:hi + dy] <= half
    return int((a & hit).sum())


def _counts(p, g, r):
    fb, gb = _boundary(p), _boundary(g)
    return [int((p & g).sum()), int((p | g).sum()), int(fb.sum()), int(gb.sum()), _matched(fb, gb, r), _matched(gb, fb, r)]


def test_fixture_exists_and_covers_the_cases():
    assert os.path.getsize(bc.GOLDEN) < 504 * 1024
    cases = {c["name"]: c for c in bc.load()}
    e = cases["ellipse_roll"]
    assert (e["H"], e["W"], e["r"], e["N"]) == (480, 854, 8, 5)
    assert e["counts"][:, 2].tolist() == [1336] * 5 and e["counts"][:, 3].tolist() == [1336] * 5
    assert e["counts"][:, 4].tolist() == [1336, 1336, 1210, 988, 636] and e["counts"][:, 5].tolist() == [1336, 1336, 1210, 988, 636]
    np.testing.assert_allclose(e["f"], [1, 1, 0.9057, 0.7395, 0.476], atol=5e-5)
    v = cases["edge_le"]
    assert v["counts"][:, 2:].tolist() == [[480, 480, 480, 480], [480, 480, 0, 0]] and v["f"].tolist() == [1.0, 0.0]      # the <= of the radius
    assert (cases["hd_shapes"]["H"], cases["hd_shapes"]["W"], cases["hd_shapes"]["r"], cases["hd_shapes"]["N"]) == (1080, 1920, 18, 2)
    for name in ("noise_37x53_r1", "noise_37x53_r3", "noise_48x64_r5", "noise_30x85_r8"):
        assert cases[name]["N"] == 2 and cases[name]["counts"][:, 2:].min() > 0
    for name in ("full_1x1", "full_2x300", "full_5x7"):
        assert not cases[name]["counts"][:, 2:].any() and cases[name]["f"].tolist() == [1.0, 1.0]
        assert cases[name]["p"].all() and not cases[name]["g"][0].any() and cases[name]["g"][1].all()
    assert max(c["r"] for c in cases.values()) >= 40
    assert any(c["thr"] == 0.3 for c in cases.values()) and any(c["soft"] for c in cases.values())


def test_host_functions_follow_the_definition():
    from osvos_pytorch_amd import results
    assert results.boundary_radius(480, 854) == 8 and results.boundary_radius(1080, 1920) == 18
    assert results.boundary_radius(37, 53) == 1 and results.boundary_radius(2160, 3840) == 36
    assert results.boundary_radius(37, 53, 3) == 3 and results.boundary_radius(480, 854, 1) == 1 and results.boundary_radius(5, 5, 12.0) == 12
    assert isinstance(results.boundary_radius(480, 854), int)
    assert results.f_measure(0, 5, 0, 0) == 0.0          # precision 1, recall 0
    assert results.f_measure(5, 0, 0, 0) == 0.0          # precision 0, recall 1
    assert results.f_measure(0, 0, 0, 0) == 1.0
    assert results.f_measure(4, 8, 0, 0) == 0.0          # precision + recall == 0
    assert results.f_measure(4, 8, 2, 2) == 2 * 0.5 * 0.25 / 0.75
    assert results.f_measure(10, 10, 10, 10) == 1.0
    for c in bc.load():
        for row, f in zip(c["counts"], c["f"]):
            assert results.f_measure(*row[2:]) == f, c["name"]
            assert 0.0 <= f <= 1.0


def test_fixture_counts_follow_from_a_second_restatement():
    for c in bc.load():
        for i in range(c["N"]):
            assert _counts(c["p"][i], c["g"][i], c["r"]) == c["counts"][i].tolist(), (c["name"], i)


def test_fixture_counts_follow_from_scipy_dilation():
    ndimage = pytest.importorskip("scipy.ndimage")
    for c in bc.load():
        r = c["r"]
        y, x = np.mgrid[-r:r + 1, -r:r + 1]
        disk = (x * x + y * y) <= r * r
        for i in range(c["N"]):
            fb, gb = _boundary(c["p"][i]), _boundary(c["g"][i])
            got = [int(fb.sum()), int(gb.sum()), int((fb & ndimage.binary_dilation(gb, structure=disk)).sum()),
                   int((gb & ndimage.binary_dilation(fb, structure=disk)).sum())]
            assert got == c["counts"][i, 2:].tolist(), (c["name"], i)


def test_case_tensors_threshold_back_to_the_masks():
    for c in bc.load():
        logits, gt = bc.tensors(c)
        t = np.float32(np.log(c["thr"] / (1.0 - c["thr"])))
        assert logits.dtype == np.float32 and logits.shape == (c["N"], 1, c["H"], c["W"])
        assert np.array_equal(logits[:, 0] > t, c["p"]) and np.array_equal(gt[:, 0] > np.float32(0.5), c["g"])
        if c["p"].any() and not c["p"].all():
            assert np.unique(np.abs(logits - t)).size > min(16, c["p"].size // 2)          # magnitudes vary per pixel
        if c["soft"]:
            assert (gt == 0.5).any() and ((gt > 0.5) & (gt < 1)).any() and ((gt > 0) & (gt < 0.5)).any()


def test_entry_points_exist_and_refuse_bad_arguments():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for name in ("osvos_boundary_ws_bytes", "osvos_mask_jf_counts"):
        assert name in _lib.PROTOTYPES and hasattr(l, name)
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    assert "osvos_boundary_ws_bytes(" in hdr and "osvos_mask_jf_counts(" in hdr
    assert l.osvos_boundary_ws_bytes(1, 480, 854) == 2 * 480 * 14 * 8          # two one-bit maps, rows padded to 64-bit words
    assert l.osvos_boundary_ws_bytes(3, 5, 64) == 2 * 3 * 5 * 8 and l.osvos_boundary_ws_bytes(1, 1, 65) == 2 * 2 * 8
    assert l.osvos_boundary_ws_bytes(0, 5, 5) == 0 and l.osvos_boundary_ws_bytes(1, 0, 5) == 0 and l.osvos_boundary_ws_bytes(1, 5, -1) == 0
    # host buffers stand in for device pointers: every one of these calls must be refused before anything is enqueued
    buf = (C.c_ulonglong * 64)()
    p = C.cast(buf, C.c_void_p)
    bad = [
        ((None, p, p, p, 1, 4, 4, 0.0, 1, 0, None), b"null"),
        ((p, None, p, p, 1, 4, 4, 0.0, 1, 0, None), b"null"),
        ((p, p, None, p, 1, 4, 4, 0.0, 1, 0, None), b"null"),
        ((p, p, p, None, 1, 4, 4, 0.0, 1, 0, None), b"null"),
        ((p, p, p, p, 1, 4, 4, 0.0, 0, 0, None), b"radius"),
        ((p, p, p, p, 1, 4, 4, 0.0, -3, 0, None), b"radius"),
        ((p, p, p, p, 1, 4, 4, 0.0, 1000, 0, None), b"radius"),
        ((p, p, p, p, 1, 0, 4, 0.0, 1, 0, None), b"size"),
        ((p, p, p, p, 1, 4, 0, 0.0, 1, 0, None), b"size"),
        ((p, p, p, p, 0, 4, 4, 0.0, 1, 0, None), b"size"),
    ]
    for args, word in bad:
        rc = l.osvos_mask_jf_counts(*args)
        assert rc < 0 and word in l.osvos_last_error(), (args[4:], rc, l.osvos_last_error())
    m = int(re_max_radius(hdr))
    assert m >= 40
    rc = l.osvos_mask_jf_counts(p, p, p, p, 1, 4, 4, 0.0, m + 1, 0, None)
    assert rc < 0 and b"radius" in l.osvos_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc, "mask_jf_counts")


def re_max_radius(hdr):
    import re
    return re.search(r"#define OSVOS_BOUNDARY_MAX_RADIUS (\d+)", hdr).group(1)


def test_evaluator_refuses_cpu_tensors_and_bad_thresholds():
    import torch
    from osvos_pytorch_amd import results
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError):
        results.boundary_f(x, x)
    with pytest.raises(RuntimeError):
        results.SequenceEvaluator().add(x, x)
    with pytest.raises(ValueError):
        results.SequenceEvaluator(threshold=1.0)
    ev = results.SequenceEvaluator()
    assert ev.frames == 0 and ev.per_frame() == ([], [])
    with pytest.raises(ValueError):
        ev.summary()
