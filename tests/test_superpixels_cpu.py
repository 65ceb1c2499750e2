"""CPU: the superpixel rules of include/osvos_hip.h as tests/superpixel_cases.py restates them -- the naive loops against the vectorised
form, the exact properties of SLIC and of the pooling, the snapping scenario, and what runs without a GPU of osvos_pytorch_amd.superpixels
and of the --snap-* rules of train_online.py.  The GPU tests compare the kernels against this restatement bit for bit."""
import numpy as np
import pytest

import superpixel_cases as sc


@pytest.mark.parametrize("kind", sc.SCENES)
@pytest.mark.parametrize("c", [(7, 9, 2, 4, 10, 3), (5, 6, 1, 2, 0, 2), (9, 13, 1, 5, 3, 2), (1, 1, 1, 2, 0, 1)], ids=sc.case_id)
def test_naive_loop_equals_the_vectorised_form(c, kind):
    h, w, n, cell, m, iters = c
    frames = sc.frames_of(kind, h, w, n)
    labels, centres = sc.slic(frames, cell, m, iters)
    want_labels, want_centres = sc.slic_naive(frames, cell, m, iters)
    assert labels.dtype == np.int32 and centres.dtype == np.int32 and centres.shape == (n, np.prod(sc.grid_shape(h, w, cell)), 6)
    assert np.array_equal(labels, want_labels) and np.array_equal(centres, want_centres)


@pytest.mark.parametrize("kind", sc.SCENES)
def test_no_iteration_gives_the_grid(kind):
    c = (40, 64, 3, 8, 10, 0)
    r = sc.reference(kind, c)
    grid = sc.home_labels(40, 64, 8)
    assert np.array_equal(r["labels"], np.broadcast_to(grid, (3, 40, 64)))
    cen = r["centres"]
    assert (cen[..., 5] == 64).all()                                         # 40 x 64 is a whole number of 8 x 8 cells
    # the rounded mean of 0..7 is floor((2 * 28 + 8) / 16) = 4
    assert np.array_equal(cen[0, :, 0], np.tile(np.arange(8) * 8 + 4, 5)) and np.array_equal(cen[0, :, 1], np.repeat(np.arange(5) * 8 + 4, 8))


def test_a_constant_frame_ties_on_colour_and_the_order_decides():
    """with compactness 0 every distance is 0: the smallest k of the 3 x 3 cells wins, which is the cell up and to the left"""
    frames = sc.frames_of("constant", 12, 16, 1)
    labels, centres = sc.slic(frames, 4, 0, 1)
    gy, gx = np.maximum(np.arange(12) // 4 - 1, 0), np.maximum(np.arange(16) // 4 - 1, 0)
    assert np.array_equal(labels[0], gy[:, None] * 4 + gx[None, :])
    assert (centres[0, :, 5] == 0).sum() == 3 + 4 - 1                        # the last row and column of clusters lost every pixel
    # with compactness > 0 a constant frame keeps the grid: a pixel is nearest to the centre of its own cell, or ties towards a smaller k
    labels, _ = sc.slic(frames, 4, 3, 2)
    d = np.abs(labels[0] - sc.home_labels(12, 16, 4))
    assert set(np.unique(d)) <= {0, 1, 4, 5}


@pytest.mark.parametrize("kind", sc.SCENES)
@pytest.mark.parametrize("c", sc.SLIC_CASES, ids=sc.case_id)
def test_labels_stay_in_the_3x3_cells_and_counts_add_up(c, kind):
    h, w, n, cell, m, iters = c
    r = sc.reference(kind, c)
    gh, gw = sc.grid_shape(h, w, cell)
    lab = r["labels"]
    assert lab.min() >= 0 and lab.max() < gh * gw
    ly, lx = lab // gw, lab % gw
    assert (np.abs(ly - (np.arange(h) // cell)[None, :, None]) <= 1).all() and (np.abs(lx - (np.arange(w) // cell)[None, None, :]) <= 1).all()
    cen = r["centres"]
    for f in range(n):
        assert np.array_equal(cen[f, :, 5], np.bincount(lab[f].ravel(), minlength=gh * gw))
    # a centre lies in the 3 x 3 cells around its cluster
    ky, kx = np.arange(gh * gw) // gw, np.arange(gh * gw) % gw
    assert (np.abs(cen[..., 0] // cell - kx) <= 1).all() and (np.abs(cen[..., 1] // cell - ky) <= 1).all()


def test_every_distance_fits_32_bits_at_the_limits():
    """cell 64, compactness 64: opposite colours either side of a line make dc as large as it gets next to large ds"""
    h = w = 150
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    frame = np.where(((xx + yy) % 97 < 48)[..., None], 255, 0).astype(np.uint8) * np.ones(3, np.uint8)
    labels = sc.home_labels(h, w, 64)
    centres = sc.update(frame, labels, None, 9)
    top = 0
    for _ in range(3):
        d, _, ok = sc.distances(frame, centres, 64, 64)
        top = max(top, int(d[ok].max()))
        labels = sc.assign(frame, centres, 64, 64)
        centres = sc.update(frame, labels, centres, 9)
    assert 2 ** 29 < top < 2 ** 31
    assert 4096 * 195075 + 4096 * 73728 < 2 ** 31 and 16384 * 36864 < 2 ** 32


def test_an_empty_cluster_keeps_its_centre():
    c = (37, 53, 2, 8, 10, 5)
    r = sc.reference("two_colour", c)
    frames = r["frames"]
    empty = r["centres"][..., 5] == 0
    assert empty.any() and not empty.all()                                   # the slanted edge empties the clusters it cuts
    for f in range(2):
        labels, centres = sc.slic_one(frames[f], 8, 10, 4)                   # one step earlier
        nxt = sc.update(frames[f], sc.assign(frames[f], centres, 8, 10), centres, centres.shape[0])
        assert np.array_equal(nxt, r["centres"][f])
        gone = nxt[:, 5] == 0
        assert np.array_equal(nxt[gone, :5], centres[gone, :5])
    # by hand: cluster 1 has no pixel
    frame = np.zeros((2, 4, 3), np.uint8)
    prev = np.array([[9, 9, 9, 9, 9, 7], [5, 4, 3, 2, 1, 8]])
    got = sc.update(frame, np.zeros((2, 4), np.int32), prev, 2)
    assert got.tolist() == [[2, 1, 0, 0, 0, 8], [5, 4, 3, 2, 1, 0]]         # x: floor((2 * 12 + 8) / 16) = 2, y: floor((2 * 4 + 8) / 16) = 1


def test_pooling_of_a_constant_superpixel_returns_the_quantised_constant():
    labels = sc.home_labels(6, 8, 2)[None]
    k = 12
    values = np.array([0.3, -0.3, 1.0 / 3, 5.0, -7.25, 1e-6, -1e-6, 0.5 / 65536, 1.5 / 65536, -0.5 / 65536, 123.456, -16000.1], np.float32)
    logits = values[labels]
    out = sc.pool(logits, labels, k)
    want = (np.rint(values.astype(np.float64) * 65536) / 65536).astype(np.float32)      # half to even: 0.5 -> 0, 1.5 -> 2, -0.5 -> -0
    assert np.array_equal(out, want[labels])
    assert out[0, 2, 6] == 0 and out[0, 4, 0] == np.float32(2.0 / 65536)     # (clusters 7 and 8 of the 3 x 4 grid)
    assert np.array_equal(out.view(np.uint32), sc.pool_naive(logits, labels, k).view(np.uint32))


def test_pooling_handles_nan_inf_and_labels_out_of_range():
    x = np.array([[[np.nan, 1.0, np.inf, -np.inf], [3e4, -3e4, 2.0, np.nan], [0.25, 7.0, -0.0, 1e-30]]], np.float32)
    lab = np.array([[[0, 0, 1, 2], [1, 2, 3, -1], [4, 5, 4, 4]]], np.int32)
    out = sc.pool(x, lab, 4)                                                  # labels 4 and 5 are outside [0, 4), -1 too
    assert out[0, 0, 0] == out[0, 0, 1] == np.float32((-16384.0 + 1.0) / 2)   # NaN is the lower clamp: background
    assert out[0, 0, 2] == out[0, 1, 0] == 16384.0 and out[0, 0, 3] == out[0, 1, 1] == -16384.0      # +-inf and large values clamp
    assert out[0, 1, 2] == 2.0
    passed = lab[0] >= 4
    passed[1, 3] = True
    assert np.array_equal(out.view(np.uint32)[0][passed], x.view(np.uint32)[0][passed])      # bit for bit: the NaN, -0.0 and 1e-30 too
    assert np.isnan(out[0, 1, 3]) and np.signbit(out[0, 2, 2])
    big = sc.awkward_logits((2, 9, 11), 4)
    lab = np.random.default_rng(5).integers(-1, 8, size=(2, 9, 11)).astype(np.int32)
    assert np.array_equal(sc.pool(big, lab, 7).view(np.uint32), sc.pool_naive(big, lab, 7).view(np.uint32))
    assert np.array_equal(sc.quantise(np.array([np.nan, np.inf, -np.inf, 16384.5, -1e9], np.float32)), [-2 ** 30, 2 ** 30, -2 ** 30, 2 ** 30, -2 ** 30])


def test_negative_sums_use_floor_division():
    """sum = -3 quanta over 2 pixels: floor((2 * -3 + 2) / 4) = -1, where C truncation of -4 / 4 ... and of -5 / 4 would give -1 too; over
    4 pixels with sum -3: floor((-6 + 4) / 8) = floor(-0.25) = -1, truncation gives 0"""
    q = np.float32(1.0 / 65536)
    x = np.array([[[-1 * q, -1 * q, -1 * q, 0.0]]], np.float32)
    out = sc.pool(x, np.zeros((1, 1, 4), np.int32), 1)
    assert (out == -q).all()
    # the positive mirror rounds half up: floor((6 + 4) / 8) = 1
    assert (sc.pool(-x, np.zeros((1, 1, 4), np.int32), 1) == q).all()
    # an exact half below zero: sum -2 over 4 -> floor((-4 + 4) / 8) = 0; sum -6 over 4 -> floor(-8 / 8) = -1
    assert (sc.pool(np.array([[[-q, -q, 0, 0]]], np.float32), np.zeros((1, 1, 4), np.int32), 1) == 0).all()
    assert (sc.pool(np.array([[[-2 * q, -2 * q, -q, -q]]], np.float32), np.zeros((1, 1, 4), np.int32), 1) == -q).all()


def test_snapping_scenario():
    """A 61 x 83 frame with a filled ellipse under +-12 colour noise, and logits that see the ellipse two pixels off, blurred (sigma 3) and
    noisy (N(0, 1.5) on +-4).  At cell 6, compactness 6, iters 3 every superpixel is pure -- none holds pixels of both classes -- so the
    pooled mask can follow the contour: on this restatement the plain mask's IoU against the truth is 0.8158 and the pooled mask's
    1.0000."""
    r = sc.snapping_reference()
    print("snapping scenario: IoU %.4f -> %.4f, %d impure pixels" % (r["iou_plain"], r["iou_pooled"], r["impure"]))
    assert r["impure"] == 0
    assert r["iou_plain"] <= 0.90
    assert r["iou_pooled"] >= 0.99


def test_check_superpixels_and_grid_shape():
    from osvos_pytorch_amd import _lib, superpixels
    assert (_lib.SUPERPIXELS_MAX_CELL, _lib.SUPERPIXELS_MAX_COMPACTNESS, _lib.SUPERPIXELS_MAX_ITERS, _lib.SUPERPIXELS_MAX_SIDE, _lib.SUPERPIXELS_MAX_K) == \
        (64, 64, 16, 16384, 2 ** 28)
    superpixels.check_superpixels(8, 10, 5)
    superpixels.check_superpixels(2, 0, 0)
    superpixels.check_superpixels(64, 64, 16)
    for bad in [(1, 10, 5), (65, 10, 5), (8, -1, 5), (8, 65, 5), (8, 10, -1), (8, 10, 17), (8.0, 10, 5), (8, True, 5), (8, 10, None)]:
        with pytest.raises(ValueError):
            superpixels.check_superpixels(*bad)
    assert superpixels.grid_shape(480, 854, 8) == (60, 107) == sc.grid_shape(480, 854, 8)
    assert superpixels.grid_shape(1, 1, 2) == (1, 1) and superpixels.grid_shape(70, 70, 64) == (2, 2)
    import inspect
    for fn in (superpixels.slic, superpixels.SuperpixelSnapper.__init__):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items() if k in sc.DEFAULTS}
        assert d == sc.DEFAULTS
    # the header carries the limits _lib mirrors
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "osvos_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define OSVOS_SUPERPIXELS_MAX_([A-Z]+) (\d+)", hdr)}
    assert got == dict(CELL=64, COMPACTNESS=64, ITERS=16, SIDE=16384, K=2 ** 28)
    with pytest.raises(RuntimeError):
        superpixels.slic(np.zeros((4, 4, 3), np.uint8))                                        # no CPU fallback
    import torch
    with pytest.raises(RuntimeError):
        superpixels.pool(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        superpixels.SuperpixelSnapper(cell=1)
    with pytest.raises(ValueError):
        superpixels.SuperpixelSnapper()(torch.zeros(4, 4))                                      # neither frames nor labels


def test_snap_flags_are_parsed_and_refused_before_gpu_work():
    import train_online
    base = ["--synthetic", "--device-augment"]
    a = train_online.parse_args(base + ["--snap-cell", "6", "--snap-compactness", "0", "--snap-iters", "16"])
    assert a.snap == dict(cell=6, compactness=0, iters=16)
    assert train_online.parse_args(base + ["--snap-cell", "8"]).snap == dict(cell=8, **{k: v for k, v in sc.DEFAULTS.items() if k != "cell"})
    assert train_online.parse_args(["--synthetic", "--multi-object", "--snap-cell", "8"]).snap["cell"] == 8
    d = train_online.parse_args(["--synthetic"])
    assert d.snap is None and d.snap_cell == 0 and (d.snap_compactness, d.snap_iters) == (10, 5)
    assert train_online.parse_args(base + ["--snap-cell", "0"]).snap is None
    for argv, word in [(["--synthetic", "--snap-cell", "8"], "--device-augment"),
                       (base + ["--snap-cell", "1"], "cell"), (base + ["--snap-cell", "65"], "cell"), (base + ["--snap-cell", "-3"], "cell"),
                       (base + ["--snap-cell", "8", "--snap-compactness", "65"], "compactness"),
                       (base + ["--snap-cell", "8", "--snap-compactness", "-1"], "compactness"),
                       (base + ["--snap-cell", "8", "--snap-iters", "17"], "iters"),
                       (base + ["--snap-iters", "-1"], "iters")]:                              # a bad value is refused with the option off, too
        with pytest.raises(SystemExit) as e:
            train_online.parse_args(argv)
        assert word in str(e.value), (argv, e.value)
