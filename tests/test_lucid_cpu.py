"""CPU: the lucid rules of include/osvos_hip.h as tests/lucid_cases.py restates them -- the two-pass fill against a brute-force search, the
smoothing and the composition against naive per-pixel loops, their exact properties, the scenario (an object moved by its own width, with
and without inpainting), and what runs without a GPU of osvos_pytorch_amd.lucid and of the --lucid* rules of train_online.py.  The GPU tests
compare the kernels against this restatement bit for bit."""
import numpy as np
import pytest

import lucid_cases as lc

SMALL = [(1, 1), (1, 7), (6, 1), (9, 9), (11, 11), (12, 15), (7, 10)]


@pytest.mark.parametrize("kind", lc.MASKS)
@pytest.mark.parametrize("h,w", SMALL)
def test_two_pass_fill_equals_the_brute_force_search(h, w, kind):
    bgr, hole = lc.frame_of("noise", h, w, 3), lc.mask_of(kind, h, w)
    assert np.array_equal(lc.fill(bgr, hole), lc.fill_brute(bgr, hole))


def test_the_three_parts_of_the_key_decide():
    """by hand.  'sides' on 11 x 11: the centre (5, 5) is 25 away from all four non-hole pixels (0, 5), (10, 5), (5, 0), (5, 10): the
    smallest qy wins, (0, 5).  (5, 3) sees (5, 0) at 9.  (6, 6): (10, 5) at 17 against (5, 10) at 17 -- the smaller qy, (5, 10).  'ring' on
    9 x 9: (4, 4) is 16 from (0, 4), (8, 4), (4, 0), (4, 8): (0, 4).  (4, 3): (4, 0) at 9.  (2, 2): (0, 2) and (2, 0) at 4 -- qy decides for
    (0, 2); and in a row of its own qx decides: hole (0, 1) between (0, 0) and (0, 2) takes (0, 0)."""
    bgr, hole = lc.frame_of("noise", 11, 11, 3), lc.mask_of("sides", 11, 11)
    out = lc.fill(bgr, hole)
    assert np.array_equal(out[5, 5], bgr[0, 5]) and np.array_equal(out[5, 3], bgr[5, 0]) and np.array_equal(out[6, 6], bgr[5, 10])
    bgr, hole = lc.frame_of("noise", 9, 9, 3), lc.mask_of("ring", 9, 9)
    out = lc.fill(bgr, hole)
    assert np.array_equal(out[4, 4], bgr[0, 4]) and np.array_equal(out[4, 3], bgr[4, 0]) and np.array_equal(out[2, 2], bgr[0, 2])
    bgr = lc.frame_of("noise", 1, 3, 3)
    assert np.array_equal(lc.fill(bgr, np.array([[0, 9, 0]], np.uint8))[0, 1], bgr[0, 0])
    # the column pass: above wins the tie with below
    assert lc.column_nearest(np.array([[0], [1], [1], [1], [0], [1]], np.uint8))[:, 0].tolist() == [0, 0, 0, 4, 4, 4]
    assert lc.column_nearest(np.ones((3, 2), np.uint8)).tolist() == [[-1, -1]] * 3


@pytest.mark.parametrize("kind", ["blob", "checker", "full", "corner"])
@pytest.mark.parametrize("h,w,radius,passes", [(7, 10, 1, 2), (9, 6, 2, 3), (5, 5, 8, 1), (1, 1, 1, 1)])
def test_smoothing_equals_the_naive_loop(h, w, radius, passes, kind):
    bgr, hole = lc.frame_of("noise", h, w, 4), lc.mask_of(kind, h, w)
    assert np.array_equal(lc.smooth(bgr, hole, radius, passes), lc.smooth_naive(bgr, hole, radius, passes))


def test_smoothing_rounds_half_up_and_clips_the_window():
    img = np.zeros((1, 2, 3), np.uint8)
    img[0, 1] = (1, 2, 255)
    out = lc.smooth(img, np.array([[1, 0]], np.uint8), 1, 1)       # n = 2: floor((2 * 1 + 2) / 4) = 1, floor((4 + 2) / 4) = 1, floor(512 / 4) = 128
    assert out[0, 0].tolist() == [1, 1, 128] and out[0, 1].tolist() == [1, 2, 255]


@pytest.mark.parametrize("c", lc.INPAINT_CASES, ids=lc.case_id)
def test_inpainting_properties(c):
    h, w, kind, radius, passes = c
    r = lc.inpaint_reference(c)
    keep = r["hole"] == 0
    assert np.array_equal(r["out"][keep], r["bgr"][keep]) and np.array_equal(r["filled"][keep], r["bgr"][keep])      # non-hole pixels never change
    if passes == 0:
        assert np.array_equal(r["out"], r["filled"])
    if not keep.any():
        assert np.array_equal(r["filled"], r["bgr"])                                                                # a full hole copies the frame
    else:                                                                                                              # every fill colour is a non-hole colour
        have = {tuple(v) for v in r["bgr"][keep]}
        assert {tuple(v) for v in r["filled"][~keep]} <= have
    assert np.array_equal(lc.inpaint(r["bgr"], r["hole"], radius, passes), r["out"])


@pytest.mark.parametrize("kind", ["identity", "shift_part", "rot30_s075", "mirror", "tone_low", "tone_high", "mixed"])
@pytest.mark.parametrize("h,w,mask", [(5, 7, "blob"), (4, 3, "checker"), (1, 1, "full")])
def test_composition_equals_the_naive_loop(h, w, mask, kind):
    bgr, bg, m = lc.frame_of("noise", h, w, 5), lc.frame_of("gradient", h, w), lc.mask_of(mask, h, w)
    M, tone = lc.params_of(kind, h, w, 3 if kind == "mixed" else 1)
    got, want = lc.compose(bgr, m, bg, M, tone), lc.compose_naive(bgr, m, bg, M, tone)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("mask", ["blob", "checker", "empty", "full"])
def test_identity_composition_is_the_frame_minus_the_mean(mask):
    h, w = 13, 17
    bgr, bg, m = lc.frame_of("noise", h, w, 6), lc.frame_of("gradient", h, w), lc.mask_of(mask, h, w)
    M, tone = lc.params_of("identity", h, w, 1)
    plain = (bgr.astype(np.float32) - np.asarray(lc.MEAN, np.float32)).transpose(2, 0, 1)
    image, gt = lc.compose(bgr, m, bg, M, tone)
    on = m != 0
    assert np.array_equal(gt[0, 0], on.astype(np.float32))
    assert np.array_equal(image[0][:, on], plain[:, on])
    back = (bg.astype(np.float32) - np.asarray(lc.MEAN, np.float32)).transpose(2, 0, 1)
    assert np.array_equal(image[0][:, ~on], back[:, ~on])
    image, _ = lc.compose(bgr, m, bgr, M, tone)                      # bg == bgr: the whole frame
    assert np.array_equal(image[0], plain)


@pytest.mark.parametrize("dx,dy", [(3, 0), (-2, 5), (0, -4), (20, 0), (-6, -6)])
def test_integer_translations_move_the_label_exactly(dx, dy):
    h, w = 14, 19
    bgr, m = lc.frame_of("noise", h, w, 7), lc.mask_of("blob", h, w)
    M = [[lc.affine_inverse(w / 2, h / 2, dx=dx, dy=dy), lc.IDENTITY]]
    assert M[0][0] == [1.0, 0.0, float(-dx), 0.0, 1.0, float(-dy)]
    image, gt = lc.compose(bgr, m, bgr, M, [[lc.NEUTRAL, lc.NEUTRAL]])
    want = np.zeros((h, w), np.float32)
    ys, xs = np.nonzero(m)
    ok = (ys + dy >= 0) & (ys + dy < h) & (xs + dx >= 0) & (xs + dx < w)
    want[ys[ok] + dy, xs[ok] + dx] = 1
    assert np.array_equal(gt[0, 0], want)
    if dx == 20:
        assert not gt.any()                                          # pushed wholly out of the frame
    moved = want != 0                                                # the object's own colours travel with it
    src = (bgr.astype(np.float32) - np.asarray(lc.MEAN, np.float32)).transpose(2, 0, 1)
    assert np.array_equal(image[0][:, ys[ok] + dy, xs[ok] + dx], src[:, ys[ok], xs[ok]]) and moved.sum() == ok.sum()


def test_tone_clamps_at_both_ends():
    h, w = 6, 8
    bgr = lc.frame_of("noise", h, w, 8)
    full = lc.mask_of("full", h, w)
    zero = (0.0, 0.0, 0.0)
    low, _ = lc.compose(bgr, full, bgr, [[lc.IDENTITY, lc.IDENTITY]], [[(256, 256, 256, -255, -255, -255), lc.NEUTRAL]], zero)
    high, _ = lc.compose(bgr, full, bgr, [[lc.IDENTITY, lc.IDENTITY]], [[(1024, 1024, 1024, 255, 255, 255), lc.NEUTRAL]], zero)
    assert (low == 0).all() and (high == 255).all()
    part, _ = lc.compose(bgr, full, bgr, [[lc.IDENTITY, lc.IDENTITY]], [[(512, 128, 0, -100, 100, 7), lc.NEUTRAL]], zero)
    v = bgr.astype(np.int64)
    want = np.stack([np.clip(2 * v[..., 0] - 100, 0, 255), np.clip(v[..., 1] * 128 * 1024 // 256 + 100 * 1024, 0, 255 << 10) / 1024.0,
                     np.full((h, w), 7)]).astype(np.float32)
    assert np.array_equal(part[0], want)
    # the largest composite stays inside int32
    assert 1024 * (255 << 10) < 2 ** 31 and (255 << 10) * 1024 + 128 < 2 ** 31


def test_scenario_moving_the_object_needs_the_inpainted_background():
    """A textured red square on a blue-green gradient, moved right by its own width.  Composited over the frame itself the object shows
    twice: every pixel of its old place still carries the object's texture.  Composited over the inpainted frame no pixel of the old place
    is closer to any of the object's colours than to the true background behind it.  (Without the inpainting step -- bg = frame -- the
    second half fails: that is the first half.)"""
    r = lc.scenario_reference()
    s = lc.SCENE
    old = np.zeros(r["mask"].shape, bool)
    old[s["y0"]:s["y0"] + s["side"], s["x0"]:s["x0"] + s["side"]] = True
    new = np.roll(old, s["side"], axis=1)
    assert np.array_equal(r["gt"] != 0, new) and not (old & new).any()
    frame = r["frame"].astype(np.float32).transpose(2, 0, 1)
    for name in ("plain", "lucid"):
        assert np.array_equal(r[name][:, new], frame[:, old]), name                   # the moved object, in both
    colours = np.unique(r["frame"][old].reshape(-1, 3), axis=0).astype(np.float64)

    def distances(image):
        px = image[:, old].T.astype(np.float64)
        d_obj = ((px[:, None, :] - colours[None]) ** 2).sum(-1).min(1)
        d_back = ((px - r["back"][old].astype(np.float64)) ** 2).sum(-1)
        return d_obj, d_back
    d_obj, d_back = distances(r["plain"])
    assert (d_obj == 0).all() and (d_back > d_obj).all()                                # the object twice
    d_obj, d_back = distances(r["lucid"])
    print("scenario: old place, squared colour distance to the background behind it at most %.0f, to the object's colours at least %.0f"
          % (d_back.max(), d_obj.min()))
    assert (d_back < d_obj).all()
    assert np.array_equal(r["bg"][r["hole"] == 0], r["frame"][r["hole"] == 0]) and (r["hole"][old] != 0).all()


def test_check_lucid_and_affine_inverse():
    from osvos_pytorch_amd import _lib, lucid
    assert (_lib.LUCID_MAX_BATCH, _lib.LUCID_MAX_SIDE, _lib.LUCID_MAX_RADIUS, _lib.LUCID_MAX_PASSES, _lib.LUCID_MAX_GAIN) == (16, 4096, 8, 8, 1024)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "osvos_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define OSVOS_LUCID_MAX_([A-Z]+) (\d+)", hdr)}
    assert got == dict(BATCH=16, SIDE=4096, RADIUS=8, PASSES=8, GAIN=1024)
    lucid.check_lucid()
    lucid.check_lucid(1.0, 0, 1, 0, 0.0, 0.0, 0.0, 0)
    lucid.check_lucid(0.5, 64, 8, 8, 4.0, 1.0, 1.0, 255)
    for bad in [dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(grow=-1), dict(grow=65), dict(grow=2.0), dict(radius=0), dict(radius=9),
                dict(passes=-1), dict(passes=9), dict(passes=True), dict(fg_shift=-1), dict(bg_shift=1.5), dict(gain=1.1), dict(offset=256),
                dict(offset=1.5), dict(gain=None)]:
        with pytest.raises(ValueError):
            lucid.check_lucid(**bad)
    import inspect
    for fn in (lucid.inpaint, lucid.LucidDream.__init__, lucid.check_lucid):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items() if k in lc.DEFAULTS}
        assert d == {k: v for k, v in lc.DEFAULTS.items() if k in d} and d
    assert lucid.affine_inverse(3.5, 2.0) == list(lc.IDENTITY) and lucid.IDENTITY == lc.IDENTITY and lucid.NEUTRAL == lc.NEUTRAL
    for args in [(10.0, 7.5, 30.0, 0.75, 2.0, -3.0, False), (4.0, 4.0, -12.5, 1.25, 0.0, 0.0, True), (0.0, 0.0, 0.0, 1.0, 5.0, 0.0, False)]:
        assert lucid.affine_inverse(*args) == lc.affine_inverse(*args)
    # the pivot is a fixed point without a shift; a shift moves it; mirroring negates the x offset of the source
    m = lucid.affine_inverse(10.0, 7.5, 25.0, 0.8)
    assert abs(m[0] * 10 + m[1] * 7.5 + m[2] - 10) < 1e-12 and abs(m[3] * 10 + m[4] * 7.5 + m[5] - 7.5) < 1e-12
    m = lucid.affine_inverse(10.0, 7.5, 0.0, 1.0, 0.0, 0.0, True)
    assert m == [-1.0, 0.0, 20.0, 0.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        lucid.affine_inverse(0, 0, 0, 0.0)
    import torch
    with pytest.raises(RuntimeError):
        lucid.inpaint(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8))                 # no CPU fallback
    with pytest.raises(RuntimeError):
        lucid.compose(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, 3, dtype=torch.uint8),
                      [[lc.IDENTITY, lc.IDENTITY]], [[lc.NEUTRAL, lc.NEUTRAL]])
    with pytest.raises(ValueError):
        lucid.inpaint(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), radius=0)      # parameters before tensors


def test_lucid_flags_are_parsed_and_refused_before_gpu_work():
    import subprocess
    import sys
    import os
    import train_online
    base = ["--synthetic", "--device-augment"]
    a = train_online.parse_args(base + ["--lucid", "0.5", "--lucid-grow", "3", "--lucid-smooth", "1,0", "--lucid-shift", "0.5,0.1", "--lucid-tone", "0.3,10"])
    assert a.lucid == dict(p=0.5, grow=3, radius=1, passes=0, fg_shift=0.5, bg_shift=0.1, gain=0.3, offset=10)
    assert train_online.parse_args(base + ["--lucid", "1"]).lucid == dict(p=1.0, fg_shift=0.25, bg_shift=0.05, gain=0.2, offset=20, **lc.DEFAULTS)
    assert train_online.parse_args(base + ["--multi-object", "--lucid", "0.25"]).lucid["p"] == 0.25
    d = train_online.parse_args(["--synthetic"])
    assert d.lucid is None and d.lucid_p == 0.0
    assert train_online.parse_args(base + ["--lucid", "0"]).lucid is None
    bad = [(["--synthetic", "--lucid", "0.5"], "--device-augment"), (["--synthetic", "--multi-object", "--lucid", "0.5"], "--device-augment"),
           (base + ["--lucid", "1.5"], "p"), (base + ["--lucid", "-0.1"], "p"), (base + ["--lucid", "0.5", "--lucid-grow", "65"], "grow"),
           (base + ["--lucid-grow", "-1"], "grow"), (base + ["--lucid-smooth", "0,3"], "radius"), (base + ["--lucid-smooth", "2,9"], "passes"),
           (base + ["--lucid-smooth", "2"], "--lucid-smooth"), (base + ["--lucid-smooth", "2.5,1"], "--lucid-smooth"),
           (base + ["--lucid-shift", "5,0"], "fg_shift"), (base + ["--lucid-shift", "0,1.5"], "bg_shift"), (base + ["--lucid-tone", "2,0"], "gain"),
           (base + ["--lucid-tone", "0.2,300"], "offset"), (base + ["--lucid-tone", "x,y"], "--lucid-tone")]
    for argv, word in bad:                                            # a bad value is refused with the option off, too
        with pytest.raises(SystemExit) as e:
            train_online.parse_args(argv)
        assert word in str(e.value), (argv, e.value)
    # in a process of its own: the refusal comes before the GPU library is loaded
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, train_online\n"
            "for argv in (['--synthetic', '--lucid', '0.5'], ['--synthetic', '--device-augment', '--lucid-smooth', '9,9']):\n"
            "    try:\n"
            "        train_online.parse_args(argv)\n"
            "        sys.exit(3)\n"
            "    except SystemExit as e:\n"
            "        assert '--lucid' in str(e), e\n"
            "from osvos_pytorch_amd import _lib\n"
            "assert _lib._lib is None\n"
            "print('refused before the library')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=repo, env=dict(os.environ, PYTHONPATH=repo), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refused before the library" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
