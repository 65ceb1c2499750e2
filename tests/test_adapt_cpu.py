"""CPU: the numpy restatements the online-adaptation GPU tests compare against (tests/adapt_cases.py) checked on their own -- the brute-force
squared distance against scipy's exact Euclidean transform, the erosion and border rules of the adaptation targets on hand-made masks, the
shared target cases (all three classes present) -- and the refusals of train_online.py's new flags, which happen before any GPU work."""
import numpy as np
import pytest

import adapt_cases as ac


def _edt_sq(src):
    from scipy.ndimage import distance_transform_edt
    return np.rint(distance_transform_edt(~src) ** 2).astype(np.int64)


@pytest.mark.parametrize("kind", [k for k in ac.MASK_KINDS if k != "empty"])
@pytest.mark.parametrize("n,h,w", [(2, 37, 65), (1, 5, 130), (3, 1, 63), (1, 33, 1)], ids=lambda v: str(v))
def test_brute_force_sqdist_equals_scipy_edt_squared(kind, n, h, w):
    mask = ac.make_mask(kind, n, h, w)
    for invert in (0, 1):
        got = ac.sqdist_of_mask(mask, invert)
        assert got.dtype == np.int32
        for k in range(n):
            src = (mask[k] != 0) != bool(invert)
            if not src.any():
                assert (got[k] == ac.NONE).all()
            else:
                assert np.array_equal(got[k].astype(np.int64), _edt_sq(src)), (kind, invert, k)


def test_sqdist_of_an_empty_image_is_none_and_images_do_not_mix():
    m = np.zeros((3, 4, 6), dtype=np.uint8)
    m[0, 1, 2] = m[2, 3, 5] = 9
    d = ac.sqdist_of_mask(m, 0)
    assert (d[1] == ac.NONE).all() and d[0, 1, 2] == 0 and d[0, 3, 5] == 4 + 9 and d[2, 0, 0] == 9 + 25
    assert (ac.sqdist_of_mask(np.ones((1, 3, 3), np.uint8), 1) == ac.NONE).all()


def test_erosion_and_border_rules_on_5x5_masks():
    full = np.ones((1, 5, 5), dtype=np.uint8)
    # the image border is not background: a mask that fills the image erodes to itself, whatever the erosion
    assert ac.eroded(full, 3).all() and ac.eroded(full, 100).all()
    # erosion 0 keeps the mask
    m = np.zeros((1, 5, 5), dtype=np.uint8)
    m[0, 1:4, 1:5] = 1                                   # 3 x 4 block that touches the right border
    assert np.array_equal(ac.eroded(m, 0), m != 0)
    # erosion 1: a pixel stays when its nearest background pixel is farther than 1 -- the border column stays, the block's rim goes
    e1 = np.zeros((1, 5, 5), dtype=bool)
    e1[0, 2, 2:5] = True
    assert np.array_equal(ac.eroded(m, 1), e1)
    # erosion 2 empties it; then every pixel is negative, whatever the logits and the distance
    assert not ac.eroded(m, 2).any()
    lab, cnt = ac.targets_reference(np.full((1, 5, 5), 9.0, np.float32), m, 0.0, 2, 1000)
    assert (lab == 0).all() and cnt.tolist() == [[0, 25, 0]]
    # distance: strictly farther than `distance` is negative; positives need logit > pos_logit, strictly; NaN is void
    lg = np.full((1, 5, 5), 1.0, np.float32)
    lg[0, 2, 3], lg[0, 2, 4], lg[0, 1, 1] = 0.5, np.nan, np.inf
    lab, cnt = ac.targets_reference(lg, m, 0.5, 1, 1)
    want = np.zeros((5, 5), np.float32)
    want[1:4, 2:5] = 1                                   # within 1 px of E = row 2, columns 2..4 ...
    want[2, 1] = 1
    want[2, 3] = want[2, 4] = -1                         # ... of which one sits exactly at the threshold and one is NaN
    assert np.array_equal(lab[0], want) and cnt.tolist() == [[8, 15, 2]]


@pytest.mark.parametrize("h,w,erosion,distance,want", ac.TARGET_CASES, ids=["48x80", "37x53", "64x96"])
def test_target_cases_hold_all_three_classes(h, w, erosion, distance, want):
    logits, prev = ac.target_case(h, w)
    lab, cnt = ac.targets_reference(logits, prev, ac.POS_LOGIT, erosion, distance)
    assert tuple(cnt[0]) == want and min(want) > 0 and sum(want) == h * w
    assert [(lab == v).sum() for v in (1, 0, -1)] == list(want)


def test_new_script_flags_are_parsed_and_refused_before_gpu_work():
    import train_online
    a = train_online.parse_args(["--synthetic", "--device-augment", "--synthetic-frames", "3", "--adapt-steps", "2", "--adapt-mix", "2",
                                 "--adapt-distance", "12", "--adapt-erosion", "2"])
    assert (a.adapt_steps, a.adapt_mix, a.adapt_distance, a.adapt_erosion, a.synthetic_frames) == (2, 2, 12, 2, 3)
    assert a.adapt_lr is None and a.adapt_prob == 0.97 and a.adapt_weight == 1.0
    d = train_online.parse_args(["--synthetic"])
    assert d.adapt_steps == 0 and d.synthetic_frames == 1 and (d.adapt_mix, d.adapt_erosion, d.adapt_distance) == (5, 15, 220)
    for argv, word in [(["--synthetic", "--adapt-steps", "2"], "--device-augment"),
                       (["--synthetic", "--multi-object", "--adapt-steps", "2"], "--multi-object"),
                       (["--synthetic", "--device-augment", "--adapt-steps", "2", "--tta-flip"], "--tta"),
                       (["--synthetic", "--device-augment", "--adapt-steps", "2", "--adapt-mix", "0"], "--adapt-mix"),
                       (["--synthetic", "--device-augment", "--adapt-steps", "2", "--adapt-prob", "1.0"], "--adapt-prob"),
                       (["--synthetic", "--device-augment", "--adapt-steps", "2", "--adapt-erosion", "-1"], "--adapt-erosion"),
                       (["--synthetic", "--device-augment", "--adapt-steps", "2", "--adapt-lr", "0"], "--adapt-lr"),
                       (["--synthetic", "--device-augment", "--adapt-steps", "-1"], "--adapt-steps"),
                       (["--synthetic", "--synthetic-frames", "2"], "--synthetic-frames"),
                       (["--device-augment", "--synthetic-frames", "2"], "--synthetic-frames"),
                       (["--synthetic", "--device-augment", "--synthetic-frames", "0"], "--synthetic-frames")]:
        with pytest.raises(SystemExit) as e:
            train_online.parse_args(argv)
        assert word in str(e.value), (argv, e.value)
