"""CPU: the numpy restatement of the motion-compensation rule (tests/flow_cases.py) is pinned here -- against a naive loop, on scenes whose
answer is known, and on the tracking scenario the feature exists for -- together with the host-side checks of osvos_pytorch_amd.flow and
the --flow-* rules of train_online.py.  The GPU tests compare the kernels against this restatement bit for bit."""
import numpy as np
import pytest

import flow_cases as fc


@pytest.mark.parametrize("c", [(9, 11, 2, 4, 3, 2, 1), (5, 3, 1, 8, 4, 2, 1), (7, 6, 1, 3, 2, 1, 0)], ids=["9x11", "5x3_frame_below_block", "7x6_odd_block"])
@pytest.mark.parametrize("kind", ["noise", "gradient"])
def test_restatement_against_the_naive_loop(c, kind):
    h, w, n, block, step, search, penalty = c
    prev, cur = fc.pair(kind, h, w, n, search)
    vec, cost = fc.block_match(prev, cur, search, block, step, penalty, median=0)
    nvec, ncost = fc.block_match_naive(prev, cur, search, block, step, penalty)
    assert vec.shape == (n,) + fc.grid_shape(h, w, step) + (2,) and vec.dtype == np.int32 and cost.dtype == np.int32
    assert np.array_equal(vec, nvec) and np.array_equal(cost, ncost)


def test_luma_is_the_integer_rule():
    bgr = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]], np.uint8)
    assert fc.luma(bgr).tolist() == [0, 255, (29 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (77 * 255 + 128) >> 8, (290 + 3000 + 2310 + 128) >> 8]
    assert 29 + 150 + 77 == 256


@pytest.mark.parametrize("c", [(45, 70, 1, 16, 4, 9, 3, 0), (37, 53, 2, 8, 4, 5, 0, 0), (33, 65, 1, 7, 5, 6, 2, 1)], ids=fc.case_id)
def test_shifted_noise_returns_the_shift_where_the_blocks_stay_inside(c):
    h, w, n, block, step, search, penalty, median = c
    r = fc.reference("noise", c)
    dx, dy = fc.shift_of(search)
    gh, gw = fc.grid_shape(h, w, step)
    off = (step - block) // 2
    top, left = np.arange(gh) * step + off, np.arange(gw) * step + off
    iy = (top >= 0) & (top + block <= h) & (top + dy >= 0) & (top + dy + block <= h)
    ix = (left >= 0) & (left + block <= w) & (left + dx >= 0) & (left + dx + block <= w)
    inside = iy[:, None] & ix[None, :]
    assert inside.sum() >= 4
    assert (r["vec"][:, inside] == (dx, dy)).all()
    assert (r["cost"][:, inside] == penalty * (abs(dx) + abs(dy))).all()


@pytest.mark.parametrize("c", fc.MATCH_CASES, ids=fc.case_id)
def test_constant_and_periodic_frames_give_zero_vectors(c):
    """every candidate of a constant frame costs the same, and a texture of period 2 x 2 repeats its zero cost at every even displacement
    inside the search range: the tie rule picks d = 0"""
    for kind in ("constant", "periodic"):
        r = fc.reference(kind, c)
        assert not r["vec"].any(), kind
        assert not r["cost"].any(), kind


def test_search_zero_gives_zero_vectors_and_the_identity_warp():
    prev, cur = fc.pair("noise", 21, 30, 2, 5)
    vec, cost = fc.block_match(prev, cur, search=0, block=8, step=4, penalty=7, median=1)
    assert not vec.any() and cost.min() > 0
    src = np.random.default_rng(0).integers(0, 256, size=(2, 21, 30), dtype=np.uint8)
    assert np.array_equal(fc.warp(src, vec, 4, fill=9), src)


def test_median_removes_a_single_outlier():
    vec = np.zeros((1, 5, 7, 2), np.int32)
    vec[..., 0], vec[..., 1] = 3, -2
    vec[0, 2, 3] = (40, 17)
    vec[0, 0, 0] = (-9, 9)                       # a corner: its clamped neighbourhood counts it four times, of nine
    out = fc.median_pass(vec)
    assert (out[..., 0] == 3).all() and (out[..., 1] == -2).all()
    # ... and a step edge between two regions stays where it is
    edge = np.zeros((1, 4, 6, 2), np.int32)
    edge[:, :, 3:, 0] = 5
    assert np.array_equal(fc.median_pass(edge), edge)


def test_warp_fills_exactly_where_the_source_leaves_the_frame():
    h, w, step = 13, 18, 4
    vec = fc.border_field(h, w, step)
    src = np.random.default_rng(1).integers(1, 256, size=(1, h, w), dtype=np.uint8)       # no zero: the fill is recognisable
    out = fc.warp(src, vec, step, fill=0)
    gh, gw = fc.grid_shape(h, w, step)
    for y in range(h):
        for x in range(w):
            dx, dy = vec[0, min(y // step, gh - 1), min(x // step, gw - 1)]
            inside = 0 <= y + dy < h and 0 <= x + dx < w
            assert out[0, y, x] == (src[0, y + dy, x + dx] if inside else 0), (y, x)
    assert (out == 0).any() and (out != 0).any()
    assert (out[0, :, w - 1] == 0).all() and (out[0, 4:8, w - 2] != 0).all()              # one pixel out at the last column only


def test_warp_moves_float_bits_untouched():
    h, w, step = 9, 10, 3
    rng = np.random.default_rng(2)
    bits = rng.integers(0, 2 ** 32, size=(1, h, w), dtype=np.uint64).astype(np.uint32)
    bits[0, 0, :4] = [0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000]                    # quiet and signalling NaNs with payloads, -0
    src = bits.view(np.float32)
    vec = np.zeros((1,) + fc.grid_shape(h, w, step) + (2,), np.int32)
    vec[..., 0], vec[..., 1] = 1, -1
    out = fc.warp(src, vec, step, fill=-0.0)
    assert out.dtype == np.float32
    want = np.full((1, h, w), 0x80000000, np.uint32)
    want[0, 1:, :w - 1] = bits[0, :h - 1, 1:]
    assert np.array_equal(out.view(np.uint32), want)
    assert 0xffc12345 in out.view(np.uint32)[0, 1]


def test_check_flow_and_grid_shape():
    from osvos_pytorch_amd import _lib, flow
    assert (_lib.FLOW_MAX_BLOCK, _lib.FLOW_MAX_STEP, _lib.FLOW_MAX_SEARCH, _lib.FLOW_MAX_PENALTY, _lib.FLOW_MAX_MEDIAN, _lib.FLOW_MAX_SIDE) == \
        (32, 32, 48, 65535, 8, 16384)
    flow.check_flow(24, 16, 4, 4, 1)
    flow.check_flow(0, 1, 1, 0, 0)
    flow.check_flow(48, 32, 32, 65535, 8)
    for bad in [(-1, 16, 4, 4, 1), (49, 16, 4, 4, 1), (24, 0, 4, 4, 1), (24, 33, 4, 4, 1), (24, 16, 0, 4, 1), (24, 16, 33, 4, 1), (24, 16, 4, -1, 1),
                (24, 16, 4, 65536, 1), (24, 16, 4, 4, -1), (24, 16, 4, 4, 9), (24.0, 16, 4, 4, 1), (24, 16, True, 4, 1)]:
        with pytest.raises(ValueError):
            flow.check_flow(*bad)
    assert flow.grid_shape(480, 854, 4) == (120, 214) == fc.grid_shape(480, 854, 4)
    assert flow.grid_shape(1, 1, 32) == (1, 1) and flow.grid_shape(33, 64, 32) == (2, 2)
    import inspect
    for fn in (flow.block_match, flow.MotionCompensator.__init__):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items() if k in fc.DEFAULTS}
        assert d == fc.DEFAULTS
    # the header carries the limits _lib mirrors
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "osvos_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define OSVOS_FLOW_MAX_([A-Z]+) (\d+)", hdr)}
    assert got == dict(BLOCK=32, STEP=32, SEARCH=48, PENALTY=65535, MEDIAN=8, SIDE=16384)
    with pytest.raises(RuntimeError):
        flow.block_match(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8))            # no CPU fallback
    import torch
    with pytest.raises(RuntimeError):
        flow.warp(torch.zeros(4, 4), torch.zeros(1, 1, 1, 2, dtype=torch.int32), 4)


def test_flow_flags_are_parsed_and_refused_before_gpu_work():
    import train_online
    base = ["--synthetic", "--device-augment"]
    a = train_online.parse_args(base + ["--track-components", "2", "--flow-search", "30", "--flow-block", "8", "--flow-step", "2", "--flow-penalty", "0",
                                        "--flow-median", "3"])
    assert a.flow == dict(search=30, block=8, step=2, penalty=0, median=3)
    a = train_online.parse_args(base + ["--adapt-steps", "2", "--flow-search", "24"])
    assert a.flow == dict(fc.DEFAULTS)
    d = train_online.parse_args(["--synthetic"])
    assert d.flow is None and d.flow_search == 0 and (d.flow_block, d.flow_step, d.flow_penalty, d.flow_median) == (16, 4, 4, 1)
    assert train_online.parse_args(base + ["--track-components", "2", "--flow-search", "0"]).flow is None
    for argv, word in [(base + ["--flow-search", "24"], "--adapt-steps or --track-components"),
                       (["--synthetic", "--track-components", "2", "--flow-search", "24"], "--device-augment"),
                       (["--synthetic", "--multi-object", "--track-components", "2", "--flow-search", "24"], "--multi-object"),
                       (["--synthetic", "--multi-object", "--device-augment", "--track-components", "2", "--flow-search", "24"], "--multi-object"),
                       (base + ["--track-components", "2", "--flow-search", "49"], "search"),
                       (base + ["--track-components", "2", "--flow-search", "-1"], "search"),
                       (base + ["--track-components", "2", "--flow-search", "24", "--flow-block", "33"], "block"),
                       (base + ["--track-components", "2", "--flow-search", "24", "--flow-step", "0"], "step"),
                       (base + ["--track-components", "2", "--flow-search", "24", "--flow-penalty", "65536"], "penalty"),
                       (base + ["--track-components", "2", "--flow-median", "9"], "median")]:
        with pytest.raises(SystemExit) as e:
            train_online.parse_args(argv)
        assert word in str(e.value), (argv, e.value)


def test_component_tracker_seed_is_refused_on_the_host():
    """the setter's shape rule needs no device: a CPU tensor of the wrong shape and a non-tensor are ValueErrors"""
    import torch
    from osvos_pytorch_amd.results import ComponentTracker
    assert isinstance(ComponentTracker.seed, property) and ComponentTracker.seed.fset is not None
    t = ComponentTracker.__new__(ComponentTracker)
    t.h, t.w, t._seed = 4, 5, torch.zeros(1, 4, 5, dtype=torch.uint8)
    assert t.seed is t._seed
    for bad in (torch.zeros(4, 5, dtype=torch.uint8), torch.zeros(1, 5, 4, dtype=torch.uint8), torch.zeros(2, 4, 5, dtype=torch.uint8), None, 3):
        with pytest.raises(ValueError):
            t.seed = bad


def test_tracking_scenario_needs_the_motion_field():
    """a textured square moves 32 pixels a frame -- more than its own 24 -- over a static textured background, next to a static distractor.
    Unwarped, the previous mask stays farther than the tracker radius from the object in every frame (the tracker would drop it); warped
    along the field it overlaps the object in every frame and never comes within the radius of the distractor."""
    t = fc.TRACK
    frames, masks, blob = fc.tracking_scene()
    assert t["speed"] >= 30 and t["speed"] > t["size"] and t["speed"] <= t["search"]
    kw = {k: t[k] for k in ("search", "block", "step", "penalty", "median")}
    prev = masks[0]
    for f in range(1, t["frames"]):
        assert not (fc.dilate(prev, t["radius"]) & masks[f]).any(), f
        vec, _ = fc.block_match(frames[f - 1:f], frames[f:f + 1], **kw)
        warped = fc.warp(prev[None].astype(np.uint8), vec, t["step"])[0] > 0
        overlap = int((warped & masks[f]).sum())
        print("frame %d: the warped previous mask covers %d of the object's %d pixels" % (f, overlap, int(masks[f].sum())))
        assert overlap > 0, f
        assert not (fc.dilate(warped, t["radius"]) & blob).any(), f
        assert not (fc.dilate(masks[f], t["radius"]) & blob).any()
        prev = masks[f]                          # what a tracker seeded with `warped` keeps: the object's component, not the distractor
