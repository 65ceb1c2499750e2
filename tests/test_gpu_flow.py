"""GPU: motion compensation on the device -- osvos_flow_block_match and osvos_flow_warp (csrc/flow.hip) against the numpy restatement of the
rule in tests/flow_cases.py, bit for bit (the rule is integer arithmetic: every comparison is np.array_equal, there is no tolerance), their
exact properties, the wrappers of osvos_pytorch_amd.flow, the tracking scenario through results.ComponentTracker, and train_online.py
--flow-search.  vec, cost, out and the workspace are pre-filled with garbage before every call."""
import ctypes as C

import numpy as np
import pytest
import torch

import flow_cases as fc
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE_INT = 0x5a5a5a5a
GARBAGE_BYTE = 0xa5
GUARD = 256


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(n, h, w, block, step, search, median):
    """a garbage-filled workspace of exactly osvos_flow_ws_bytes bytes inside a larger buffer: (the whole buffer, the size asked for)"""
    from osvos_pytorch_amd import _lib
    need = int(_lib.lib().osvos_flow_ws_bytes(n, h, w, block, step, search, median))
    assert need >= 2 * n * h * w
    return torch.full((need + GUARD,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8), need


def _match_rc(prev, cur, block, step, search, penalty, median, with_cost=True, ws=None):
    """one osvos_flow_block_match call through _lib on CUDA uint8 [N,H,W,3] tensors -> (rc, vec, cost or None, ws buffer, ws bytes)"""
    from osvos_pytorch_amd import _lib
    n, h, w = (int(v) for v in cur.shape[:3])
    gh, gw = fc.grid_shape(h, w, max(step, 1))
    vec = torch.full((n, gh, gw, 2), GARBAGE_INT, device="cuda", dtype=torch.int32)
    cost = torch.full((n, gh, gw), GARBAGE_INT, device="cuda", dtype=torch.int32) if with_cost else None
    buf, need = ws if ws is not None else _ws(n, h, w, block, step, search, median)
    vp = C.c_void_p
    rc = _lib.lib().osvos_flow_block_match(vp(prev.data_ptr()), vp(cur.data_ptr()), vp(vec.data_ptr()), vp(cost.data_ptr()) if with_cost else None,
                                           vp(buf.data_ptr()), n, h, w, block, step, search, penalty, median, _stream())
    return rc, vec, cost, buf, need


def _match(prev, cur, block, step, search, penalty, median, with_cost=True):
    from osvos_pytorch_amd import _lib
    rc, vec, cost, buf, need = _match_rc(prev, cur, block, step, search, penalty, median, with_cost)
    _lib.check(rc, "flow_block_match")
    assert bool((buf[need:] == GARBAGE_BYTE).all()), "the call wrote past osvos_flow_ws_bytes"
    return vec, cost


def _warp_rc(src, vec, step, fill, out=None):
    from osvos_pytorch_amd import _lib
    n, h, w = (int(v) for v in src.shape)
    if out is None:
        out = torch.full_like(src, float("nan")) if src.dtype == torch.float32 else torch.full_like(src, GARBAGE_BYTE)
    vp = C.c_void_p
    rc = _lib.lib().osvos_flow_warp(vp(src.data_ptr()), 1 if src.dtype == torch.float32 else 0, vp(vec.data_ptr()), vp(out.data_ptr()), n, h, w, step,
                                    float(fill), _stream())
    return rc, out


def _warp(src, vec, step, fill):
    from osvos_pytorch_amd import _lib
    rc, out = _warp_rc(src, vec, step, fill)
    _lib.check(rc, "flow_warp")
    return out


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t).view(np.uint32)


def _against_restatement(kind, c):
    h, w, n, block, step, search, penalty, median = c
    r = fc.reference(kind, c)
    vec, cost = _match(_dev(r["prev"]), _dev(r["cur"]), block, step, search, penalty, median)
    vec, cost = _np(vec), _np(cost)
    print("%s %s: %d of %d vectors and %d of %d costs differ" % (fc.case_id(c), kind, int((vec != r["vec"]).any(-1).sum()), cost.size,
                                                                int((cost != r["cost"]).sum()), cost.size))
    assert np.array_equal(cost, r["cost"])
    assert np.array_equal(vec, r["vec"])


@pytest.mark.parametrize("kind", fc.SCENES)
@pytest.mark.parametrize("c", fc.MATCH_CASES, ids=fc.case_id)
def test_block_match_against_the_restatement(c, kind):
    _against_restatement(kind, c)


@pytest.mark.parametrize("kind", fc.SCENES)
def test_block_match_on_a_davis_sized_frame(kind):
    _against_restatement(kind, fc.LARGE_CASE)


def _warp_sources(n, h, w, seed):
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    bits = rng.integers(0, 2 ** 32, size=(n, h, w), dtype=np.uint64).astype(np.uint32)      # every bit pattern, NaNs of any payload among them
    bits.reshape(-1)[:4] = [0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000][:bits.size]
    return u8, bits.view(np.float32)


@pytest.mark.parametrize("c", fc.MATCH_CASES, ids=fc.case_id)
def test_warp_along_the_matched_fields(c):
    h, w, n, block, step, search, penalty, median = c
    u8, f32 = _warp_sources(n, h, w, 5)
    for kind in ("noise", "gradient"):
        vec = fc.reference(kind, c)["vec"]
        got = _warp(_dev(u8), _dev(vec), step, 7)
        assert np.array_equal(_np(got), fc.warp(u8, vec, step, 7)), kind
        got = _warp(_dev(f32), _dev(vec), step, -0.0)
        assert np.array_equal(_bits(got), fc.warp(f32, vec, step, -0.0).view(np.uint32)), kind


@pytest.mark.parametrize("h,w,n,step", [(13, 18, 2, 4), (37, 300, 1, 5), (1, 1, 1, 1), (40, 64, 1, 32), (9, 7, 1, 3)])
def test_warp_along_a_field_that_leaves_every_border(h, w, n, step):
    vec = fc.border_field(h, w, step, n)
    u8, f32 = _warp_sources(n, h, w, 6)
    want = fc.warp(u8, vec, step, 255)
    assert np.array_equal(_np(_warp(_dev(u8), _dev(vec), step, 255)), want)
    got = _warp(_dev(f32), _dev(vec), step, float("inf"))
    assert np.array_equal(_bits(got), fc.warp(f32, vec, step, np.inf).view(np.uint32))
    # a field with vectors far beyond any frame
    far = np.full_like(vec, 2 ** 31 - 1)
    far[..., 1] = -2 ** 31
    assert np.array_equal(_np(_warp(_dev(u8), _dev(far), step, 3)), np.full_like(u8, 3))


def test_search_zero_gives_zero_vectors_and_the_identity_warp():
    h, w, n = 37, 53, 2
    prev, cur = fc.pair("noise", h, w, n, 5)
    vec, cost = _match(_dev(prev), _dev(cur), 8, 4, 0, 9, 1)
    want_vec, want_cost = fc.block_match(prev, cur, 0, 8, 4, 9, 1)
    assert not _np(vec).any() and np.array_equal(_np(cost), want_cost) and not want_vec.any()
    u8, f32 = _warp_sources(n, h, w, 7)
    assert np.array_equal(_np(_warp(_dev(u8), vec, 4, 9)), u8)
    assert np.array_equal(_bits(_warp(_dev(f32), vec, 4, 1.5)), f32.view(np.uint32))


def test_frames_of_a_batch_are_independent_and_calls_repeat():
    for c in [(40, 64, 3, 4, 1, 3, 0, 0), (37, 53, 2, 16, 4, 7, 2, 2)]:
        h, w, n, block, step, search, penalty, median = c
        prev, cur = (_dev(a) for a in fc.pair("noise", h, w, n, search))
        vec, cost = _match(prev, cur, *c[3:])
        again = _match(prev, cur, *c[3:])
        assert torch.equal(vec, again[0]) and torch.equal(cost, again[1])
        for i in range(n):
            one = _match(prev[i:i + 1].contiguous(), cur[i:i + 1].contiguous(), *c[3:])
            assert torch.equal(vec[i:i + 1], one[0]) and torch.equal(cost[i:i + 1], one[1]), i
        assert not torch.equal(cost[0], cost[1])
        src = _dev(_warp_sources(n, h, w, 8)[0])
        out = _warp(src, vec, step, 0)
        assert torch.equal(out, _warp(src, vec, step, 0))
        for i in range(n):
            assert torch.equal(out[i:i + 1], _warp(src[i:i + 1].contiguous(), vec[i:i + 1].contiguous(), step, 0))


def test_cost_may_be_null():
    c = (45, 70, 1, 16, 4, 9, 3, 1)
    r = fc.reference("noise", c)
    vec, cost = _match(_dev(r["prev"]), _dev(r["cur"]), *c[3:], with_cost=False)
    assert cost is None and np.array_equal(_np(vec), r["vec"])


def test_workspace_size_query():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    # the two luma planes, and with median passes a second vector grid; 0 for what the call refuses
    assert l.osvos_flow_ws_bytes(1, 480, 854, 16, 4, 24, 0) >= 2 * 480 * 854
    assert l.osvos_flow_ws_bytes(1, 480, 854, 16, 4, 24, 1) >= 2 * 480 * 854 + 120 * 214 * 8
    for bad in [(0, 8, 8, 8, 4, 2, 0), (1, 0, 8, 8, 4, 2, 0), (1, 8, 16385, 8, 4, 2, 0), (1, 8, 8, 33, 4, 2, 0), (1, 8, 8, 8, 0, 2, 0), (1, 8, 8, 8, 4, 49, 0),
                (1, 8, 8, 8, 4, 2, 9), (1, 8, 8, 8, 4, -1, 0)]:
        assert l.osvos_flow_ws_bytes(*bad) == 0, bad


def test_bad_arguments_return_an_error_and_launch_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    h, w = 12, 20
    prev, cur = (_dev(a) for a in fc.pair("noise", h, w, 1, 3))
    good = (8, 4, 3, 1, 1)
    for bad, word in [((0, 4, 3, 1, 1), b"block"), ((33, 4, 3, 1, 1), b"block"), ((8, 0, 3, 1, 1), b"step"), ((8, 33, 3, 1, 1), b"step"),
                      ((8, 4, -1, 1, 1), b"search"), ((8, 4, 49, 1, 1), b"search"), ((8, 4, 3, -1, 1), b"penalty"), ((8, 4, 3, 65536, 1), b"penalty"),
                      ((8, 4, 3, 1, -1), b"median"), ((8, 4, 3, 1, 9), b"median")]:
        rc, vec, cost, buf, _ = _match_rc(prev, cur, *bad, ws=_ws(1, h, w, *good[:3], good[4]))
        assert rc < 0 and word in l.osvos_last_error(), (bad, l.osvos_last_error())
        torch.cuda.synchronize()
        assert bool((vec == GARBAGE_INT).all()) and bool((cost == GARBAGE_INT).all()) and bool((buf == GARBAGE_BYTE).all()), bad
    vp = C.c_void_p
    vec = torch.full((1, 3, 5, 2), GARBAGE_INT, device="cuda", dtype=torch.int32)
    buf, _ = _ws(1, h, w, 8, 4, 3, 1)
    args = (1, h, w, 8, 4, 3, 1, 1, _stream())
    assert l.osvos_flow_block_match(None, vp(cur.data_ptr()), vp(vec.data_ptr()), None, vp(buf.data_ptr()), *args) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_flow_block_match(vp(prev.data_ptr()), vp(cur.data_ptr()), None, None, vp(buf.data_ptr()), *args) < 0
    assert l.osvos_flow_block_match(vp(prev.data_ptr()), vp(cur.data_ptr()), vp(vec.data_ptr()), None, None, *args) < 0
    assert l.osvos_flow_block_match(vp(prev.data_ptr()), vp(cur.data_ptr()), vp(vec.data_ptr()), None, vp(buf.data_ptr()), 0, h, w, 8, 4, 3, 1, 1, _stream()) < 0
    assert l.osvos_flow_block_match(vp(prev.data_ptr()), vp(cur.data_ptr()), vp(vec.data_ptr()), None, vp(buf.data_ptr()), 1, h, 16385, 8, 4, 3, 1, 1, _stream()) < 0
    torch.cuda.synchronize()
    assert bool((vec == GARBAGE_INT).all()) and bool((buf == GARBAGE_BYTE).all())
    with pytest.raises(RuntimeError):
        _lib.check(-1, "flow_block_match")
    # the warp
    src = _dev(_warp_sources(1, h, w, 9)[0])
    field = torch.zeros((1, 3, 5, 2), device="cuda", dtype=torch.int32)
    for step, fill, word in [(0, 0, b"step"), (33, 0, b"step"), (4, 256, b"fill"), (4, -1, b"fill"), (4, 0.5, b"fill"), (4, float("nan"), b"fill")]:
        rc, out = _warp_rc(src, field, step, fill)
        assert rc < 0 and word in l.osvos_last_error(), (step, fill, l.osvos_last_error())
        torch.cuda.synchronize()
        assert bool((out == GARBAGE_BYTE).all())
    rc, _ = _warp_rc(src, field, 4, 0, out=src)
    assert rc < 0 and b"out" in l.osvos_last_error()
    assert l.osvos_flow_warp(vp(src.data_ptr()), 2, vp(field.data_ptr()), vp(buf.data_ptr()), 1, h, w, 4, C.c_float(0), _stream()) < 0 and b"dtype" in l.osvos_last_error()
    assert l.osvos_flow_warp(None, 0, vp(field.data_ptr()), vp(buf.data_ptr()), 1, h, w, 4, C.c_float(0), _stream()) < 0
    assert l.osvos_flow_warp(vp(src.data_ptr()), 0, vp(field.data_ptr()), vp(buf.data_ptr()), 1, 0, w, 4, C.c_float(0), _stream()) < 0
    torch.cuda.synchronize()
    assert bool((buf == GARBAGE_BYTE).all())


def test_wrappers_match_the_direct_calls():
    from osvos_pytorch_amd import flow
    c = (45, 70, 1, 16, 4, 9, 3, 1)
    r = fc.reference("noise", c)
    prev, cur = _dev(r["prev"]), _dev(r["cur"])
    kw = dict(search=9, block=16, step=4, penalty=3, median=1)
    vec, cost = flow.block_match(prev, cur, **kw)
    assert vec.dtype == torch.int32 and cost.dtype == torch.int32 and np.array_equal(_np(vec), r["vec"]) and np.array_equal(_np(cost), r["cost"])
    one = flow.block_match(prev[0], cur[0], **kw)                                          # [H,W,3] for one frame
    assert torch.equal(one[0], vec) and torch.equal(one[1], cost)
    u8, f32 = _warp_sources(1, 45, 70, 10)
    want = fc.warp(u8, r["vec"], 4, 0)
    for shaped in (_dev(u8), _dev(u8)[:, None], _dev(u8)[0]):
        out = flow.warp(shaped, vec, 4)
        assert out.shape == shaped.shape and out.dtype == torch.uint8 and np.array_equal(_np(out).reshape(want.shape), want)
    mask = _dev(u8 > 127)
    out = flow.warp(mask, vec, 4, fill=1)
    assert out.dtype == torch.bool and np.array_equal(_np(out), fc.warp((u8 > 127).astype(np.uint8), r["vec"], 4, 1) > 0)
    out = flow.warp(_dev(f32), vec, 4, fill=-0.0)
    assert out.dtype == torch.float32 and np.array_equal(_bits(out), fc.warp(f32, r["vec"], 4, -0.0).view(np.uint32))
    with pytest.raises(ValueError):
        flow.block_match(prev, cur[:, :-1], **kw)
    with pytest.raises(ValueError):
        flow.block_match(prev.float(), cur.float(), **kw)
    with pytest.raises(ValueError):
        flow.block_match(prev, cur, search=49)
    with pytest.raises(ValueError):
        flow.warp(_dev(u8), vec[:, :-1], 4)
    with pytest.raises(ValueError):
        flow.warp(_dev(u8), vec, 4, fill=256)
    with pytest.raises(ValueError):
        flow.warp(_dev(u8).to(torch.int32), vec, 4)


def test_motion_compensator_chains_frames_and_resets():
    from osvos_pytorch_amd import flow
    h, w, n = 45, 70, 4
    rng = np.random.default_rng(11)
    big = rng.integers(0, 256, size=(h + 40, w + 40, 3), dtype=np.uint8)
    frames = np.stack([big[20 - 2 * f:20 - 2 * f + h, 20 + 3 * f:20 + 3 * f + w] for f in range(n)])      # a steady pan
    fr = _dev(frames)
    kw = dict(search=6, block=8, step=4, penalty=2, median=1)
    mask = _dev(rng.integers(0, 2, size=(1, h, w), dtype=np.uint8))
    mc = flow.MotionCompensator(**kw)
    assert mc.warp(mask) is mask and mc.vec is None                                         # before any update: the identity
    batch = mc.update(fr).clone()
    assert tuple(batch.shape) == (n,) + fc.grid_shape(h, w, 4) + (2,) and not bool(batch[0].any())      # no stored frame: frame 0 has a zero field
    assert torch.equal(mc.warp(mask), mask)
    want = fc.block_match(frames[:-1], frames[1:], **kw)[0]
    assert np.array_equal(_np(batch[1:]), want)
    step_by_step = flow.MotionCompensator(**kw)
    for f in range(n):
        v = step_by_step.update(fr[f])                                                      # [H,W,3]: one frame
        assert tuple(v.shape) == (1,) + tuple(batch.shape[1:]) and torch.equal(v[0], batch[f]), f
        if f:
            assert np.array_equal(_np(step_by_step.warp(mask)), fc.warp(_np(mask), want[f - 1:f], 4, 0))
            assert np.array_equal(_np(step_by_step.warp(mask[:, None] > 0, fill=1)), fc.warp(_np(mask), want[f - 1:f], 4, 1)[:, None] > 0)
    # a second batch continues from the stored last frame; after reset() it starts over
    more = mc.update(fr[:2])
    assert np.array_equal(_np(more[0]), fc.block_match(frames[3:4], frames[0:1], **kw)[0][0]) and torch.equal(more[1], batch[1])
    assert bool(more[0].any())
    mc.reset()
    assert mc.vec is None and mc.warp(mask) is mask
    assert not bool(mc.update(fr[:2])[0].any())
    with pytest.raises(ValueError):
        mc.update(fr[:, :-1])
    with pytest.raises(ValueError):
        mc.warp(torch.cat([mask, mask]))


def test_tracking_scenario_through_the_tracker():
    """tests/test_flow_cpu.py shows on the restatement that the unwarped previous mask never comes near the object and the warped one
    always overlaps it; here the product runs it: ComponentTracker(radius=2) alone loses the object in frame 1, with its seed moved along
    the motion field it keeps the object and drops the distractor in every frame"""
    from osvos_pytorch_amd import flow
    from osvos_pytorch_amd.results import ComponentTracker
    t = fc.TRACK
    frames, masks, blob = fc.tracking_scene()
    logits_h = fc.tracking_logits(masks, blob)
    fr, logits, first = _dev(frames), _dev(logits_h), _dev(masks[0])
    plain = ComponentTracker(first, t["radius"])
    out = plain(logits[0:1])
    assert np.array_equal(_np(out[0, 0]) > 0, masks[0])                                    # frame 0: the annotation itself seeds it
    out = plain(logits[1:2])
    assert not (_np(out[0, 0]) > 0).any() and not _np(plain.seed).any()                    # frame 1: the object is 8 pixels from the seed: dropped
    assert plain.summary() == {"seen": 4, "kept": 1, "frames": 2}

    mc = flow.MotionCompensator(**{k: t[k] for k in ("search", "block", "step", "penalty", "median")})
    tracker = ComponentTracker(first, t["radius"])
    assert tuple(tracker.seed.shape) == (1, t["h"], t["w"]) and tracker.seed.dtype == torch.uint8
    for f in range(t["frames"]):
        mc.update(fr[f])
        tracker.seed = mc.warp(tracker.seed)
        out = tracker(logits[f:f + 1])
        assert np.array_equal(_np(out[0, 0]) > 0, masks[f]), f                              # the object kept, the distractor dropped
        assert np.array_equal(_np(tracker.seed[0]) != 0, masks[f]), f
    assert tracker.summary() == {"seen": 2 * t["frames"], "kept": t["frames"], "frames": t["frames"]}
    with pytest.raises(ValueError):
        tracker.seed = tracker.seed[0]
    with pytest.raises(ValueError):
        tracker.seed = tracker.seed.cpu()


def _train_online(tmp, *extra):
    r = script_runner.train_online(tmp, "--device-augment", "--synthetic-frames", "3", *extra, frames=3)
    return r.stdout, r.masks


def test_train_online_with_motion_compensation(tmp_path):
    """the option on, with both consumers; and --flow-search 0 against the command without the option, byte for byte.  (The two compared
    commands run without --track-components: after five epochs from an untrained network the logits of this synthetic run sit within the
    last bits of the threshold, and two runs of the SAME command with the tracker -- no --flow option on either -- met 3 and 112 components
    on an MI355X and wrote different masks, while without the tracker the written bytes repeat.  A comparison with the tracker on would
    test that, not this option.)"""
    out, _ = _train_online(tmp_path / "on", "--track-components", "2", "--flow-search", "8", "--flow-block", "8", "--adapt-steps", "2", "--adapt-mix", "2",
                           "--adapt-distance", "12", "--adapt-erosion", "2")
    assert "Online training time" in out and "J&F on blackswan:" in out and "Components kept on blackswan:" in out, out[-2000:]
    assert "Online adaptation on blackswan: 2 frames seen" in out, out[-2000:]
    # --flow-search 0 is the loop without the option: the same bytes on disk
    _, off = _train_online(tmp_path / "off", "--flow-search", "0")
    _, plain = _train_online(tmp_path / "plain")
    assert off == plain
