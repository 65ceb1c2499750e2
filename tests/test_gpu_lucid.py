"""GPU: lucid first-frame synthesis on the device -- osvos_lucid_inpaint and osvos_lucid_compose (csrc/lucid.hip) against the numpy
restatement of the rule in tests/lucid_cases.py, bit for bit (the rule is integer arithmetic: every comparison is np.array_equal, there is no
tolerance), the refusals, the wrappers of osvos_pytorch_amd.lucid, the scenario through LucidDream, and train_online.py --lucid.  Outputs
and the workspace are pre-filled with garbage before every call."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import lucid_cases as lc
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE_BYTE = 0xa5
GUARD = 256


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t).view(np.uint32)


def _inpaint_rc(bgr, hole, radius, passes, ws_passes=None):
    """one osvos_lucid_inpaint call through _lib on CUDA tensors -> (rc, out, ws buffer, ws bytes)"""
    from osvos_pytorch_amd import _lib
    h, w = (int(v) for v in hole.shape)
    need = int(_lib.lib().osvos_lucid_inpaint_ws_bytes(h, w, passes if ws_passes is None else ws_passes))
    out = torch.full((h, w, 3), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
    buf = torch.full((need + GUARD,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
    vp = C.c_void_p
    rc = _lib.lib().osvos_lucid_inpaint(vp(bgr.data_ptr()), vp(hole.data_ptr()), vp(out.data_ptr()), h, w, radius, passes, vp(buf.data_ptr()), _stream())
    return rc, out, buf, need


def _inpaint(bgr, hole, radius, passes):
    from osvos_pytorch_amd import _lib
    rc, out, buf, need = _inpaint_rc(bgr, hole, radius, passes)
    _lib.check(rc, "lucid_inpaint")
    assert need >= 4 * hole.numel() and bool((buf[need:] == GARBAGE_BYTE).all()), "the call wrote past osvos_lucid_inpaint_ws_bytes"
    return out


def _compose_rc(bgr, mask, bg, M, tone, mean=lc.MEAN, n=None, h=None, w=None):
    from osvos_pytorch_amd import _lib
    M, tone = np.ascontiguousarray(np.asarray(M, np.float64)), np.ascontiguousarray(np.asarray(tone, np.int32))
    n = M.shape[0] if n is None else n
    hh, ww = (int(v) for v in mask.shape)
    image = torch.full((max(n, 1), 3, hh, ww), float("nan"), device="cuda", dtype=torch.float32)
    gt = torch.full((max(n, 1), 1, hh, ww), float("nan"), device="cuda", dtype=torch.float32)
    vp = C.c_void_p
    rc = _lib.lib().osvos_lucid_compose(vp(bgr.data_ptr()), vp(mask.data_ptr()), vp(bg.data_ptr()), vp(M.ctypes.data), vp(tone.ctypes.data),
                                        (C.c_float * 3)(*mean), vp(image.data_ptr()), vp(gt.data_ptr()), n, hh if h is None else h,
                                        ww if w is None else w, _stream())
    return rc, image, gt


def _compose(bgr, mask, bg, M, tone, mean=lc.MEAN):
    from osvos_pytorch_amd import _lib
    rc, image, gt = _compose_rc(bgr, mask, bg, M, tone, mean)
    _lib.check(rc, "lucid_compose")
    return image, gt


def _inpaint_against_restatement(c):
    h, w, kind, radius, passes = c
    r = lc.inpaint_reference(c)
    out = _np(_inpaint(_dev(r["bgr"]), _dev(r["hole"]), radius, passes))
    print("%s: %d of %d pixels differ" % (lc.case_id(c), int((out != r["out"]).any(-1).sum()), h * w))
    assert np.array_equal(out, r["out"])
    if passes:                                                        # and the pure fill
        assert np.array_equal(_np(_inpaint(_dev(r["bgr"]), _dev(r["hole"]), radius, 0)), r["filled"])


@pytest.mark.parametrize("c", lc.INPAINT_CASES, ids=lc.case_id)
def test_inpaint_against_the_restatement(c):
    _inpaint_against_restatement(c)


def test_inpaint_on_a_davis_sized_frame():
    _inpaint_against_restatement(lc.INPAINT_LARGE)


def _compose_against_restatement(c):
    r = lc.compose_reference(c)
    image, gt = _compose(_dev(r["bgr"]), _dev(r["mask"]), _dev(r["bg"]), r["M"], r["tone"])
    print("%s: %d of %d image words and %d of %d labels differ" % (lc.case_id(c), int((_bits(image) != r["image"].view(np.uint32)).sum()), r["image"].size,
                                                                  int((_np(gt) != r["gt"]).sum()), r["gt"].size))
    assert np.array_equal(_bits(image), r["image"].view(np.uint32))
    assert np.array_equal(_np(gt), r["gt"])


@pytest.mark.parametrize("c", lc.COMPOSE_CASES, ids=lc.case_id)
def test_compose_against_the_restatement(c):
    _compose_against_restatement(c)


def test_compose_on_a_davis_sized_frame():
    _compose_against_restatement(lc.COMPOSE_LARGE)


def test_samples_of_a_batch_are_independent_and_calls_repeat():
    c = (37, 53, "blob", "mixed", 16)
    r = lc.compose_reference(c)
    bgr, mask, bg = _dev(r["bgr"]), _dev(r["mask"]), _dev(r["bg"])
    image, gt = _compose(bgr, mask, bg, r["M"], r["tone"])
    again = _compose(bgr, mask, bg, r["M"], r["tone"])
    assert np.array_equal(_bits(image), _bits(again[0])) and torch.equal(gt, again[1])
    for i in (0, 7, 15):
        one = _compose(bgr, mask, bg, r["M"][i:i + 1], r["tone"][i:i + 1])
        assert np.array_equal(_bits(image[i:i + 1]), _bits(one[0])) and torch.equal(gt[i:i + 1], one[1]), i
    assert not torch.equal(gt[0], gt[1])


def test_identity_composition_equals_augment_frame():
    """on a frame with an empty mask and bg = the frame: osvos_augment_frame's identity output, bit for bit; and with a mask, wherever it is
    set"""
    from osvos_pytorch_amd.augment import augment_frame
    h, w = 37, 53
    bgr = _dev(lc.frame_of("noise", h, w, 9))
    M, tone = lc.params_of("identity", h, w, 1)
    for kind in ("empty", "blob"):
        mask = _dev(lc.mask_of(kind, h, w))
        want, want_gt = augment_frame(bgr, (mask != 0).to(torch.uint8) * 255, flip=False, rot=None)
        image, gt = _compose(bgr, mask, bgr, M, tone)
        assert np.array_equal(_bits(image[0]), _bits(want)) and torch.equal(gt[0], want_gt), kind


def test_bad_arguments_return_an_error_and_launch_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    h, w = 12, 20
    bgr, mask, bg = _dev(lc.frame_of("noise", h, w, 1)), _dev(lc.mask_of("blob", h, w)), _dev(lc.frame_of("gradient", h, w))
    good_m, good_t = lc.params_of("rot30_s075", h, w, 2)

    def refused(word, M=good_m, tone=good_t, **kw):
        rc, image, gt = _compose_rc(bgr, mask, bg, M, tone, **kw)
        assert rc < 0 and word in l.osvos_last_error(), (word, rc, l.osvos_last_error())
        torch.cuda.synchronize()
        assert bool(torch.isnan(image).all()) and bool(torch.isnan(gt).all()), word

    refused(b"N", n=0)
    refused(b"N", M=good_m * 9, tone=good_t * 9, n=17)
    refused(b"N", n=-1)
    refused(b"size", h=0)
    refused(b"size", w=4097)
    refused(b"size", h=4097)
    for k in range(6):
        for v in (float("nan"), float("inf"), -float("inf")):
            m = np.array(good_m, np.float64)
            m[1, 1, k] = v
            refused(b"finite", M=m)
        m = np.array(good_m, np.float64)
        m[0, 0, k] = -(2.0 ** 18 + 1) if k in (2, 5) else 64.5
        refused(b"matrix", M=m)
        m[0, 0, k] = 2.0 ** 18 if k in (2, 5) else -64.0               # the limits themselves are taken
        assert _compose_rc(bgr, mask, bg, m, good_t)[0] == 0
    for k, v in [(0, -1), (1, 1025), (2, 2 ** 20), (3, -256), (4, 256), (5, -2 ** 31)]:
        t = np.array(good_t, np.int64)
        t[1, 0, k] = v
        refused(b"gain" if k < 3 else b"offset", tone=t.astype(np.int32))
    vp = C.c_void_p
    image = torch.full((1, 3, h, w), float("nan"), device="cuda")
    gt = torch.full((1, 1, h, w), float("nan"), device="cuda")
    m, t, mean = np.array(good_m, np.float64), np.array(good_t, np.int32), (C.c_float * 3)(*lc.MEAN)
    ptrs = [vp(bgr.data_ptr()), vp(mask.data_ptr()), vp(bg.data_ptr()), vp(m.ctypes.data), vp(t.ctypes.data), mean, vp(image.data_ptr()), vp(gt.data_ptr())]
    for i in range(8):
        a = list(ptrs)
        a[i] = None
        assert l.osvos_lucid_compose(*a, 1, h, w, _stream()) < 0 and b"null" in l.osvos_last_error(), i
    torch.cuda.synchronize()
    assert bool(torch.isnan(image).all()) and bool(torch.isnan(gt).all())
    with pytest.raises(RuntimeError):
        _lib.check(-1, "lucid_compose")
    # the inpainting
    hole = _dev(lc.mask_of("blob", h, w))
    for radius, passes, word in [(0, 1, b"radius"), (9, 1, b"radius"), (-1, 1, b"radius"), (2, -1, b"passes"), (2, 9, b"passes")]:
        rc, out, buf, _ = _inpaint_rc(bgr, hole, radius, passes, ws_passes=1)
        assert rc < 0 and word in l.osvos_last_error(), (radius, passes, l.osvos_last_error())
        torch.cuda.synchronize()
        assert bool((out == GARBAGE_BYTE).all()) and bool((buf == GARBAGE_BYTE).all())
    out = torch.full((h, w, 3), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
    buf = torch.full((l.osvos_lucid_inpaint_ws_bytes(h, w, 3) + GUARD,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
    fp, hp, op, bp = vp(bgr.data_ptr()), vp(hole.data_ptr()), vp(out.data_ptr()), vp(buf.data_ptr())
    tail = (2, 3)
    assert l.osvos_lucid_inpaint(None, hp, op, h, w, *tail, bp, _stream()) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, None, op, h, w, *tail, bp, _stream()) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, hp, None, h, w, *tail, bp, _stream()) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, hp, op, h, w, *tail, None, _stream()) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, hp, op, 0, w, *tail, bp, _stream()) < 0 and b"size" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, hp, op, h, 4097, *tail, bp, _stream()) < 0 and b"size" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, hp, fp, h, w, *tail, bp, _stream()) < 0 and b"overlaps" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, hp, op, h, w, *tail, op, _stream()) < 0 and b"overlaps" in l.osvos_last_error()
    assert l.osvos_lucid_inpaint(fp, hp, op, h, w, *tail, vp(buf.data_ptr() + 2), _stream()) < 0 and b"aligned" in l.osvos_last_error()
    torch.cuda.synchronize()
    assert bool((out == GARBAGE_BYTE).all()) and bool((buf == GARBAGE_BYTE).all())


def test_workspace_size_query():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    assert l.osvos_lucid_inpaint_ws_bytes(480, 854, 0) == 4 * 480 * 854
    assert l.osvos_lucid_inpaint_ws_bytes(480, 854, 3) == l.osvos_lucid_inpaint_ws_bytes(480, 854, 8) >= 7 * 480 * 854
    for bad in [(0, 8, 1), (8, 0, 1), (4097, 8, 1), (8, 4097, 1), (8, 8, -1), (8, 8, 9)]:
        assert l.osvos_lucid_inpaint_ws_bytes(*bad) == 0, bad


def test_wrappers_match_the_direct_calls():
    from osvos_pytorch_amd import lucid
    c = lc.INPAINT_CASES[4]
    h, w, kind, radius, passes = c
    r = lc.inpaint_reference(c)
    bgr, hole = _dev(r["bgr"]), _dev(r["hole"])
    out = lucid.inpaint(bgr, hole, radius, passes)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and np.array_equal(_np(out), r["out"])
    big = torch.empty(1 << 18, device="cuda", dtype=torch.int32)
    assert torch.equal(lucid.inpaint(bgr, hole, radius=radius, passes=passes, ws=big), out)
    assert np.array_equal(_np(lucid.inpaint(bgr, hole, passes=0)), r["filled"])
    c = lc.COMPOSE_CASES[8]
    r = lc.compose_reference(c)
    bgr, mask, bg = _dev(r["bgr"]), _dev(r["mask"]), _dev(r["bg"])
    image, gt = lucid.compose(bgr, mask, bg, r["M"].tolist(), r["tone"].tolist())
    assert tuple(image.shape) == (3, 3, 37, 53) and tuple(gt.shape) == (3, 1, 37, 53) and image.dtype == gt.dtype == torch.float32
    assert np.array_equal(_bits(image), r["image"].view(np.uint32)) and np.array_equal(_np(gt), r["gt"])
    zero = lucid.compose(bgr, mask, bg, r["M"], r["tone"], meanval=(0.0, 0.0, 0.0))[0]
    assert np.array_equal(_bits(zero), lc.compose(r["bgr"], r["mask"], r["bg"], r["M"], r["tone"], (0.0, 0.0, 0.0))[0].view(np.uint32))
    bad_m = r["M"].copy()
    bad_m[0, 0, 0] = 65.0
    bad_t = r["tone"].copy()
    bad_t[0, 1, 4] = 256
    for args in [(bgr.float(), mask, bg, r["M"], r["tone"]), (bgr, mask[:, :-1], bg, r["M"], r["tone"]), (bgr, mask, bg[:-1], r["M"], r["tone"]),
                 (bgr, mask, bg, bad_m, r["tone"]), (bgr, mask, bg, r["M"], bad_t), (bgr, mask, bg, r["M"][:, :1], r["tone"][:, :1]),
                 (bgr, mask, bg, np.repeat(r["M"], 6, 0), np.repeat(r["tone"], 6, 0)), (bgr, mask, bg, r["M"], r["tone"].astype(np.float32))]:
        with pytest.raises(ValueError):
            lucid.compose(*args)
    with pytest.raises(ValueError):
        lucid.inpaint(bgr, hole[:-1])
    with pytest.raises(ValueError):
        lucid.inpaint(bgr, hole, passes=9)


def test_scenario_through_lucid_dream():
    """tests/test_lucid_cpu.py pins the scenario on the restatement; here LucidDream makes the hole (the mask grown through
    results.distance_map), inpaints and composes it, and gives the restatement's bytes; its draws come from Python's random in the documented
    order, and batch(n) is one launch over n of them"""
    from osvos_pytorch_amd import lucid
    r = lc.scenario_reference()
    s = lc.SCENE
    frame, mask = _dev(r["frame"]), _dev(r["mask"])
    dream = lucid.LucidDream(frame, mask, meanval=(0.0, 0.0, 0.0), **lc.DEFAULTS)
    assert np.array_equal(_np(dream.hole), r["hole"]) and np.array_equal(_np(dream.bg), r["bg"])
    assert dream.box == (s["x0"], s["x0"] + s["side"] - 1, s["y0"], s["y0"] + s["side"] - 1)
    assert dream.pivot == (s["x0"] + s["side"] / 2, s["y0"] + s["side"] / 2) and (dream.box_w, dream.box_h) == (s["side"], s["side"])
    image, gt = lucid.compose(frame, mask, dream.bg, r["M"], r["tone"], (0.0, 0.0, 0.0))
    assert np.array_equal(_bits(image[0]), r["lucid"].view(np.uint32)) and np.array_equal(_np(gt[0, 0]), r["gt"])
    image, _ = lucid.compose(frame, mask, frame, r["M"], r["tone"], (0.0, 0.0, 0.0))
    assert np.array_equal(_bits(image[0]), r["plain"].view(np.uint32))
    # the draws
    random.seed(11)
    draws = [dream.draw() for _ in range(3)]
    state = random.getstate()
    random.seed(11)
    got = dream.batch(3)
    assert random.getstate() == state
    want = lc.compose(r["frame"], r["mask"], r["bg"], [d[0] for d in draws], [d[1] for d in draws], (0.0, 0.0, 0.0))
    assert np.array_equal(_bits(got["image"]), want[0].view(np.uint32)) and np.array_equal(_np(got["gt"]), want[1])
    random.seed(11)
    one = dream()
    assert tuple(one["image"].shape) == (3, s["h"], s["w"]) and tuple(one["gt"].shape) == (1, s["h"], s["w"])
    assert np.array_equal(_bits(one["image"]), want[0][0].view(np.uint32))
    random.seed(11)
    mirror = random.random() < 0.5
    u = [random.random() for _ in range(12)]
    fg = lc.affine_inverse(dream.pivot[0], dream.pivot[1], 60 * u[0] - 30, 0.5 * u[1] + 0.75, (2 * u[2] - 1) * 0.25 * s["side"],
                           (2 * u[3] - 1) * 0.25 * s["side"], mirror)
    assert draws[0][0][0] == fg and draws[0][1][0][:3] == [int(round(256 * (1 + 0.2 * (2 * u[8] - 1))))] * 3
    assert draws[0][1][1][3:] == [int(round(20 * (2 * u[11] - 1)))] * 3
    # an empty mask: nothing to cut out, the frame's centre as the pivot
    empty = lucid.LucidDream(frame, torch.zeros_like(mask))
    assert empty.box is None and empty.pivot == (s["w"] / 2, s["h"] / 2) and torch.equal(empty.bg, frame) and not bool(empty().get("gt").any())
    with pytest.raises(ValueError):
        lucid.LucidDream(frame, mask, grow=65)
    with pytest.raises(ValueError):
        dream.batch(17)


def _run_script(tmp, *args):
    return script_runner.train_online(tmp, *args).stdout


def _train_online(tmp, *extra):
    r = script_runner.train_online(tmp, "--device-augment", *extra, frames=1)
    return r.stdout, r.masks[0]


def _losses(out):
    return [float(line.split()[1]) for line in out.splitlines() if line.startswith("Loss: ")]


def test_train_online_with_lucid_samples(tmp_path):
    """the option on: finite losses; and --lucid 0 against the command without the option, byte for byte"""
    out, _ = _train_online(tmp_path / "on", "--lucid", "0.5")
    losses = _losses(out)
    assert "Online training time" in out and "J&F on blackswan:" in out and losses and np.isfinite(losses).all(), out[-2000:]
    _, off = _train_online(tmp_path / "off", "--lucid", "0")
    _, plain = _train_online(tmp_path / "plain")
    assert off == plain


def test_train_online_multi_object_with_lucid_samples(tmp_path):
    """every object fine-tuned on lucid samples of its own binary mask"""
    out = _run_script(tmp_path / "on", "--device-augment", "--multi-object", "--lucid", "0.5")
    assert "J&F on blackswan (2 objects):" in out and np.isfinite(_losses(out)).all() and len(_losses(out)) >= 2, out[-2000:]
