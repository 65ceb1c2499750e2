"""CPU: the object-centred zoom without a device -- the invariants of the box rule (tests/roi_cases.py, the numpy int64 restatement the GPU
test holds the kernel to), the argument checks of the three entry points through the built library (a refused call launches nothing), the
Python layer's own checks, osvos_pytorch_amd.sequence with a recording stand-in for roi.RoiZoom in the style of test_sequence_cpu.py, and
train_online.py's --zoom options."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import roi_cases as rc
import test_sequence_cpu as ts
from osvos_pytorch_amd import roi, sequence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, F, CPU = ts.H, ts.W, ts.F, ts.CPU


def _check_box(mask, canvas, margin, zoom):
    h, w = mask.shape
    min_h, min_w = rc.min_size((h, w), canvas, zoom)
    trace = {}
    x0, y0, bw, bh = rc.box_rule(mask, canvas, margin[0], margin[1], min_w, min_h, trace)
    what = (mask.shape, canvas, margin, zoom, (x0, y0, bw, bh))
    assert 0 <= x0 and 0 <= y0 and bw >= 1 and bh >= 1 and x0 + bw <= w and y0 + bh <= h, what          # inside the frame
    t = rc.tight(mask)
    if t is None:
        assert (x0, y0, bw, bh) == (0, 0, w, h), what
        return
    xa, xb, ya, yb = t
    assert x0 <= xa and xb < x0 + bw and y0 <= ya and yb < y0 + bh, what                                  # holds the tight box
    assert bw >= min_w and bh >= min_h, what
    if not trace["clamped"]:
        assert abs(bw * canvas[0] - bh * canvas[1]) < max(canvas), what                                   # the canvas's aspect, up to the ceiling


def test_box_rule_invariants_on_the_named_and_on_random_masks():
    count = 0
    sizes = [(h, w) for h, w, _ in rc.FRAME_SIZES] + [(5, 3), (1, 1), (1, 40), (64, 7)]
    for h, w in sizes:
        masks = [rc.named_mask(name, h, w) for name in rc.MASK_NAMES] + [rc.random_mask(h, w, s) for s in range(12)]
        for canvas in rc.CANVASES + [(40, 24), (3, 200)]:
            canvas = canvas or (h, w)
            for margin in rc.MARGINS + [(0, 3), (7, 1)]:
                for zoom in rc.ZOOMS + [1.5, 1000.0]:
                    for m in masks:
                        _check_box(m, canvas, margin, zoom)
                        count += 1
    assert count > 10000
    # the documented cases: an empty mask is the full frame; the bar's aspect growth overshoots W and is capped (so the aspect is lost)
    assert rc.box_rule(rc.named_mask("empty", 30, 85), (30, 85), 25, 8, 43, 15) == (0, 0, 85, 30)
    trace = {}
    assert rc.box_rule(rc.named_mask("bar", 30, 85), (30, 85), 0, 0, 1, 1, trace) == (0, 0, 85, 30) and trace["clamped"]
    # one worked by hand: pixel (8, 8) of 16 x 16, margin (25, 8) -> pad 9, box 19 wide at -1 -> capped to the frame
    assert rc.box_rule(rc.named_mask("mid_pixel", 16, 16), (16, 16), 25, 8, 8, 8) == (0, 0, 16, 16)
    # ... and one the frame does not cap: pixel x 32, y 24 of 48 x 64, margin (0, 0), minimum 16 x 12 on a 24 x 40 canvas: 1 x 1 -> 16 x 12
    # at x0 = 32 - 15 / 2 = 25, y0 = 24 - 11 / 2 = 19 -> bw * Hc = 384 < bh * Wc = 480 -> bw = 480 / 24 = 20 at x0 = 25 - 4 / 2 = 23
    assert rc.box_rule(rc.named_mask("mid_pixel", 48, 64), (24, 40), 0, 0, 16, 12) == (23, 19, 20, 12)


def test_the_python_layer_mirrors_the_rule_inputs_and_refuses_bad_values_and_cpu_tensors():
    from osvos_pytorch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    assert int(re.search(r"#define OSVOS_ROI_BOX_PARTS (\d+)", hdr).group(1)) == _lib.ROI_BOX_PARTS == 64
    for size, canvas, zoom in [((480, 854), (480, 854), 2.0), ((480, 854), (480, 854), 1), ((30, 85), (17, 31), 4), ((16, 16), (24, 40), 1.5),
                               ((37, 53), (1, 1), 3)]:
        assert roi.min_size(size, canvas, zoom) == rc.min_size(size, canvas, zoom)
    assert roi.min_size((480, 854), (480, 854), 2.0) == (240, 427) and roi.min_size((30, 85), (100, 100), 1) == (30, 85)
    roi.check_zoom(0, 0, 1)
    roi.check_zoom(25, 8, 2.0)
    for bad in [(-1, 8, 2.0), (25, -1, 2.0), (25.0, 8, 2.0), (25, True, 2.0), (25, 8, 0.99), (25, 8, float("nan")), (25, 8, float("inf")), (25, 8, None)]:
        with pytest.raises(ValueError):
            roi.check_zoom(*bad)
    with pytest.raises(ValueError):
        roi.RoiZoom(lambda x: [x], max_zoom=0.5)
    with pytest.raises(ValueError):
        roi.RoiZoom(lambda x: [x], canvas=(0, 10))
    import inspect
    for fn in (roi.mask_box, roi.RoiZoom.__init__):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items() if k in ("margin_pct", "margin_px", "max_zoom")}
        assert d == dict(margin_pct=25, margin_px=8, max_zoom=2.0)
    assert inspect.signature(roi.paste).parameters["outside"].default == -20.0 == inspect.signature(roi.RoiZoom.__init__).parameters["outside"].default
    # no CPU fallback
    box = torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        roi.mask_box(torch.zeros(1, 4, 4, dtype=torch.bool), (4, 4))
    with pytest.raises(RuntimeError):
        roi.crop_view(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), box, (4, 4))
    with pytest.raises(RuntimeError):
        roi.paste(torch.zeros(1, 4, 4), box, (4, 4))
    with pytest.raises(RuntimeError):
        roi.RoiZoom(lambda x: [x])(torch.zeros(4, 4, 3, dtype=torch.uint8))


def test_argument_errors_of_the_three_entry_points_launch_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    p = C.c_void_p(4096)          # never dereferenced: every call below is refused before its launch
    good = dict(N=1, H=30, W=85, Hc=24, Wc=40, pct=25, px=8, min_w=20, min_h=12)

    def box(mask=p, out=p, ws=p, **kw):
        a = dict(good, **kw)
        return l.osvos_roi_box(mask, out, a["N"], a["H"], a["W"], a["Hc"], a["Wc"], a["pct"], a["px"], a["min_w"], a["min_h"], ws, None)

    def view(bgr=p, bx=p, mean=(C.c_float * 3)(1, 2, 3), out=p, **kw):
        a = dict(good, **kw)
        return l.osvos_roi_view(bgr, bx, mean, out, a["N"], a["H"], a["W"], a["Hc"], a["Wc"], None)

    def paste(lg=p, bx=p, out=p, **kw):
        a = dict(good, **kw)
        return l.osvos_roi_paste(lg, bx, out, a["N"], a["Hc"], a["Wc"], a["H"], a["W"], -20.0, None)

    def refused(rc_, word):
        err = l.osvos_last_error()
        assert rc_ < 0 and word in err, (rc_, err)

    for kw in (dict(mask=None), dict(out=None), dict(ws=None)):
        refused(box(**kw), b"null")
    for kw in (dict(bgr=None), dict(bx=None), dict(mean=None), dict(out=None)):
        refused(view(**kw), b"null")
    for kw in (dict(lg=None), dict(bx=None), dict(out=None)):
        refused(paste(**kw), b"null")
    for side in ("H", "W", "Hc", "Wc"):
        for v in (0, -3, 16385):
            for call in (box, view, paste):
                refused(call(**{side: v, "min_w": 1, "min_h": 1}), b"bad size")
    for call in (box, view, paste):
        refused(call(N=0), b"N 0 frames")
    refused(box(pct=-1), b"negative margin")
    refused(box(px=-1), b"negative margin")
    refused(box(min_w=86), b"minimum size")
    refused(box(min_h=31), b"minimum size")
    refused(box(min_w=-1), b"minimum size")
    with pytest.raises(RuntimeError):
        _lib.check(box(min_h=31), "roi_box")


C_ROI = 17.0


class Roi(object):
    """like roi.RoiZoom: (frame_u8, prev_mask) -> logits [1,1,H,W]; positive on about half of the pixels, many of them near zero"""

    def __init__(self, rec, c=C_ROI):
        self.rec, self.c, self.frames, self.prevs = rec, c, [], []

    def __call__(self, frame_u8, prev):
        self.rec.add("roi")
        self.frames.append(frame_u8)
        self.prevs.append(prev)
        return raw_of(frame_u8, self.c)


def raw_of(frame_u8, c=C_ROI):
    return (frame_u8[None, None, :, :, 0].float() - 128.0 - c) / 4.0


def test_single_object_zoom_runs_on_the_full_frame_first_then_around_the_final_mask_moved_by_the_flow():
    rec = ts.Rec()
    zoom, crf, snap, flow = Roi(rec), ts.Crf(rec), ts.Snap(rec), ts.Flow(rec)
    trackers = []
    data, loader = ts.samples(rec, with_image=False)          # (DeviceTestFrames raw_only: no 'image' for a frame without annotation)
    forward = sequence.FrameForward(ts.Net(rec), roi=zoom)
    assert not forward.needs_image and forward.roi_prev is None
    seq = sequence.SingleObjectSequence(loader, forward, CPU, "blackswan", flow=flow, crf=crf, snap=snap,
                                        make_tracker=lambda m: trackers.append(ts.Tracker(rec, m)) or trackers[-1])
    got = list(seq)
    assert rec.of(0) == ["flow.update", "roi", "crf", "snap", "tracker.build", "tracker"]
    later = ["flow.update", "flow.warp.seed", "flow.warp.mask", "roi", "crf", "snap", "tracker"]
    assert rec.of(1) == later and rec.of(2) == later
    assert "net" not in {e[0] for e in rec.log}
    want = [ts.chain(raw_of(s["frame_u8"])) for s in data]
    for f in range(F):
        assert zoom.frames[f] is data[f]["frame_u8"] and torch.equal(got[f][1], want[f])
    # frame 0: no previous mask; frame f + 1: the FINAL mask of frame f, moved by the flow before the zoom sees it
    assert zoom.prevs[0] is None
    masks = [x for x in flow.warped if x.dtype == torch.bool]
    assert len(masks) == 2
    for f in (0, 1):
        assert torch.equal(masks[f], want[f] > 0) and torch.equal(zoom.prevs[f + 1], torch.roll(want[f] > 0, 1, -1))
        assert not torch.equal(want[f] > 0, raw_of(data[f]["frame_u8"]) > 0)          # (final and raw masks differ: the check means something)
    assert torch.equal(forward.roi_prev, want[2] > 0) and forward.match_prev is None and seq.prev_mask is None


def test_zoom_takes_precedence_and_without_flow_the_mask_is_handed_over_as_it_is():
    rec = ts.Rec()
    zoom = Roi(rec)
    data, loader = ts.samples(rec)
    forward = sequence.FrameForward(ts.Net(rec), ts.Tta(rec), None, ts.Matcher(rec, previous=False), roi=zoom)
    got = list(sequence.SingleObjectSequence(loader, forward, CPU, "blackswan"))
    assert [rec.of(f) for f in range(F)] == [["set_reference", "roi"]] + [["roi"]] * (F - 1)
    assert zoom.prevs[0] is None and all(torch.equal(zoom.prevs[f + 1], got[f][1] > 0) for f in range(F - 1))
    assert forward.match_prev is None                          # (the matcher does not ask for the previous mask: nothing is kept for it)


def test_without_roi_the_frame_forward_makes_exactly_the_calls_it_made():
    rec = ts.Rec()
    net = ts.Net(rec)
    data, loader = ts.samples(rec)
    forward = sequence.FrameForward(net, None, None, None, None)
    assert forward.roi is None and forward.needs_image
    seq = sequence.SingleObjectSequence(loader, forward, CPU, "blackswan", flow=ts.Flow(rec))
    for f, (fname, fused, gt) in enumerate(seq):
        assert fused is net.out[-1] and torch.equal(fused, data[f]["image"][:, :1])
    assert rec.log == [(s, f) for f in range(F) for s in ("flow.update", "net")]          # no warp: nothing is carried over
    assert forward.roi_prev is None and forward.match_prev is None
    forward.remember(torch.ones(1, 1, H, W))
    assert forward.roi_prev is None
    import inspect
    assert list(inspect.signature(sequence.FrameForward.__init__).parameters) == ["self", "net", "tta", "adapter", "matcher", "roi"]
    assert inspect.signature(sequence.FrameForward.__init__).parameters["roi"].default is None


def test_multi_object_zoom_remembers_the_raw_output_of_each_object():
    K, rec = 2, ts.Rec()
    g = torch.Generator().manual_seed(11)
    frames = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8) for f in range(F)]
    first = torch.zeros(H, W, dtype=torch.uint8)
    first[1:3, 1:4], first[3:5, 4:7] = 1, 2
    zooms, images = [], []

    def forward_of(net):
        zooms.append(Roi(rec, c=C_ROI + 8.0 * len(zooms)))
        return sequence.FrameForward(net, roi=zooms[-1])

    logits, trackers, _ = sequence.multi_object_sequence(
        frames, [first, None, None], K, lambda k: ts.Net(rec), forward_of, lambda img: images.append(img), crf=ts.Crf(rec), snap=ts.Snap(rec),
        make_tracker=lambda m: ts.Tracker(rec, m), chunk=2)
    assert images == [] and len(zooms) == K                    # needs_image is False: the identity pass is never made
    stages = [e[0] for e in rec.log]
    assert stages == ["roi"] * (K * F) + ["crf"] * 4 + ["labels", "snap", "snap"] * 2 + ["tracker.build", "tracker", "tracker"] * 2
    for k in range(K):
        raw = [raw_of(fr, zooms[k].c) for fr in frames]
        assert all(zooms[k].frames[f] is frames[f] for f in range(F))
        # frame 0 on the full frame; then the RAW output of the previous frame, not the final mask of the post chain
        assert zooms[k].prevs[0] is None and all(torch.equal(zooms[k].prevs[f + 1], raw[f] > 0) for f in range(F - 1))
        assert any(not torch.equal(raw[f] > 0, ts.chain(raw[f]) > 0) for f in range(F - 1))
        assert torch.equal(logits[k], torch.stack([ts.chain(r[0, 0]) for r in raw]))


def test_zoom_flags_are_parsed_and_refused_before_gpu_work():
    import train_online
    base = ["--synthetic", "--device-augment"]
    d = train_online.parse_args(["--synthetic"])
    assert d.roi is None and d.zoom == 0 and (d.zoom_margin, d.zoom_canvas, d.zoom_outside) == ("25,8", "", -20.0)
    assert train_online.parse_args(base + ["--zoom", "0", "--zoom-margin", "10,2", "--zoom-canvas", "240x427"]).roi is None
    assert train_online.parse_args(base + ["--zoom", "2"]).roi == dict(canvas=None, margin_pct=25, margin_px=8, max_zoom=2.0, outside=-20.0)
    a = train_online.parse_args(["--synthetic", "--multi-object", "--zoom", "1", "--zoom-margin", "0,0", "--zoom-canvas", "240x427", "--zoom-outside", "-30"])
    assert a.roi == dict(canvas=(240, 427), margin_pct=0, margin_px=0, max_zoom=1.0, outside=-30.0)
    # the later stages combine, and the flow may move the zoom's mask alone
    a = train_online.parse_args(base + ["--zoom", "2", "--crf-iters", "2", "--snap-cell", "8", "--track-components", "4", "--flow-search", "8"])
    assert a.roi and a.crf and a.snap and a.flow and a.track_components == 4
    assert train_online.parse_args(base + ["--zoom", "2", "--flow-search", "8"]).flow["search"] == 8
    refusals = [(base + ["--zoom", "2", "--tta-flip"], "--tta-scales / --tta-flip"),
                (base + ["--zoom", "2", "--tta-scales", "0.75,1"], "--tta-scales / --tta-flip"),
                (base + ["--zoom", "2", "--match-gain", "4"], "--match-gain"),
                (base + ["--zoom", "2", "--synthetic-frames", "3", "--adapt-steps", "2"], "--adapt-steps"),
                (["--synthetic", "--zoom", "2"], "--device-augment"),
                (base + ["--zoom", "0.5"], "--zoom takes"), (base + ["--zoom", "-1"], "--zoom takes"), (base + ["--zoom", "nan"], "--zoom takes"),
                (base + ["--zoom-margin=-1,0"], "margin_pct"), (base + ["--zoom", "2", "--zoom-margin", "25"], "--zoom-margin"),
                (base + ["--zoom", "2", "--zoom-margin", "a,b"], "--zoom-margin"), (base + ["--zoom", "2", "--zoom-canvas", "0x40"], "--zoom-canvas"),
                (base + ["--zoom", "2", "--zoom-canvas", "480"], "--zoom-canvas"), (base + ["--zoom", "2", "--zoom-outside", "nan"], "--zoom-outside")]
    for argv, word in refusals:
        with pytest.raises(SystemExit) as e:
            train_online.parse_args(argv)
        assert "--zoom" in str(e.value) and word in str(e.value), (argv, e.value)
    with pytest.raises(SystemExit) as e:          # without the zoom the flow's own rule stands, in its own words
        train_online.parse_args(base + ["--flow-search", "8"])
    assert "--flow-search needs --adapt-steps or --track-components" in str(e.value)
