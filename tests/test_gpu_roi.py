"""GPU: the object-centred zoom on the device -- osvos_roi_box, osvos_roi_view and osvos_roi_paste (csrc/roi.hip) against tests/roi_cases.py:
the box bit for bit against the numpy int64 rule (and again on the same buffers: no state is carried between calls), the view and the paste
against the float64 restatement of the sampling rule applied to the cropped arrays, their exactness properties bit for bit (the full-frame
box at the frame's size is osvos_tta_view's output; a canvas of the box's size passes through the paste with inf and NaN; `outside` exactly
everywhere else), the scalar and the 16-byte store forms against each other, osvos_pytorch_amd.roi.RoiZoom around a stub and around the real
network, and train_online.py --zoom.

Bounds (tests/tta_cases.py; the arithmetic is osvos_tta_view's and osvos_tta_fuse's, so their derivations hold).  View: |diff| <=
VIEW_BOUND = 16 * 2^-24 * 256.  Paste: |diff| <= fuse_bound(1, M) = 10 * 2^-23 * M inside the box, M the case's largest |logit|.
Outputs are pre-filled with garbage; the osvos_* calls go through _lib."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import roi_cases as rc
import tta_cases as tc
import trained_fixture as tf
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE = 7.25e33
SIZE_IDS = ["%dx%dx%d" % s for s in rc.FRAME_SIZES]
VP = C.c_void_p


def _stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def _dirty(shape, offset=0):
    """a garbage-filled float32 CUDA tensor of `shape` that starts `offset` floats into its storage"""
    n = int(np.prod(shape))
    return torch.full((n + offset,), GARBAGE, device="cuda", dtype=torch.float32)[offset:].view(*shape)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _workspace(n):
    from osvos_pytorch_amd import _lib
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (n * _lib.ROI_BOX_PARTS * 4,), device="cuda", dtype=torch.int32)      # (garbage: contents irrelevant)


def _box(mask, canvas, margin, min_wh, out=None, ws=None):
    """one osvos_roi_box call on a uint8 / bool CUDA tensor [N,H,W] -> (int32 CUDA tensor [N,4], ws)"""
    from osvos_pytorch_amd import _lib
    n, h, w = mask.shape
    out = torch.full((n, 4), -77777, device="cuda", dtype=torch.int32) if out is None else out
    ws = _workspace(n) if ws is None else ws
    _lib.check(_lib.lib().osvos_roi_box(VP(mask.data_ptr()), VP(out.data_ptr()), n, h, w, canvas[0], canvas[1], margin[0], margin[1], min_wh[0], min_wh[1],
                                        VP(ws.data_ptr()), _stream()), "roi_box")
    return out, ws


def _view(fr, box, canvas, offset=0):
    """one osvos_roi_view call: uint8 CUDA [N,H,W,3], int32 CUDA [N,4] -> float32 CUDA [N,3,Hc,Wc]"""
    from osvos_pytorch_amd import _lib
    n, h, w, _ = fr.shape
    out = _dirty((n, 3) + tuple(canvas), offset)
    mean = (C.c_float * 3)(*rc.MEANVAL)
    _lib.check(_lib.lib().osvos_roi_view(VP(fr.data_ptr()), VP(box.data_ptr()), mean, VP(out.data_ptr()), n, h, w, canvas[0], canvas[1], _stream()), "roi_view")
    return out


def _paste(lg, box, size, outside, offset=0):
    """one osvos_roi_paste call: float32 CUDA [N,Hc,Wc], int32 CUDA [N,4] -> float32 CUDA [N,H,W]"""
    from osvos_pytorch_amd import _lib
    n, hc, wc = lg.shape
    out = _dirty((n,) + tuple(size), offset)
    _lib.check(_lib.lib().osvos_roi_paste(VP(lg.data_ptr()), VP(box.data_ptr()), VP(out.data_ptr()), n, hc, wc, size[0], size[1], outside, _stream()), "roi_paste")
    return out


def _tta_view(fr, hv, wv):
    from osvos_pytorch_amd import _lib
    n, h, w, _ = fr.shape
    out = _dirty((n, 3, hv, wv))
    mean = (C.c_float * 3)(*rc.MEANVAL)
    _lib.check(_lib.lib().osvos_tta_view(VP(fr.data_ptr()), mean, VP(out.data_ptr()), n, h, w, hv, wv, 0, _stream()), "tta_view")
    return out


def _dev_box(host):
    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).cuda()


@pytest.mark.parametrize("h,w,n", rc.FRAME_SIZES, ids=SIZE_IDS)
def test_box_kernel_is_the_integer_rule_bit_for_bit_and_keeps_no_state(h, w, n):
    batches = rc.mask_batches(h, w, n) + [("random%d" % s, np.stack([rc.random_mask(h, w, 10 * s + k) for k in range(n)])) for s in range(4)]
    calls = 0
    for name, host in batches:
        mask = torch.from_numpy(host).cuda()
        for canvas in rc.CANVASES:
            canvas = canvas or (h, w)
            for margin in rc.MARGINS:
                for zoom in rc.ZOOMS:
                    min_h, min_w = rc.min_size((h, w), canvas, zoom)
                    want = rc.boxes(host, canvas, margin[0], margin[1], zoom)
                    got, ws = _box(mask, canvas, margin, (min_w, min_h))
                    assert np.array_equal(got.cpu().numpy(), want), (name, canvas, margin, zoom, got.cpu().numpy(), want)
                    # again on the same output and workspace, as the first call left them; and after a call on another mask
                    again, _ = _box(mask, canvas, margin, (min_w, min_h), out=got, ws=ws)
                    assert np.array_equal(again.cpu().numpy(), want), (name, canvas, margin, zoom)
                    calls += 2
        other = torch.from_numpy(rc.named_mask("full", h, w)[None].repeat(n, 0)).cuda()
        _box(other, (h, w), (25, 8), (1, 1), ws=ws)
        third, _ = _box(mask, (h, w), (25, 8), rc.min_size((h, w), (h, w), 2)[::-1], ws=ws)
        assert np.array_equal(third.cpu().numpy(), rc.boxes(host, (h, w), 25, 8, 2)), name
    # a mask that starts at every byte offset of a 16-byte word (the scalar head), as bool and as bytes with other values than 1
    host = np.stack([rc.named_mask("two_blobs", h, w) * 255] * n)
    want = rc.boxes(host, (24, 40), 25, 8, 2)
    for offset in range(1, 16):
        buf = torch.full((n * h * w + offset,), 1, device="cuda", dtype=torch.uint8)
        m = buf[offset:].view(n, h, w)
        m.copy_(torch.from_numpy(host))
        assert m.data_ptr() % 16 == offset
        got, _ = _box(m, (24, 40), (25, 8), rc.min_size((h, w), (24, 40), 2)[::-1])
        assert np.array_equal(got.cpu().numpy(), want), offset
    from osvos_pytorch_amd import roi
    assert np.array_equal(roi.mask_box(torch.from_numpy(host > 0).cuda()[:, None], (24, 40)).cpu().numpy(), want)
    print("box %dx%d (N %d): %d calls, every one the numpy rule" % (h, w, n, calls))


def _cases(h, w, n):
    """(name, masks [n,h,w], canvas, boxes int32 [n,4]) over the named masks, the canvases and three (margin, zoom) settings"""
    out = []
    for i, (name, host) in enumerate(rc.mask_batches(h, w, n)):
        for canvas in rc.CANVASES:
            canvas = canvas or (h, w)
            for margin, zoom in (((25, 8), 2), ((0, 0), 4), ((100, 0), 1)):
                out.append((name, host, canvas, rc.boxes(host, canvas, margin[0], margin[1], zoom)))
    return out


@pytest.mark.parametrize("h,w,n", rc.FRAME_SIZES, ids=SIZE_IDS)
def test_view_kernel_is_the_tta_view_of_the_cropped_frame(h, w, n):
    host = tc.frames(h, w, n)
    fr = torch.from_numpy(host).cuda()
    worst, seen = 0.0, set()
    for name, _, canvas, boxes in _cases(h, w, n):
        key = (canvas, boxes.tobytes())
        if key in seen:
            continue
        seen.add(key)
        got = _view(fr, _dev_box(boxes), canvas)
        diff = float(np.abs(got.cpu().numpy().astype(np.float64) - rc.view_reference(host, boxes, canvas)).max())
        worst = max(worst, diff)
        assert diff <= tc.VIEW_BOUND, (name, canvas, boxes, diff)
        # an output 4 bytes off a 16-byte boundary (the one-pixel store form) holds the same bits
        assert _same_bits(_view(fr, _dev_box(boxes), canvas, offset=1), got), (name, canvas)
    # the full-frame box at the frame's size: osvos_tta_view's bits (which are osvos_augment_frame's identity output)
    full = _dev_box([[0, 0, w, h]] * n)
    assert _same_bits(_view(fr, full, (h, w)), _tta_view(fr, h, w)) and _same_bits(_view(fr, full, (h, w), offset=3), _tta_view(fr, h, w))
    # ... and on any canvas the full-frame box is osvos_tta_view at that size
    assert _same_bits(_view(fr, full, (17, 31)), _tta_view(fr, 17, 31)) and _same_bits(_view(fr, full, (24, 40)), _tta_view(fr, 24, 40))
    # a one-pixel box: the pixel minus the mean on every canvas pixel (both taps are that pixel, their weights sum to 1 up to rounding, as in
    # osvos_tta_view on a one-pixel source)
    one = _dev_box([[w - 1, h - 1, 1, 1]] * n)
    want = (host[:, h - 1, w - 1].astype(np.float32) - np.asarray(rc.MEANVAL, dtype=np.float32))[:, :, None, None] * np.ones((1, 1, 5, 7), np.float32)
    assert np.abs(_view(fr, one, (5, 7)).cpu().numpy() - want).max() <= tc.VIEW_BOUND
    print("view %dx%d (N %d): %d distinct (canvas, box) cases, worst |diff| %.2e of %.2e allowed" % (h, w, n, len(seen), worst, tc.VIEW_BOUND))


@pytest.mark.parametrize("h,w,n", rc.FRAME_SIZES, ids=SIZE_IDS)
def test_paste_kernel_resamples_into_the_box_and_writes_outside_everywhere_else(h, w, n):
    worst, seen = 0.0, set()
    for name, _, canvas, boxes in _cases(h, w, n):
        key = (canvas, boxes.tobytes())
        if key in seen:
            continue
        seen.add(key)
        lg_host = tc.logits(n, canvas[0], canvas[1], len(seen))
        lg, box = torch.from_numpy(lg_host).cuda(), _dev_box(boxes)
        outside = -20.0 if len(seen) % 2 else 3.4e38
        got = _paste(lg, box, (h, w), outside)
        ref, inside = rc.paste_reference(lg_host, boxes, (h, w), outside)
        out = got.cpu().numpy()
        big = float(np.abs(lg_host).max())
        diff = float(np.abs(out.astype(np.float64) - ref)[inside].max())
        worst = max(worst, diff / tc.fuse_bound(1, big))
        assert diff <= tc.fuse_bound(1, big), (name, canvas, boxes, diff)
        assert np.array_equal(out[~inside].view(np.uint32), np.full(int((~inside).sum()), np.float32(outside)).view(np.uint32)), (name, canvas, boxes)
        assert _same_bits(_paste(lg, box, (h, w), outside, offset=1), got), (name, canvas)
    print("paste %dx%d (N %d): %d distinct (canvas, box) cases, worst |diff| %.2f of the bound" % (h, w, n, len(seen), worst))


@pytest.mark.parametrize("h,w,n", rc.FRAME_SIZES, ids=SIZE_IDS)
def test_paste_of_a_canvas_of_the_boxs_size_passes_through_bit_for_bit(h, w, n):
    boxes = [(0, 0, w, h), (3, 2, w - 5, h - 4), (w - 4, h - 3, 4, 3), (1, 0, 1, h), (0, h - 1, w, 1)]
    for x0, y0, bw, bh in boxes:
        lg_host = tc.logits(n, bh, bw, 5)
        lg_host[0, 0, 0], lg_host[n - 1, bh - 1, bw - 1], lg_host[0, bh // 2, bw // 3] = np.inf, -np.inf, np.nan
        lg = torch.from_numpy(lg_host).cuda()
        box = _dev_box([[x0, y0, bw, bh]] * n)
        for offset in (0, 1):
            got = _paste(lg, box, (h, w), float("-inf"), offset=offset)
            assert _same_bits(got[:, y0:y0 + bh, x0:x0 + bw], lg), (x0, y0, bw, bh, offset)
            rest = np.ones((n, h, w), dtype=bool)
            rest[:, y0:y0 + bh, x0:x0 + bw] = False
            assert bool(np.all(np.isneginf(got.cpu().numpy()[rest]))), (x0, y0, bw, bh, offset)


def _stub(calls):
    def forward(x):
        calls.append(tuple(x.shape))
        return [0.05 * (x[:, 1:2] - x[:, 2:3])]          # green minus red (the frames are BGR)
    return forward


@pytest.mark.parametrize("h,w,n", [(37, 53, 2), (30, 85, 1), (48, 64, 1)], ids=["37x53x2", "30x85x1", "48x64x1"])
def test_roi_zoom_around_a_stub_forward_is_the_composition_of_the_three_references(h, w, n):
    from osvos_pytorch_amd import roi
    host = tc.frames(h, w, n, seed=5)
    fr = torch.from_numpy(host).cuda()
    stub_bound = 0.05 * (2 * tc.VIEW_BOUND + 4 * 2.0 ** -24 * 512)          # two view errors; the subtraction and the product round once each, below 512
    for canvas, margin, zoom, outside, (name, masks) in [(None, (25, 8), 2.0, -20.0, rc.mask_batches(h, w, n)[-1]), ((24, 40), (0, 0), 4, -7.5, rc.mask_batches(h, w, n)[6]),
                                                         ((17, 31), (100, 0), 1, -20.0, rc.mask_batches(h, w, n)[9])]:
        calls = []
        z = roi.RoiZoom(_stub(calls), canvas, margin[0], margin[1], zoom, outside)
        prev = torch.from_numpy(masks > 0).cuda()[:, None]          # bool [N,1,H,W], as FrameForward.remember keeps it
        got = z(fr if n > 1 else fr[0], prev)
        cv = canvas or (h, w)
        assert tuple(got.shape) == (n, 1, h, w) and calls == [(n, 3) + cv]
        boxes = rc.boxes(masks, cv, margin[0], margin[1], zoom)
        assert np.array_equal(z.box.cpu().numpy(), boxes)
        view = rc.view_reference(host, boxes, cv)
        maps = float(np.float32(0.05)) * (view[:, 1] - view[:, 2])
        ref, inside = rc.paste_reference(maps, boxes, (h, w), outside)
        bound = tc.fuse_bound(1, float(np.abs(maps).max())) + stub_bound
        out = got[:, 0].cpu().numpy()
        diff = float(np.abs(out.astype(np.float64) - ref)[inside].max())
        print("RoiZoom around the stub %dx%d, canvas %s, %s: |diff| %.2e of %.2e allowed" % (h, w, cv, name, diff, bound))
        assert diff <= bound, diff
        assert np.all(out[~inside] == np.float32(outside))
        # the wrappers are the kernels: the same bits as the calls through _lib, with and without out=
        box = roi.mask_box(prev, cv, margin[0], margin[1], zoom)
        v = roi.crop_view(fr, box, cv)
        assert _same_bits(v, _view(fr, box, cv)) and _same_bits(roi.crop_view(fr, box, cv, out=_dirty((n, 3) + cv)), v)
        y = _stub([])(v)[0]
        assert _same_bits(roi.paste(y, box, (h, w), outside), got) and _same_bits(_paste(y[:, 0].contiguous(), box, (h, w), outside)[:, None], got)
        assert _same_bits(roi.paste(y, box, (h, w), outside, out=_dirty((n, 1, h, w))), got)
        assert torch.equal(roi.mask_box(prev, cv, margin[0], margin[1], zoom, out=torch.zeros_like(box)), box)
    # no previous mask, and an empty one: the full frame, so the stub on the plain view
    plain = _stub([])(_tta_view(fr, h, w))[0]
    z = roi.RoiZoom(_stub([]))
    assert _same_bits(z(fr), plain) and _same_bits(z(fr, torch.zeros((n, 1, h, w), device="cuda", dtype=torch.bool)), plain)
    assert np.array_equal(z.box.cpu().numpy(), [[0, 0, w, h]] * n)
    with pytest.raises(ValueError):
        z(fr, torch.zeros((n, 1, h + 1, w), device="cuda", dtype=torch.bool))
    with pytest.raises(ValueError):
        roi.crop_view(fr, z.box.long(), (h, w))
    with pytest.raises(ValueError):
        roi.paste(plain, z.box, (h, w), out=torch.empty((n, h, w), device="cuda"))


@pytest.fixture(scope="module")
def trained_net():
    wts, _, _ = tf.train_like()
    return tf.build(wts, "fp32x3")


def test_roi_zoom_around_the_real_network_with_an_empty_previous_mask_is_the_plain_forward(trained_net):
    """30x85 frame of the trained-like fixture's kind, stored as the uint8 BGR frame a decoder would hand over"""
    from oracle import synth
    from osvos_pytorch_amd import roi
    from osvos_pytorch_amd.augment import augment_frame
    net = trained_net
    x, _ = synth.trainable_frame(1, 30, 85, seed=tf.RECIPE["frame_seed"] + 97)
    mean = np.asarray(rc.MEANVAL, dtype=np.float32).reshape(3, 1, 1)
    img = torch.from_numpy(np.clip(np.rint(x[0] + mean), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()).cuda()
    with torch.no_grad():
        plain = net.forward(augment_frame(img, None, False, None)[0][None])[-1]
        zoom = roi.RoiZoom(net.forward)
        assert _same_bits(zoom(img, torch.zeros((1, 1, 30, 85), device="cuda", dtype=torch.bool)), plain)
        assert _same_bits(zoom(img), plain)
        # around a small previous mask, enlarged up to four times: the box is the rule's, finite logits inside it, `outside` elsewhere
        prev = torch.zeros((1, 1, 30, 85), device="cuda", dtype=torch.bool)
        prev[..., 10:18, 30:45] = True
        zoom = roi.RoiZoom(net.forward, None, 0, 1, 4.0)
        zoomed = zoom(img, prev)
    x0, y0, bw, bh = (int(v) for v in zoom.box.cpu().numpy()[0])
    assert (x0, y0, bw, bh) == tuple(rc.boxes(prev[:, 0].cpu().numpy(), (30, 85), 0, 1, 4.0)[0]) and bw < 85 and bh < 30
    out = zoomed[0, 0].cpu().numpy()
    inside = np.zeros((30, 85), dtype=bool)
    inside[y0:y0 + bh, x0:x0 + bw] = True
    assert np.all(np.isfinite(out[inside])) and np.all(out[~inside] == np.float32(-20.0))
    print("RoiZoom around the network: box %s, mask pixels plain %d, zoomed %d of %d" % ((x0, y0, bw, bh), int((plain > 0).sum()), int((zoomed > 0).sum()), 30 * 85))


def test_train_online_multi_object_with_zoom(tmp_path):
    """two objects, each network on the crop around its own previous raw output; the masks keep the frame's size"""
    r = script_runner.train_online(tmp_path, "--multi-object", "--zoom", "2", frames=1)
    assert "J&F on blackswan (2 objects):" in r.stdout and "J&F on blackswan object 2:" in r.stdout, r.stdout[-2000:]
    png = r.masks[0]
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[12:16] == b"IHDR"
    assert struct.unpack(">II", png[16:24]) == (64, 48)          # width, height of script_runner's default frame


def test_train_online_single_object_with_zoom_over_a_moving_sequence(tmp_path):
    """three frames, the ellipse moving right: frames 1 and 2 run on the crop around the previous final mask, before the tracker"""
    r = script_runner.train_online(tmp_path, "--device-augment", "--synthetic-frames", "3", "--zoom", "2", "--zoom-margin", "10,2", "--track-components", "4",
                                   frames=3)
    assert "J&F on blackswan:" in r.stdout and "Components kept on blackswan:" in r.stdout, r.stdout[-2000:]
    for png in r.masks:
        assert struct.unpack(">II", png[16:24]) == (64, 48)
