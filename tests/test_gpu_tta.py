"""GPU: test-time augmentation on the device -- osvos_tta_view and osvos_tta_fuse (csrc/tta.hip) against the float64 restatement of the
sampling rule in tests/tta_cases.py, their exactness properties bit for bit (the same-size view is osvos_augment_frame's identity output, a
mirrored view is the plain one with its columns reversed, a same-size logit map passes through the fuse with inf and NaN), the scalar and
the 16-byte store forms against each other, osvos_pytorch_amd.tta.TestTimeAugment around a stub and around the real network, and
train_online.py --tta-scales --tta-flip.

Bounds (tests/tta_cases.py).  View: |diff| <= 16 * 2^-24 * 256 (2.4e-4): the inputs are exact integers below 256 and each weight carries one
rounding; the two lerps and the mean subtraction add at most eight fp32 roundings of magnitudes below 256; the bound is twice that.
Fuse: |diff| <= (8 + 2 V) * 2^-23 * M with M the case's largest |logit|: twice a count of at most 8 roundings per sample and 2 per
accumulated view.  Outputs are pre-filled with garbage; the osvos_* calls go through _lib."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tta_cases as tc
import trained_fixture as tf
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE = 7.25e33
SIZE_IDS = ["%dx%dx%d" % s for s in tc.FRAME_SIZES]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dirty(shape, offset=0):
    """a garbage-filled float32 CUDA tensor of `shape` that starts `offset` floats into its storage"""
    n = int(np.prod(shape))
    return torch.full((n + offset,), GARBAGE, device="cuda", dtype=torch.float32)[offset:].view(*shape)


def _view(fr, hv, wv, flip, offset=0):
    """one osvos_tta_view call on a uint8 CUDA tensor [N,H,W,3] -> float32 CUDA tensor [N,3,hv,wv]"""
    from osvos_pytorch_amd import _lib
    n, h, w, _ = fr.shape
    out = _dirty((n, 3, hv, wv), offset)
    mean = (C.c_float * 3)(*tc.MEANVAL)
    _lib.check(_lib.lib().osvos_tta_view(C.c_void_p(fr.data_ptr()), mean, C.c_void_p(out.data_ptr()), n, h, w, hv, wv, int(flip), _stream()), "tta_view")
    return out


def _fuse_rc(views, flips, size, weights=None, offset=0, V=None):
    from osvos_pytorch_amd import _lib
    n = views[0].shape[0]
    h, w = size
    out = _dirty((n, h, w), offset)
    k = len(views)
    ia = C.c_int * k
    wt = (C.c_float * k)(*weights) if weights is not None else None
    rc = _lib.lib().osvos_tta_fuse(_lib.ptr_array([v.data_ptr() for v in views]), ia(*[v.shape[1] for v in views]), ia(*[v.shape[2] for v in views]),
                                   ia(*[int(f) for f in flips]), wt, k if V is None else V, C.c_void_p(out.data_ptr()), n, h, w, _stream())
    return rc, out


def _fuse(views, flips, size, weights=None, offset=0):
    """one osvos_tta_fuse call on float32 CUDA tensors [N,hv,wv] -> float32 CUDA tensor [N,H,W]"""
    from osvos_pytorch_amd import _lib
    rc, out = _fuse_rc(views, flips, size, weights, offset)
    _lib.check(rc, "tta_fuse")
    return out


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("h,w,n", tc.FRAME_SIZES, ids=SIZE_IDS)
def test_view_kernel_against_the_float64_rule_and_its_exact_properties(h, w, n):
    from osvos_pytorch_amd.augment import augment_frame
    host = tc.frames(h, w, n)
    fr = torch.from_numpy(host).cuda()
    targets = [tc.view_size(h, w, s) for s in tc.SCALES + (2.5,)] + [(1, w), (h, 1), (1, 1), (1, 2 * w + 1)]
    worst = 0.0
    for hv, wv in targets:
        plain, flipped = _view(fr, hv, wv, False), _view(fr, hv, wv, True)
        ref = tc.view_reference(host, hv, wv)
        diff = float(np.abs(plain.cpu().numpy().astype(np.float64) - ref).max())
        worst = max(worst, diff)
        assert diff <= tc.VIEW_BOUND, (hv, wv, diff)
        assert _same_bits(flipped, plain.flip(3)), (hv, wv)
        # the one-pixel store form (an output 4 bytes off a 16-byte boundary) writes the same bits as the 16-byte form
        assert _same_bits(_view(fr, hv, wv, False, offset=1), plain) and _same_bits(_view(fr, hv, wv, True, offset=3), flipped), (hv, wv)
        if (hv, wv) == (h, w):
            for k in range(n):
                assert _same_bits(plain[k], augment_frame(fr[k], None, False, None)[0]), k
    print("view %dx%d (N %d): worst |diff| %.2e of %.2e allowed" % (h, w, n, worst, tc.VIEW_BOUND))


def test_view_kernel_on_a_one_pixel_source():
    host = np.array([[[[3, 200, 77]]], [[[255, 0, 128]]]], dtype=np.uint8)          # [2,1,1,3]
    fr = torch.from_numpy(host).cuda()
    for hv, wv in [(1, 1), (3, 5), (4, 8)]:
        for flip in (False, True):
            out = _view(fr, hv, wv, flip).cpu().numpy()
            want = (host.astype(np.float32).transpose(0, 3, 1, 2) - np.asarray(tc.MEANVAL, dtype=np.float32).reshape(1, 3, 1, 1)) * np.ones((1, 1, hv, wv), np.float32)
            assert np.abs(out - want).max() <= tc.VIEW_BOUND and np.abs(out.astype(np.float64) - tc.view_reference(host, hv, wv, flip)).max() <= tc.VIEW_BOUND


@pytest.mark.parametrize("h,w,n", tc.FRAME_SIZES, ids=SIZE_IDS)
def test_fuse_kernel_exact_cases(h, w, n):
    a_host, b_host = tc.logits(n, h, w, 1), tc.logits(n, h, w, 2)
    planted = a_host.copy()
    planted[0, 0, 0], planted[n - 1, h - 1, w - 1], planted[0, h // 2, w // 3] = np.inf, -np.inf, np.nan
    a, b, p = torch.from_numpy(a_host).cuda(), torch.from_numpy(b_host).cuda(), torch.from_numpy(planted).cuda()
    # V = 1, same size, unflipped, weight 1 (explicit and the default 1 / V): bit-identical, inf and NaN included
    assert _same_bits(_fuse([p], [False], (h, w), [1.0]), p) and _same_bits(_fuse([p], [False], (h, w)), p)
    assert _same_bits(_fuse([p], [False], (h, w), offset=1), p)
    # V = 2, the same map twice, weights 0.5
    assert _same_bits(_fuse([a, a], [False, False], (h, w), [0.5, 0.5]), a) and _same_bits(_fuse([a, a], [False, False], (h, w)), a)
    # V = 2, same size, one marked flipped
    want = np.float32(0.5) * a_host + np.float32(0.5) * b_host[..., ::-1]
    got = _fuse([a, b], [False, True], (h, w), [0.5, 0.5])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert _same_bits(_fuse([a, b], [False, True], (h, w), offset=1), got)


def _six_views(h, w, n, scales=(0.75, 1.0, 1.25)):
    host, flips = [], []
    for i, s in enumerate(scales):
        hv, wv = tc.view_size(h, w, s)
        for f in (False, True):
            host.append(tc.logits(n, hv, wv, 10 + 2 * i + int(f)))
            flips.append(f)
    return host, flips


@pytest.mark.parametrize("h,w,n", tc.FRAME_SIZES, ids=SIZE_IDS)
def test_fuse_kernel_six_views_against_the_float64_rule(h, w, n):
    host, flips = _six_views(h, w, n)
    dev = [torch.from_numpy(v).cuda() for v in host]
    big = max(float(np.abs(v).max()) for v in host)
    unequal = [0.3, 0.05, 0.25, 0.1, 0.2, 0.1]
    for weights in (None, unequal):
        got = _fuse(dev, flips, (h, w), weights)
        ref = tc.fuse_reference(host, flips, (h, w), None if weights is None else [float(np.float32(x)) for x in weights])
        diff = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print("fuse %dx%d (N %d) V 6 %s weights: |diff| %.2e of %.2e allowed" % (h, w, n, "default" if weights is None else "unequal", diff, tc.fuse_bound(6, big)))
        assert diff <= tc.fuse_bound(6, big), diff
        # the one-pixel store form, and a view that starts one float into its storage (4-byte aligned only): the same bits
        assert _same_bits(_fuse(dev, flips, (h, w), weights, offset=1), got)
        shifted = []
        for v in dev:
            s = _dirty(tuple(v.shape), offset=1)
            s.copy_(v)
            assert s.data_ptr() % 16 == 4
            shifted.append(s)
        assert _same_bits(_fuse(shifted, flips, (h, w), weights), got)


def test_fuse_kernel_sixteen_views_and_the_view_count_limits():
    from osvos_pytorch_amd import _lib
    h, w, n = 30, 85, 2
    host, flips = _six_views(h, w, n, scales=(0.5, 0.6, 0.75, 0.9, 1.0, 1.1, 1.25, 1.5))
    assert len(host) == 16
    dev = [torch.from_numpy(v).cuda() for v in host]
    big = max(float(np.abs(v).max()) for v in host)
    weights = [float(np.float32((i + 1) / 136.0)) for i in range(16)]
    for wts in (None, weights):
        got = _fuse(dev, flips, (h, w), wts)
        diff = float(np.abs(got.cpu().numpy().astype(np.float64) - tc.fuse_reference(host, flips, (h, w), wts)).max())
        print("fuse 30x85 V 16: |diff| %.2e of %.2e allowed" % (diff, tc.fuse_bound(16, big)))
        assert diff <= tc.fuse_bound(16, big), diff
    l = _lib.lib()
    rc, _ = _fuse_rc(dev + dev[:1], flips + [False], (h, w))
    assert rc < 0 and b"V 17 views" in l.osvos_last_error()
    rc, _ = _fuse_rc(dev, flips, (h, w), V=0)
    assert rc < 0 and b"V 0 views" in l.osvos_last_error()


def _stub(calls):
    def forward(x):
        calls.append(tuple(x.shape))
        return [0.01 * x.sum(1, keepdim=True)]
    return forward


@pytest.mark.parametrize("h,w,n", [(37, 53, 2), (30, 85, 1)], ids=["37x53x2", "30x85x1"])
def test_test_time_augment_around_a_stub_forward(h, w, n):
    from osvos_pytorch_amd import tta
    host = tc.frames(h, w, n, seed=5)
    fr = torch.from_numpy(host).cuda()
    calls = []
    scales = (0.75, 1.0, 1.25)
    fused, maps, plan = tta.TestTimeAugment(_stub(calls), scales, flip=True)(fr if n > 1 else fr[0], return_views=True)
    assert plan == tta.plan(h, w, scales, True) and len(maps) == 6 and tuple(fused.shape) == (n, 1, h, w)
    assert calls == [(2 * n, 3) + tc.view_size(h, w, s) for s in scales]          # one call per scale, the plain and the mirrored view in one batch
    ref_maps = [0.01 * tc.view_reference(host, hv, wv, f).sum(1) for hv, wv, f in plan]
    ref = tc.fuse_reference(ref_maps, [f for _, _, f in plan], (h, w))
    big = max(float(np.abs(m).max()) for m in ref_maps)
    bound = tc.fuse_bound(6, big) + 0.03 * tc.VIEW_BOUND
    diff = float(np.abs(fused[:, 0].cpu().numpy().astype(np.float64) - ref).max())
    print("TestTimeAugment around the stub %dx%d: |diff| %.2e of %.2e allowed" % (h, w, diff, bound))
    assert diff <= bound, diff
    # return_views hands back exactly the maps that were fused: the stub on the views, and their fuse is the result
    for i, s in enumerate(scales):
        hv, wv = tc.view_size(h, w, s)
        both = 0.01 * torch.cat([tta.make_view(fr, hv, wv, False), tta.make_view(fr, hv, wv, True)]).sum(1, keepdim=True)
        assert _same_bits(maps[2 * i], both[:n]) and _same_bits(maps[2 * i + 1], both[n:])
    assert _same_bits(tta.fuse_views(maps, [f for _, _, f in plan], (h, w)), fused)
    assert _same_bits(_fuse([m[:, 0].contiguous() for m in maps], [f for _, _, f in plan], (h, w))[:, None], fused)
    # without flip: batch N per call; explicit weights reach the kernel
    calls.clear()
    wts = [0.5, 0.25, 0.25]
    f2, m2, p2 = tta.TestTimeAugment(_stub(calls), scales, weights=wts)(fr, return_views=True)
    assert calls == [(n, 3) + tc.view_size(h, w, s) for s in scales] and [f for _, _, f in p2] == [False] * 3
    assert _same_bits(f2, tta.fuse_views(m2, [False] * 3, (h, w), wts)) and not _same_bits(f2, tta.fuse_views(m2, [False] * 3, (h, w)))


@pytest.fixture(scope="module")
def trained_net():
    wts, _, _ = tf.train_like()
    return tf.build(wts, "fp32x3")


def test_test_time_augment_around_the_real_network(trained_net):
    """30x85 frame of the trained-like fixture's kind (oracle/synth.trainable_frame, stored as the uint8 BGR frame a decoder would hand over)"""
    from oracle import synth
    from osvos_pytorch_amd import tta
    from osvos_pytorch_amd.augment import augment_frame
    net = trained_net
    x, _ = synth.trainable_frame(1, 30, 85, seed=tf.RECIPE["frame_seed"] + 97)
    mean = np.asarray(tc.MEANVAL, dtype=np.float32).reshape(3, 1, 1)
    img = torch.from_numpy(np.clip(np.rint(x[0] + mean), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()).cuda()
    with torch.no_grad():
        plain = net.forward(augment_frame(img, None, False, None)[0][None])[-1]
        one = tta.TestTimeAugment(net.forward, (1.0,), False)(img)
        assert _same_bits(one, plain)
        fused, maps, plan = tta.TestTimeAugment(net.forward, (0.75, 1, 1.25), True)(img, return_views=True)
    assert tuple(fused.shape) == (1, 1, 30, 85) and bool(torch.isfinite(fused).all())
    host = [m[:, 0].cpu().numpy() for m in maps]
    big = max(float(np.abs(m).max()) for m in host)
    diff = float(np.abs(fused[:, 0].cpu().numpy().astype(np.float64) - tc.fuse_reference(host, [f for _, _, f in plan], (30, 85))).max())
    print("TestTimeAugment around the network: |diff| %.2e of %.2e allowed; mask pixels plain %d, fused %d of %d"
          % (diff, tc.fuse_bound(6, big), int((plain > 0).sum()), int((fused > 0).sum()), 30 * 85))
    assert diff <= tc.fuse_bound(6, big), diff
    assert int((plain > 0).sum()) > 0 and int((fused > 0).sum()) > 0


def test_train_online_with_test_time_augmentation(tmp_path):
    r = script_runner.train_online(tmp_path, "--device-augment", "--tta-scales", "0.75,1,1.25", "--tta-flip")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Online training time" in r.stdout and "J&F on blackswan:" in r.stdout, r.stdout[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path), "Results", "blackswan", "00000.png"))


def test_train_online_multi_object_with_test_time_augmentation(tmp_path):
    """the --multi-object loop takes tta(frame) per object network: two objects, mirrored views, merged label map, J and F per object"""
    r = script_runner.train_online(tmp_path, "--multi-object", "--tta-flip")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "J&F on blackswan (2 objects):" in r.stdout and "J&F on blackswan object 2:" in r.stdout, r.stdout[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path), "Results", "blackswan", "00000.png"))


def test_device_test_frames_hand_over_the_decoded_frame_and_skip_the_identity_pass_when_asked():
    """train_online.DeviceTestFrames: 'frame_u8' is the decoded frame; raw_only (test-time augmentation on) makes 'image' only where an
    annotation needs the pass for its 'gt'"""
    import train_online
    from osvos_pytorch_amd.augment import augment_frame
    from osvos_pytorch_amd.davis_io import ArrayFrames
    img = tc.frames(30, 85, 1)[0]
    lab = (tc.frames(30, 85, 1, seed=3)[0, :, :, 0] > 127).astype(np.uint8) * 255
    frames = ArrayFrames([(img, lab), (img, None)])
    dev = torch.device("cuda:0")
    plain = list(train_online.DeviceTestFrames(frames, dev, 2))
    raw = list(train_online.DeviceTestFrames(frames, dev, 2, raw_only=True))
    want = augment_frame(torch.from_numpy(img).cuda(), None, False, None)[0][None]
    for s in plain + raw:
        assert np.array_equal(s["frame_u8"].cpu().numpy(), img)
    assert [sorted(s) for s in plain] == [["fname", "frame_u8", "gt", "image"], ["fname", "frame_u8", "image"]]
    assert [sorted(s) for s in raw] == [["fname", "frame_u8", "gt", "image"], ["fname", "frame_u8"]]
    assert _same_bits(plain[1]["image"], want) and _same_bits(raw[0]["gt"], plain[0]["gt"])
