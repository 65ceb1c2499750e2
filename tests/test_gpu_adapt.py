"""GPU: online adaptation over the sequence -- osvos_mask_sqdist and osvos_adapt_targets (csrc/distance.hip) bit for bit against the numpy
restatements of tests/adapt_cases.py, the void rule of the class-balanced loss (OSVOS_CBCE_VOID, csrc/loss.hip) against the float64 oracle on
the non-void pixels, osvos_pytorch_amd.adapt.OnlineAdapter around a stub and around the real network, and train_online.py --adapt-steps.

Bounds.  Distance maps, labels and counts are integers and raw float comparisons: exact, no tolerance.  Void loss: the bars of
test_gpu_ops.test_cbce_loss_and_grad (rtol 1e-5 on the loss, rtol 2e-5 / atol 2e-8 * max on the gradient); the gradient at void pixels is
+0.0 bit for bit.  Outputs are pre-filled with garbage; the osvos_* calls go through _lib."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import adapt_cases as ac
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE = 7.25e33
VOID, PER_IMAGE, ZEROED = 4, 1, 2          # OSVOS_CBCE_VOID, OSVOS_CBCE_PER_IMAGE, OSVOS_CBCE_SCRATCH_ZEROED
vp = C.c_void_p


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _dirty(shape, offset=0):
    n = int(np.prod(shape))
    return torch.full((n + offset,), GARBAGE, device="cuda", dtype=torch.float32)[offset:].view(*shape)


def _shifted(host, offset):
    """the float32 array on the device, starting `offset` floats into its storage"""
    t = _dirty(host.shape, offset)
    t.copy_(torch.from_numpy(host))
    return t


# ---- distance maps ---------------------------------------------------------------------------------------------------------------------

def _sqdist_rc(mask, invert, dims=None, null=()):
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    n, h, w = dims or mask.shape
    out = torch.full(tuple(mask.shape), -77, device="cuda", dtype=torch.int32)
    ws = torch.full((max(1, int(l.osvos_mask_sqdist_ws_bytes(*mask.shape)) // 4),), -5, device="cuda", dtype=torch.int32)
    rc = l.osvos_mask_sqdist(None if "mask" in null else vp(mask.data_ptr()), int(invert), None if "out" in null else vp(out.data_ptr()), n, h, w,
                             None if "ws" in null else vp(ws.data_ptr()), _stream())
    return rc, out


@pytest.mark.parametrize("kind", ac.MASK_KINDS)
@pytest.mark.parametrize("n,h,w", ac.SQDIST_SIZES, ids=["%dx%dx%d" % s for s in ac.SQDIST_SIZES])
def test_sqdist_bit_exact(n, h, w, kind):
    from osvos_pytorch_amd import _lib, results
    host = ac.make_mask(kind, n, h, w)
    dev = torch.from_numpy(host).cuda()
    for invert in (0, 1):
        rc, out = _sqdist_rc(dev, invert)
        _lib.check(rc, "mask_sqdist")
        want = ac.sqdist_of_mask(host, invert)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (kind, invert, int((got != want).sum()))
        assert np.array_equal(results.distance_map(dev, invert=bool(invert)).cpu().numpy(), want)
    assert _lib.SQDIST_NONE == ac.NONE


def test_sqdist_host_wrapper_shapes_and_argument_errors():
    from osvos_pytorch_amd import _lib, results
    l = _lib.lib()
    host = ac.make_mask("p0.002", 2, 37, 65)
    want = ac.sqdist_of_mask(host, 0)
    dev = torch.from_numpy(host).cuda()
    d = results.distance_map(dev[:, None].float())                 # [N,1,H,W] float: non-zero = set
    assert d.dtype == torch.int32 and tuple(d.shape) == (2, 37, 65) and np.array_equal(d.cpu().numpy(), want)
    assert np.array_equal(results.distance_map(dev[1] != 0).cpu().numpy(), want[1:2])      # [H,W] bool
    small = torch.zeros((1, 4, 4), device="cuda", dtype=torch.uint8)
    for dims in ((1, 4097, 4), (1, 4, 4097), (0, 4, 4), (1, 0, 4)):
        rc, _ = _sqdist_rc(small, 0, dims=dims)
        assert rc < 0 and b"sides 1..4096" in l.osvos_last_error(), dims
        assert l.osvos_mask_sqdist_ws_bytes(*dims) == 0 and l.osvos_adapt_ws_bytes(*dims) == 0
    for null in ("mask", "out", "ws"):
        rc, _ = _sqdist_rc(small, 0, null=(null,))
        assert rc < 0 and b"null" in l.osvos_last_error(), null
    assert l.osvos_mask_sqdist_ws_bytes(1, 4096, 4096) == 4 * 4096 * 4096
    with pytest.raises(ValueError):
        results.distance_map(torch.zeros((1, 2, 4097), device="cuda", dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        results.distance_map(torch.zeros((1, 4, 4), dtype=torch.uint8))


# ---- adaptation targets ----------------------------------------------------------------------------------------------------------------

def _targets(logits, prev, pos_logit, erosion, distance):
    """one osvos_adapt_targets call on host arrays [N,H,W] -> (label [N,H,W] float32, counts [N,3] int64) host arrays"""
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    n, h, w = logits.shape
    x, m = torch.from_numpy(logits).cuda(), torch.from_numpy(prev).cuda()
    label = _dirty((n, h, w))
    counts = torch.full((n, 3), -9, device="cuda", dtype=torch.int64)
    ws = torch.full((int(l.osvos_adapt_ws_bytes(n, h, w)) // 4,), -5, device="cuda", dtype=torch.int32)
    _lib.check(l.osvos_adapt_targets(vp(x.data_ptr()), vp(m.data_ptr()), float(pos_logit), erosion, distance, vp(label.data_ptr()),
                                     vp(counts.data_ptr()), n, h, w, vp(ws.data_ptr()), _stream()), "adapt_targets")
    return label.cpu().numpy(), counts.cpu().numpy()


def _same_labels(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("h,w,erosion,distance,want", ac.TARGET_CASES, ids=["48x80", "37x53", "64x96"])
def test_targets_bit_exact_on_the_shared_cases(h, w, erosion, distance, want):
    from osvos_pytorch_amd import adapt
    logits, prev = ac.target_case(h, w)
    ref = ac.targets_reference(logits, prev, ac.POS_LOGIT, erosion, distance)
    got = _targets(logits, prev, ac.POS_LOGIT, erosion, distance)
    assert _same_labels(got, ref) and tuple(got[1][0]) == want
    # the host entry point: prob 0.97 is this logit
    label, counts = adapt.adaptation_targets(torch.from_numpy(logits).cuda()[:, None], torch.from_numpy(prev).cuda(), prob=0.97, erosion=erosion,
                                             distance=distance)
    assert tuple(label.shape) == (1, 1, h, w) and label.dtype == torch.float32 and counts.dtype == torch.int64
    assert _same_labels((label[:, 0].cpu().numpy(), counts.cpu().numpy()), ref)


def test_targets_edge_values_and_extremes():
    h, w, erosion, distance, _ = ac.TARGET_CASES[0]
    logits, prev = ac.target_case(h, w)
    t = np.float32(ac.POS_LOGIT)
    inside = np.argwhere(ac.eroded(prev, erosion)[0])
    (y0, x0), (y1, x1), (y2, x2) = inside[0], inside[len(inside) // 2], inside[-1]
    logits[0, y0, x0], logits[0, y1, x1], logits[0, y2, x2] = t, np.nan, np.inf          # exactly at the threshold, NaN, +inf: void, void, positive
    ref = ac.targets_reference(logits, prev, ac.POS_LOGIT, erosion, distance)
    assert ref[0][0, y0, x0] == -1 and ref[0][0, y1, x1] == -1 and ref[0][0, y2, x2] == 1
    assert _same_labels(_targets(logits, prev, ac.POS_LOGIT, erosion, distance), ref)
    # an erosion that empties E: everything negative, whatever the distance
    for dist in (0, 100000):
        got = _targets(logits, prev, ac.POS_LOGIT, 40, dist)
        assert (got[0] == 0).all() and got[1].tolist() == [[0, h * w, 0]]
        assert _same_labels(got, ac.targets_reference(logits, prev, ac.POS_LOGIT, 40, dist))
    # a distance beyond the image: nothing negative
    for dist in (200, 100000):
        got = _targets(logits, prev, ac.POS_LOGIT, erosion, dist)
        assert got[1][0, 1] == 0 and _same_labels(got, ac.targets_reference(logits, prev, ac.POS_LOGIT, erosion, dist))
    # a mask that fills the image erodes to itself
    got = _targets(logits, np.full_like(prev, 3), ac.POS_LOGIT, 1000, 0)
    assert got[1][0, 1] == 0 and _same_labels(got, ac.targets_reference(logits, np.full_like(prev, 3), ac.POS_LOGIT, 1000, 0))


def test_targets_two_images_with_different_masks():
    h, w = 37, 53
    l0, p0 = ac.target_case(h, w, seed=1)
    l1, _ = ac.target_case(h, w, seed=2)
    p1 = (ac.ellipse(h, w, cx=0.3, cy=0.4, ry=0.3, rx=0.15).astype(np.uint8) * 200)[None]
    logits, prev = np.concatenate([l0, l1]), np.concatenate([p0, p1])
    for erosion, distance in ((0, 3), (2, 5)):
        ref = ac.targets_reference(logits, prev, ac.POS_LOGIT, erosion, distance)
        assert _same_labels(_targets(logits, prev, ac.POS_LOGIT, erosion, distance), ref)
        assert not np.array_equal(ref[1][0], ref[1][1])
    # an image without a mask next to one with: all negative, and the neighbour untouched
    prev[0] = 0
    ref = ac.targets_reference(logits, prev, ac.POS_LOGIT, 0, 3)
    assert ref[1][0].tolist() == [0, h * w, 0] and _same_labels(_targets(logits, prev, ac.POS_LOGIT, 0, 3), ref)


# ---- void pixels in the class-balanced loss ----------------------------------------------------------------------------------------------

def _cbce(outs, label, mode, flags, n_img=None, offset=0, scratch=None, counts=None, want_rc=False):
    """one osvos_cbce_step_ex call.  outs: list of float32 host arrays (heads) of one shape, label: host array of that shape.
    -> (losses float32 host [heads], grads: list of CUDA tensors, scratch CUDA uint8 tensor)"""
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    k = len(outs)
    n_img = n_img or outs[0].shape[0]
    dev_outs = [_shifted(np.ascontiguousarray(o, dtype=np.float32), offset) for o in outs]
    lab = _shifted(np.ascontiguousarray(label, dtype=np.float32), offset)
    grads = [_dirty(o.shape, offset) for o in outs]
    losses = torch.full((k,), GARBAGE, device="cuda", dtype=torch.float32)
    if scratch is None:
        scratch = torch.zeros(int(l.osvos_cbce_scratch_bytes(k, n_img, flags)), device="cuda", dtype=torch.uint8)
        flags |= ZEROED
    rc = l.osvos_cbce_step_ex((vp * k)(*[vp(o.data_ptr()) for o in dev_outs]), vp(lab.data_ptr()), (vp * k)(*[vp(losses.data_ptr() + 4 * i) for i in range(k)]),
                              (vp * k)(*[vp(g.data_ptr()) for g in grads]), vp(scratch.data_ptr()), lab.numel(), n_img, mode, flags,
                              vp(counts.data_ptr()) if counts is not None else None, k, (C.c_float * k)(*([1.0] * k)), None, _stream())
    if want_rc:
        return rc
    _lib.check(rc, "cbce_step_ex")
    return losses.cpu().numpy(), grads, scratch


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def _void_inputs(shape, share, seed=3):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal(shape) * 4).astype(np.float32)
    lab = (rng.random(shape) > 0.8).astype(np.float32)
    lab[rng.random(shape) < share] = -1.0
    return logits, lab


def _void_reference(logits, lab, mode):
    """float64 oracle on the non-void pixels, flattened to one image; batch_average divides by the images of the call, as without void"""
    from oracle import c_oracle
    live = lab >= 0
    grad = np.zeros(logits.shape, dtype=np.float64)
    if not live.any():
        return 0.0, grad
    x, y = logits[live].astype(np.float64)[None], lab[live].astype(np.float64)[None]
    loss, g = c_oracle.cbce(x, y, 0 if mode == 0 else 2)
    if mode == 1:
        loss, g = loss / logits.shape[0], g / logits.shape[0]
    grad[live] = g[0]
    return loss, grad


VOID_SHAPES = [((2, 1, 37, 53), 0), ((3, 1, 7, 9), 0), ((2, 1, 32, 48), 0), ((2, 1, 32, 48), 1)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("share", [0.3, 1.0, 0.0], ids=["void30", "allvoid", "novoid"])
@pytest.mark.parametrize("shape,offset", VOID_SHAPES, ids=["2x37x53", "3x7x9", "2x32x48", "2x32x48+4B"])
def test_void_loss_against_the_float64_oracle_on_the_non_void_pixels(shape, offset, share, mode):
    from osvos_pytorch_amd import _lib
    logits, lab = _void_inputs(shape, share)
    assert (share == 1.0) == bool((lab < 0).all()) and (share == 0.0) == bool((lab >= 0).all())
    ref_loss, ref_grad = _void_reference(logits, lab, mode)
    losses, grads, scratch = _cbce([logits], lab, mode, VOID, offset=offset)
    assert grads[0].data_ptr() % 16 == 4 * offset
    assert scratch.numel() == _lib.lib().osvos_cbce_scratch_bytes(1, shape[0], 0) + 8 and int(scratch.max()) == 0
    grad = grads[0].cpu().numpy()
    print("void loss %s mode %d share %.1f: loss %.8g ref %.8g; max |dgrad| %.3e" % (shape, mode, share, losses[0], ref_loss, np.abs(grad - ref_grad).max()))
    assert np.isfinite(losses[0]) and abs(losses[0] - ref_loss) <= 1e-5 * abs(ref_loss) + 1e-12
    np.testing.assert_allclose(grad, ref_grad, rtol=2e-5, atol=2e-8 * np.abs(ref_grad).max())
    assert (_bits(grad)[lab < 0] == 0).all()                       # +0.0f, written over the garbage
    if share == 1.0:
        assert losses[0] == 0.0 and (_bits(grad) == 0).all()
    if share == 0.0:                                               # no void pixel: the numbers of the call without the flag
        l0, g0, _ = _cbce([logits], lab, mode, 0, offset=offset)
        assert np.array_equal(_bits(l0), _bits(losses)) and np.array_equal(_bits(g0[0]), _bits(grad))


@pytest.mark.parametrize("mode", [0, 1])
def test_void_loss_per_image_with_one_image_entirely_void(mode):
    shape = (3, 1, 32, 48)
    logits, lab = _void_inputs(shape, 0.3, seed=5)
    lab[1] = -1.0
    losses, grads, scratch = _cbce([logits], lab, mode, VOID | PER_IMAGE)
    assert int(scratch.max()) == 0 and scratch.numel() == 8 * 3 + 16 * 3 + 8 + 8 * 3
    singles = [_cbce([logits[i:i + 1]], lab[i:i + 1], mode, VOID) for i in (0, 2)]
    want = np.float32(singles[0][0][0]) + np.float32(singles[1][0][0])
    print("per-image void: loss %.8g, sum of the single calls %.8g" % (losses[0], want))
    assert np.isfinite(losses[0]) and abs(losses[0] - want) <= 1e-6 * abs(want)
    grad = grads[0]
    assert np.array_equal(_bits(grad[0:1]), _bits(singles[0][1][0])) and np.array_equal(_bits(grad[2:3]), _bits(singles[1][1][0]))
    assert (_bits(grad[1]) == 0).all()
    # odd image size: the element-wise sweep of the per-image mode
    logits, lab = _void_inputs((3, 1, 7, 9), 0.3, seed=6)
    lab[0] = -1.0
    losses, grads, _ = _cbce([logits], lab, mode, VOID | PER_IMAGE)
    singles = [_cbce([logits[i:i + 1]], lab[i:i + 1], mode, VOID) for i in (1, 2)]
    want = np.float32(singles[0][0][0]) + np.float32(singles[1][0][0])
    assert abs(losses[0] - want) <= 1e-6 * abs(want) and (_bits(grads[0][0]) == 0).all()
    assert np.array_equal(_bits(grads[0][1:2]), _bits(singles[0][1][0])) and np.array_equal(_bits(grads[0][2:3]), _bits(singles[1][1][0]))


def test_void_loss_five_heads_equal_five_single_head_calls():
    shape = (2, 1, 37, 53)
    _, lab = _void_inputs(shape, 0.3)
    heads = [(np.random.default_rng(20 + k).standard_normal(shape) * 4).astype(np.float32) for k in range(5)]
    for flags in (VOID, VOID | PER_IMAGE):
        losses, grads, scratch = _cbce(heads, lab, 1, flags)
        assert int(scratch.max()) == 0
        for k in range(5):
            l1, g1, _ = _cbce([heads[k]], lab, 1, flags)
            assert abs(l1[0] - losses[k]) <= 1e-6 * abs(l1[0]), k
            assert np.array_equal(_bits(g1[0]), _bits(grads[k])), k


def test_void_loss_twenty_calls_on_one_scratch_never_zeroed_again():
    from osvos_pytorch_amd import _lib
    shape = (2, 1, 32, 48)
    scratch = torch.zeros(int(_lib.lib().osvos_cbce_scratch_bytes(1, 2, VOID | PER_IMAGE)), device="cuda", dtype=torch.uint8)
    for it in range(20):
        logits, lab = _void_inputs(shape, (0.0, 0.3, 1.0, 0.6)[it % 4], seed=100 + it)
        flags = VOID | (PER_IMAGE if it % 2 else 0)
        l1, g1, _ = _cbce([logits], lab, it % 3, flags | ZEROED, scratch=scratch)
        assert int(scratch.max()) == 0, it
        l2, g2, fresh = _cbce([logits], lab, it % 3, flags)
        assert int(fresh.max()) == 0, it
        assert abs(l1[0] - l2[0]) <= 1e-6 * abs(l2[0]) and np.array_equal(_bits(g1[0]), _bits(g2[0])), it


def test_void_flag_with_external_counts_is_an_argument_error_and_minus_one_without_the_flag_is_a_negative():
    from osvos_pytorch_amd import _lib, autograd
    assert autograd.CBCE_VOID == VOID
    shape = (2, 1, 37, 53)
    logits, lab = _void_inputs(shape, 0.3)
    counts = torch.tensor([100.0, 3922.0, 2.0], device="cuda")
    rc = _cbce([logits], lab, 1, VOID, counts=counts, want_rc=True)
    assert rc < 0 and b"void" in _lib.lib().osvos_last_error()
    with pytest.raises(RuntimeError):
        autograd.cbce_step(torch.from_numpy(logits).cuda(), torch.from_numpy(lab).cuda(), 1, counts=counts, void_labels=True)
    # today's behaviour stays: without the flag a label of -1 is a negative-class pixel
    for offset in (0, 1):
        for mode in (0, 1, 2):
            a = _cbce([logits], lab, mode, 0, offset=offset)
            b = _cbce([logits], np.where(lab < 0, np.float32(0), lab), mode, 0, offset=offset)
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1][0]), _bits(b[1][0]))
            assert a[2].numel() == 32 and int(a[2].max()) == 0


def test_void_labels_through_the_python_layers():
    """cbce_step(void_labels=True), the drop-in's void_pixels= with autograd behind it, and TrainLoop.micro_batch's refusal off the fused path"""
    from layers.osvos_layers import class_balanced_cross_entropy_loss
    from osvos_pytorch_amd.layers.osvos_layers import class_balanced_cross_entropy_loss_step, class_balanced_cross_entropy_loss_step_multi
    from osvos_pytorch_amd.train_common import TrainLoop
    shape = (2, 1, 37, 53)
    logits, lab = _void_inputs(shape, 0.3)
    x, y = torch.from_numpy(logits).cuda(), torch.from_numpy(lab).cuda()
    for size_average, mode in ((True, 0), (False, 1)):
        ref_loss, ref_grad = _void_reference(logits, lab, mode)
        loss, grad = class_balanced_cross_entropy_loss_step(x, y, size_average=size_average, grad_scale=0.5, void_labels=True)
        assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)
        np.testing.assert_allclose(grad.cpu().numpy(), 0.5 * ref_grad, rtol=2e-5, atol=2e-8 * np.abs(ref_grad).max())
        losses, grads = class_balanced_cross_entropy_loss_step_multi([x, x], y, size_average=size_average, grad_scales=[0.5, 0.5], void_labels=True)
        assert np.array_equal(_bits(grads[0]), _bits(grad)) and np.array_equal(_bits(grads[1]), _bits(grad))
        # the drop-in: label in {0, 1} and a void map; differentiable (loss * 3 -> gradient * 3)
        xr = x.clone().requires_grad_()
        out = class_balanced_cross_entropy_loss(xr, (y > 0.5).float(), size_average=size_average, void_pixels=(y < 0).float())
        assert abs(float(out.detach()) - ref_loss) <= 1e-5 * abs(ref_loss)
        (out * 3).backward()
        np.testing.assert_allclose(xr.grad.cpu().numpy(), 3 * ref_grad, rtol=2e-5, atol=2e-8 * 3 * np.abs(ref_grad).max())
        assert (_bits(xr.grad)[lab < 0] == 0).all()
    stub = _StubNet().cuda()
    loop = TrainLoop(stub, torch.optim.SGD(stub.parameters(), lr=1e-8), mode='online', n_ave_grad=1, loss_fn=class_balanced_cross_entropy_loss)
    with pytest.raises(RuntimeError):
        loop.micro_batch(torch.zeros((1, 3, 8, 8), device="cuda"), torch.zeros((1, 1, 8, 8), device="cuda"), void_labels=True)


# ---- the adapter -----------------------------------------------------------------------------------------------------------------------

class _StubNet(torch.nn.Module):
    """one learnable 1x1 convolution (logit = channel 0 at the start) that records (tag of the input, gradients enabled) per call"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 1, 1)
        with torch.no_grad():
            self.conv.weight.copy_(torch.tensor([1.0, 0.0, 0.0]).view(1, 3, 1, 1))
            self.conv.bias.zero_()
        self.calls = []

    def forward(self, x):
        self.calls.append((float(x[0, 1, 0, 0]), torch.is_grad_enabled()))
        return [self.conv(x)]


def _stub_adapter(logits, steps, mix, weight=0.25):
    from osvos_pytorch_amd import adapt
    h, w = logits.shape[-2:]
    stub = _StubNet().cuda()
    image = torch.zeros((1, 3, h, w), device="cuda")
    image[0, 0] = torch.from_numpy(logits[0]).cuda()
    image[0, 1] = 111.0                                            # tag: the current frame
    draws = []

    def first_inputs():
        first = torch.zeros((1, 3, h, w), device="cuda")
        first[0, 0] = torch.from_numpy(np.where(ac.ellipse(h, w), 4.0, -4.0).astype(np.float32)).cuda()
        first[0, 1] = 222.0                                        # tag: the annotated first frame
        draws.append(first)
        return first, torch.from_numpy(ac.ellipse(h, w).astype(np.float32)).cuda()[None, None]

    ad = adapt.OnlineAdapter(stub, torch.optim.SGD(stub.parameters(), lr=1e-7), first_inputs, steps=steps, mix=mix, weight=weight, prob=0.97,
                             erosion=2, distance=9)
    kinds = []
    inner = ad.loop.micro_batch

    def spy(inputs, gts, epoch=0, void_labels=False, grad_scale=1.0):
        kinds.append((void_labels, grad_scale, float(gts.min())))
        return inner(inputs, gts, epoch, void_labels=void_labels, grad_scale=grad_scale)
    ad.loop.micro_batch = spy
    return ad, stub, image, kinds, draws


def test_adapter_around_a_stub_network_order_and_kind_of_the_steps():
    h, w, _, _, want = ac.TARGET_CASES[0]
    logits, prev = ac.target_case(h, w)
    ad, stub, image, kinds, draws = _stub_adapter(logits, steps=5, mix=2)
    assert ad.loop.n_ave_grad == 1
    before = stub.conv.weight.detach().clone(), stub.conv.bias.detach().clone()
    with torch.no_grad():                                          # as the test loop of train_online.py calls it
        out = ad(image, torch.from_numpy(prev).cuda())
    cur, first = 111.0, 222.0
    assert stub.calls == [(cur, False), (first, True), (cur, True), (first, True), (cur, True), (first, True), (cur, False)]
    assert kinds == [(False, 1.0, 0.0), (True, 0.25, -1.0), (False, 1.0, 0.0), (True, 0.25, -1.0), (False, 1.0, 0.0)]
    assert len(draws) == 3 and ad.loop.steps == 5
    assert ad.summary() == {"adapted": 1, "skipped": 0, "steps": 5}
    assert tuple(out.shape) == (1, 1, h, w) and not out.requires_grad and bool(torch.isfinite(out).all())
    assert not (torch.equal(stub.conv.weight.detach(), before[0]) and torch.equal(stub.conv.bias.detach(), before[1]))
    # a second frame without a confident pixel: no positive target, only the first-frame steps run
    image2 = image.clone()
    image2[0, 0] = -4.0
    stub.calls.clear()
    kinds.clear()
    ad(image2, out > 0)
    assert stub.calls == [(cur, False), (first, True), (first, True), (first, True), (cur, False)]
    assert [k[0] for k in kinds] == [False] * 3
    assert ad.summary() == {"adapted": 1, "skipped": 1, "steps": 8}
    # steps = 0: one plain forward, nothing else
    ad0, stub0, image0, kinds0, draws0 = _stub_adapter(logits, steps=0, mix=2)
    out0 = ad0(image0, torch.from_numpy(prev).cuda())
    assert stub0.calls == [(cur, False)] and not kinds0 and not draws0 and ad0.summary() == {"adapted": 0, "skipped": 0, "steps": 0}
    assert torch.equal(out0, stub0.conv(image0))


def _real_net(seed=0):
    import networks.vgg_osvos as vo
    torch.manual_seed(seed)
    net = vo.OSVOS(pretrained=0).cuda()
    net.set_precision("fp32x3")
    return net


def _two_frames(h=48, w=64):
    rng = np.random.RandomState(11)
    base = (rng.randn(1, 3, h, w) * 40).astype(np.float32)
    frames = [torch.from_numpy(np.roll(base, 4 * f, axis=3).copy()).cuda() for f in range(2)]
    gt = torch.from_numpy(ac.ellipse(h, w).astype(np.float32)).cuda()[None, None]
    return frames, gt


def test_adapter_around_the_real_network_with_zero_steps_is_the_plain_forward():
    from osvos_pytorch_amd import adapt
    from osvos_pytorch_amd.train_common import make_sgd
    net = _real_net()
    frames, gt = _two_frames()
    before = [p.detach().clone() for p in net.parameters()]
    ad = adapt.OnlineAdapter(net, make_sgd(net, 'online', lr=1e-3), lambda: (frames[0], gt), steps=0)
    prev = gt > 0.5
    with torch.no_grad():
        for f in frames:
            out = ad(f, prev)
            assert np.array_equal(_bits(out), _bits(net.forward(f)[-1]))
            prev = out > 0
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert ad.summary() == {"adapted": 0, "skipped": 0, "steps": 0}


def test_adapter_around_the_real_network_with_two_steps_trains():
    from osvos_pytorch_amd import adapt
    from osvos_pytorch_amd.train_common import make_sgd
    net = _real_net()
    frames, gt = _two_frames()
    before = [p.detach().clone() for p in net.parameters()]
    ad = adapt.OnlineAdapter(net, make_sgd(net, 'online', lr=1e-3), lambda: (frames[0], gt), steps=2, mix=2, prob=0.5, erosion=2, distance=9)
    prev = gt > 0.5
    with torch.no_grad():
        for f in frames:
            out = ad(f, prev)
            assert tuple(out.shape) == (1, 1, 48, 64) and bool(torch.isfinite(out).all())
            prev = gt > 0.5
    s = ad.summary()
    assert s["adapted"] + s["skipped"] == 2 and s["steps"] == 2 + s["adapted"]
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())


def _run_script(tmp_path, extra):
    return script_runner.train_online(tmp_path, "--device-augment", "--synthetic-frames", "3", *extra, height=64, width=96)


def test_train_online_with_online_adaptation(tmp_path):
    r = _run_script(tmp_path, ["--adapt-steps", "2", "--adapt-mix", "2", "--adapt-distance", "12", "--adapt-erosion", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Online training time" in r.stdout and "J&F on blackswan:" in r.stdout, r.stdout[-2000:]
    assert "Online adaptation on blackswan: 2 frames seen" in r.stdout, r.stdout[-2000:]
    for f in range(3):
        assert os.path.exists(os.path.join(str(tmp_path), "Results", "blackswan", "%05d.png" % f))


def test_train_online_three_synthetic_frames_without_adaptation(tmp_path):
    r = _run_script(tmp_path, ["--adapt-mix", "2", "--adapt-distance", "12", "--adapt-erosion", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "J&F on blackswan:" in r.stdout and "over 3 frames" in r.stdout and "Online adaptation" not in r.stdout, r.stdout[-2000:]
    for f in range(3):
        assert os.path.exists(os.path.join(str(tmp_path), "Results", "blackswan", "%05d.png" % f))
