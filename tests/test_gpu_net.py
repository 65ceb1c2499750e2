"""GPU parity tests of the whole hot path through the drop-in API (networks.vgg_osvos.OSVOS +
layers.osvos_layers.class_balanced_cross_entropy_loss) against
  (a) the golden vectors produced by the real reference (tests/golden/*.npz), and
  (b) the torch-CPU functional oracle on the same seeded inputs at larger sizes up to 854x480.
Tolerances (SURVEY.md 8d, fp32 path): max |dlogit| <= 1e-3 * std(logit), loss rel <= 1e-5,
per-tensor gradient rel-L2 <= 1e-3, mask IoU(logit > 0) >= 1 - 1e-3."""
import numpy as np
import pytest
import torch

from golden_util import CASES, check_grad, check_grad_either, grad_keys, load_case

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3      # x std(logit)
LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-3
IOU_TOL = 1e-3


# the two fp32 arithmetics of the convolutions: exact fp32 MFMA and f32x3 (three-way bf16 split on the bf16 matrix pipe);
# both are held to the same fp32 bars.  The module's default is fp32x3, so every un-parametrised test of the GPU tier runs under it;
# OSVOS_TEST_PRECISION=fp32 runs them on the exact kernels instead.
FP32_MODES = ["fp32", "fp32x3", "fp32x3b2", "fp32h2", "fp32x3h2"]


def build_net(wts, precision=None):
    import os
    import networks.vgg_osvos as vo
    net = vo.OSVOS(pretrained=0)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in wts.items()})
    net = net.cuda()
    precision = precision or os.environ.get("OSVOS_TEST_PRECISION", "")
    if precision:
        net.set_precision(precision)
    return net


def iou(a, b):
    a, b = a > 0, b > 0
    u = np.logical_or(a, b).sum()
    return 1.0 if u == 0 else np.logical_and(a, b).sum() / u


@pytest.mark.parametrize("precision", FP32_MODES)
@pytest.mark.parametrize("name", CASES)
def test_forward_matches_reference_golden(name, precision):
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    g, wts, x, m = load_case(name)
    net = build_net(wts, precision)
    with torch.no_grad():
        outs = net.forward(torch.from_numpy(x).cuda())
    assert len(outs) == 5
    gt = torch.from_numpy(m).cuda()
    for i, o in enumerate(outs):
        ref = g["f32|out%d" % i]
        assert tuple(o.shape) == ref.shape
        err = np.abs(o.cpu().numpy() - ref).max()
        assert err <= LOGIT_TOL * ref.std(), (name, i, err, ref.std())
        assert iou(o.cpu().numpy(), ref) >= 1 - IOU_TOL
        l = cbce(o, gt, size_average=False).item()
        assert abs(l - g["f32|parent|heads"][i]) <= LOSS_RTOL * abs(g["f32|parent|heads"][i]), (name, i, l)


@pytest.mark.parametrize("precision", FP32_MODES)
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", ["online", "parent"])
def test_gradients_match_reference_golden(name, mode, precision):
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    g, wts, x, m = load_case(name)
    net = build_net(wts, precision)
    xin = torch.from_numpy(x)
    xin.requires_grad_()                      # train_online.py:121-122: requires_grad then .to(device)
    xd = xin.cuda()
    gt = torch.from_numpy(m).cuda()
    outs = net.forward(xd)
    if mode == "online":
        loss = cbce(outs[-1], gt, size_average=False)
    else:
        losses = [cbce(o, gt, size_average=False) for o in outs]
        loss = (1 - 60 / 240) * sum(losses[:-1]) + losses[-1]
    pre = "f32|%s|" % mode
    assert abs(loss.item() - float(g[pre + "loss"])) <= LOSS_RTOL * abs(float(g[pre + "loss"]))
    loss /= 5
    loss.backward()
    have = {k: v.grad for k, v in net.named_parameters() if v.grad is not None}
    for k in grad_keys(g, pre + "grad|"):
        if k == "input":
            check_grad_either(g, mode, k, xin.grad.numpy(), GRAD_RTOL, what=name)
        elif k.startswith("upscale"):
            assert k not in have               # frozen deconvs: gradient intentionally not formed
        else:
            check_grad_either(g, mode, k, have[k].cpu().numpy(), GRAD_RTOL, what=name)
    if mode == "online":
        assert "score_dsn.0.weight" not in have


def test_sgd_trajectory_matches_reference_golden():
    """2 optimizer steps of the online loop (train_online.py:79-88,112-149) with nAveGrad = 2."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    g, wts, x, m = load_case("c48x64")
    net = build_net(wts)
    from osvos_pytorch_amd.train_common import make_sgd
    opt = make_sgd(net, "online", lr=1e-8, fused=False)      # the scripts' own parameter-group table on torch.optim.SGD (FusedSGD: test_gpu_ops)
    w0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    losses = []
    xd, gt = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    for it in range(4):
        outs = net.forward(xd)
        loss = cbce(outs[-1], gt, size_average=False)
        losses.append(loss.item())
        loss /= 2
        loss.backward()
        if it % 2 == 1:
            opt.step()
            opt.zero_grad()
    np.testing.assert_allclose(losses, g["sgd|losses"], rtol=2e-5)
    sd = net.state_dict()
    for k in w0:
        check_grad(g, "sgd|delta|", k, (sd[k] - w0[k]).cpu().numpy(), 3e-3, what="sgd")


def _oracle_run(wts, x, m, dtype, channels_last=False):
    from oracle import torch_ref
    p = torch_ref.as_leaf_params(wts, dtype=dtype)
    xin = torch.from_numpy(x).to(dtype)
    if channels_last:       # the reference CPU path's other ATen/oneDNN code path (different summation order)
        xin = xin.contiguous(memory_format=torch.channels_last)
    xin.requires_grad_()
    outs = torch_ref.forward(p, xin)
    losses = [torch_ref.cbce_loss(o, torch.from_numpy(m).to(dtype), size_average=False) for o in outs]
    (0.5 * sum(losses[:-1]) + losses[-1]).backward()
    grads = {k: v.grad.double() for k, v in p.items() if v.grad is not None and not k.startswith("upscale")}
    grads["input"] = xin.grad.double()
    return [o.detach().double().numpy() for o in outs], [l.item() for l in losses], grads


_ORACLE_CACHE = {}


def _oracle_runs_cached(shape):
    if shape not in _ORACLE_CACHE:
        from oracle import synth
        n, h, w = shape
        wts, x, m = synth.calibrated_problem(n, h, w, seed=21)
        _ORACLE_CACHE.clear()          # one shape at a time (the 854x480 float64 tape is large)
        _ORACLE_CACHE[shape] = (wts, x, m, _oracle_run(wts, x, m, torch.float64), _oracle_run(wts, x, m, torch.float32),
                                _oracle_run(wts, x, m, torch.float32, channels_last=True)[2])
    return _ORACLE_CACHE[shape]


@pytest.mark.parametrize("shape,precision", [((2, 120, 214), "fp32"), ((2, 120, 214), "fp32x3"), ((1, 240, 427), "fp32"),
                                             ((1, 480, 854), "fp32"), ((1, 480, 854), "fp32x3")])
def test_full_size_against_cpu_oracle(shape, precision):
    """Same seeded frame through the torch-CPU oracle (float64 = ground truth, float32 = the
    reference CPU path) and the HIP path; parent-style deep supervision (side weight 0.5) so one
    backward exercises every gradient.  On this un-trained He-init net the reference's OWN fp32
    gradients sit up to 4e-3 (rel-L2) from float64 for the stage-0 tensors, and move by 10x with
    the memory format torch happens to run (NCHW vs channels_last kernels: ReLU / arg-max flips at
    near-ties are chaotic), so the bar is: within 1e-3 of float64, or no worse than 2x the
    reference fp32 CPU path's own distance from float64 (worse of its two code paths)."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    wts, x, m, (t_outs, t_losses, t_grads), (r_outs, r_losses, r_grads), r_grads_cl = _oracle_runs_cached(shape)

    net = build_net(wts, precision)
    xg = torch.from_numpy(x).requires_grad_()
    outs = net.forward(xg.cuda())
    gt = torch.from_numpy(m).cuda()
    losses = [cbce(o, gt, size_average=False) for o in outs]
    (0.5 * sum(losses[:-1]) + losses[-1]).backward()
    for i in range(5):
        truth = t_outs[i]
        got = outs[i].detach().cpu().double().numpy()
        ref_err = np.abs(r_outs[i] - truth).max()
        assert np.abs(got - truth).max() <= max(LOGIT_TOL * truth.std(), 1.5 * ref_err), (shape, i)
        assert iou(got, truth) >= 1 - IOU_TOL
        assert abs(losses[i].item() - t_losses[i]) <= max(LOSS_RTOL * abs(t_losses[i]), 1.5 * abs(r_losses[i] - t_losses[i]))
    have = {k: v.grad.cpu().double() for k, v in net.named_parameters() if v.grad is not None}
    have["input"] = xg.grad.double()
    report = []
    for k, truth in t_grads.items():
        err = float((have[k] - truth).norm() / (truth.norm() + 1e-30))
        ref_err = max(float((r_grads[k] - truth).norm() / (truth.norm() + 1e-30)),
                      float((r_grads_cl[k] - truth).norm() / (truth.norm() + 1e-30)))
        report.append((err / max(GRAD_RTOL, 2.0 * ref_err), k, err, ref_err))
    report.sort(reverse=True)
    print("%s gradients (ours vs f64 | reference-f32 vs f64):" % precision, [(k, "%.1e" % e, "%.1e" % r) for _, k, e, r in report])
    assert report[0][0] <= 1.0, report[0]


def test_intermediate_activations_via_ws_query():
    """layer-by-layer check of the saved activations (diagnostic granularity for the C orchestration)."""
    import ctypes as C
    import torch.nn.functional as F
    from oracle import synth, torch_ref
    from osvos_pytorch_amd import _lib
    from osvos_pytorch_amd.autograd import OSVOSNetFunction
    n, h, w = 1, 45, 67
    wts, x, _ = synth.calibrated_problem(n, h, w, seed=5)
    net = build_net(wts)
    xg = torch.from_numpy(x).cuda().requires_grad_()
    outs = net.forward(xg)
    ws = outs[0].grad_fn.saved_tensors[0]
    p = {k: torch.from_numpy(v) for k, v in wts.items()}
    cur = torch.from_numpy(x)
    names = torch_ref.trunk_conv_names()
    l = 0
    lib = _lib.lib()
    for si in range(5):
        if si > 0:
            cur = F.max_pool2d(cur, 2, 2, ceil_mode=True)
        for nm in names[si]:
            cur = F.relu(F.conv2d(cur, p[nm + ".weight"], p[nm + ".bias"], padding=1))
            off, el, ch, hh, ww = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
            dt = net._runtime.dtype
            _lib.check(lib.osvos_net_ws_query(n, h, w, dt, l, C.byref(off), C.byref(el), C.byref(ch), C.byref(hh), C.byref(ww)))
            fmt = lib.osvos_net_ws_format(dt, l)
            assert fmt == 0
            act = ws[off.value:off.value + 4 * el.value].view(torch.float32).view(n, hh.value, ww.value, ch.value)
            got = act.permute(0, 3, 1, 2).cpu()
            err = float((got - cur).abs().max() / (cur.abs().max() + 1e-30))
            assert err < 1e-4, ("trunk conv", l, err)
            l += 1


def test_cpu_tensors_are_refused():
    from oracle import synth
    net2 = build_net(synth.make_weights(1))
    with pytest.raises(RuntimeError):
        net2.forward(torch.zeros(1, 3, 16, 16))       # CPU tensor: no fallback


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 48, 64)])
def test_generic_transposed_conv_head_matches_the_reference_semantics(shape):
    """upscale[i].weight NOT diagonal (the reference runs arbitrary [16,16,k,k] ConvTranspose2d weights, vgg_osvos.py:46,68; only
    interp_surgery + lr 0 make them bilinear-diagonal in practice): the generic head (csrc/head_generic.hip) must reproduce the
    float64 oracle -- logits of all five heads, losses, and EVERY gradient including the deconv weights themselves, which the
    commuted fast head never forms.  Also: perturbing one off-diagonal tap flips a net from the fast to the generic path."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    from oracle import synth, torch_ref
    n, h, w = shape
    wts, x, m = synth.calibrated_problem(n, h, w, seed=31)
    rng = np.random.RandomState(5)
    for i in range(4):      # dense, un-structured deconv weights of the size of the bilinear ones
        k = 4 << i
        wts["upscale.%d.weight" % i] = (wts["upscale.%d.weight" % i] + rng.randn(16, 16, k, k).astype(np.float32) * (0.5 / k)).astype(np.float32)
        wts["upscale_.%d.weight" % i] = (wts["upscale_.%d.weight" % i] * (1.0 + 0.3 * rng.randn(1, 1, k, k))).astype(np.float32)
    p = torch_ref.as_leaf_params(wts, dtype=torch.float64)
    xin = torch.from_numpy(x).double().requires_grad_()
    outs_t = torch_ref.forward(p, xin)
    losses_t = [torch_ref.cbce_loss(o, torch.from_numpy(m).double(), size_average=False) for o in outs_t]
    (0.5 * sum(losses_t[:-1]) + losses_t[-1]).backward()

    net = build_net(wts)
    xg = torch.from_numpy(x).requires_grad_()
    outs = net.forward(xg.cuda())
    assert net._runtime.generic_head
    gt = torch.from_numpy(m).cuda()
    losses = [cbce(o, gt, size_average=False) for o in outs]
    (0.5 * sum(losses[:-1]) + losses[-1]).backward()
    for i in range(5):
        truth = outs_t[i].detach().numpy()
        got = outs[i].detach().cpu().double().numpy()
        assert np.abs(got - truth).max() <= LOGIT_TOL * truth.std(), (shape, i, np.abs(got - truth).max(), truth.std())
        assert abs(losses[i].item() - losses_t[i].item()) <= 2e-5 * abs(losses_t[i].item()), (shape, i)
    have = {k: v.grad for k, v in net.named_parameters() if v.grad is not None}
    assert set(have) == {k for k, v in p.items() if v.grad is not None}          # incl. upscale.* and upscale_.*
    worst = []
    for k, v in p.items():
        e = float((have[k].cpu().double() - v.grad).norm() / (v.grad.norm() + 1e-30))
        worst.append((e, k))
    worst.sort(reverse=True)
    print("generic head gradients vs float64:", [(k, "%.1e" % e) for e, k in worst[:6]])
    assert worst[0][0] <= 2e-3, worst[0]          # (stage-0 tensors carry the usual ReLU / arg-max flip noise of an un-trained net)
    assert float((xg.grad.double() - xin.grad).norm() / xin.grad.norm()) <= 5e-3
    # a second backward accumulates in place (deconv gradients included)
    net.set_inplace_grad_accumulation(True)
    outs = net.forward(torch.from_numpy(x).cuda())
    losses = [cbce(o, gt, size_average=False) for o in outs]
    (0.5 * sum(losses[:-1]) + losses[-1]).backward()
    for k in ("upscale.2.weight", "upscale_.1.weight", "fuse.weight", "stages.3.1.weight"):
        e = float((net.state_dict(keep_vars=True)[k].grad.cpu().double() - 2 * p[k].grad).norm() / (2 * p[k].grad).norm())
        assert e <= 2e-3, (k, e)
    # fast path <-> generic path switch follows the weights
    wts2 = synth.make_weights(1)
    fast = build_net(wts2)
    with torch.no_grad():
        fast.forward(torch.from_numpy(x).cuda())
        assert not fast._runtime.generic_head
        fast.upscale[1].weight[0, 1, 2, 2] = 0.25
        fast.forward(torch.from_numpy(x).cuda())
        assert fast._runtime.generic_head
    # round 6: the generic head also runs on the bf16 trunk (it refused until round 5)
    fast.set_precision("bf16")
    with torch.no_grad():
        fast.forward(torch.from_numpy(x).cuda())
    assert fast._runtime.generic_head


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 48, 64)])
def test_generic_transposed_conv_head_on_the_bf16_trunk(shape):
    """vgg_osvos.py:46,68 runs ANY [16,16,k,k] ConvTranspose2d weights; with precision 'bf16' (bf16 trunk tensors, fp32 head) the generic head must
    deliver what the fast head delivers in that precision: logits within the bf16 bars of the float64 oracle, the deconv / fuse / score_dsn gradients
    (formed in fp32 from fp32 side_prep outputs) close to float64, the trunk gradients within the bf16 gradient bar -- and the side_prep
    convolutions must have read the bf16 copy of dprep the generic backward now writes (a missing copy = garbage trunk gradients)."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    from oracle import synth, torch_ref
    n, h, w = shape
    wts, x, m = synth.calibrated_problem(n, h, w, seed=31)
    rng = np.random.RandomState(5)
    for i in range(4):
        k = 4 << i
        wts["upscale.%d.weight" % i] = (wts["upscale.%d.weight" % i] + rng.randn(16, 16, k, k).astype(np.float32) * (0.5 / k)).astype(np.float32)
        wts["upscale_.%d.weight" % i] = (wts["upscale_.%d.weight" % i] * (1.0 + 0.3 * rng.randn(1, 1, k, k))).astype(np.float32)
    p = torch_ref.as_leaf_params(wts, dtype=torch.float64)
    xin = torch.from_numpy(x).double().requires_grad_()
    outs_t = torch_ref.forward(p, xin)
    losses_t = [torch_ref.cbce_loss(o, torch.from_numpy(m).double(), size_average=False) for o in outs_t]
    (0.5 * sum(losses_t[:-1]) + losses_t[-1]).backward()
    res = {}
    for prec in ("bf16", "fp32"):
        net = build_net(wts).set_precision(prec)
        outs = net.forward(torch.from_numpy(x).cuda().requires_grad_())
        assert net._runtime.generic_head
        gt = torch.from_numpy(m).cuda()
        losses = [cbce(o, gt, size_average=False) for o in outs]
        (0.5 * sum(losses[:-1]) + losses[-1]).backward()
        res[prec] = ([o.detach().cpu().double().numpy() for o in outs], {k: v.grad.cpu().double() for k, v in net.named_parameters() if v.grad is not None})
    outs_b, grads_b = res["bf16"]
    for i in range(5):
        truth = outs_t[i].detach().numpy()
        assert np.abs(outs_b[i] - truth).max() <= 0.1 * truth.std(), (shape, i, np.abs(outs_b[i] - truth).max(), truth.std())
    assert set(grads_b) == set(res["fp32"][1])
    errs = sorted(((float((grads_b[k] - p[k].grad).norm() / (p[k].grad.norm() + 1e-30)), k) for k in grads_b), reverse=True)
    print("generic head on the bf16 trunk, gradients vs float64:", [(k, "%.1e" % e) for e, k in errs[:6]])
    # (the head's gradients are formed in fp32, but FROM the bf16 trunk's side_prep outputs and from upstream gradients that depend on bf16-noisy
    #  logits: they carry the trunk's noise; score_dsn biases are cancelling sums -- measured 0.29 on one of them, 0.19 on the worst trunk tensor)
    for e, k in errs:
        assert e <= (0.25 if k.startswith(("stages.", "side_prep.")) else 0.4), (k, e)
    fp = res["fp32"][1]
    for k in grads_b:
        if k.startswith("upscale"):      # deconv weight gradients exist and follow the fp32 run's
            assert float((grads_b[k] - fp[k]).norm() / (fp[k].norm() + 1e-30)) <= 0.4, k


def test_batch_and_odd_sizes_no_grad_inference():
    """inference path of train_online.py:172-189 (no_grad, sigmoid on the host)"""
    from oracle import synth, torch_ref
    from layers.osvos_layers import sigmoid_np
    for (n, h, w) in [(3, 33, 41), (1, 1, 1), (1, 2, 3), (2, 101, 135)]:
        if h * w >= 64:
            wts, x, _ = synth.calibrated_problem(n, h, w, seed=9)
        else:      # head calibration needs a map with a spread; tiny frames use the raw He-init heads
            wts, x = synth.make_weights(1), synth.make_frame(n, h, w, 9)
        net = build_net(wts)
        with torch.no_grad():
            got = net.forward(torch.from_numpy(x).cuda())[-1].cpu().numpy()
            ref = torch_ref.forward({k: torch.from_numpy(v) for k, v in wts.items()}, torch.from_numpy(x))[-1].numpy()
        assert np.abs(got - ref).max() <= max(LOGIT_TOL * ref.std(), 1e-5 * np.abs(ref).max(), 1e-6), (n, h, w)
        assert np.abs(sigmoid_np(got) - sigmoid_np(ref)).max() < 1e-4


@pytest.mark.parametrize("precision", ["fp32x3", "bf16", "fp32", "fp32h2", "fp32x2", "bf16w2"])
def test_inference_forward_skips_backward_only_outputs_and_keeps_every_logit_bit(precision):
    """OSVOS_FLAG_INFERENCE (round 6): under torch.no_grad() (train_online.py:172-181) the forward writes neither the one-bit ReLU
    masks nor the pool-code bytes -- which only a backward reads -- and runs in the inference-sized workspace; the five logit maps must be
    bit-identical to the ones of a forward that a backward could follow, at even and odd sizes.  The module's parameters are trainable, as
    in the product: OSVOS.forward reads grad mode itself (autograd.wants_backward), so the no_grad forward here IS the flagged one -- until
    that decision existed both forwards of this test were the training forward.  What the flagged call writes, and the same identity at
    the library call: tests/test_gpu_inference_forward.py."""
    from oracle import synth
    for (n, h, w) in [(2, 60, 107), (1, 33, 41), (2, 48, 64)]:
        wts, x, _ = synth.calibrated_problem(n, h, w, seed=12)
        net = build_net(wts).set_precision(precision)
        xs = torch.from_numpy(x).cuda()
        with torch.no_grad():
            a = [o.clone() for o in net.forward(xs)]
        b = net.forward(xs.clone().requires_grad_())
        for u, v in zip(a, b):
            assert torch.equal(u, v.detach()), (precision, n, h, w)


def test_forward_is_hipgraph_capturable():
    """the whole forward (two streams, ~45 launches, no allocation inside the library) replays from a
    captured graph and reproduces the eager result bit for bit"""
    from oracle import synth
    wts, x, _ = synth.calibrated_problem(2, 60, 107, seed=4)
    net = build_net(wts)
    xs = torch.from_numpy(x).cuda()
    with torch.no_grad():
        for _ in range(2):
            eager = [o.clone() for o in net.forward(xs)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = net.forward(xs)
        xs.copy_(torch.from_numpy(x[::-1].copy()).cuda())      # new input in the captured buffer (batch order flipped)
        g.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e.flip(0))


@pytest.mark.parametrize("shape", [(2, 120, 214), (1, 240, 427)])
def test_bf16_mfma_precision_mode(shape):
    """net.set_precision('bf16'): conv forward/data-gradient on bf16 MFMA operands, fp32 accumulate, fp32 tensors,
    head / loss / skinny weight gradients in fp32.  Bars against float64 truth: logits
    <= 0.1 std, gradient rel-L2 <= 0.25, loss rel <= 1e-2, and both within a small factor of what the reference CPU
    path itself delivers under torch bf16 autocast (measured: ours and autocast land within 2x of each other, either
    way, head by head -- bf16 rounding noise is chaotic on this un-trained net)."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    from oracle import synth, torch_ref
    n, h, w = shape
    wts, x, m = synth.calibrated_problem(n, h, w, seed=21)
    t_outs, t_losses, t_grads = _oracle_run(wts, x, m, torch.float64)
    # the reference CPU path under bf16 autocast (what PyTorch itself calls bf16 training)
    p = torch_ref.as_leaf_params(wts)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        a_outs = torch_ref.forward(p, torch.from_numpy(x))
    a_losses = [torch_ref.cbce_loss(o.float(), torch.from_numpy(m), size_average=False) for o in a_outs]
    (0.5 * sum(a_losses[:-1]) + a_losses[-1]).backward()
    a_err = {k: float((v.grad.double() - t_grads[k]).norm() / t_grads[k].norm()) for k, v in p.items() if k in t_grads}

    net = build_net(wts).set_precision("bf16")
    xg = torch.from_numpy(x).requires_grad_()
    outs = net.forward(xg.cuda())
    gt = torch.from_numpy(m).cuda()
    losses = [cbce(o, gt, size_average=False) for o in outs]
    (0.5 * sum(losses[:-1]) + losses[-1]).backward()
    lerr = [abs(losses[i].item() - t_losses[i]) / abs(t_losses[i]) for i in range(5)]
    aerr = [abs(a_losses[i].item() - t_losses[i]) / abs(t_losses[i]) for i in range(5)]
    print("bf16 loss rel err (ours | torch-CPU autocast):", ["%.1e|%.1e" % (e, a) for e, a in zip(lerr, aerr)])
    for i in range(5):
        got = outs[i].detach().cpu().double().numpy()
        assert np.abs(got - t_outs[i]).max() <= 0.1 * t_outs[i].std(), (shape, i, np.abs(got - t_outs[i]).max())
        assert lerr[i] <= min(1e-2, max(2e-3, 4.0 * aerr[i])), (i, losses[i].item(), t_losses[i], a_losses[i].item())
    have = {k: v.grad.cpu().double() for k, v in net.named_parameters() if v.grad is not None}
    rep = sorted(((float((have[k] - t_grads[k]).norm() / t_grads[k].norm()), a_err[k], k) for k in have), reverse=True)
    print("bf16 gradients (ours | torch-CPU autocast) vs f64:", [(k, "%.1e" % e, "%.1e" % a) for e, a, k in rep[:8]],
          "fused IoU", iou(outs[4].detach().cpu().numpy(), t_outs[4]))
    for e, a, k in rep:
        assert e <= 0.25 and e <= max(2.5 * a, 6e-2), (k, e, a)


def test_bf16_store_mode_within_the_bf16_bars(tmp_path):
    """bf16-store mode (the default of precision 'bf16'; OSVOS_BF16_STORE=0 = fp32 tensors): trunk activations / gradients live in HBM as bf16 only.  Same bars against float64 as the default
    bf16 mode (logits <= 0.1 std, loss rel <= 1e-2, gradient rel-L2 <= 0.25), and close to the default bf16 mode itself."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent('''
        import sys, numpy as np, torch
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import test_gpu_net as T
        from oracle import synth
        from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
        wts, x, m = synth.calibrated_problem(2, 120, 214, seed=21)
        net = T.build_net(wts).set_precision("bf16")
        xg = torch.from_numpy(x).cuda().requires_grad_()
        outs = net.forward(xg)
        gt = torch.from_numpy(m).cuda()
        losses = [cbce(o, gt, size_average=False) for o in outs]
        (0.5 * sum(losses[:-1]) + losses[-1]).backward()
        res = {"out%%d" %% i: o.detach().cpu().numpy() for i, o in enumerate(outs)}
        res.update({"loss%%d" %% i: np.array(l.item()) for i, l in enumerate(losses)})
        res.update({"g:" + k: v.grad.cpu().numpy() for k, v in net.named_parameters() if v.grad is not None})
        res["dx"] = xg.grad.cpu().numpy()
        np.savez(sys.argv[1], **res)
    ''') % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = {}
    for flag in ("0", "1"):
        out = str(tmp_path / ("s%s.npz" % flag))
        subprocess.run([sys.executable, "-c", code, out], check=True, env=dict(os.environ, OSVOS_BF16_STORE=flag), timeout=900)
        got[flag] = dict(np.load(out))
    from oracle import synth
    wts, x, m = synth.calibrated_problem(2, 120, 214, seed=21)
    t_outs, t_losses, t_grads = _oracle_run(wts, x, m, torch.float64)
    a, b = got["0"], got["1"]
    for i in range(5):
        assert np.abs(b["out%d" % i] - t_outs[i]).max() <= 0.1 * t_outs[i].std(), i
        assert abs(float(b["loss%d" % i]) - t_losses[i]) / abs(t_losses[i]) <= 1e-2, i
    worst = []
    for k, tg in t_grads.items():
        if "g:" + k not in b:
            continue
        e1 = float(np.linalg.norm(b["g:" + k].astype(np.float64) - tg.numpy()) / np.linalg.norm(tg.numpy()))
        e0 = float(np.linalg.norm(a["g:" + k].astype(np.float64) - tg.numpy()) / np.linalg.norm(tg.numpy()))
        worst.append((e1, e0, k))
        assert e1 <= 0.25 and e1 <= max(2.0 * e0, 6e-2), (k, e1, e0)
    assert len(worst) > 30
    worst.sort(reverse=True)
    print("bf16-store gradients vs f64 (store | default bf16):", [(k, "%.1e" % e1, "%.1e" % e0) for e1, e0, k in worst[:6]])
    rel = float(np.linalg.norm(b["dx"] - a["dx"]) / np.linalg.norm(a["dx"]))
    print("input gradient, store vs default bf16 mode: rel-L2 %.2e" % rel)
    assert np.isfinite(b["dx"]).all() and rel <= 0.5


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 30, 85), (1, 9, 7), (1, 16, 16)])
def test_bf16_store_mode_odd_sizes_stay_close_to_fp32(shape):
    """ceil-mode pooling / partial windows / 1x1 frames through the bf16 kernels (bf16 pooling, bf16 masks, bf16-input weight
    gradients): logits within 0.25 std of the fp32 mode (tiny frames are noisy), every gradient finite and within 0.5 rel-L2 of the fp32 mode"""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    from oracle import synth
    n, h, w = shape
    wts, x, m = synth.calibrated_problem(n, h, w, seed=33)
    res = {}
    for prec in ("fp32", "bf16"):
        net = build_net(wts).set_precision(prec)
        outs = net.forward(torch.from_numpy(x).cuda())
        gt = torch.from_numpy(m).cuda()
        (0.5 * sum(cbce(o, gt, size_average=False) for o in outs[:-1]) + cbce(outs[-1], gt, size_average=False)).backward()
        res[prec] = ([o.detach().cpu() for o in outs], {k: v.grad.cpu() for k, v in net.named_parameters() if v.grad is not None})
    for a, b in zip(*[res[p][0] for p in ("fp32", "bf16")]):
        tol = max(0.25 * max(float(a.std()) if a.numel() > 1 else 0.0, 3.0), 0.05 * float(a.abs().max()))      # (the 1x1 problem calibrates to huge logits)
        assert torch.isfinite(b).all() and float((a - b).abs().max()) <= tol
    for k, ga in res["fp32"][1].items():
        gb = res["bf16"][1][k]
        assert torch.isfinite(gb).all(), k
        if float(ga.norm()) > 0:
            assert float((ga - gb).norm() / ga.norm()) <= 0.5, (k, float((ga - gb).norm() / ga.norm()))


@pytest.mark.parametrize("inplace", [False, True])
def test_partially_frozen_layers_get_the_right_gradients(inplace):
    """A conv whose weight is frozen while its bias trains (and the other way round) still receives the trainable half: the
    weight-gradient kernel forms both halves in one launch, the unwanted one goes to scratch (the bias target was
    returned uninitialised).  Checked against the all-trainable run, with and without in-place .grad accumulation."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    from oracle import synth
    wts, x, m = synth.calibrated_problem(1, 37, 53, seed=9)
    xd, gt = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()

    def run(freeze):
        net = build_net(wts)
        net.set_inplace_grad_accumulation(inplace)
        named = dict(net.named_parameters())
        for k in freeze:
            named[k].requires_grad_(False)
        for rep in range(2 if inplace else 1):          # second pass accumulates into the existing .grad in place
            outs = net.forward(xd)
            loss = sum(cbce(o, gt, size_average=False) for o in outs)
            loss.backward()
        return {k: (None if v.grad is None else v.grad.clone()) for k, v in named.items()}

    full = run([])
    part = run(["stages.2.3.weight", "stages.0.0.bias", "side_prep.1.weight", "stages.4.5.bias"])
    for k in ("stages.2.3.weight", "stages.0.0.bias", "side_prep.1.weight", "stages.4.5.bias"):
        assert part[k] is None, k
    for k in ("stages.2.3.bias", "stages.0.0.weight", "side_prep.1.bias", "stages.4.5.weight", "stages.1.1.weight", "fuse.weight"):
        assert part[k] is not None and torch.equal(part[k], full[k]), k


def test_bf16_mode_conv1_1_weight_gradient_on_the_bf16_pipe_matches_the_fp32_kernel():
    """bf16-store mode: conv1_1's weight gradient runs on the bf16 matrix pipe (pixel-major dY tile + im2col tile gathered with
    ds_read_b64_tr_b16); the exact fp32 skinny kernel fed with the same bf16 dY is the checker.  The only arithmetic difference is the
    bf16 rounding of the 3-channel input (which the mode's forward conv1_1 applies as well): weight gradient within 3e-3 rel-L2, bias
    gradient (fp32 column sums of the bf16 dY in both) within 1e-5; odd sizes and a batch."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    from oracle import synth
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for (n, h, w) in [(2, 37, 53), (1, 120, 214), (3, 16, 17)]:
        wts, x, m = synth.calibrated_problem(n, h, w, seed=13)
        xd, gt = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
        got = {}
        for on in (0, 1):
            prev = l.osvos_debug_set_c3_bf16(on)
            try:
                net = build_net(wts, "bf16")
                outs = net.forward(xd)
                sum(cbce(o, gt, size_average=False) for o in outs).backward()
                torch.cuda.synchronize()
                got[on] = (net.stages[0][0].weight.grad.double().cpu(), net.stages[0][0].bias.grad.double().cpu(), net.stages[0][2].weight.grad.double().cpu())
            finally:
                l.osvos_debug_set_c3_bf16(prev)
        dw = float((got[1][0] - got[0][0]).norm() / got[0][0].norm())
        db = float((got[1][1] - got[0][1]).norm() / got[0][1].norm())
        print("conv1_1 wgrad bf16-pipe vs fp32 kernel at %dx%dx%d: dW rel-L2 %.2e, db rel-L2 %.2e" % (n, h, w, dw, db))
        assert dw <= 3e-3 and db <= 1e-5, ((n, h, w), dw, db)
        assert torch.equal(got[1][2], got[0][2])          # everything else in the network is untouched


@pytest.mark.parametrize("precision", ["bf16", "fp32x3"])
def test_one_bit_relu_masks_change_nothing_but_the_bytes_read(tmp_path, precision):
    """bf16-store mode and f32x3 (stages 1-3 there): the forward also writes the sign bits of every activation that later masks a data gradient, and the data gradients
    read one 32-bit word per (pixel, 32 channels) instead of the activation (csrc/maskbits.h).  Same predicate (stored bf16 value > 0), so
    (stored fp32 value > 0 in f32x3), so
    logits, losses, every parameter gradient and the input gradient must equal the OSVOS_MASK_BITS=0 run BIT FOR BIT -- odd sizes (partial
    tiles on both axes), a batch, and the 107-pixel-wide shape whose conv4_x take the LDS-DMA kernel's epilogue."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent('''
        import sys, numpy as np, torch
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import test_gpu_net as T
        from oracle import synth
        from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
        res = {}
        for tag, (n, h, w) in {"a": (2, 37, 53), "b": (1, 120, 214), "c": (2, 240, 427)}.items():
            wts, x, m = synth.calibrated_problem(n, h, w, seed=5)
            net = T.build_net(wts, sys.argv[2])
            xg = torch.from_numpy(x).requires_grad_()
            outs = net.forward(xg.cuda())
            gt = torch.from_numpy(m).cuda()
            losses = [cbce(o, gt, size_average=False) for o in outs]
            (0.5 * sum(losses[:-1]) + losses[-1]).backward()
            for i, o in enumerate(outs):
                res["%%s:out%%d" %% (tag, i)] = o.detach().cpu().numpy()
            for k, v in net.named_parameters():
                if v.grad is not None:
                    res["%%s:g:%%s" %% (tag, k)] = v.grad.cpu().numpy()
            res[tag + ":dx"] = xg.grad.numpy()
        np.savez(sys.argv[1], **res)
    ''') % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = {}
    variants = {"0": dict(OSVOS_MASK_BITS="0"), "1": dict(OSVOS_MASK_BITS="1")}
    if precision == "bf16":      # the same for the forward pool fused into the bf16 convolutions' epilogue (max of the same stored bf16 values)
        variants["nopool"] = dict(OSVOS_MASK_BITS="1", OSVOS_FUSE_POOL="0")
    for tag, env in variants.items():
        out = str(tmp_path / ("m%s.npz" % tag))
        # (OSVOS_X3_KSPLIT=1: a layer that writes bits is never cut along K; the comparison run must sum in the same order)
        subprocess.run([sys.executable, "-c", code, out, precision], check=True, env=dict(os.environ, OSVOS_X3_KSPLIT="1", OSVOS_X3_STREAMK="0", **env), timeout=900)
        got[tag] = dict(np.load(out))
    for other in [t for t in variants if t != "1"]:
        a, b = got[other], got["1"]
        assert a.keys() == b.keys() and len(a) > 120
        for k in a:
            assert np.isfinite(b[k]).all(), k
            assert np.array_equal(a[k], b[k]), (other, k, float(np.abs(a[k] - b[k]).max()))


def test_pooling_fused_into_the_convolutions_is_bit_identical_to_its_own_launches(tmp_path):
    """f32x3 with the default OSVOS_FUSE_POOL=1: the four max-pools run in the epilogue of each stage's last convolution (csrc/epi.h).  Same
    values, same order of operations: logits, losses and every gradient must equal the OSVOS_FUSE_POOL=0 run (own pooling launches) BIT FOR
    BIT -- at odd sizes (ceil-mode partial windows on both axes) and batch 2.  Both runs pin the K decomposition of every launch
    (OSVOS_X3_KSPLIT=1, OSVOS_X3_STREAMK=0): a fused launch is never cut into partial-sum launches, so with the automatic choice the two
    runs would sum the deep layers in different orders, and on this un-trained net that alone moves whole gradient tensors by ~1e-2."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent('''
        import sys, numpy as np, torch
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import test_gpu_net as T
        from oracle import synth
        from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
        res = {}
        for tag, (n, h, w) in {"a": (2, 37, 53), "b": (1, 120, 214), "c": (1, 61, 107)}.items():
            wts, x, m = synth.calibrated_problem(n, h, w, seed=9)
            net = T.build_net(wts, "fp32x3")
            xg = torch.from_numpy(x).requires_grad_()
            outs = net.forward(xg.cuda())
            gt = torch.from_numpy(m).cuda()
            losses = [cbce(o, gt, size_average=False) for o in outs]
            (0.5 * sum(losses[:-1]) + losses[-1]).backward()
            for i, o in enumerate(outs):
                res["%%s:out%%d" %% (tag, i)] = o.detach().cpu().numpy()
            for k, v in net.named_parameters():
                if v.grad is not None:
                    res["%%s:g:%%s" %% (tag, k)] = v.grad.cpu().numpy()
            res[tag + ":dx"] = xg.grad.numpy()
        np.savez(sys.argv[1], **res)
    ''') % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = {}
    for fuse in ("0", "1"):
        out = str(tmp_path / ("f%s.npz" % fuse))
        env = dict(os.environ, OSVOS_FUSE_POOL=fuse, OSVOS_X3_KSPLIT="1", OSVOS_X3_STREAMK="0")
        subprocess.run([sys.executable, "-c", code, out], check=True, env=env, timeout=900)
        got[fuse] = dict(np.load(out))
    a, b = got["0"], got["1"]
    assert a.keys() == b.keys() and len(a) > 120
    for k in a:      # the fused epilogues see exactly the values the pooling launches would read
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))


def test_deferred_backward_join_changes_nothing_but_the_schedule(tmp_path):
    """OSVOS_DEFER_JOIN=1 (opt-in): backwards return before their weight-gradient tail has finished on the side streams and the next forward
    runs under it; TrainLoop joins before every optimizer step.  Same kernels, same accumulation order: the weights after two optimizer
    steps (2 x nAveGrad micro-batches of the parent loop, all five heads) must be BIT-IDENTICAL to the default schedule.  A race on the
    workspace (freed while the side streams still read it) or a missing join would show up here."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent('''
        import sys, numpy as np, torch
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import test_gpu_net as T
        from oracle import synth
        from osvos_pytorch_amd.train_common import TrainLoop, make_sgd
        n_ave = 3
        frames = [synth.calibrated_problem(1, 96, 160, seed=5 + k) for k in range(2)]
        net = T.build_net(frames[0][0], "fp32x3")
        loop = TrainLoop(net, make_sgd(net, "parent", lr=1e-9), mode="parent", n_ave_grad=n_ave)
        for it in range(4 * n_ave):
            _, x, m = frames[it %% 2]
            junk = torch.empty(1 << 26, device="cuda")       # allocator churn between micro-batches: a workspace released too early gets reused
            junk.fill_(float(it))
            del junk
            loop.micro_batch(torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(m).cuda(), epoch=it)
        loop.finish()
        torch.cuda.synchronize()
        assert loop.steps == 4
        np.savez(sys.argv[1], **{k: v.cpu().numpy() for k, v in net.state_dict().items()})
    ''') % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = {}
    for flag in ("0", "1"):
        out = str(tmp_path / ("d%s.npz" % flag))
        subprocess.run([sys.executable, "-c", code, out], check=True, env=dict(os.environ, OSVOS_DEFER_JOIN=flag), timeout=900)
        got[flag] = dict(np.load(out))
    changed = 0
    for k in got["0"]:
        assert np.array_equal(got["0"][k], got["1"][k]), k
    assert len(got["0"]) == 52


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_retain_graph_second_backward_and_autograds_own_error_without_it(precision):
    """vgg_osvos.py:59-74 is plain autograd in the reference: `loss.backward(retain_graph=True)` followed by another backward on the same
    graph works, a second backward WITHOUT it raises autograd's "backward through the graph a second time".  Here the activation workspace
    rides in the Function's saved-tensor slot: kept under retain_graph, released after a plain backward.  The backward writes no buffer of
    the forward, so the second pass must return the first one's gradients BIT FOR BIT (all five heads, every parameter, the input)."""
    from oracle import synth
    from osvos_pytorch_amd.layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    wts, x, m = synth.calibrated_problem(1, 64, 96, seed=21)
    net = build_net(wts, precision)
    xin = torch.from_numpy(x).cuda().requires_grad_()
    gt = torch.from_numpy(m).cuda()

    def grads():
        g = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        g["input"] = xin.grad.detach().clone()
        net.zero_grad(set_to_none=True)
        xin.grad = None
        return g

    outs = net.forward(xin)
    loss = sum(cbce(o, gt, size_average=False) for o in outs)
    loss.backward(retain_graph=True)
    first = grads()
    loss.backward()
    second = grads()
    assert set(first) == set(second) and len(first) > 40
    for k in first:
        assert torch.equal(first[k], second[k]), k
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        loss.backward()


@pytest.mark.gpu
def test_pool_code_bytes_change_nothing_but_the_bytes_read_bf16(tmp_path):
    """Round 5, bf16-store mode: the forward's pooling (fused epilogue of the stage's last convolution, or its own launch) writes one code
    byte per pooled element and maxpool_bwd reads it instead of the pool's input (OSVOS_POOL_CODE=1, default).  Logits, losses and EVERY
    gradient must equal the run that recomputes the argmax from the input (OSVOS_POOL_CODE=0) BIT FOR BIT, with the pools fused and not
    (OSVOS_FUSE_POOL=0/1: the epilogue's bytes against the pooling kernel's), at odd sizes with clipped windows on both axes and at batch 12.
    (The LDS-DMA convolution of the deep stages, whose pooling then runs as its own launch, only engages at the BASELINE size: the
    854x480 batch-12 parity test of tests/test_gpu_baseline_configs.py runs through it.)"""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent('''
        import sys, numpy as np, torch
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import test_gpu_net as T
        from oracle import synth
        from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
        res = {}
        for tag, (n, h, w) in {"a": (2, 37, 53), "b": (2, 120, 214), "c": (12, 61, 107)}.items():
            wts, x, m = synth.calibrated_problem(n, h, w, seed=9)
            net = T.build_net(wts, "bf16")
            xg = torch.from_numpy(x).requires_grad_()
            outs = net.forward(xg.cuda())
            gt = torch.from_numpy(m).cuda()
            losses = [cbce(o, gt, size_average=False) for o in outs]
            (0.5 * sum(losses[:-1]) + losses[-1]).backward()
            for i, o in enumerate(outs):
                res["%%s:out%%d" %% (tag, i)] = o.detach().cpu().numpy()
            for k, v in net.named_parameters():
                if v.grad is not None:
                    res["%%s:g:%%s" %% (tag, k)] = v.grad.cpu().numpy()
            res[tag + ":dx"] = xg.grad.numpy()
        np.savez(sys.argv[1], **res)
    ''') % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = {}
    for fuse, pc in (("1", "0"), ("1", "1"), ("0", "1"), ("0", "0")):
        out = str(tmp_path / ("f%s%s.npz" % (fuse, pc)))
        env = dict(os.environ, OSVOS_FUSE_POOL=fuse, OSVOS_POOL_CODE=pc)
        subprocess.run([sys.executable, "-c", code, out], check=True, env=env, timeout=900)
        got[fuse + pc] = dict(np.load(out))
    base = got["10"]
    assert len(base) > 120
    for tag in ("11", "01", "00"):
        assert got[tag].keys() == base.keys()
        for k in base:
            assert np.array_equal(got[tag][k], base[k]), (tag, k, float(np.abs(got[tag][k] - base[k]).max()))


@pytest.mark.gpu
def test_weight_gradient_halves_on_two_streams_equal_the_whole_launch(tmp_path):
    """osvos_net_backward enqueues every weight gradient either whole (one side stream, OSVOS_THREE_STREAMS=0; everything on the caller's stream,
    OSVOS_TWO_STREAMS=0) or as two halves of one WgradCall: partial slabs on the weight-gradient stream, their reduce on the third stream (the
    default).  Same kernels, same slabs, same order of summation: every parameter gradient and the input gradient must be BYTE-EQUAL across the
    three settings, for every weight-gradient family and piece count (exact fp32; f32x3 with 3, 2 and FP16-pair pieces, side_prep on its S16 form;
    the bf16-store mode, side_prep on the Cout = 16 route of the bf16 kernel).  All five heads; the streams are read when the runtime is
    built: one subprocess per setting."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent('''
        import sys, numpy as np, torch
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import test_gpu_net as T
        from oracle import synth
        from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
        res = {}
        wts, x, m = synth.calibrated_problem(1, 64, 96, seed=21)
        for prec in ("fp32", "fp32x3", "fp32x3b2", "fp32h2", "bf16"):
            net = T.build_net(wts, prec)
            xg = torch.from_numpy(x).cuda().requires_grad_()
            gt = torch.from_numpy(m).cuda()
            sum(cbce(o, gt, size_average=False) for o in net.forward(xg)).backward()
            torch.cuda.synchronize()
            for k, v in net.named_parameters():
                if v.grad is not None:
                    res["%%s:%%s" %% (prec, k)] = v.grad.cpu().numpy()
            res[prec + ":input"] = xg.grad.cpu().numpy()
        np.savez(sys.argv[1], **res)
    ''') % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = {}
    for tag, env in (("three", {}), ("two", {"OSVOS_THREE_STREAMS": "0"}), ("one", {"OSVOS_TWO_STREAMS": "0"})):
        out = str(tmp_path / (tag + ".npz"))
        subprocess.run([sys.executable, "-c", code, out], check=True, env=dict(os.environ, **env), timeout=900)
        got[tag] = dict(np.load(out))
    base = got["three"]
    for prec in ("fp32", "fp32x3", "fp32x3b2", "fp32h2", "bf16"):
        assert sum(k.startswith(prec + ":") for k in base) > 40, prec
    for tag in ("two", "one"):
        assert got[tag].keys() == base.keys()
        for k in base:
            assert np.isfinite(base[k]).all(), k
            assert got[tag][k].tobytes() == base[k].tobytes(), (tag, k, float(np.abs(got[tag][k] - base[k]).max()))


@pytest.mark.gpu
def test_op_level_x3_pieces_and_network_calls_do_not_see_each_other():
    """ops.set_x3_pieces is the arithmetic of the OP-LEVEL f32x3 entries on this thread; a network call takes its pieces from its precision.
    Neither leaks into the other: an 'fp32x3' forward + backward after set_x3_pieces(2) equals the one without it byte for byte, and an
    op-level conv3x3_x3 (default three pieces) gives the same bytes before and after an 'fp32x2' network step."""
    from oracle import synth
    from osvos_pytorch_amd import ops
    from osvos_pytorch_amd.layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    wts, x, m = synth.calibrated_problem(1, 64, 96, seed=21)
    gt = torch.from_numpy(m).cuda()

    def step(precision):
        net = build_net(wts, precision)
        xin = torch.from_numpy(x).cuda().requires_grad_()
        outs = net.forward(xin)
        sum(cbce(o, gt, size_average=False) for o in outs).backward()
        res = {"out%d" % i: o.detach().clone() for i, o in enumerate(outs)}
        res.update({k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
        res["input"] = xin.grad.detach().clone()
        return res

    g = torch.Generator().manual_seed(7)
    xo = torch.randn(1, 16, 24, 64, generator=g).cuda()
    wo = (torch.randn(64, 64, 3, 3, generator=g) / 24).cuda()
    bo = torch.randn(64, generator=g).cuda()
    op = lambda: ops.conv3x3_x3(xo, ops.pack_x3(wo), bo, 64, relu=True)
    try:
        plain = step("fp32x3")
        ops.set_x3_pieces(2)
        y2 = op()
        under2 = step("fp32x3")
        assert torch.equal(op(), y2)                         # ... and the op-level setting survives the network call
        ops.set_x3_pieces(3)
        before = op()
        assert not torch.equal(before, y2)                   # (the setting does reach the op-level entry)
        step("fp32x2")
        after = op()
    finally:
        ops.set_x3_pieces(3)
    assert set(plain) == set(under2) and len(plain) > 45
    for k in plain:
        assert torch.isfinite(plain[k]).all(), k
        assert plain[k].cpu().numpy().tobytes() == under2[k].cpu().numpy().tobytes(), k
    assert before.cpu().numpy().tobytes() == after.cpu().numpy().tobytes()
