"""GPU: both heads of the network -- the commuted fast head (csrc/head.hip: head_lowres, head_upsample, head_bwd4 + osvos_head_grads_finalize)
and the generic transposed-convolution head (csrc/head_generic.hip) -- as the NETWORK launches them, against float64 on the device's own
side_prep maps (tests/head_cases.py).

Reference being matched: vgg_osvos.py:68-72 (score_dsn, upscale / upscale_, center_crop, cat, fuse), restated in oracle/torch_ref.py forward()
and cut out of it by head_cases.head_reference.  The head is exactly linear, so with the four side_prep maps read back from the workspace
(osvos_net_ws_query 17..20) every output and every gradient is a closed-form float64 number: no ReLU / arg-max flip noise, bars of 3e-6
(outputs) and 1e-5 (gradients) instead of the 1e-3 of the net-level tests.  d/dprep has no query index; it is pinned through what consumes it:
side_prep[i].bias.grad (its per-channel pixel sum) and side_prep[i].weight.grad (a 3x3 weight gradient on the device's own stage output).

Measured on an MI355X (worst over shapes, weight kinds and upstream sets; rel = max |error| / max |reference|): see the docstrings of the tests."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import head_cases as hc
from match_cases import bf16_round
from test_gpu_net import build_net
from test_gpu_ops import rel_err

pytestmark = pytest.mark.gpu

OUT_BAR = 3e-6          # outputs: the op-level head test's bar (test_head_lowres_upsample_and_backward_at_the_baseline_crop_sets)
GRAD_BAR = 1e-5         # head parameter gradients; scalar biases: <= 1e-5 |ref| + 1e-3 (the op-level test's form)
BWD_SHAPES = [(2, 37, 53), (1, 2, 3), (3, 33, 41)]


# ------------------------------------------------------------------------------------------------------------------------------ harness

@functools.lru_cache(maxsize=None)
def _base_problem(shape):
    """(weights with diagonal deconvs, frame) -- heads calibrated on the frame where it is large enough (tiny frames: raw He-init heads, as
    test_batch_and_odd_sizes_no_grad_inference); WRAP: calibrated on (1,48,64) and reused (no CPU trunk forward at 4 x 515 x 511)"""
    from oracle import synth
    n, h, w = shape
    if shape == hc.WRAP:
        return _base_problem((1, 48, 64))[0], synth.make_frame(n, h, w, 41)
    if h * w >= 64:
        wts, x, _ = synth.calibrated_problem(n, h, w, seed=31)
        return wts, x
    return synth.make_weights(1), synth.make_frame(n, h, w, 9)


def _query(net, ws, n, h, w, which):
    """workspace tensor `which` as CPU float64 NCHW (+ its storage format: 0 fp32, 1 bf16; the side_prep maps 17..20 are fp32 in every precision)"""
    from osvos_pytorch_amd import _lib
    lib = _lib.lib()
    dt = net._runtime.dtype
    off, el, ch, hh, ww = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.osvos_net_ws_query(n, h, w, dt, which, C.byref(off), C.byref(el), C.byref(ch), C.byref(hh), C.byref(ww)), "net_ws_query")
    fmt = int(lib.osvos_net_ws_format(dt, which)) if which < 17 else 0
    tdt, size = (torch.bfloat16, 2) if fmt == 1 else (torch.float32, 4)
    t = ws[off.value:off.value + size * el.value].view(tdt).view(n, hh.value, ww.value, ch.value)
    return t.permute(0, 3, 1, 2).double().cpu().contiguous(), fmt, ch.value


def _read_forward(net, ws, shape):
    """the four side_prep maps and the four side-branch inputs of a forward, read before anything else touches the workspace"""
    from osvos_pytorch_amd.autograd import FEATURE_LAYERS
    n, h, w = shape
    preps, feats, fmts = [], [], []
    for i in range(4):
        p, _, ch = _query(net, ws, n, h, w, 17 + i)
        assert ch == 16 and tuple(p.shape) == (n, 16) + hc.side_sizes(h, w)[i]
        assert float(p.abs().max()) > 0 and bool(torch.isfinite(p).all()), ("side_prep map", i)
        preps.append(p)
        if shape == hc.WRAP:      # (half a gigabyte in float64, and no test looks at them)
            continue
        f, fmt, _ = _query(net, ws, n, h, w, FEATURE_LAYERS[i])
        feats.append(f)
        fmts.append(fmt)
    return preps, feats, fmts


class Run:
    pass


def _device_run(kind, shape, precision, douts_list, freeze=(), inplace=False):
    """one net, one forward + backward per entry of douts_list (None: forward only); returns a Run with the device's outputs, side_prep maps,
    side-branch inputs and the parameter gradients left in .grad after the last backward"""
    n, h, w = shape
    base, x = _base_problem(shape)
    wts = hc.apply_weight_kind(base, kind)
    net = build_net(wts, precision)
    if inplace:
        net.set_inplace_grad_accumulation(True)
    named = dict(net.named_parameters())
    for k in freeze:
        named[k].requires_grad_(False)
    r = Run()
    r.wts, r.passes = wts, []
    for douts in douts_list:
        xg = torch.from_numpy(x).cuda().requires_grad_()
        outs = net.forward(xg)
        ws = outs[0].grad_fn.saved_tensors[0]
        preps, feats, fmts = _read_forward(net, ws, shape)
        r.passes.append((preps, feats, fmts, [o.detach().cpu() for o in outs]))
        if douts is not None:
            used = [j for j in range(5) if douts[j] is not None]
            torch.autograd.backward([outs[j] for j in used], [douts[j].cuda() for j in used])
        del ws, outs
    torch.cuda.synchronize()
    r.generic = bool(net._runtime.generic_head)
    r.grads = {k: (None if v.grad is None else v.grad.detach().cpu()) for k, v in named.items()}
    r.preps, r.feats, r.fmts, r.outs = r.passes[-1]
    return r


def _reference(r, shape, douts, pass_idx=-1):
    n, h, w = shape
    preps = [p.clone().requires_grad_() for p in r.passes[pass_idx][0]]
    return hc.head_reference(preps, hc.head_params(r.wts), h, w, douts if douts is not None else [None] * 5)


_CASES = {}


def _case(kind, shape, precision, upstream):
    """device run + float64 reference of one (weight kind, shape, precision, upstream set), shared by the tests that look at different parts of it"""
    key = (kind, shape, precision, upstream)
    if key not in _CASES:
        n, h, w = shape
        douts = None if upstream is None else hc.upstream_gradients(upstream, n, h, w, 1000 + h)
        r = _device_run(kind, shape, precision, [douts])
        r.douts = douts
        r.ref_outs, r.ref_dpreps, r.ref_grads = _reference(r, shape, douts)
        _CASES[key] = r
    return _CASES[key]


def _check_outputs(outs, ref_outs, what):
    errs = []
    for i in range(5):
        got, ref = outs[i], ref_outs[i]
        e = rel_err(got, ref)[0]
        errs.append(e)
        assert e < OUT_BAR, (what, i, e)
        # first and last three rows / columns: where a wrong crop offset shows
        for sl in ((Ellipsis, slice(0, 3), slice(None)), (Ellipsis, slice(-3, None), slice(None)), (Ellipsis, slice(0, 3)), (Ellipsis, slice(-3, None))):
            eb = rel_err(got[sl], ref[sl])[0]
            assert eb < OUT_BAR, (what, i, "border", eb)
    return errs


def _check_head_gradients(r, what):
    """every head parameter gradient of run `r` against r.ref_grads at the tight bar; a parameter whose head got no upstream gradient: None
    where OSVOSNetFunction.backward does not want it (upscale_[i] without side i; score_dsn without any side; the deconv weights on the fast
    head), exactly zero where it wants it and no head reaches it (fuse.* without the fused head, score_dsn[i] without side i among other sides,
    upscale[i] without the fused head) -- anything else is the garbage of an unwritten torch.empty target"""
    d = r.douts
    have_fused, have_side = d[4] is not None, [d[i] is not None for i in range(4)]
    report = {}

    def close(name):
        got, ref = r.grads[name], r.ref_grads[name]
        assert got is not None and ref is not None and bool(torch.isfinite(got).all()), (what, name)
        if ref.numel() == 1:
            err = abs(float(got) - float(ref))
            assert err <= GRAD_BAR * abs(float(ref)) + 1e-3, (what, name, float(got), float(ref))
            report[name] = err / (abs(float(ref)) + 1e-30)
        else:
            report[name] = e = rel_err(got, ref)[0]
            assert e <= GRAD_BAR, (what, name, e)

    def zero(name):
        got = r.grads[name]
        assert r.ref_grads[name] is None
        assert got is not None and got.shape == r.ref_grads_shapes[name] and bool((got == 0).all()), (what, name, "not exactly zero")

    r.ref_grads_shapes = {k: torch.Size(np.shape(r.wts[k])) for k in hc.HEAD_PARAM_NAMES}
    for name in ("fuse.weight", "fuse.bias"):
        (close if have_fused else zero)(name)
    for i in range(4):
        for name in ("score_dsn.%d.weight" % i, "score_dsn.%d.bias" % i):
            if not any(have_side):
                assert r.grads[name] is None and r.ref_grads[name] is None, (what, name)
            else:
                (close if have_side[i] else zero)(name)
        up, up1 = "upscale.%d.weight" % i, "upscale_.%d.weight" % i
        if not r.generic:
            assert r.grads[up] is None and r.grads[up1] is None, (what, i)      # frozen by lr 0 in both reference scripts: never formed
            continue
        (close if have_fused else zero)(up)
        if have_side[i]:
            close(up1)
        else:
            assert r.grads[up1] is None and r.ref_grads[up1] is None, (what, up1)
    return report


def _conv_weight_grad(x, dy):
    """weight gradient of Conv2d(k=3, p=1): x [N,C,h,w], dy [N,16,h,w] -> [16,C,3,3], in the operands' dtype"""
    return torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dy, padding=1)


def _other_bf16_neighbour(v, rounded):
    """the bfloat16 on the other side of `v` from bf16_round(v) (float64 arrays; finite values)"""
    u = rounded.astype(np.float32).view(np.uint32).astype(np.int64)
    away = np.where((v > rounded) == (rounded >= 0), u + 0x10000, u - 0x10000)      # one bf16 step towards v: up in magnitude if v lies beyond
    away = np.where((rounded == 0), np.where(v > 0, 0x00010000, 0x80010000), away)     # (from zero: the smallest bf16 of v's sign)
    return (away & 0xffffffff).astype(np.uint32).view(np.float32).astype(np.float64)


def _admit_bf16_ties(dp64, delta, x, got_w, got_b, ref_w, ref_b):
    """The device rounds ITS fp32 dprep to bf16; the reference rounds the float64 value.  An element that lies within `delta` (the fp32
    evaluation error of dprep) of the midpoint of two bfloat16 may legitimately land on either: measured on an MI355X, fast head, (2,37,53),
    scale 0: ONE element at 0.5000153 of a bf16 step, side_prep.0.bias[2] off by exactly that step (2^-12 = 3.5e-5 of the maximum), every
    other channel exact.  For such elements, and no others, both roundings are admitted: the other one is taken, best element first, as long
    as it brings the reference closer to the device's bias AND weight gradient of that channel (sum of squares, both scaled by their maxima),
    and the references are corrected by it.  Every other element stays pinned to round-to-nearest-even, and the bars do not move."""
    n, c16, h, w = dp64.shape
    rne = bf16_round(dp64.astype(np.float32)).astype(np.float64)
    alt = _other_bf16_neighbour(dp64, rne)
    amb = np.abs(dp64 - 0.5 * (rne + alt)) <= delta
    xp = None if x is None else np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    ref_w, ref_b = (None if ref_w is None else ref_w.copy()), ref_b.copy()
    sw, sb = (1.0 if ref_w is None else np.abs(ref_w).max() + 1e-30), np.abs(ref_b).max() + 1e-30
    flipped = 0
    for c in range(c16):
        idx = np.argwhere(amb[:, c])
        if len(idx) == 0:
            continue
        def score():
            return ((got_b[c] - ref_b[c]) / sb) ** 2 + (0.0 if ref_w is None else float((((got_w[c] - ref_w[c]) / sw) ** 2).sum()))
        def move(j, sign):
            b, y, xx = idx[j]
            step = sign * (alt[b, c, y, xx] - rne[b, c, y, xx])
            ref_b[c] += step
            if ref_w is not None:
                ref_w[c] += step * xp[b, :, y:y + 3, xx:xx + 3]
        left = list(range(len(idx)))
        while left:          # steepest descent: the one element whose other rounding explains the device's two gradients best, until none does
            now, gains = score(), []
            for j in left:
                move(j, 1.0)
                gains.append(now - score())
                move(j, -1.0)
            j = int(np.argmax(gains))
            if gains[j] <= 0:
                break
            move(left.pop(j), 1.0)
            flipped += 1
    return ref_w, ref_b, int(amb.sum()), flipped


def _check_side_prep_gradients(r, what, precision, weights=True):
    """d/dprep_i through its two consumers.  Bar per tensor: 4 x the error torch's own float32 CPU evaluation of the same quantity from the same
    operands has against float64, floor 1e-5; in fp32 / fp32x3 also < 1e-4 flat (anything looser adds nothing over the net-level tests'
    6e-4 floor).  bf16 store precision: the convolutions read the bf16 copy of dprep and bf16 activations -- the reference rounds its float64
    dprep to bf16 first (ties within the fp32 evaluation error of dprep: _admit_bf16_ties), the activations come out of the workspace as bf16
    already.
    Measured on an MI355X, worst over the cases (device | torch float32): fp32 weight 8.4e-7 | 1.2e-6, bias 1.3e-6 | 1.0e-6; fp32x3 weight
    8.3e-7 | 1.2e-6, bias 1.4e-6 | 1.0e-6; bf16 store weight 2.6e-7 | 3.1e-7, bias 3.9e-8 | 3.9e-8 (3.5e-5 before the tie was admitted);
    WRAP, fp32, bias 1.6e-6 | 3.2e-7.  Every bar is therefore the 1e-5 floor."""
    report = {}
    h, w = r.outs[0].shape[2:]
    if precision == "bf16":
        _, dp32, _ = hc.head_reference([p.float().requires_grad_() for p in r.preps], hc.head_params(r.wts, torch.float32), h, w, r.douts)
    for i in range(4):
        dp = r.ref_dpreps[i]
        assert all(f == (1 if precision == "bf16" else 0) for f in r.fmts)
        if precision == "bf16":
            dp64 = dp.numpy()
            dp = torch.from_numpy(bf16_round(dp.float().numpy())).double()
        cases = [("side_prep.%d.bias" % i, dp.sum((0, 2, 3)), dp.float().sum((0, 2, 3)))]
        if weights:
            cases.append(("side_prep.%d.weight" % i, _conv_weight_grad(r.feats[i], dp), _conv_weight_grad(r.feats[i].float(), dp.float())))
        cases = [(name, ref, rel_err(ref32, ref)[0]) for name, ref, ref32 in cases]      # torch float32 against float64: on the same operands
        if precision == "bf16":
            delta = 4.0 * float((dp32[i].double() - r.ref_dpreps[i]).abs().max())
            rw, rb, n_amb, n_flip = _admit_bf16_ties(dp64, delta, r.feats[i].numpy(), r.grads["side_prep.%d.weight" % i].double().numpy(),
                                                     r.grads["side_prep.%d.bias" % i].double().numpy(), cases[1][1].numpy(), cases[0][1].numpy())
            report["ties.%d" % i] = (float(n_amb), float(n_flip))
            cases = [(cases[0][0], torch.from_numpy(rb), cases[0][2]), (cases[1][0], torch.from_numpy(rw), cases[1][2])]
        for name, ref, e32 in cases:
            got = r.grads[name]
            assert got is not None and got.shape == ref.shape
            e = rel_err(got, ref)[0]
            bar = max(4.0 * e32, 1e-5)
            report[name] = (e, e32)
            assert e <= bar, (what, name, e, e32)
            if precision != "bf16":
                assert e < 1e-4, (what, name, e)
    return report


# -------------------------------------------------------------------------------------------------------------------------------- forward

FWD_CASES = [(kind, prec, shape) for kind in hc.WEIGHT_KINDS for prec in ("fp32", "fp32x3", "bf16") for shape in hc.SMALL] + \
            [(kind, "fp32", hc.WRAP) for kind in ("diagonal", "dense")]


@pytest.mark.parametrize("kind,precision,shape", FWD_CASES, ids=lambda v: "x".join(str(a) for a in v) if isinstance(v, tuple) else None)
def test_forward_of_both_heads_on_the_devices_own_side_prep_maps(kind, precision, shape):
    """All five outputs against float64 on the side_prep maps of the same forward, whole map and borders, <= 3e-6 of the reference's maximum.
    The weight kind decides the head: interp_surgery's deconvs take the fast one, dense and per-channel-diagonal ones the generic one.
    At WRAP head_upsample_generic_kernel's grid-stride loop takes its second trip (head_cases.wrap_facts).
    Measured on an MI355X, worst output per weight kind (fp32 | fp32x3 | bf16 | WRAP fp32): diagonal 7.8e-7 | 5.3e-7 | 5.5e-7 | 2.2e-7,
    dense 8.2e-7 | 4.9e-7 | 4.9e-7 | 3.9e-7, per-channel 7.7e-7 | 7.6e-7 | 8.6e-7 | -."""
    upstream = "all" if (kind, precision, shape, "all") in DPREP_CASES else None      # (a case the backward tests need anyway: run it once)
    r = _case(kind, shape, precision, upstream)
    assert r.generic == hc.GENERIC[kind], (kind, r.generic)
    errs = _check_outputs(r.outs, r.ref_outs, (kind, precision, shape))
    print("head outputs vs float64", kind, precision, shape, ["%.1e" % e for e in errs])


@pytest.mark.parametrize("kind", hc.WEIGHT_KINDS)
def test_inference_forward_of_both_heads(kind):
    """torch.no_grad() on a module without trainable parameters runs the inference layout (OSVOS_FLAG_INFERENCE, workspace of fwd_total bytes).
    forward_features hands out a view of that workspace; its storage IS the workspace, and the side_prep maps sit below fwd_total at the
    offsets osvos_net_ws_query reports -- so the inference outputs are compared with float64 on the inference forward's own maps."""
    from osvos_pytorch_amd import _lib
    shape = n, h, w = (2, 37, 53)
    base, x = _base_problem(shape)
    wts = hc.apply_weight_kind(base, kind)
    net = build_net(wts, "fp32")
    for p in net.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        outs, feat, fmt = net.forward_features(torch.from_numpy(x).cuda(), 3)
    assert net._runtime.generic_head == hc.GENERIC[kind]
    ws = torch.empty(0, dtype=torch.uint8, device=feat.device).set_(feat.untyped_storage())
    assert ws.numel() == _lib.lib().osvos_net_ws_bytes_infer(n, h, w, net._runtime.dtype) < _lib.lib().osvos_net_ws_bytes(n, h, w, net._runtime.dtype)
    preps, _, _ = _read_forward(net, ws, shape)
    ref_outs, _, _ = hc.head_reference([p.requires_grad_() for p in preps], hc.head_params(wts), h, w, [None] * 5)
    _check_outputs([o.cpu() for o in outs], ref_outs, (kind, "inference"))
    with torch.no_grad():
        again = net.forward(torch.from_numpy(x).cuda())
    assert all(torch.equal(a, b) for a, b in zip(again, outs))


# ------------------------------------------------------------------------------------------------------------------------------- backward

BWD_CASES = [(kind, prec, shape, up) for kind in hc.WEIGHT_KINDS for prec in ("fp32", "fp32x3") for shape in BWD_SHAPES for up in hc.UPSTREAM] + \
            [(kind, "fp32", hc.WRAP, "all") for kind in ("diagonal", "dense")]


@pytest.mark.parametrize("kind,precision,shape,upstream", BWD_CASES, ids=lambda v: "x".join(str(a) for a in v) if isinstance(v, tuple) else None)
def test_backward_of_both_heads_parameter_gradients(kind, precision, shape, upstream):
    """What the NETWORK launches -- head_bwd4 (four scales in one launch) + osvos_head_grads_finalize, or head_bwd_generic + head_tapsum +
    the generic parameter-gradient kernels -- against float64 on the device's own side_prep maps: fuse.*, score_dsn.*, and on the generic head
    upscale.* / upscale_.*, <= 1e-5 of the reference's maximum (scalar biases <= 1e-5 |ref| + 1e-3).  Heads without an upstream gradient:
    None or exactly zero, as OSVOSNetFunction.backward prescribes (see _check_head_gradients).  At WRAP every scale of head_bwd_body /
    head_bwd_generic_kernel and of head_tapsum_kernel takes a second trip through its grid-stride loop.
    Measured on an MI355X, worst over the small shapes, both precisions | at WRAP: fuse.weight 2.1e-7 | 1.2e-7, fuse.bias 5.0e-8 | 3.1e-8,
    score_dsn.weight 1.8e-7 | 1.4e-7, score_dsn.bias 7.9e-7 | 5.0e-7, upscale.weight 8.3e-8 | 1.1e-7, upscale_.weight 8.1e-7 | 2.8e-7:
    nothing at WRAP comes near 1e-5, so no tensor needs a bar of its own there."""
    r = _case(kind, shape, precision, upstream)
    assert r.generic == hc.GENERIC[kind]
    if shape == hc.WRAP:
        facts = hc.wrap_facts(*shape)
        assert all(facts[("bwd", i)] and facts[("tapsum", i)] for i in range(4))
    rep = _check_head_gradients(r, (kind, precision, shape, upstream))
    fam = {}
    for k, e in rep.items():          # worst per tensor family
        f = ".".join(a for a in k.split(".") if not a.isdigit())
        fam[f] = max(fam.get(f, 0.0), e)
    print("head gradients vs float64", kind, precision, shape, upstream, [(f, "%.1e" % e) for f, e in sorted(fam.items())])


DPREP_CASES = BWD_CASES + [(kind, "bf16", (2, 37, 53), "all") for kind in ("diagonal", "dense")]


@pytest.mark.parametrize("kind,precision,shape,upstream", DPREP_CASES, ids=lambda v: "x".join(str(a) for a in v) if isinstance(v, tuple) else None)
def test_dprep_through_the_side_prep_gradients(kind, precision, shape, upstream):
    """side_prep[i].bias.grad = per-channel pixel sum of dprep_i; side_prep[i].weight.grad = 3x3 weight gradient of the device's own stage
    output (osvos_net_ws_query 3, 6, 9, 12) with dprep_i -- both against float64 from head_reference's dprep_i.  bf16 store precision, both
    heads: the convolutions read the bf16 copy dprep_b, which head.hip forms with a __bf16 conversion and head_generic.hip with f32_to_bf16;
    the reference rounds its dprep to bf16 and reads the activations as bf16.  WRAP: the bias only (the float64 weight gradient of a
    128-channel 258 x 256 x 4 map is too slow for this tier); it is the one check of dprep's VALUES on the pixels of the second trip."""
    r = _case(kind, shape, precision, upstream)
    rep = _check_side_prep_gradients(r, (kind, precision, shape, upstream), precision, weights=shape != hc.WRAP)
    print("side_prep gradients vs float64 (device | torch float32)", kind, precision, shape, upstream,
          [(k, "%.1e" % e, "%.1e" % e32) for k, (e, e32) in rep.items()])
    if shape == hc.WRAP:
        _CASES.pop((kind, shape, precision, upstream), None)      # the large case is done: free it


def test_generic_head_accumulates_in_place_and_honours_frozen_parameters():
    """Generic head, (2,37,53), fp32.  (a) in-place accumulation: two backwards on different upstream gradients leave the SUM of the two float64
    references in every head parameter's .grad (the second one adds inside the kernels).  (b) fuse.weight frozen, deconv weights trainable
    (grads[50] == NULL, grads[i] wanted): upscale.*.grad as before, fuse.weight.grad None.  (c) no fused head: upscale[i].weight.grad is
    exactly zero (the hipMemsetAsync branch of osvos_net_backward), upscale_[i] formed."""
    shape = n, h, w = (2, 37, 53)
    d1 = hc.upstream_gradients("all", n, h, w, 501)
    d2 = hc.upstream_gradients("all", n, h, w, 502)
    r = _device_run("dense", shape, "fp32", [d1, d2], inplace=True)
    assert r.generic
    _, _, g1 = _reference(r, shape, d1, 0)
    _, _, g2 = _reference(r, shape, d2, 1)
    r.douts, r.ref_grads = d1, {k: g1[k] + g2[k] for k in g1}
    _check_head_gradients(r, "two backwards accumulated in place")

    f = _device_run("dense", shape, "fp32", [d1], freeze=("fuse.weight",))
    f.douts = d1
    _, _, f.ref_grads = _reference(f, shape, d1)
    assert f.grads["fuse.weight"] is None
    f.grads["fuse.weight"] = f.ref_grads["fuse.weight"].float()      # (not formed: taken out of the comparison below)
    _check_head_gradients(f, "fuse.weight frozen")

    s = _case("dense", shape, "fp32", "sides_only")
    for i in range(4):
        g = s.grads["upscale.%d.weight" % i]
        assert g is not None and g.shape == (16, 16, 4 << i, 4 << i) and bool((g == 0).all()), i
        assert s.grads["upscale_.%d.weight" % i] is not None and float(s.grads["upscale_.%d.weight" % i].abs().max()) > 0


# --------------------------------------------------------------------------------------------------------- which head: osvos_deconv_diag_check

def _diag_check(w):
    """(max |off-diagonal tap|, max |w[c][c] - w[0][0]|) as the kernel reports them; the result buffer is pre-filled with NaN"""
    from osvos_pytorch_amd import _lib
    from osvos_pytorch_amd._glue import stream
    wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).cuda()
    out = torch.full((2,), float("nan"), device="cuda", dtype=torch.float32)
    _lib.check(_lib.lib().osvos_deconv_diag_check(C.c_void_p(wd.data_ptr()), int(w.shape[0]), int(w.shape[2]), C.c_void_p(out.data_ptr()), stream()),
               "deconv_diag_check")
    return tuple(float(v) for v in out.cpu())


@pytest.mark.parametrize("k", [4, 8, 16, 32])
def test_deconv_diag_check_reports_exact_maxima(k):
    """interp_surgery's weights: (0, 0).  One changed tap -- the first / last diagonal element of the tensor, the first / last off-diagonal
    one -- is reported with its exact float32 value in the right slot, the other slot stays 0.  k = 32: the last index is 262 143, the fourth
    trip of the 256-workgroup grid-stride loop."""
    base = hc.diagonal_deconv(k)
    assert _diag_check(base) == (0.0, 0.0)
    f = base[0, 0]
    v = np.float32(0.3)
    for idx in [(0, 1, 0, 0), (15, 14, k - 1, k - 1), (3, 9, k // 2, 1)]:          # off-diagonal
        w = base.copy()
        w[idx] = v
        assert _diag_check(w) == (float(v), 0.0), idx
        w[idx] = -v
        assert _diag_check(w) == (float(v), 0.0), idx
    for idx in [(0, 0, 0, 0), (15, 15, k - 1, k - 1), (7, 7, 1, k // 2)]:           # diagonal: a block that is not block [0][0] any more
        w = base.copy()
        w[idx] = v
        assert _diag_check(w) == (0.0, float(abs(np.float32(v - f[idx[2], idx[3]])))), idx
    assert (k * k * 256 - 1) // (256 * 256) == {4: 0, 8: 0, 16: 0, 32: 3}[k]      # trips before the last element's


def test_deconv_diag_check_on_special_values():
    """the smallest subnormal off the diagonal is not 'diagonal'; -0.0 off the diagonal is; inf is reported as inf; NaN -- off the diagonal, on a
    diagonal block other than [0][0], in block [0][0] itself -- must never pass as diagonal (fmaxf drops a NaN operand: the kernel maps NaN
    to +inf before its maximum).  The fast head would ignore such a tap and return finite logits where the reference returns NaN."""
    from osvos_pytorch_amd.autograd import NetRuntime
    k = 8
    base = hc.diagonal_deconv(k)
    tiny = np.float32(1e-45)
    assert tiny > 0
    w = base.copy()
    w[2, 11, 3, 3] = tiny
    assert _diag_check(w)[0] != 0.0
    w = base.copy()
    w[~np.eye(16, dtype=bool)] = -0.0
    assert _diag_check(w) == (0.0, 0.0)
    w = base.copy()
    w[2, 11, 3, 3] = -np.inf
    assert _diag_check(w) == (float("inf"), 0.0)
    w = base.copy()
    w[5, 5, 2, 2] = np.inf
    assert _diag_check(w) == (0.0, float("inf"))
    others = [torch.from_numpy(hc.diagonal_deconv(kk)).cuda() for kk in (4, 16, 32)]
    assert NetRuntime._deconv_is_diagonal([others[0], torch.from_numpy(base).cuda()] + others[1:])
    for idx, slot in [((2, 11, 3, 3), 0), ((5, 5, 2, 2), 1), ((0, 0, 2, 2), 1)]:
        w = base.copy()
        w[idx] = np.nan
        got = _diag_check(w)
        assert not (got[slot] == 0.0), (idx, got)
        assert not NetRuntime._deconv_is_diagonal([others[0], torch.from_numpy(w).cuda()] + others[1:]), idx


def test_a_nan_deconv_tap_takes_the_generic_head_and_reaches_the_fused_map():
    """upscale.2.weight[3,3,1,1] = NaN: the reference's fused map is NaN wherever that tap lands; so must ours be (generic head), and finite
    exactly where the reference is"""
    from oracle import torch_ref
    shape = n, h, w = (1, 48, 64)
    base, x = _base_problem(shape)
    wts = hc.apply_weight_kind(base, "diagonal")
    wts["upscale.2.weight"][3, 3, 1, 1] = np.nan
    net = build_net(wts, "fp32")
    with torch.no_grad():
        fused = net.forward(torch.from_numpy(x).cuda())[-1].cpu()
        ref = torch_ref.forward({k: torch.from_numpy(v) for k, v in wts.items()}, torch.from_numpy(x))[-1]
    assert net._runtime.generic_head
    assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref).all())
    assert torch.equal(torch.isnan(fused), torch.isnan(ref))


# ------------------------------------------------------------------------------------------------------------ head_lowres past its grid

def test_head_lowres_past_its_grid():
    """ops.head_lowres with N h w = 725 x 725 = 525 625 > 2048 x 256: head_lowres_f32_kernel's grid-stride loop takes a second trip (the 1080p
    case of test_gpu_ops.py stops 5 888 pixels short of it); against the float64 1x1 convolutions at that test's 2e-6"""
    from osvos_pytorch_amd import ops
    n, h, w = 1, 725, 725
    assert n * h * w > hc.LOWRES_CAP * hc.THREADS
    g = torch.Generator().manual_seed(725)
    prep = torch.randn(n, h, w, 16, generator=g)
    wd, bd, wf = torch.randn(16, generator=g), torch.randn(1, generator=g), torch.randn(16, generator=g)
    score, fpart = ops.head_lowres(prep.cuda(), wd.cuda(), bd.cuda(), wf.cuda())
    p64 = prep.double()
    ref_s = (p64 * wd.double()).sum(-1) + bd.double()
    ref_f = (p64 * wf.double()).sum(-1)
    assert rel_err(score.cpu(), ref_s)[0] < 2e-6
    assert rel_err(fpart.cpu(), ref_f)[0] < 2e-6
    # the pixels of the second trip on their own
    first = hc.LOWRES_CAP * hc.THREADS
    assert rel_err(score.cpu().flatten()[first:], ref_s.flatten()[first:])[0] < 2e-6 and rel_err(fpart.cpu().flatten()[first:], ref_f.flatten()[first:])[0] < 2e-6
