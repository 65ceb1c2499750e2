"""GPU: the inference forward (OSVOS_FLAG_INFERENCE of osvos_net_forward) against the training forward, at the library call and through
torch.no_grad().

include/osvos_hip.h promises that the flag changes what the call WRITES -- no one-bit ReLU masks, no pool-code bytes, nothing beyond
osvos_net_ws_bytes_infer -- and not one bit of the five logit maps.  The small frames below are where the promise can break: the f32x3
launcher cuts conv3_2 / conv4_1 / conv4_2 along K as soon as their launch carries no sign bits and still has a partial-sum workspace
(tests/test_conv_plan_cpu.py plans both forms on the CPU); the bf16 store mode takes its `pool_code == nullptr` and `y_bits == nullptr` arms
on the p64, DMA and plain tiles only here.  Every case runs each form of the call twice, on a workspace filled with 0x5A and with 0xA5: a byte
that differs from its fill in either run was written (a value cannot equal both fills), and logits that differ between the two runs were
computed from something the call did not write itself (stale partial sums, stream-K tickets, sign words).

The weights are oracle.synth's (heads calibrated on the frame; raw He-init heads below 64 pixels, as in test_gpu_net.py), the float64
reference is oracle/torch_ref.py, and the bars against it are test_gpu_net.py's own for the unflagged forward: LOGIT_TOL x std(logit) for
fp32 / fp32x3 / fp32h2, 0.1 x std (test_bf16_mfma_precision_mode) for bf16 / bf16w2.  'fp32x2' has no logit bar in that file (set_precision's
docstring: "NOT inside every flat fp32 bar"), so it is held to bit identity only."""
import ctypes as C
import functools

import pytest
import torch

import head_cases as hc
from test_conv_plan_cpu import STAGE_C, TRUNK, _has_bits
from test_gpu_net import LOGIT_TOL, build_net

pytestmark = pytest.mark.gpu

FRAMES = [(2, 48, 64), (1, 33, 41), (2, 37, 53), (1, 1, 1), (1, 2, 3), (2, 60, 107)]
PRECISIONS = ["fp32", "fp32x3", "fp32h2", "fp32x2", "bf16", "bf16w2"]
# every precision at every frame on the commuted head; 'fp32x3b2' (the forward of 'fp32x3') once; the generic head on both trunk formats
CASES = [(p, f, "diagonal") for f in FRAMES for p in PRECISIONS] + [("fp32x3b2", (2, 48, 64), "diagonal")] + \
        [(p, (2, 37, 53), "dense") for p in ("fp32x3", "bf16")]
F64_FRAMES = [(2, 48, 64), (1, 33, 41)]
F64_BARS = {"fp32": LOGIT_TOL, "fp32x3": LOGIT_TOL, "fp32h2": LOGIT_TOL, "bf16": 0.1, "bf16w2": 0.1}      # x std(logit); see the module docstring
_ids = lambda v: "x".join(str(a) for a in v) if isinstance(v, tuple) else None


# ------------------------------------------------------------------------------------------------------------------------------ harness

@functools.lru_cache(maxsize=None)
def _problem(frame):
    from oracle import synth
    n, h, w = frame
    if h * w >= 64:
        wts, x, _ = synth.calibrated_problem(n, h, w, seed=12)
        return wts, x
    return synth.make_weights(1), synth.make_frame(n, h, w, 9)


@functools.lru_cache(maxsize=2)
def _net(frame, kind):
    return build_net(hc.apply_weight_kind(_problem(frame)[0], kind))


@functools.lru_cache(maxsize=None)
def _truth(frame):
    """the five logit maps in float64 (oracle/torch_ref.py), computed once per frame"""
    from oracle import torch_ref
    wts, x = _problem(frame)
    with torch.no_grad():
        return [o.clone() for o in torch_ref.forward(torch_ref.as_leaf_params(wts, dtype=torch.float64, requires_grad=False), torch.from_numpy(x).double())]


def _ws_bytes(rt, frame):
    from osvos_pytorch_amd import _lib
    n, h, w = frame
    return int(_lib.lib().osvos_net_ws_bytes_infer(n, h, w, rt.dtype)), int(_lib.lib().osvos_net_ws_bytes(n, h, w, rt.dtype))


def _packed(net):
    params = [p.detach().contiguous() for p in net.parameters()]
    net._runtime.ensure_packed(params)
    return params


def _library_forward(net, x, ws, flagged):
    """osvos_net_forward as OSVOSNetFunction.forward calls it (the module's packs, dtype word and side stream), with or without the flag"""
    from osvos_pytorch_amd import _glue, _lib
    rt, (n, _, h, w) = net._runtime, x.shape
    outs = [torch.empty((n, 1, h, w), device=x.device, dtype=torch.float32) for _ in range(5)]
    _lib.check(_lib.lib().osvos_net_forward(C.c_void_p(x.data_ptr()), C.c_void_p(rt.wbuf.data_ptr()), C.c_void_p(ws.data_ptr()),
                                            _lib.ptr_array([o.data_ptr() for o in outs]), n, h, w,
                                            rt.cdtype_fwd() | (_lib.INFERENCE if flagged else 0), _glue.stream(), rt.auxf(x.device)), "net_forward")
    torch.cuda.synchronize()
    return outs


class Run:
    pass


@functools.lru_cache(maxsize=None)
def _run(precision, frame, kind):
    """both forms of the call on a 0x5A and on a 0xA5 workspace of osvos_net_ws_bytes bytes: logits and which bytes each form wrote"""
    net = _net(frame, kind).set_precision(precision)
    _packed(net)
    x = torch.from_numpy(_problem(frame)[1]).cuda()
    r = Run()
    r.generic = bool(net._runtime.generic_head)
    r.infer_bytes, r.total_bytes = _ws_bytes(net._runtime, frame)
    written = {}
    for flagged in (False, True):
        logits = []
        for fill in (0x5A, 0xA5):
            ws = torch.full((r.total_bytes,), fill, dtype=torch.uint8, device="cuda")
            logits.append(_library_forward(net, x, ws, flagged))
            written[flagged] = (ws != fill) if fill == 0x5A else written[flagged] | (ws != fill)
            del ws
        name = "flagged" if flagged else "plain"
        setattr(r, name, [o.cpu() for o in logits[0]])
        setattr(r, name + "_fill_independent", all(torch.equal(a, b) for a, b in zip(*logits)))
    r.n_plain, r.n_flagged = int(written[False].sum()), int(written[True].sum())
    r.flagged_beyond = int(written[True][r.infer_bytes:].sum())
    r.plain_beyond = int(written[False][r.infer_bytes:].sum())
    r.flagged_only = int((written[True] & ~written[False]).sum())
    return r


def _backward_only_bytes(precision, frame):
    """what only a backward reads, by the layout rule of net.cpp's ws_layout: N h w cout / 8 bytes of sign bits per trunk activation that later
    masks a data gradient and keeps its bits (test_conv_plan_cpu._has_bits restates use_mask_bits / act_is_a_mask), plus, in the bf16 store
    mode, one code byte per pooled element"""
    from osvos_pytorch_amd import _lib
    from osvos_pytorch_amd.autograd import PRECISIONS as TABLE
    n, h, w = frame
    dt = TABLE[precision][0]
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append((hs[-1] + 1) // 2)
        ws.append((ws[-1] + 1) // 2)
    total = sum(n * hs[si] * ws[si] * cout // 8 for l, (_, si, _, _, cout) in enumerate(TRUNK) if _has_bits(l, dt))
    if dt == _lib.F32_BF16MFMA:
        total += sum(n * hs[si] * ws[si] * STAGE_C[si - 1] for si in range(1, 5))
    return total


# ------------------------------------------------------------------------------------------------------------- C: the library call

@pytest.mark.parametrize("precision,frame,kind", CASES, ids=_ids)
def test_flagged_logits_are_the_unflagged_bits(precision, frame, kind):
    """The five logit maps of the flagged call are the unflagged call's, torch.equal.  A flagged forward that only drops the sign bits and
    keeps handing conv3_2 / conv4_1 / conv4_2 the partial-sum workspace fails this in fp32x3 at 2x48x64 (and at every other frame of the
    list that has a conv4 larger than one tile): those three launches are then cut along K in 4 / 4 / 8 and summed by a finalize launch."""
    r = _run(precision, frame, kind)
    assert r.generic == hc.GENERIC[kind]
    for i, (a, b) in enumerate(zip(r.flagged, r.plain)):
        assert bool(torch.isfinite(b).all()), (precision, frame, kind, i)
        assert torch.equal(a, b), (precision, frame, kind, i, float((a - b).abs().max()))


def test_fp32x3b2_runs_the_forward_of_fp32x3():
    a, b = _run("fp32x3b2", (2, 48, 64), "diagonal"), _run("fp32x3", (2, 48, 64), "diagonal")
    assert all(torch.equal(u, v) for u, v in zip(a.flagged, b.flagged)) and all(torch.equal(u, v) for u, v in zip(a.plain, b.plain))


@pytest.mark.parametrize("precision,frame,kind", CASES, ids=_ids)
def test_what_the_flagged_call_writes(precision, frame, kind):
    """(a) nothing at or beyond osvos_net_ws_bytes_infer; (b) no byte the unflagged call leaves alone; (c) at least the sign bits and pool
    codes fewer than the unflagged call; (d) neither form reads a byte of the workspace it did not write (same logits on both fills)."""
    r = _run(precision, frame, kind)
    assert 0 < r.infer_bytes < r.total_bytes
    assert r.flagged_beyond == 0, (precision, frame, kind)                                                   # (a)
    assert r.plain_beyond == 0, (precision, frame, kind)           # (the training forward writes nothing of the backward's either)
    assert r.flagged_only == 0, (precision, frame, kind)                                                     # (b)
    extra = _backward_only_bytes(precision, frame)
    assert (extra == 0) == (precision == "fp32")
    assert r.n_plain - r.n_flagged >= extra, (precision, frame, kind, r.n_plain, r.n_flagged, extra)         # (c)
    assert r.n_flagged > 0
    assert r.flagged_fill_independent and r.plain_fill_independent, (precision, frame, kind)                 # (d)


@pytest.mark.parametrize("frame", F64_FRAMES, ids=_ids)
@pytest.mark.parametrize("precision", sorted(F64_BARS))
def test_flagged_logits_against_float64(precision, frame):
    r = _run(precision, frame, "diagonal")
    for i, (got, truth) in enumerate(zip(r.flagged, _truth(frame))):
        err, std = float((got.double() - truth).abs().max()), float(truth.std(unbiased=False))
        print("flagged %s %s head %d: max |dlogit| %.3g = %.3g std" % (precision, frame, i, err, err / std))
        assert err <= F64_BARS[precision] * std, (precision, frame, i, err, std)


# ------------------------------------------------------------------------------------------------------------- D: torch.no_grad()

def _storage_bytes(view):
    return torch.empty(0, dtype=torch.uint8, device=view.device).set_(view.untyped_storage()).numel()


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_no_grad_on_a_trainable_module_takes_the_inference_forward(precision):
    """A module whose parameters require grad, under torch.no_grad() / torch.inference_mode(): the forward-only workspace, outputs that
    require no grad, and the bits of a forward that a backward follows.  (Without the grad-mode decision in OSVOS.forward the workspace
    behind forward_features' view has osvos_net_ws_bytes bytes: autograd reports needs_input_grad for such parameters under no_grad too.)"""
    frame = n, h, w = (2, 48, 64)
    wts, x = _problem(frame)
    net = build_net(wts, precision)
    assert all(p.requires_grad for p in net.parameters())
    xs = torch.from_numpy(x).cuda()
    infer_bytes, total_bytes = _ws_bytes(net._runtime, frame)
    with torch.no_grad():
        outs, feat, _ = net.forward_features(xs, 9)
        plain = net.forward(xs)
    assert _storage_bytes(feat) == infer_bytes < total_bytes
    assert all(not o.requires_grad and o.grad_fn is None for o in plain)
    with torch.inference_mode():
        outs_im, feat_im, _ = net.forward_features(xs, 9)
        plain_im = net.forward(xs)
    assert _storage_bytes(feat_im) == infer_bytes
    train = net.forward(xs.clone().requires_grad_())
    assert all(o.requires_grad for o in train)
    assert train[0].grad_fn.saved_tensors[0].numel() == total_bytes          # with grad enabled ctx keeps the full workspace
    torch.autograd.backward(train, [torch.ones_like(o) for o in train])
    assert all(p.grad is not None for k, p in net.named_parameters() if not k.startswith("upscale"))
    for i in range(5):
        for other in (outs, plain_im, outs_im, [o.detach() for o in train]):
            assert torch.equal(plain[i], other[i]), (precision, i)
    # forward_features mirrors forward with grad enabled too: the full workspace, the same bits
    outs_g, feat_g, _ = net.forward_features(xs, 9)
    assert _storage_bytes(feat_g) == total_bytes and all(torch.equal(a, b) for a, b in zip(outs_g, plain))


def test_training_step_is_the_unflagged_library_calls_bit_for_bit():
    """With grad enabled nothing changes: forward + backward through autograd give the logits and every gradient of osvos_net_forward
    (no flag) + osvos_net_backward called by hand on the same packs -- the extra forward argument shifts no gradient."""
    from osvos_pytorch_amd import _glue, _lib
    frame = n, h, w = (2, 37, 53)
    wts, x = _problem(frame)
    net = build_net(wts, "fp32x3")
    rt = net._runtime
    xg = torch.from_numpy(x).cuda().requires_grad_()
    outs = net.forward(xg)
    douts = [d.cuda() for d in hc.upstream_gradients("all", n, h, w, 3)]
    torch.autograd.backward(outs, douts)
    params = _packed(net)
    ws = torch.empty(_ws_bytes(rt, frame)[1], dtype=torch.uint8, device="cuda")
    outs_c = _library_forward(net, xg.detach(), ws, False)
    targets = [None if i < 8 else torch.empty_like(p) for i, p in enumerate(params)]      # (the commuted head forms no deconv gradients)
    dx = torch.empty_like(xg)
    assert not rt.generic_head
    _lib.check(_lib.lib().osvos_net_backward(C.c_void_p(rt.wbuf.data_ptr()), C.c_void_p(ws.data_ptr()), _lib.ptr_array([d.data_ptr() for d in douts]),
                                             _lib.ptr_array([None if t is None else t.data_ptr() for t in targets]), C.c_void_p(dx.data_ptr()),
                                             n, h, w, rt.cdtype_bwd(), 0, _glue.stream(), rt.aux(xg.device), rt.aux2(xg.device)), "net_backward")
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), b) for a, b in zip(outs, outs_c))
    assert torch.equal(xg.grad, dx) and float(dx.abs().max()) > 0
    for (k, p), t in zip(net.named_parameters(), targets):
        if t is None:
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, t) and bool(torch.isfinite(t).all()), k
