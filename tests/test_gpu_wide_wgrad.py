"""The wide 3x3 weight gradients at op level, where each workgroup walks MANY patches: wgrad_f32x3_kernel (csrc/wgrad_f32x3.hip) in its
three-piece, two-piece, FP16-pair "h2" and skinny S16 forms, wgrad_bf16_kernel<0> and wgrad_bf16pm_kernel<4 | 8> (csrc/wgrad_bf16.hip), and
the slab reduce they share.  The shapes (tests/wide_wgrad_cases.py, pinned on the CPU by test_wide_wgrad_cases_cpu.py through
osvos_wgrad_wide_plan) reach walks of 4-5 patches with the next patch prefetched from inside the k-loop, the dead prefetch behind the last
patch, short last splits, splits that cross from one image into the next, both f32x3 patch heights, both arms of the block map and more than
64 splits; before, only whole-network tests did, with one layer's gradient one tensor among thirty under a 1e-3 bar.  Integer operands make
every summation order exact, so a-d and f compare bit for bit: a dropped, repeated or shifted pixel, patch or split cannot pass.

The kinds (wide_wgrad_cases.KINDS): x3 / x3b2 / x3h2 = ops.conv3x3_wgrad(dtype=F32_X3) under ops.set_x3_pieces(3 / 2 / 22), *_s16 the same
at Cout 16; bf16_f32t = ops.conv3x3_wgrad(dtype=F32_BF16MFMA) on fp32 tensors; bf16_act / bf16_act16 = ops.conv3x3_wgrad_bf16act."""
import contextlib
import ctypes as C

import pytest
import torch

import wide_wgrad_cases as wc

pytestmark = pytest.mark.gpu


def _ops():
    from osvos_pytorch_amd import ops
    return ops


def _ids(pairs):
    return ["%s-%s" % ("x".join(map(str, s)), k) for s, k in pairs]


@contextlib.contextmanager
def _pieces(kind):
    """the x3 kinds' pieces per operand on this thread, restored to the default afterwards"""
    pieces = wc.KINDS[kind][2]
    if pieces is None:
        yield
        return
    ops = _ops()
    try:
        ops.set_x3_pieces(pieces)
        yield
    finally:
        ops.set_x3_pieces(3)


def _dtype(kind):
    from osvos_pytorch_amd._lib import F32_BF16MFMA, F32_X3
    return F32_X3 if wc.KINDS[kind][0] == "x3" else F32_BF16MFMA


def _device_operands(kind, x, dy, cout_s=None):
    """CPU NCHW operands -> (x dense NHWC, dy NHWC with channel stride cout_s) on the GPU, fp32 or bf16 as the kind reads them"""
    t = wc.KINDS[kind][3]
    return wc.x_nhwc(x, t).cuda(), wc.dy_nhwc(dy, cout_s, t).cuda()


def _wgrad(kind, xg, dyg, cin, cout, **kw):
    ops = _ops()
    with _pieces(kind):
        if wc.KINDS[kind][1] == "bf16act":
            return ops.conv3x3_wgrad_bf16act(xg, dyg, cin, cout, **kw)
        return ops.conv3x3_wgrad(xg, dyg, cin, cout, dtype=_dtype(kind), **kw)


def _wgrad_into(kind, xg, dyg, cin, cout, dw, db):
    """overwrite mode (accumulate = 0) into the caller's buffers, which the ops wrappers do not offer: straight through the C ABI"""
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    n, h, w, cin_s = xg.shape
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(l.osvos_wgrad_ws_bytes(n, h, w, cin_s, cout, _dtype(kind)), device="cuda", dtype=torch.uint8)
    with _pieces(kind):
        if wc.KINDS[kind][1] == "bf16act":
            _lib.check(l.osvos_conv3x3_wgrad_bf16act(p(xg), p(dyg), p(ws), p(dw), p(db), n, h, w, cin, cin_s, cout, dyg.shape[3], 0, stream), "wgrad_bf16act")
        else:
            _lib.check(l.osvos_conv3x3_wgrad(p(xg), p(dyg), p(ws), p(dw), p(db), n, h, w, cin, cin_s, cout, dyg.shape[3], 0, _dtype(kind), stream), "wgrad")
    torch.cuda.synchronize()


def _assert_equals(got, ref, what):
    """exact equality with the integer float64 reference (fp32 holds these integers exactly)"""
    got = got.double().cpu()
    assert torch.equal(got, ref), "%s: %d of %d entries differ, largest difference %g" % (
        what, int((got != ref).sum()), ref.numel(), float((got - ref).abs().nan_to_num(nan=float("inf")).max()))


def _exact_into_nan_buffers(kind, shape, x, dy, dw_ref, db_ref, what, cout_s=None):
    """the kind's result, written in overwrite mode into NaN-filled buffers, equals the reference; returns (x, dy, dw, db) on the device"""
    cin, cout = shape[3], shape[4]
    xg, dyg = _device_operands(kind, x, dy, cout_s)
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    db = torch.full((cout,), float("nan"), device="cuda")
    _wgrad_into(kind, xg, dyg, cin, cout, dw, db)
    _assert_equals(dw, dw_ref, "dw " + what)
    _assert_equals(db, db_ref, "db " + what)
    return xg, dyg, dw, db


@pytest.mark.parametrize("shape,kind", wc.LONG, ids=_ids(wc.LONG))
def test_integer_operands_give_the_exact_gradient(shape, kind):
    """a. x integers in [-3, 3] with 40 % zeros, dY in {-1, 0, 1}: exact in bf16, FP16 and fp32 and every partial sum below 2^24, so the
    result must EQUAL the integer reference whatever the summation order.  Results land in NaN-filled buffers; then the ops wrapper with
    fresh buffers (same bytes), accumulation (exactly twice the reference) and a run without the bias gradient."""
    cin, cout = shape[3], shape[4]
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    what = "%s %s" % (shape, kind)
    xg, dyg, dw, db = _exact_into_nan_buffers(kind, shape, x, dy, dw_ref, db_ref, what)
    dw1, db1 = _wgrad(kind, xg, dyg, cin, cout)
    assert torch.equal(dw1, dw) and torch.equal(db1, db)
    dw2, db2 = _wgrad(kind, xg, dyg, cin, cout, accumulate_into=(dw.clone(), db.clone()))
    _assert_equals(dw2, 2 * dw_ref, "accumulated dw " + what)
    _assert_equals(db2, 2 * db_ref, "accumulated db " + what)
    dw3, db3 = _wgrad(kind, xg, dyg, cin, cout, want_bias=False)
    assert db3 is None
    _assert_equals(dw3, dw_ref, "dw without bias " + what)


@pytest.mark.parametrize("schedule", wc.SCHEDULES)
@pytest.mark.parametrize("shape,kind", wc.SCALED, ids=_ids(wc.SCALED))
def test_scaled_operands_give_the_exact_gradient(shape, kind, schedule):
    """b. the same integers with dY times 2^a(p) and X times 2^b(p) per patch p of the f32x3 kernel's geometry (wide_wgrad_cases.
    schedule_exponents): rising along each split's walk -- in the h2 form the running block exponent of dY, of X or of both drops at several
    patches of one split and the nine accumulators are rescaled --, falling (the exponent never changes after the first patch), and with an
    all-zero patch first and another mid-walk.  Still exact for every kind (3 N H W 2^8 < 2^24): a wrong ldexp amount, a rescale taken from
    the other operand's exponent or an exchange slot read at the wrong parity cannot pass."""
    x, dy, dw_ref, db_ref = wc.scaled_case(shape, schedule)
    _exact_into_nan_buffers(kind, shape, x, dy, dw_ref, db_ref, "%s %s %s" % (shape, kind, schedule))


@pytest.mark.parametrize("shape,kind", wc.TINY, ids=_ids(wc.TINY))
def test_tiny_shapes_are_exact(shape, kind):
    """c. one pixel; H below the patch height and W below the patch width; two one-patch images walked by one workgroup: every load guard
    is live and the only split holds every patch"""
    cin, cout = shape[3], shape[4]
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    what = "%s %s" % (shape, kind)
    xg, dyg, dw, db = _exact_into_nan_buffers(kind, shape, x, dy, dw_ref, db_ref, what)
    dw2, db2 = _wgrad(kind, xg, dyg, cin, cout, accumulate_into=(dw.clone(), db.clone()))
    _assert_equals(dw2, 2 * dw_ref, "accumulated dw " + what)
    _assert_equals(db2, 2 * db_ref, "accumulated db " + what)


STRIDED = [(s, cs, k) for s, cs in wc.STRIDED for k in wc.X3_KINDS + wc.BF16_KINDS]


@pytest.mark.parametrize("shape,cout_s,kind", STRIDED, ids=["%s/%d-%s" % ("x".join(map(str, s)), cs, k) for s, cs, k in STRIDED])
def test_strided_dy_is_exact(shape, cout_s, kind):
    """d. Cout 128 in a channel stride of 136 and 64 in 72, the padding channels holding 2^100: a read of one of them cannot hide -- in the
    h2 form a padding channel that reached the max-exchange would wreck the block exponent of every patch."""
    cin, cout = shape[3], shape[4]
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    xg, dyg, dw, db = _exact_into_nan_buffers(kind, shape, x, dy, dw_ref, db_ref, "%s/%d %s" % (shape, cout_s, kind), cout_s)
    assert dyg.shape[3] == cout_s and float(dyg[..., cout:].float().min()) == wc.PAD_FILL
    dw2, db2 = _wgrad(kind, xg, dyg, cin, cout, accumulate_into=(dw.clone(), db.clone()))
    _assert_equals(dw2, 2 * dw_ref, "accumulated dw %s/%d %s" % (shape, cout_s, kind))
    _assert_equals(db2, 2 * db_ref, "accumulated db %s/%d %s" % (shape, cout_s, kind))


@pytest.mark.parametrize("kind", wc.S16_KINDS)
def test_strided_dy_at_cout_16_is_refused_or_exact(kind):
    """d. the S16 form needs a dense dY (Cout_s == 16): a strided one must be refused or take the exact fp32 fallback -- and then still be
    exact.  On an MI355X: not refused, the dispatch falls through to the exact fp32 skinny kernel, and the result is exact."""
    shape, cout_s = wc.S16_STRIDED
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    try:
        _exact_into_nan_buffers(kind, shape, x, dy, dw_ref, db_ref, "%s/%d %s" % (shape, cout_s, kind), cout_s)
        print("S16 %s with dY stride %d: taken by the fallback, exact" % (kind, cout_s))
    except RuntimeError as e:
        print("S16 %s with dY stride %d: refused (%s)" % (kind, cout_s, e))


# the project's standing bars against float64: 3e-5 max-rel and 1e-5 rel-L2 on dw, 3e-5 max-rel on db (test_wgrad_f32x3,
# test_gpu_conv1_1_wgrad.py); or twice the CPU float32 comparator's own distance from float64 where that is larger (the rule of
# test_full_size_against_cpu_oracle).  Two pieces per operand: the weight-gradient bar of test_f32x3_kernels_with_two_pieces_per_operand
# (test_gpu_ops.py: `w2 < 5e-5` rel-L2), with the max-rel bar in the same ratio to it as the standing ones (3x).
BAR_MAX, BAR_L2 = 3e-5, 1e-5
BAR_L2_TWO_PIECES = 5e-5
BAR_MAX_TWO_PIECES = 3 * BAR_L2_TWO_PIECES
RANDOM = [(s, k) for s, k in wc.LONG if s not in (wc.X3_MANY_SPLITS, wc.BF16_MANY_SPLITS)]


@pytest.mark.parametrize("shape,kind", RANDOM, ids=_ids(RANDOM))
def test_random_operands_against_float64(shape, kind):
    """e. dy = randn * exp(randn), x the same made post-ReLU like, against float64 of the same values.  The bf16 kinds: both rounded to bf16
    beforehand, so the reference sees exactly the MFMA operands and what remains is fp32 accumulation.  Bars: BAR_MAX / BAR_L2 above (two
    pieces per operand: BAR_*_TWO_PIECES) or 2x the CPU float32 comparator, whichever is larger; dw max-rel, dw rel-L2 and db max-rel.

    Measured on an MI355X, dw max-rel / dw rel-L2 / db max-rel, kernel | CPU float32 comparator:
        2,18,40,512,512  x3         1.64e-07 / 2.66e-07 / 2.39e-07 | 5.15e-07 / 5.11e-07 / 1.39e-06
        2,18,40,512,512  x3b2       4.41e-06 / 4.42e-06 / 2.39e-07 | 5.15e-07 / 5.11e-07 / 1.39e-06
        2,18,40,512,512  x3h2       8.76e-07 / 2.27e-07 / 2.39e-07 | 5.15e-07 / 5.11e-07 / 1.39e-06
        2,19,215,128,128 x3         2.50e-07 / 2.08e-07 / 1.08e-07 | 1.23e-06 / 8.73e-07 / 1.96e-06
        2,19,215,128,128 x3b2       5.57e-06 / 4.44e-06 / 1.08e-07 | 1.23e-06 / 8.73e-07 / 1.96e-06
        2,19,215,128,128 x3h2       1.73e-07 / 1.86e-07 / 1.08e-07 | 1.23e-06 / 8.73e-07 / 1.96e-06
        3,30,70,256,256  x3         4.23e-07 / 3.01e-07 / 1.28e-07 | 1.60e-06 / 7.75e-07 / 1.38e-06
        3,30,70,256,256  x3b2       7.61e-06 / 4.38e-06 / 1.28e-07 | 1.60e-06 / 7.75e-07 / 1.38e-06
        3,30,70,256,256  x3h2       3.88e-07 / 2.52e-07 / 1.28e-07 | 1.60e-06 / 7.75e-07 / 1.38e-06
        2,19,215,512,16  x3_s16     1.09e-07 / 2.04e-07 / 1.55e-07 | 4.17e-07 / 8.63e-07 / 1.38e-06
        2,19,215,512,16  x3b2_s16   4.83e-06 / 4.56e-06 / 1.55e-07 | 4.17e-07 / 8.63e-07 / 1.38e-06
        2,19,215,512,16  x3h2_s16   8.44e-08 / 1.83e-07 / 1.55e-07 | 4.17e-07 / 8.63e-07 / 1.38e-06
        3,17,65,512,512  bf16_f32t  3.35e-07 / 1.56e-07 / 7.30e-08 | 1.26e-06 / 6.28e-07 / 1.65e-07
        3,17,65,512,512  bf16_act   3.28e-07 / 1.76e-07 / 8.57e-08 | 1.26e-06 / 6.28e-07 / 1.65e-07
        3,9,195,512,448  bf16_f32t  3.65e-07 / 1.99e-07 / 8.04e-08 | 1.87e-06 / 7.99e-07 / 1.78e-07
        3,9,195,512,448  bf16_act   3.65e-07 / 1.99e-07 / 8.34e-08 | 1.87e-06 / 7.99e-07 / 1.78e-07
        3,21,150,128,64  bf16_f32t  2.98e-07 / 1.73e-07 / 4.08e-08 | 1.10e-06 / 5.39e-07 / 6.10e-08
        3,21,150,128,64  bf16_act   2.98e-07 / 1.73e-07 / 5.52e-08 | 1.10e-06 / 5.39e-07 / 6.10e-08
        3,21,150,128,16  bf16_act16 2.88e-07 / 1.70e-07 / 9.60e-08 | 9.71e-07 / 5.46e-07 / 8.23e-08
    (the split slabs make the kernels' sums pairwise-like: closer to float64 than the CPU's fp32 convolution; two pieces per operand cost 4-8e-6)"""
    cin, cout = shape[3], shape[4]
    x, dy, (dw_ref, db_ref), (dw_cpu, db_cpu) = wc.random_case(shape, wc.is_bf16_kind(kind))
    xg, dyg = _device_operands(kind, x, dy)
    dw, db = _wgrad(kind, xg, dyg, cin, cout)
    e_dw, e_db = wc.rel_err(dw.cpu(), dw_ref), wc.rel_err(db.cpu(), db_ref)
    c_dw, c_db = wc.rel_err(dw_cpu, dw_ref), wc.rel_err(db_cpu, db_ref)
    print("wide wgrad %s %s vs float64: kernel dw max %.2e l2 %.2e db max %.2e | CPU fp32 dw max %.2e l2 %.2e db max %.2e"
          % (shape, kind, e_dw[0], e_dw[1], e_db[0], c_dw[0], c_dw[1], c_db[0]))
    two = wc.KINDS[kind][2] == 2
    assert e_dw[0] <= max(BAR_MAX_TWO_PIECES if two else BAR_MAX, 2 * c_dw[0]), (shape, kind, e_dw, c_dw)
    assert e_dw[1] <= max(BAR_L2_TWO_PIECES if two else BAR_L2, 2 * c_dw[1]), (shape, kind, e_dw, c_dw)
    assert e_db[0] <= max(BAR_MAX, 2 * c_db[0]), (shape, kind, e_db, c_db)


WORKSPACE = [(wc.X3_LONG[1], "x3"), (wc.BF16_LONG[0], "bf16_act")]


@pytest.mark.parametrize("shape,kind", WORKSPACE, ids=_ids(WORKSPACE))
def test_workspace_is_written_inside_its_slabs_only(shape, kind):
    """f. a caller's workspace of the queried size plus a 4 KiB tail, all of it a byte pattern: the tail is untouched, and so is everything
    behind the kernel's own nsplit slabs and bias partials (size from the plan query; the public query also covers the exact fp32 kernel and,
    in the bf16 family, the form with more splits), the workspace was used, and the result is still the exact gradient.  One byte short is
    refused."""
    from osvos_pytorch_amd._lib import lib
    n, h, w, cin, cout = shape
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    xg, dyg = _device_operands(kind, x, dy)
    queried = lib().osvos_wgrad_ws_bytes(n, h, w, cin, cout, _dtype(kind))
    own = wc.own_ws_bytes(shape, wc.plan(shape, kind))
    assert 0 < own <= queried
    ws = torch.full((queried + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
    dw, db = _wgrad(kind, xg, dyg, cin, cout, ws=ws)
    torch.cuda.synchronize()
    assert bool((ws[queried:] == 0xA5).all()), "%s wrote behind the queried workspace" % kind
    assert bool((ws[own:] == 0xA5).all()), "%s wrote behind its own slabs" % kind
    assert not bool((ws[:own] == 0xA5).all())                                          # ... and it did use the workspace it was given
    _assert_equals(dw, dw_ref, "dw %s own workspace" % kind)
    _assert_equals(db, db_ref, "db %s own workspace" % kind)
    with pytest.raises(RuntimeError):
        _wgrad(kind, xg, dyg, cin, cout, ws=ws[:queried - 1])                          # too small a workspace is refused, not used


SAME_BYTES = [(wc.X3_LONG[1], k) for k in wc.X3_KINDS] + [(wc.S16_LONG, k) for k in wc.S16_KINDS] + [(wc.BF16_LONG[0], k) for k in wc.BF16_KINDS] + [
    (wc.ACT16_LONG, "bf16_act16")]


@pytest.mark.parametrize("shape,kind", SAME_BYTES, ids=_ids(SAME_BYTES))
def test_two_calls_give_the_same_bytes(shape, kind):
    """g. every kernel writes per-split slabs and the reduce sums them in a fixed order: no atomics, so the same inputs give the same bytes"""
    cin, cout = shape[3], shape[4]
    x, dy, _, _ = wc.random_case(shape, wc.is_bf16_kind(kind))
    xg, dyg = _device_operands(kind, x, dy)
    dw1, db1 = _wgrad(kind, xg, dyg, cin, cout)
    dw2, db2 = _wgrad(kind, xg, dyg, cin, cout)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    assert bool(torch.isfinite(dw1).all()) and float(dw1.abs().max()) > 0
