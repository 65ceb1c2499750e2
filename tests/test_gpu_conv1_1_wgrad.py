"""conv1_1's weight gradient at op level, where each workgroup walks MANY patches (csrc/wgrad_small_f32.hip): wgrad_c3_f32_kernel with fp32
and with bf16 dY, wgrad_c3_bf16_kernel, and the reduce they share.  The shapes (tests/conv1_1_wgrad_cases.py, pinned on the CPU by
test_conv1_1_wgrad_cases_cpu.py) reach the register prefetch of the next patch, the bf16 kernel's dead prefetch, a short last split, a split
that crosses from one image into the next and more than 64 splits; before, only whole-network tests at full frame size did, with conv1_1's
gradient one tensor among thirty under a 1e-3 bar.

Three ways to run the layer ("kind"):
    f32         ops.conv3x3_wgrad, fp32 dY                          -> wgrad_c3_f32_kernel
    f32_bf16dy  ops.conv3x3_wgrad_c3_bf16dy, c3-bf16 switch off     -> wgrad_c3_f32_kernel widening a bf16 dY on load
    bf16pipe    ops.conv3x3_wgrad_c3_bf16dy, switch on (default)    -> wgrad_c3_bf16_kernel (Cout 64 only)"""
import contextlib
import ctypes as C

import pytest
import torch

import conv1_1_wgrad_cases as wc

pytestmark = pytest.mark.gpu

KINDS = ["f32", "f32_bf16dy", "bf16pipe"]


def _ops():
    from osvos_pytorch_amd import ops
    return ops


@contextlib.contextmanager
def _c3_bf16(on):
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    prev = l.osvos_debug_set_c3_bf16(int(on))
    try:
        yield
    finally:
        l.osvos_debug_set_c3_bf16(prev)


def _device_operands(kind, x, dy, cout_s=None):
    """CPU NCHW operands -> (x NHWC8 fp32, dy NHWC fp32 | bf16) on the GPU, in the formats the kind reads"""
    return wc.x_nhwc8(x).cuda(), wc.dy_nhwc(dy, cout_s, torch.float32 if kind == "f32" else torch.bfloat16).cuda()


def _wgrad(kind, xg, dyg, cout, **kw):
    ops = _ops()
    if kind == "f32":
        return ops.conv3x3_wgrad(xg, dyg, 3, cout, **kw)
    with _c3_bf16(kind == "bf16pipe"):
        return ops.conv3x3_wgrad_c3_bf16dy(xg, dyg, cout, **kw)


def _wgrad_into(kind, xg, dyg, cout, dw, db):
    """overwrite mode (accumulate = 0) into the caller's buffers, which the ops wrappers do not offer: straight through the C ABI"""
    from osvos_pytorch_amd import _lib
    from osvos_pytorch_amd._lib import F32, F32_BF16MFMA
    l = _lib.lib()
    n, h, w, _ = xg.shape
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if kind == "f32":
        ws = torch.empty(l.osvos_wgrad_ws_bytes(n, h, w, 8, cout, F32), device="cuda", dtype=torch.uint8)
        _lib.check(l.osvos_conv3x3_wgrad(p(xg), p(dyg), p(ws), p(dw), p(db), n, h, w, 3, 8, cout, dyg.shape[3], 0, F32, stream), "wgrad")
    else:
        ws = torch.empty(l.osvos_wgrad_ws_bytes(n, h, w, 8, cout, F32_BF16MFMA), device="cuda", dtype=torch.uint8)
        with _c3_bf16(kind == "bf16pipe"):
            _lib.check(l.osvos_conv3x3_wgrad_c3_bf16dy(p(xg), p(dyg), p(ws), p(dw), p(db), n, h, w, cout, dyg.shape[3], 0, stream), "wgrad_c3_bf16dy")
    torch.cuda.synchronize()


def _assert_equals(got, ref, what):
    """exact equality with the integer float64 reference (fp32 holds these integers exactly)"""
    got = got.double().cpu()
    assert torch.equal(got, ref), "%s: %d of %d entries differ, largest difference %g" % (
        what, int((got != ref).sum()), ref.numel(), float((got - ref).abs().nan_to_num(nan=float("inf")).max()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", wc.SHAPES, ids=str)
def test_integer_operands_give_the_exact_gradient(shape, kind):
    """a. x integers in [-3, 3], dY in {-1, 0, 1}: exact in bf16 and fp32 and every partial sum below 2^24, so the result must EQUAL the
    integer reference whatever the summation order -- a dropped, repeated or shifted pixel, patch or split cannot pass, whatever its size.
    Results land in NaN-filled buffers; then accumulation (exactly twice the reference) and a run without the bias gradient."""
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    xg, dyg = _device_operands(kind, x, dy)
    dw = torch.full((wc.COUT, 3, 3, 3), float("nan"), device="cuda")
    db = torch.full((wc.COUT,), float("nan"), device="cuda")
    _wgrad_into(kind, xg, dyg, wc.COUT, dw, db)
    _assert_equals(dw, dw_ref, "dw %s %s" % (shape, kind))
    _assert_equals(db, db_ref, "db %s %s" % (shape, kind))
    dw1, db1 = _wgrad(kind, xg, dyg, wc.COUT)                                          # the ops wrapper, fresh buffers
    assert torch.equal(dw1, dw) and torch.equal(db1, db)
    dw2, db2 = _wgrad(kind, xg, dyg, wc.COUT, accumulate_into=(dw.clone(), db.clone()))
    _assert_equals(dw2, 2 * dw_ref, "accumulated dw %s %s" % (shape, kind))
    _assert_equals(db2, 2 * db_ref, "accumulated db %s %s" % (shape, kind))
    dw3, db3 = _wgrad(kind, xg, dyg, wc.COUT, want_bias=False)
    assert db3 is None
    _assert_equals(dw3, dw_ref, "dw without bias %s %s" % (shape, kind))


# the project's standing bars for this kernel against float64: 3e-5 max-rel (test_conv3x3_dgrad_and_wgrad), 1e-5 rel-L2
# (test_wgrad_many_patches_and_splits); or twice the CPU float32 comparator's own distance from float64 where that is larger
# (the rule of test_full_size_against_cpu_oracle)
BAR_MAX, BAR_L2 = 3e-5, 1e-5


@pytest.mark.parametrize("kind", ["f32", "bf16pipe"])
@pytest.mark.parametrize("shape", wc.SHAPES, ids=str)
def test_random_operands_against_float64(shape, kind):
    """b. dy = randn * exp(randn), image randn, against float64 of the same values.  bf16pipe: x rounded to bf16 beforehand and dy drawn as
    bf16, so the reference sees exactly the MFMA operands and what remains is fp32 accumulation.  Bars: BAR_MAX / BAR_L2 above or 2x the CPU
    float32 comparator, whichever is larger; dw max-rel, dw rel-L2 and db max-rel.

    Measured on an MI355X, dw max-rel / dw rel-L2 / db max-rel, kernel | CPU float32 comparator:
        3,51,600   f32       1.91e-07 / 2.17e-07 / 1.62e-07 | 3.88e-06 / 2.74e-06 / 2.97e-06
        3,51,600   bf16pipe  1.47e-07 / 1.26e-07 / 8.68e-08 | 3.38e-06 / 2.24e-06 / 3.33e-07
        3,67,616   f32       2.05e-07 / 2.61e-07 / 2.48e-07 | 3.99e-06 / 3.30e-06 / 2.67e-06
        3,67,616   bf16pipe  1.12e-07 / 1.28e-07 / 8.27e-08 | 3.35e-06 / 2.77e-06 / 3.07e-07
        4,115,600  f32       3.37e-07 / 3.34e-07 / 4.11e-07 | 3.10e-06 / 2.32e-06 / 3.58e-06
        4,115,600  bf16pipe  1.50e-07 / 1.41e-07 / 9.24e-08 | 2.03e-06 / 1.89e-06 / 3.12e-07
    (the split slabs make the kernels' sums pairwise-like: an order of magnitude closer to float64 than the CPU's fp32 convolution)"""
    bf16 = kind == "bf16pipe"
    x, dy, (dw_ref, db_ref), (dw_cpu, db_cpu) = wc.random_case(shape, bf16)
    xg, dyg = _device_operands(kind, x, dy)
    dw, db = _wgrad(kind, xg, dyg, wc.COUT)
    e_dw, e_db = wc.rel_err(dw.cpu(), dw_ref), wc.rel_err(db.cpu(), db_ref)
    c_dw, c_db = wc.rel_err(dw_cpu, dw_ref), wc.rel_err(db_cpu, db_ref)
    print("conv1_1 wgrad %s %s vs float64: kernel dw max %.2e l2 %.2e db max %.2e | CPU fp32 dw max %.2e l2 %.2e db max %.2e"
          % (shape, kind, e_dw[0], e_dw[1], e_db[0], c_dw[0], c_dw[1], c_db[0]))
    assert e_dw[0] <= max(BAR_MAX, 2 * c_dw[0]), (shape, kind, e_dw, c_dw)
    assert e_dw[1] <= max(BAR_L2, 2 * c_dw[1]), (shape, kind, e_dw, c_dw)
    assert e_db[0] <= max(BAR_MAX, 2 * c_db[0]), (shape, kind, e_db, c_db)


@pytest.mark.parametrize("shape", wc.SHAPES, ids=str)
def test_bf16_pipe_next_to_the_fp32_kernel_on_an_unrounded_image(shape):
    """continuity with test_bf16_mode_conv1_1_weight_gradient_on_the_bf16_pipe_matches_the_fp32_kernel: the same bf16 dY and an fp32 image
    that is NOT bf16-representable; the only difference is the bf16 rounding of the image (2^-9 relative per element), within that test's
    3e-3 rel-L2 -- and not zero, which is how this file knows the switch really selects two kernels.  The bias gradients (fp32 column sums
    of the same bf16 dY in both) agree to summation order.  Measured on an MI355X: dW rel-L2 1.63e-03 / 1.67e-03 / 1.68e-03 for the three
    shapes, db rel-L2 1.2e-07."""
    x, dy = wc.random_operands(shape, seed=7)
    assert not torch.equal(x.bfloat16().float(), x)
    xg, dyg = _device_operands("bf16pipe", x, dy)
    dw0, db0 = _wgrad("f32_bf16dy", xg, dyg, wc.COUT)
    dw1, db1 = _wgrad("bf16pipe", xg, dyg, wc.COUT)
    d_dw, d_db = wc.rel_err(dw1, dw0)[1], wc.rel_err(db1, db0)[1]
    print("conv1_1 wgrad %s bf16 pipe vs fp32 kernel, same bf16 dY: dW rel-L2 %.2e, db rel-L2 %.2e" % (shape, d_dw, d_db))
    assert 0 < d_dw <= 3e-3 and d_db <= 1e-5, (shape, d_dw, d_db)


NARROW = [("f32", 32, 32), ("f32", 12, 16), ("f32", 64, 72), ("f32_bf16dy", 32, 32), ("f32_bf16dy", 12, 16), ("f32_bf16dy", 64, 72),
          ("bf16pipe", 64, 72)]


@pytest.mark.parametrize("kind,cout,cout_s", NARROW)
def test_narrow_and_strided_dy_is_exact(kind, cout, cout_s):
    """c. Cout < 64 (the `co < Cout` guards, the reduce grid Cout * 28) and a dY whose channel stride exceeds Cout, its padding channels
    holding 2^100: integer operands, exact equality.  The narrower dY is the leading channels of the Cout = 64 draw, so the reference is the
    leading rows of the same float64 gradient."""
    shape = wc.SHAPES[0]
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    xg, dyg = _device_operands(kind, x, dy[:, :cout], cout_s)
    assert dyg.shape[3] == cout_s and (cout_s == cout or float(dyg[..., cout:].float().min()) == wc.PAD_FILL)
    dw = torch.full((cout, 3, 3, 3), float("nan"), device="cuda")
    db = torch.full((cout,), float("nan"), device="cuda")
    _wgrad_into(kind, xg, dyg, cout, dw, db)
    _assert_equals(dw, dw_ref[:cout], "dw %s Cout %d/%d" % (kind, cout, cout_s))
    _assert_equals(db, db_ref[:cout], "db %s Cout %d/%d" % (kind, cout, cout_s))
    dw2, db2 = _wgrad(kind, xg, dyg, cout, accumulate_into=(dw.clone(), db.clone()))
    _assert_equals(dw2, 2 * dw_ref[:cout], "accumulated dw %s Cout %d/%d" % (kind, cout, cout_s))
    _assert_equals(db2, 2 * db_ref[:cout], "accumulated db %s Cout %d/%d" % (kind, cout, cout_s))


@pytest.mark.parametrize("kind", KINDS)
def test_workspace_is_written_inside_its_slabs_only(kind):
    """d. a caller's workspace of the queried size plus a 4 KiB tail, all of it a byte pattern: the tail is untouched, and so is everything
    behind the kernel's own slabs ([nsplit][64][32] partial tiles, then [nsplit][64] bias partials; the query covers the kernel with more
    splits, and the generic kernel's slabs where those are larger), and the result is still the exact gradient."""
    from osvos_pytorch_amd._lib import F32, F32_BF16MFMA, lib
    ops = _ops()
    shape = wc.SHAPES[1]
    x, dy, dw_ref, db_ref = wc.integer_case(shape)
    xg, dyg = _device_operands(kind, x, dy)
    plan = ops.wgrad_c3_plan(*shape, kind == "bf16pipe")
    queried = lib().osvos_wgrad_ws_bytes(*shape, 8, wc.COUT, F32 if kind == "f32" else F32_BF16MFMA)
    own = plan["nsplit"] * wc.SLAB_FLOATS_PER_SPLIT * 4
    assert own <= wc.ws_bytes_needed(ops.wgrad_c3_plan(*shape, False), ops.wgrad_c3_plan(*shape, True)) <= queried
    ws = torch.full((queried + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
    dw, db = _wgrad(kind, xg, dyg, wc.COUT, ws=ws)
    torch.cuda.synchronize()
    assert bool((ws[queried:] == 0xA5).all()), "%s wrote behind the queried workspace" % kind
    assert bool((ws[own:] == 0xA5).all()), "%s wrote behind its own slabs" % kind
    assert not bool((ws[:own] == 0xA5).all())                                          # ... and it did use the workspace it was given
    _assert_equals(dw, dw_ref, "dw %s own workspace" % kind)
    _assert_equals(db, db_ref, "db %s own workspace" % kind)
    with pytest.raises(RuntimeError):
        _wgrad(kind, xg, dyg, wc.COUT, ws=ws[:queried - 1])                            # too small a workspace is refused, not used


@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_the_same_bytes(kind):
    """e. both kernels write per-split slabs and reduce them in a fixed order: no atomics, so the same inputs give the same bytes"""
    shape = wc.SHAPES[2]
    x, dy, _, _ = wc.random_case(shape, kind != "f32")
    xg, dyg = _device_operands(kind, x, dy)
    dw1, db1 = _wgrad(kind, xg, dyg, wc.COUT)
    dw2, db2 = _wgrad(kind, xg, dyg, wc.COUT)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    assert bool(torch.isfinite(dw1).all()) and float(dw1.abs().max()) > 0
