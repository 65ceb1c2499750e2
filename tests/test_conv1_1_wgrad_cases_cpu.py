"""Pins tests/conv1_1_wgrad_cases.py, the shapes and operands of test_gpu_conv1_1_wgrad.py: through the library's own plan query
(osvos_wgrad_c3_plan, host only) every regime the GPU tests claim to reach is asserted here, for both of conv1_1's weight-gradient kernels,
so a later retune of the split targets fails loudly instead of silently returning the tests to one patch per workgroup.  Also the condition
the exact-equality tests rest on: with the integer operands the float64 reference is integral and below 2^24."""
import pytest
import torch

import conv1_1_wgrad_cases as wc

KERNELS = [False, True]
IDS = ["f32", "bf16pipe"]


def _plan(shape, bf16_dy):
    from osvos_pytorch_amd import ops
    return ops.wgrad_c3_plan(*shape, bf16_dy)


@pytest.mark.parametrize("bf16_dy", KERNELS, ids=IDS)
@pytest.mark.parametrize("shape", wc.SHAPES, ids=str)
def test_plan_is_the_table(shape, bf16_dy):
    n, h, w = shape
    p = _plan(shape, bf16_dy)
    pw, ph = wc.PATCH[bf16_dy]
    assert p["npx"] == -(-w // pw) and p["npy"] == -(-h // ph) and p["npatches"] == n * p["npx"] * p["npy"]
    assert p["nsplit"] == -(-p["npatches"] // p["per_split"]) and (p["nsplit"] - 1) * p["per_split"] < p["npatches"]
    npatches, per_split, nsplit, tail, span = wc.TABLE[shape][bf16_dy]
    assert (p["npatches"], p["per_split"], p["nsplit"], wc.tail(p)) == (npatches, per_split, nsplit, tail), p
    spans = wc.spanning_splits(p)
    assert (spans[0] if spans else None) == span, spans
    # the last patch column and the last patch row are partial in this kernel's patch geometry
    assert w % pw != 0 and h % ph != 0


@pytest.mark.parametrize("bf16_dy", KERNELS, ids=IDS)
def test_the_shapes_reach_every_regime_of_each_kernel(bf16_dy):
    plans = [_plan(s, bf16_dy) for s in wc.SHAPES]
    assert any(p["per_split"] >= 2 and wc.tail(p) < p["per_split"] for p in plans)       # prefetch loop + a short last split
    assert any(p["per_split"] >= 3 for p in plans)                                       # a prefetch issued under a prefetched patch
    assert all(p["nsplit"] > 64 for p in plans)                                          # the reduce's `sp += 64` loop
    assert any(wc.spanning_splits(p) for p in plans)                                     # a split with patches of two images
    assert all(p["nsplit"] * p["per_split"] >= p["npatches"] for p in plans)


@pytest.mark.parametrize("bf16_dy", KERNELS, ids=IDS)
@pytest.mark.parametrize("shape", wc.OLD_SHAPES, ids=str)
def test_the_earlier_shapes_walk_one_patch_per_workgroup(shape, bf16_dy):
    """the gap: the largest shapes the op-level and bf16-switch tests fed these kernels never entered the prefetch loop"""
    p = _plan(shape, bf16_dy)
    assert p["per_split"] == 1 and p["nsplit"] == p["npatches"]


@pytest.mark.parametrize("shape", wc.SHAPES, ids=str)
def test_workspace_query_covers_both_kernels(shape):
    """slabs [nsplit][64][32] + [nsplit][64] floats of whichever kernel has more splits; the public query may return more (the same shape
    can be sent to the generic kernel, whose slabs are [nsplit][9][Cout][8]), never less -- for the dtype either entry point asks with"""
    from osvos_pytorch_amd import _lib
    need = wc.ws_bytes_needed(_plan(shape, False), _plan(shape, True))
    for dtype in (_lib.F32, _lib.F32_BF16MFMA):
        for cout in (64, 32, 12):
            assert _lib.lib().osvos_wgrad_ws_bytes(*shape, 8, cout, dtype) >= need, (shape, dtype, cout)


def test_plan_query_rejects_bad_arguments():
    from osvos_pytorch_amd import _lib
    assert _lib.lib().osvos_wgrad_c3_plan(0, 8, 8, 0, None) < 0


@pytest.mark.parametrize("shape", wc.SHAPES, ids=str)
def test_integer_operands_make_every_summation_order_exact(shape):
    n, h, w = shape
    x, dy, dw, db = wc.integer_case(shape)
    assert x.shape == (n, 3, h, w) and dy.shape == (n, wc.COUT, h, w)
    assert torch.equal(x, x.round()) and float(x.min()) == -3 and float(x.max()) == 3
    assert sorted(dy.unique().tolist()) == [-1.0, 0.0, 1.0]
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy)      # exact in bf16
    assert 3 * n * h * w < 2 ** 24                                                              # bound of every partial sum
    for t in (dw, db):
        assert t.dtype == torch.float64 and torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24
    assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0
    # the padded layouts: channels 3..7 of x zero, padding channels of dy large and finite
    x8 = wc.x_nhwc8(x)
    assert x8.shape == (n, h, w, 8) and float(x8[..., 3:].abs().max()) == 0 and torch.equal(x8[..., :3].permute(0, 3, 1, 2), x)
    d72 = wc.dy_nhwc(dy, 72, torch.bfloat16)
    assert d72.shape == (n, h, w, 72) and torch.equal(d72[..., :64].float().permute(0, 3, 1, 2), dy)
    assert bool((d72[..., 64:].float() == wc.PAD_FILL).all())
    # a narrower dy is the leading channels of the same draw, so its reference is the leading rows
    assert torch.equal(wc.integer_operands(shape, cout=12)[1], dy[:, :12])


def test_random_bf16_operands_are_bf16_values():
    x, dy, ref64, ref32 = wc.random_case(wc.SHAPES[0], True)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy)
    assert ref64[0].dtype == torch.float64 and ref32[0].dtype == torch.float32
    e = wc.rel_err(ref32[0], ref64[0])
    assert 0 < e[1] < 1e-4, e      # the comparator is an fp32 computation of the same values: close to, not equal to, float64
