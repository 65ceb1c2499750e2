"""Pins tests/relu_mask_cases.py, the post-ReLU operands of test_gpu_relu_zero_operands.py: what is planted is there, in both dtypes, at every shape
the GPU test uses, and the rule `expected_dx` evaluates is autograd's own (vgg_osvos.py: conv -> ReLU -> conv)."""
import pytest
import torch
import torch.nn.functional as F

import relu_mask_cases as rc

DTYPES = [torch.float32, torch.bfloat16]
SHAPES = rc.mask_shapes() + rc.pool_shapes()


def _neg_zero(t):
    return (t == 0) & torch.signbit(t)


def _pos_zero(t):
    return (t == 0) & ~torch.signbit(t)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_post_relu_mask_holds_what_it_promises(shape, dtype):
    n, c, h, w = shape
    m = rc.post_relu_mask(shape, 5, dtype)
    assert m.shape == shape and m.dtype == dtype
    assert torch.equal(m, rc.post_relu_mask(shape, 5, dtype))                        # deterministic
    f = m.float()
    assert bool((f >= 0).all()) and bool(torch.isfinite(f).all())
    assert not bool(((f > 0) & (f < rc.TINY)).any())                                 # no denormals
    share = float((f == 0).float().mean())
    assert 0.35 <= share <= 0.65, (shape, share)
    assert int(_neg_zero(f).sum()) >= 8
    assert int((f == rc.TINY).sum()) >= 8 and int((f == rc.SMALL).sum()) >= 8
    pos = rc.special_positions(c, w)
    assert len(set(pos)) >= 8
    for ch, col in pos:
        assert bool(_neg_zero(f[0, ch, 0, col])) and float(f[0, ch, 1, col]) == rc.TINY and float(f[0, ch, 2, col]) == rc.SMALL
    assert bool(_pos_zero(f[0, :, h // 2, :]).all())                                 # the dead row
    bc = min(c, 32)
    blocks = rc.block_pixels(c, h, w)
    assert len(blocks) == max(c // 32, 1)
    for g, (dy_, dx_), (ly_, lx_) in blocks:
        assert bool(_pos_zero(f[n - 1, bc * g: bc * g + bc, dy_, dx_]).all()), g      # fully dead block
        assert bool((f[n - 1, bc * g: bc * g + bc, ly_, lx_] > 0).all()), g           # fully live block
    assert bool(_pos_zero(f[n - 1, 0, h - 1, w - 1])) and float(f[n - 1, c - 1, h - 1, w - 1]) > 0
    # one draw for both dtypes: the bf16 mask is the rounding of the fp32 one, and the two agree on who is alive
    m32 = rc.post_relu_mask(shape, 5, torch.float32)
    assert torch.equal(m32.bfloat16().float(), rc.post_relu_mask(shape, 5, torch.bfloat16).float())
    assert torch.equal(m32 > 0, m > 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_the_rule_on_the_planted_values(dtype):
    v = torch.tensor([-0.0, 0.0, rc.TINY, rc.SMALL, rc.LIVE, 1.5]).to(dtype)
    assert v.float().tolist() == [0.0, 0.0, rc.TINY, rc.SMALL, rc.LIVE, 1.5]        # exact in bf16 as well
    assert bool(torch.signbit(v.float()[0]))
    assert (v > 0).tolist() == [False, False, True, True, True, True]
    if dtype == torch.bfloat16:      # the kernels read a stored bf16 as a signed 16-bit integer: > 0 there is the same rule
        assert (v.view(torch.int16) > 0).tolist() == (v > 0).tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_pack_mask_bits(dtype):
    m = rc.post_relu_mask((2, 64, 9, 11), 3, dtype).permute(0, 2, 3, 1).contiguous()
    bits = rc.pack_mask_bits(m)
    assert bits.shape == (2, 9, 11, 2) and bits.dtype == torch.int32
    for ch in (0, 1, 31, 32, 63):
        assert torch.equal(((bits[..., ch // 32].long() >> (ch % 32)) & 1).bool(), m[..., ch] > 0), ch
    n, c, h, w = 2, 64, 9, 11
    for g, (dy_, dx_), (ly_, lx_) in rc.block_pixels(c, h, w):
        assert int(bits[n - 1, dy_, dx_, g]) == 0 and int(bits[n - 1, ly_, lx_, g]) == -1      # dead block: no bit; live block: all 32


@pytest.mark.parametrize("shape", [(2, 7, 9, 16, 32), (1, 8, 7, 32, 64)], ids=str)
def test_expected_dx_is_autograd_of_conv_relu_conv(shape):
    """the mask IS the ReLU output: relu(mask) == mask and its gradient gate is mask > 0 -- dead at +0.0 and -0.0, live at 2^-126"""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(9)
    mask = rc.post_relu_mask((n, cin, h, w), 11, torch.float32)
    z = mask.double().requires_grad_()                       # the first convolution's output
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / 7
    dy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    a = F.relu(z)
    assert torch.equal(a.detach(), mask.double())
    F.conv2d(a, wt, None, padding=1).backward(dy)
    ref = rc.expected_dx(z.shape, wt, dy, a.detach())
    assert float((z.grad - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((z.grad[mask <= 0] == 0).all()) and int((z.grad != 0).sum()) == int((mask > 0).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", rc.pool_shapes(), ids=str)
def test_pool_input_windows(shape, dtype):
    n, c, h, w = shape
    x = rc.pool_input(shape, 7, dtype)
    f = x.float()
    assert x.dtype == dtype and bool((f >= 0).all())
    base = rc.post_relu_mask(shape, 7, dtype).float()        # (its share of zeros is pinned above; the windows only add zeros to the last image)
    assert torch.equal(f[: n - 1], base[: n - 1]) and torch.equal(f[n - 1, 7::8], base[n - 1, 7::8])
    ho, wo = (h + 1) // 2, (w + 1) // 2
    sites = rc.pool_window_sites(h, w)
    assert (0, 0) in sites and (ho - 1, wo - 1) in sites and len([s for s in sites if s[0] == ho - 1]) == wo and len([s for s in sites if s[1] == wo - 1]) == ho
    for oy, ox in sites:
        win = f[n - 1, :, 2 * oy: 2 * oy + 2, 2 * ox: 2 * ox + 2]            # clipped at the border like the pooling's window
        assert bool(_pos_zero(win[0]).all())
        assert bool(_neg_zero(win[1]).all())
        assert bool((win[2] == 0).all())
        for q in range(4):
            full = torch.zeros(2, 2)
            full[q // 2, q % 2] = rc.LIVE
            assert torch.equal(win[3 + q], full[: win.shape[1], : win.shape[2]]), (oy, ox, q)
    mixed = f[n - 1, 2, 0:2, 0:2]
    assert torch.signbit(mixed).flatten().tolist() == [False, True, True, False]
    dead = rc.all_zero_windows(x)
    assert dead.shape == x.shape and bool(dead[n - 1, 0:3, 0:2, 0:2].all()) and not bool(dead[n - 1, 3:7, 0:2, 0:2].any())
    assert bool((f[dead] == 0).all())
    # every position of a window is the single live one somewhere, and clipped windows exist where a size is odd
    if h % 2:
        assert bool(dead[n - 1, 5, h - 1, :].all())         # live corner (1, 0) falls outside a window clipped to one row
    if w % 2:
        assert bool(dead[n - 1, 4, :, w - 1].all())         # live corner (0, 1) falls outside a window clipped to one column
