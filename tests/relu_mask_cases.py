"""TEST INFRASTRUCTURE: post-ReLU operands for the masked data gradients and the pooling kernels, shared by test_relu_mask_cases_cpu.py (which
pins what is planted here, so the GPU tests cannot become vacuous) and test_gpu_relu_zero_operands.py.

In the network the ReLU mask of a data gradient is the saved post-ReLU activation of the previous layer (vgg_osvos.py: conv -> ReLU -> conv):
about half of its entries are exactly +0.0 and whole 32-channel blocks can be dead.  The rule of the kernels is y = 0 where mask <= 0
(csrc/kernels.h, csrc/maskbits.h): +0.0 and -0.0 are dead, the smallest positive normal is live.  A mask drawn from randn holds none of these.
Denormals are not planted: whether they count as zero is not pinned by the reference."""
import torch

TINY = 2.0 ** -126          # smallest positive normal fp32 (and bf16)
SMALL = 2.0 ** -100         # positive, survives rounding to bf16 as a positive bf16
N_SPECIAL = 16              # positions planted per special value (the CPU test asks for at least 8)
LIVE = 0.75                 # the single live element of the pooling windows (bf16-representable)


def special_positions(c, w, n_special=N_SPECIAL):
    """(channel, column) of the k-th planted special value in its row: a stride of 37 over the row's (column, channel) elements"""
    flat = sorted({(k * 37) % (w * c) for k in range(n_special)})
    return [(f % c, f // c) for f in flat]


def block_pixels(c, h, w):
    """[(g, dead (y, x), live (y, x))] for every 32-channel block g (channel counts below 32: one block of all channels), in the LAST image"""
    return [(g, (h - 2, (2 + 3 * g) % w), (h - 3, (1 + 3 * g) % w)) for g in range(max(c // 32, 1))]


def post_relu_mask(shape, seed, dtype=torch.float32):
    """NCHW tensor of `dtype` (torch.float32 or torch.bfloat16): relu(randn), rounded to bf16 first when that is the dtype, with planted
         image 0, row 0 / 1 / 2        -0.0 / 2^-126 / 2^-100 at special_positions()
         image 0, row H // 2           dead (all +0.0)
         last image, row H - 2 / H - 3 per 32-channel block one fully dead / fully live pixel (block_pixels())
         last image, last pixel        dead in channel 0, live in the last channel
    (with N = 1 image 0 IS the last image: the planted rows 0, 1, 2, H // 2, H - 3, H - 2, H - 1 stay distinct because H >= 7 is asserted)
    The same seed gives the same draw for both dtypes: the bf16 tensor is the rounding of the fp32 one (the planted values are exact in bf16)."""
    n, c, h, w = shape
    assert h >= 7 and w >= 2 and c >= 2, shape
    g = torch.Generator().manual_seed(seed)
    m = torch.relu(torch.randn(n, c, h, w, generator=g))
    if dtype == torch.bfloat16:
        m = m.bfloat16().float()
    else:
        assert dtype == torch.float32, dtype
    for row, val in ((0, -0.0), (1, TINY), (2, SMALL)):
        for ch, col in special_positions(c, w):
            m[0, ch, row, col] = val
    m[0, :, h // 2, :] = 0.0
    bc = min(c, 32)
    for blk, (dy_, dx_), (ly_, lx_) in block_pixels(c, h, w):
        m[n - 1, bc * blk: bc * blk + bc, dy_, dx_] = 0.0
        m[n - 1, bc * blk: bc * blk + bc, ly_, lx_] = 1.0 + torch.arange(bc, dtype=torch.float32) / 64
    m[n - 1, 0, h - 1, w - 1] = 0.0
    m[n - 1, c - 1, h - 1, w - 1] = 1.5
    return m.to(dtype)


def expected_dx(x_shape, w, dy, mask):
    """float64 reference of the masked data gradient: conv2d_input(...) * (mask > 0), the rule evaluated on the mask's values as stored"""
    dx = torch.nn.grad.conv2d_input(tuple(x_shape), w.double(), dy.double(), padding=1)
    return dx * (mask > 0)


def pack_mask_bits(mask_nhwc):
    """[N,H,W,C] -> int32 [N,H,W,C/32]: bit b of word g = (mask[..., 32 g + b] > 0)   (csrc/maskbits.h)"""
    n, h, w, c = mask_nhwc.shape
    assert c % 32 == 0
    pos = (mask_nhwc > 0).long().reshape(n, h, w, c // 32, 32)
    words = (pos << torch.arange(32)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


# 2 x 2 windows planted into the pooling input, by channel % 8 (7: left as drawn); rows of the window top to bottom
POOL_WINDOWS = (
    ((0.0, 0.0), (0.0, 0.0)),            # all +0.0
    ((-0.0, -0.0), (-0.0, -0.0)),        # all -0.0
    ((0.0, -0.0), (-0.0, 0.0)),          # mixed zeros
    ((LIVE, 0.0), (0.0, 0.0)),           # a single live element in each of the four corners
    ((0.0, LIVE), (0.0, 0.0)),
    ((0.0, 0.0), (LIVE, 0.0)),
    ((0.0, 0.0), (0.0, LIVE)),
)


def pool_window_sites(h, w):
    """(oy, ox) of the windows that receive POOL_WINDOWS in the last image: two inner ones, the whole last window row and the whole last window
    column -- clipped (ceil mode) where H or W is odd"""
    ho, wo = (h + 1) // 2, (w + 1) // 2
    sites = {(0, 0), (1, wo // 2)}
    sites |= {(ho - 1, ox) for ox in range(wo)}
    sites |= {(oy, wo - 1) for oy in range(ho)}
    return sorted(sites)


def pool_input(shape, seed, dtype=torch.float32):
    """post_relu_mask with POOL_WINDOWS written over it (windows at the border are clipped by the tensor's edge, as the pooling clips them)"""
    n, c, h, w = shape
    x = post_relu_mask(shape, seed, dtype).float()
    for oy, ox in pool_window_sites(h, w):
        for k, pat in enumerate(POOL_WINDOWS):
            p = torch.tensor(pat)[: h - 2 * oy, : w - 2 * ox]
            x[n - 1, k::8, 2 * oy: 2 * oy + 2, 2 * ox: 2 * ox + 2] = p
    return x.to(dtype)


def all_zero_windows(x):
    """bool NCHW, true at every element whose 2 x 2 ceil-mode window holds no positive value"""
    n, c, h, w = x.shape
    top = torch.nn.functional.max_pool2d(x.double(), 2, 2, ceil_mode=True)
    return (top.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :h, :w] <= 0)


# layers (N, H, W, Cin, Cout) whose data gradient (Cout -> Cin channels, mask of Cin channels) the GPU test runs; DEEP: K long enough to cut
LAYERS = [(2, 17, 35, 64, 64), (1, 33, 70, 64, 128), (1, 9, 11, 128, 64)]
DEEP = (1, 15, 27, 64, 256)
POOL_C = (8, 64, 96)
POOL_HW = ((9, 13), (7, 2), (30, 54))
POOL_N = 2


def layer_seed(layer):
    return 1000 + sum(p * q for p, q in zip(layer, (1, 3, 5, 7, 11)))


def mask_shapes():
    return [(n, cin, h, w) for n, h, w, cin, _ in LAYERS + [DEEP]]


def pool_shapes():
    return [(POOL_N, c, h, w) for c in POOL_C for h, w in POOL_HW]
