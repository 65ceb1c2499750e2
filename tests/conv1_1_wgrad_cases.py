"""TEST INFRASTRUCTURE: shapes, operands and references for conv1_1's weight gradient (csrc/wgrad_small_f32.hip: wgrad_c3_f32_kernel,
wgrad_c3_bf16_kernel and their shared reduce), shared by test_conv1_1_wgrad_cases_cpu.py (which pins the regime each shape reaches, so the GPU
tests cannot quietly fall back to one patch per workgroup) and test_gpu_conv1_1_wgrad.py.

The two plans have no clamp on the number of splits, so below ~256 (fp32 kernel, 32 x 8 pixel patches) / ~1024 (bf16-pipe kernel, 16 x 8)
patches every workgroup walks ONE patch: the register prefetch of the next patch, the bf16 kernel's dead prefetch behind the last one, a
short last split, a split that crosses from one image into the next and the reduce's second trip over the splits are then never run.
SHAPES are the smallest that reach all of these, for both kernels (plans recomputed on the CPU; the CPU test asserts them):

    N,H,W       fp32 kernel: patches / per_split / nsplit / tail      bf16-pipe kernel
    3,51,600    399 / 2 / 200 / 1, split 66 spans images 0 -> 1       798 / 1 / 798 / 1
    3,67,616    540 / 3 / 180 / 3                                     1053 / 2 / 527 / 1, split 175 spans images 0 -> 1
    4,115,600   1140 / 5 / 228 / 5                                    2280 / 3 / 760 / 3

Nothing here touches a GPU."""
import functools

import torch
import torch.nn.functional as F

SHAPES = [(3, 51, 600), (3, 67, 616), (4, 115, 600)]
OLD_SHAPES = [(1, 64, 70), (1, 120, 214)]         # the largest the op-level / bf16-switch tests fed these kernels before: one patch per workgroup
COUT = 64
PATCH = {False: (32, 8), True: (16, 8)}           # (width, height) in pixels: fp32 kernel / bf16-pipe kernel
SLAB_FLOATS_PER_SPLIT = 64 * 32 + 64              # workspace layout: [nsplit][64 co][32 j] partial tiles, then [nsplit][64] bias partials
# the table above, as the CPU test asserts it: shape -> bf16_dy -> (npatches, per_split, nsplit, tail, first split spanning two images | None)
TABLE = {
    (3, 51, 600): {False: (399, 2, 200, 1, 66), True: (798, 1, 798, 1, None)},
    (3, 67, 616): {False: (540, 3, 180, 3, None), True: (1053, 2, 527, 1, 175)},
    (4, 115, 600): {False: (1140, 5, 228, 5, None), True: (2280, 3, 760, 3, None)},
}


# ---- plan arithmetic on the dict ops.wgrad_c3_plan returns ---------------------------------------------------------------------------
def tail(plan):
    """patches of the last split"""
    return plan["npatches"] - (plan["nsplit"] - 1) * plan["per_split"]


def spanning_splits(plan):
    """splits whose patch range holds patches of two images (patches are numbered x fastest, then y, then image)"""
    per_image = plan["npx"] * plan["npy"]
    out = []
    for s in range(plan["nsplit"]):
        first = s * plan["per_split"]
        last = min(first + plan["per_split"], plan["npatches"]) - 1
        if first // per_image != last // per_image:
            out.append(s)
    return out


def ws_bytes_needed(plan_f32, plan_bf16):
    """what the two kernels write at most, rounded like the library's size queries (256 bytes)"""
    need = max(plan_f32["nsplit"], plan_bf16["nsplit"]) * SLAB_FLOATS_PER_SPLIT * 4
    return (need + 255) // 256 * 256


# ---- operands (CPU, NCHW fp32) -------------------------------------------------------------------------------------------------------
def integer_operands(shape, cout=COUT, seed=0):
    """x: integers in [-3, 3] (3 channels), dy: integers in {-1, 0, 1}; exact in bf16 and fp32, and every partial sum of the weight
    gradient stays below 3 N H W < 2^24, so ANY summation order is exact in fp32.  dy of a smaller cout is the leading channels of the
    cout = 64 draw (one reference serves them all)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 + seed + h)
    x = torch.randint(-3, 4, (n, 3, h, w), generator=g).float()
    dy = torch.randint(-1, 2, (n, COUT, h, w), generator=g).float()
    return x, dy[:, :cout].contiguous()


def random_operands(shape, cout=COUT, seed=0, bf16=False):
    """the recipe of test_wgrad_f32x3: dy = randn * exp(randn) (a gradient's wide range), the image plain randn.  bf16: both rounded to bf16
    (RNE, what `(__bf16)v` does in the kernel), so that a float64 reference of these values sees exactly what the MFMAs see."""
    n, h, w = shape
    g = torch.Generator().manual_seed(2000 + seed + h)
    x = torch.randn(n, 3, h, w, generator=g)
    dy = torch.randn(n, cout, h, w, generator=g) * torch.exp(torch.randn(n, cout, h, w, generator=g))
    if bf16:
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    return x, dy


def x_nhwc8(x):
    """NCHW [N,3,H,W] -> NHWC8 fp32 (channels 3..7 zero: the layout conv1_1's input is stored in)"""
    n, c, h, w = x.shape
    assert c == 3
    out = torch.zeros(n, h, w, 8)
    out[..., :3] = x.permute(0, 2, 3, 1)
    return out


PAD_FILL = 2.0 ** 100       # large, finite, exact in bf16 and fp32: a read of a padding channel cannot hide


def dy_nhwc(dy, cout_s=None, dtype=torch.float32):
    """NCHW [N,cout,H,W] -> NHWC with channel stride cout_s (default dense), padding channels filled with PAD_FILL"""
    n, c, h, w = dy.shape
    cout_s = cout_s or c
    out = torch.full((n, h, w, cout_s), PAD_FILL)
    out[..., :c] = dy.permute(0, 2, 3, 1)
    return out.to(dtype)


# ---- references ----------------------------------------------------------------------------------------------------------------------
def conv_backward(x, dy, dtype):
    """(dW [cout,3,3,3], db [cout]) of a 3x3 / padding 1 convolution by autograd in `dtype`: float64 = the reference, float32 = the CPU
    comparator whose own distance from float64 sets the bar"""
    cout = dy.shape[1]
    w0 = torch.zeros(cout, 3, 3, 3, dtype=dtype, requires_grad=True)
    b0 = torch.zeros(cout, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype), w0, b0, padding=1).backward(dy.to(dtype))
    return w0.grad, b0.grad


@functools.lru_cache(maxsize=None)
def integer_case(shape):
    """(x, dy, dW float64, db float64) with integer operands at cout = 64; computed once per process, callers must not write into them"""
    x, dy = integer_operands(shape)
    return (x, dy) + conv_backward(x, dy, torch.float64)


@functools.lru_cache(maxsize=None)
def random_case(shape, bf16):
    """(x, dy, (dW, db) in float64, (dW, db) of the CPU float32 comparator on the identical values); once per process, read only"""
    x, dy = random_operands(shape, bf16=bf16)
    return x, dy, conv_backward(x, dy, torch.float64), conv_backward(x, dy, torch.float32)


def rel_err(a, b):
    """(max |a - b| / max |b|, ||a - b|| / ||b||) in float64"""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)), float((a - b).norm() / (b.norm() + 1e-30))
