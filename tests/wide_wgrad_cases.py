"""TEST INFRASTRUCTURE: kinds, shapes, operands and references for the WIDE 3x3 weight gradients on the matrix pipe -- wgrad_f32x3_kernel
(csrc/wgrad_f32x3.hip: three-piece, two-piece, FP16-pair "h2" and the skinny S16 forms) and wgrad_bf16_kernel / wgrad_bf16pm_kernel<4|8>
(csrc/wgrad_bf16.hip) -- shared by test_wide_wgrad_cases_cpu.py (which pins, through the library's own plan query osvos_wgrad_wide_plan,
the regime each shape reaches) and test_gpu_wide_wgrad.py.

Every op-level shape these kernels were fed before gives per_split <= 3 with a full last split; the shapes below are the smallest found
that reach, per family: a walk of >= 4 patches per workgroup (the next patch prefetched from inside the k-loop, the dead prefetch behind the
last one), a last split shorter than the others, a split that crosses from one image into the next, both patch heights of f32x3, partial
last patch columns and rows, both arms of the block map, several cout and cin tiles, and more than 64 splits (the reduce's second trip).
Plans as the library reports them (TABLE, asserted by the CPU test):

    f32x3 (16 x ph pixel patches)  ph  patches per_split nsplit tail  first spanning split  workgroups  map
    2,18,40,512,512                6   18      5         4      3     1                     256         1
    2,19,215,128,128               4   140     3         47     2     23                    188         0
    3,30,70,256,256                6   75      5         15     5     -                     240         1
    2,3,2380,64,128                4   298     3         100    1     49                    200         1
    2,19,215,512,16 (S16)          4   140     3         47     2     23                    188         0

    bf16 (32 x 8 pixel patches)    fp32 tensors, wgrad_bf16_kernel<0>                | bf16 tensors, wgrad_bf16pm_kernel<4 | 8>
    3,17,65,512,512                27 / 4 / 7 / tail 3 / spans 2 / 448 wg / map 1    | <8>: 27 / 5 / 6 / tail 2 / spans 1 / 192 wg / map 1
    3,9,195,512,448                42 / 5 / 9 / tail 2 / spans 2 / 504 wg / map 1    | <4>: the same plan
    3,21,150,128,64                45 / 3 / 15 / tail 3 / - / 30 wg / map 0          | <4>: the same plan
    3,2,1380,128,128               132 / 2 / 66 / tail 2 / - / 264 wg / map 1        | <8>: 132 / 2 / 66 / tail 2 / - / 132 wg / map 0
    3,21,150,128,16                (Cout 16 on fp32 tensors is the skinny kernel's)  | <4>, 16 live rows: 45 / 3 / 15 / tail 3 / - / 30 wg / map 0

Nothing here touches a GPU."""
import functools

import torch
import torch.nn.functional as F

from conv1_1_wgrad_cases import PAD_FILL, dy_nhwc, rel_err, spanning_splits, tail      # noqa: F401  (re-exported: one set of helpers)

# ---- kinds: one way to run the layer at op level ---------------------------------------------------------------------------------------
# name -> (family, entry, x3 pieces | None, tensors)
KINDS = {
    "x3": ("x3", "wgrad", 3, torch.float32),                 # wgrad_f32x3_kernel<ph,4,0,1,3>
    "x3b2": ("x3", "wgrad", 2, torch.float32),               # ... NP = 2
    "x3h2": ("x3", "wgrad", 22, torch.float32),              # ... NP = 2, HP = 1
    "x3_s16": ("x3", "wgrad", 3, torch.float32),             # the S16 forms: Cout 16, Cin % 128 == 0
    "x3b2_s16": ("x3", "wgrad", 2, torch.float32),
    "x3h2_s16": ("x3", "wgrad", 22, torch.float32),
    "bf16_f32t": ("bf16", "wgrad", None, torch.float32),     # wgrad_bf16_kernel<0>
    "bf16_act": ("bf16", "bf16act", None, torch.bfloat16),   # wgrad_bf16pm_kernel<4> (Cout % 128 != 0) / <8>
    "bf16_act16": ("bf16", "bf16act", None, torch.bfloat16),  # the 64-cout tile with 16 live rows
}
X3_KINDS, S16_KINDS, BF16_KINDS = ["x3", "x3b2", "x3h2"], ["x3_s16", "x3b2_s16", "x3h2_s16"], ["bf16_f32t", "bf16_act"]


def kinds_for(shape):
    """every kind that takes a (N, H, W, Cin, Cout) shape"""
    cin, cout = shape[3], shape[4]
    if cout == 16:
        return (S16_KINDS if cin % 128 == 0 else []) + ["bf16_act16"]
    return X3_KINDS + BF16_KINDS


def is_bf16_kind(kind):
    return KINDS[kind][0] == "bf16"


def plan(shape, kind):
    """what the launcher of `kind` does with the shape: the dict of ops.wgrad_wide_plan (host only)"""
    from osvos_pytorch_amd import ops
    from osvos_pytorch_amd._lib import F32_BF16MFMA, F32_X3
    family, _, _, tensors = KINDS[kind]
    return ops.wgrad_wide_plan(*shape, F32_X3 if family == "x3" else F32_BF16MFMA, tensors == torch.bfloat16)


def own_ws_bytes(shape, p):
    """the kernel's own slabs [nsplit][9][Cout][Cin_s] and bias partials [nsplit][Cout], fp32, from the front of the workspace"""
    return p["nsplit"] * (9 * shape[4] * shape[3] + shape[4]) * 4


# ---- shapes (N, H, W, Cin, Cout) -------------------------------------------------------------------------------------------------------
X3_LONG = [(2, 18, 40, 512, 512), (2, 19, 215, 128, 128), (3, 30, 70, 256, 256)]
X3_MANY_SPLITS = (2, 3, 2380, 64, 128)                   # nsplit 100: the shared reduce's second trip (too many pixels for the scaled operands)
S16_LONG = (2, 19, 215, 512, 16)
BF16_LONG = [(3, 17, 65, 512, 512), (3, 9, 195, 512, 448), (3, 21, 150, 128, 64)]
BF16_MANY_SPLITS = (3, 2, 1380, 128, 128)
ACT16_LONG = (3, 21, 150, 128, 16)
# where each kind is held to its long walks: the f32x3 kinds on the f32x3 shapes, the bf16 kinds on theirs
LONG = ([(s, k) for s in X3_LONG + [X3_MANY_SPLITS] for k in X3_KINDS] + [(S16_LONG, k) for k in S16_KINDS]
        + [(s, k) for s in BF16_LONG + [BF16_MANY_SPLITS] for k in BF16_KINDS] + [(ACT16_LONG, "bf16_act16")])
# the scaled operands follow the f32x3 kernel's patch geometry: every kind on the f32x3 long-walk shapes
SCALED_SHAPES = X3_LONG + [S16_LONG]
SCALED = [(s, k) for s in SCALED_SHAPES for k in kinds_for(s)]
# max_split clamps to 1 and every load guard is live: one pixel; H < patch height and W < patch width; two one-patch images in one split
TINY_PIXELS = [(1, 1, 1), (1, 3, 5), (2, 4, 16)]
TINY = ([(p + (64, 64), k) for p in TINY_PIXELS for k in X3_KINDS + BF16_KINDS] + [(p + (128, 16), k) for p in TINY_PIXELS for k in S16_KINDS]
        + [(p + (64, 16), "bf16_act16") for p in TINY_PIXELS])
# strided dY: (shape, channel stride of dY); the padding channels hold PAD_FILL
STRIDED = [((2, 19, 215, 128, 128), 136), ((2, 19, 215, 128, 64), 72)]
S16_STRIDED = (S16_LONG, 24)

# the largest shapes the op-level tests fed these kernels before (test_gpu_ops.py), per family: per_split <= 3, full last splits
OLD_X3_SHAPES = [(1, 13, 21, 64, 64), (2, 30, 54, 128, 64), (1, 60, 107, 64, 128), (1, 25, 37, 64, 64), (3, 6, 16, 64, 64), (1, 121, 215, 64, 64),
                 (2, 30, 54, 128, 256), (1, 25, 37, 64, 128), (2, 5, 17, 64, 128),                               # test_wgrad_f32x3
                 (1, 33, 70, 64, 128), (2, 24, 40, 128, 64), (1, 20, 24, 256, 256),                              # ..._two_pieces_per_operand
                 (1, 18, 40, 512, 512), (1, 40, 64, 128, 16)]                                                    # ..._fp16_pairs
OLD_BF16_SHAPES = [(1, 9, 11, 64, 64), (2, 17, 35, 64, 128), (1, 33, 70, 128, 64), (1, 60, 107, 192, 128), (3, 8, 40, 64, 64),   # test_wgrad_bf16_mfma, _bf16act_
                   (2, 30, 54, 256, 256), (1, 60, 107, 128, 256)]                                                # ..._forms_are_bit_identical

# the table of the docstring: (shape, kind) -> (ph, npatches, per_split, nsplit, tail, first spanning split | None, workgroups, map, wide)
TABLE = {
    ((2, 18, 40, 512, 512), "x3"): (6, 18, 5, 4, 3, 1, 256, 1, 0),
    ((2, 19, 215, 128, 128), "x3"): (4, 140, 3, 47, 2, 23, 188, 0, 0),
    ((3, 30, 70, 256, 256), "x3"): (6, 75, 5, 15, 5, None, 240, 1, 0),
    ((2, 3, 2380, 64, 128), "x3"): (4, 298, 3, 100, 1, 49, 200, 1, 0),
    ((2, 19, 215, 512, 16), "x3_s16"): (4, 140, 3, 47, 2, 23, 188, 0, 0),
    ((3, 17, 65, 512, 512), "bf16_f32t"): (8, 27, 4, 7, 3, 2, 448, 1, 0),
    ((3, 17, 65, 512, 512), "bf16_act"): (8, 27, 5, 6, 2, 1, 192, 1, 1),
    ((3, 9, 195, 512, 448), "bf16_f32t"): (8, 42, 5, 9, 2, 2, 504, 1, 0),
    ((3, 9, 195, 512, 448), "bf16_act"): (8, 42, 5, 9, 2, 2, 504, 1, 0),
    ((3, 21, 150, 128, 64), "bf16_f32t"): (8, 45, 3, 15, 3, None, 30, 0, 0),
    ((3, 21, 150, 128, 64), "bf16_act"): (8, 45, 3, 15, 3, None, 30, 0, 0),
    ((3, 2, 1380, 128, 128), "bf16_f32t"): (8, 132, 2, 66, 2, None, 264, 1, 0),
    ((3, 2, 1380, 128, 128), "bf16_act"): (8, 132, 2, 66, 2, None, 132, 0, 1),
    ((3, 21, 150, 128, 16), "bf16_act16"): (8, 45, 3, 15, 3, None, 30, 0, 0),
}


def table_row(p):
    spans = spanning_splits(p)
    return (p["ph"], p["npatches"], p["per_split"], p["nsplit"], tail(p), spans[0] if spans else None, p["blocks"], p["map"], p["wide"])


# ---- operands (CPU, NCHW fp32), drawn at the widest channel counts and sliced ----------------------------------------------------------
CMAX = 512


@functools.lru_cache(maxsize=None)
def _integer_draw(pixels):
    n, h, w = pixels
    g = torch.Generator().manual_seed(3000 + 7 * h + w)
    x = torch.randint(-3, 4, (n, CMAX, h, w), generator=g).float()
    x = x * (torch.rand(n, CMAX, h, w, generator=g) > 0.4)                      # post-ReLU like: about 40 % zeros
    dy = torch.randint(-1, 2, (n, CMAX, h, w), generator=g).float()
    return x, dy


def integer_operands(shape):
    """x: integers in [-3, 3] with about 40 % zeros, dy: integers in {-1, 0, 1} -- exact in bf16, FP16 and fp32, and every partial sum of the
    weight gradient stays below 3 N H W < 2^24, so ANY summation order is exact in fp32.  Narrower tensors are the leading channels of the
    512-channel draw of the same pixels."""
    n, h, w, cin, cout = shape
    x, dy = _integer_draw((n, h, w))
    return x[:, :cin].contiguous(), dy[:, :cout].contiguous()


SCHEDULES = ["rise_dy", "rise_x", "rise_both", "fall", "zeros"]
MAX_EXP_SUM = 8           # max a + max b of every schedule: 3 N H W 2^8 < 2^24 up to 21845 pixels


def patch_index(shape):
    """[N,H,W] long tensors (patch number, position of the patch in its split's walk) in the f32x3 kernel's own geometry: 16 x ph pixel
    patches numbered x fastest, then y, then image; split s walks patches [s per_split, (s + 1) per_split)"""
    n, h, w = shape[:3]
    p = plan(shape, "x3_s16" if shape[4] == 16 else "x3")
    img = torch.arange(n).view(n, 1, 1)
    py = (torch.arange(h) // p["ph"]).view(1, h, 1)
    px = (torch.arange(w) // p["pw"]).view(1, 1, w)
    patch = (img * p["npy"] + py) * p["npx"] + px
    return patch, patch % p["per_split"], p["per_split"]


def schedule_exponents(shape, schedule):
    """(a, b, live): per-pixel exponents of dY's and X's power-of-two scale and the 0 / 1 mask of the pixels kept, [N,H,W] each.
    rise_*: the scale RISES along each split's walk, so the h2 kernel's running block exponent of that operand drops at several patches of one
    split and the nine accumulators are rescaled; fall: it falls, so the exponent is set by the first patch and never changes; zeros: an
    all-zero patch comes first and another sits mid-walk (the "no data seen yet" start and the exponent of a zero maximum), the rest rises."""
    patch, j, per_split = patch_index(shape)
    steps = max(per_split - 1, 1)
    one, both = (MAX_EXP_SUM // steps) * j, (MAX_EXP_SUM // 2 // steps) * j
    zero, live = torch.zeros_like(j), torch.ones_like(j)
    if schedule == "rise_dy":
        return one, zero, live
    if schedule == "rise_x":
        return zero, one, live
    if schedule == "rise_both":
        return both, both, live
    if schedule == "fall":
        return both.max() - both, both.max() - both, live
    assert schedule == "zeros"
    return both, both, ((j != 0) & (j != per_split // 2)).long()


def scaled_operands(shape, schedule):
    """the integer operands with dY times 2^a(p) and X times 2^b(p), p the patch the pixel belongs to.  (X's halo pixels carry the
    neighbouring patch's scale: the kernel takes its maximum over the halo it stages.)"""
    x, dy = integer_operands(shape)
    a, b, live = schedule_exponents(shape, schedule)
    return x * (live * 2.0 ** b).unsqueeze(1).float(), dy * (live * 2.0 ** a).unsqueeze(1).float()


def random_operands(shape, bf16=False):
    """the recipe of test_wgrad_f32x3: dy = randn * exp(randn) (a gradient's wide range), x the same made post-ReLU like.  bf16: both rounded
    to bf16 (RNE), so that a float64 reference of these values sees exactly what the MFMAs see."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(4000 + 7 * h + w + cin)
    x = torch.randn(n, cin, h, w, generator=g) * torch.exp(torch.randn(n, cin, h, w, generator=g))
    x = x * (torch.rand(n, cin, h, w, generator=g) > 0.4)
    dy = torch.randn(n, cout, h, w, generator=g) * torch.exp(torch.randn(n, cout, h, w, generator=g))
    if bf16:
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    return x, dy


def x_nhwc(x, dtype=torch.float32):
    """NCHW -> dense NHWC (the wide kernels take Cin == Cin_s only)"""
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


# ---- references ------------------------------------------------------------------------------------------------------------------------
def conv_backward(x, dy, dtype):
    """(dW [cout,cin,3,3], db [cout]) of a 3x3 / padding 1 convolution by autograd in `dtype`: float64 = the reference, float32 = the CPU
    comparator whose own distance from float64 sets the bar"""
    cout, cin = dy.shape[1], x.shape[1]
    w0 = torch.zeros(cout, cin, 3, 3, dtype=dtype, requires_grad=True)
    b0 = torch.zeros(cout, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype), w0, b0, padding=1).backward(dy.to(dtype))
    return w0.grad, b0.grad


@functools.lru_cache(maxsize=None)
def integer_case(shape):
    """(x, dy, dW float64, db float64); computed once per process, callers must not write into them"""
    x, dy = integer_operands(shape)
    return (x, dy) + conv_backward(x, dy, torch.float64)


@functools.lru_cache(maxsize=None)
def scaled_case(shape, schedule):
    x, dy = scaled_operands(shape, schedule)
    return (x, dy) + conv_backward(x, dy, torch.float64)


@functools.lru_cache(maxsize=None)
def random_case(shape, bf16):
    """(x, dy, (dW, db) in float64, (dW, db) of the CPU float32 comparator on the identical values); once per process, read only"""
    x, dy = random_operands(shape, bf16)
    return x, dy, conv_backward(x, dy, torch.float64), conv_backward(x, dy, torch.float32)
