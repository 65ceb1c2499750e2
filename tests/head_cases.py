"""The side-output / fuse head (reference networks/vgg_osvos.py:68-72) as a float64 function of the four 16-channel side_prep maps, shared by
tests/test_head_cases_cpu.py and tests/test_gpu_head_in_net.py.

The head is the only exactly linear part of the network: score_dsn, two transposed convolutions per scale, centre crop, cat and fuse.  Given the
side_prep maps a device run produced, every head output -- and, for chosen upstream gradients, every head gradient -- is a closed-form float64
computation with no ReLU or arg-max decision in it, so it can be held to 1e-5 inside the network.  Pure torch / numpy, no device code.

`wrap_facts` restates which grid-stride loop of csrc/head.hip and csrc/head_generic.hip takes a second trip at a shape; the constants it uses:
  OSVOS_HEAD_MAX_BLOCKS = 1024 .......... include/osvos_hip.h:314   (head_bwd_f32 / head_bwd4_f32 / head_bwd_generic: osvos_head_bwd_blocks)
  lanes per low-resolution pixel 1/4/16/64  csrc/head.hip:301        (tpp[] of osvos_head_bwd_blocks)
  4096 workgroups ....................... csrc/head_generic.hip:256 (head_upsample_generic_kernel)
  128 / 32 / 8 / 2 chunks per tap ....... csrc/head_generic.hip:290 (head_tapsum_kernel, scales 0..3)
  2048 workgroups ....................... csrc/head.hip:274         (head_lowres_f32_kernel)
all with 256 threads per workgroup."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref

N_SCALES = torch_ref.N_SCALES
SIDE_CH = torch_ref.SIDE_CH

SMALL = [(1, 1, 1), (1, 2, 3), (2, 37, 53), (3, 33, 41), (1, 30, 85), (1, 48, 64)]
WRAP = (4, 515, 511)
UPSTREAM = ["all", "fused_only", "sides_only", "side1_and_fused"]
WEIGHT_KINDS = ["diagonal", "dense", "perchannel"]
GENERIC = {"diagonal": False, "dense": True, "perchannel": True}      # which head the weight kind demands

HEAD_PARAM_NAMES = (["upscale.%d.weight" % i for i in range(N_SCALES)] + ["upscale_.%d.weight" % i for i in range(N_SCALES)] +
                    [n % i for i in range(N_SCALES) for n in ("score_dsn.%d.weight", "score_dsn.%d.bias")] + ["fuse.weight", "fuse.bias"])

THREADS = 256
HEAD_MAX_BLOCKS = 1024                  # include/osvos_hip.h:314
BWD_TPP = (1, 4, 16, 64)                # csrc/head.hip:301
UPSAMPLE_GENERIC_CAP = 4096             # csrc/head_generic.hip:256
TAPSUM_CAPS = (128, 32, 8, 2)           # csrc/head_generic.hip:290
LOWRES_CAP = 2048                       # csrc/head.hip:274


def side_sizes(H, W):
    """(h_i, w_i) of the four side_prep maps: ceil-mode 2x2 pooling, once more per scale (vgg_osvos.py:136-145)"""
    out, h, w = [], H, W
    for _ in range(N_SCALES):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def wrap_facts(N, H, W, max_blocks=HEAD_MAX_BLOCKS):
    """{(kernel, scale): does its grid-stride loop take a second trip at [N, H, W]}.  kernel: 'upsample_generic' (scale None), 'tapsum',
    'bwd' (head_bwd_body of the fast head and head_bwd_generic_kernel share osvos_head_bwd_blocks), 'lowres'."""
    facts = OrderedDict()
    facts[("upsample_generic", None)] = N * H * W > UPSAMPLE_GENERIC_CAP * THREADS
    for i, (h, w) in enumerate(side_sizes(H, W)):
        npix = N * h * w
        facts[("tapsum", i)] = npix > TAPSUM_CAPS[i] * THREADS
        facts[("bwd", i)] = npix * BWD_TPP[i] > max_blocks * THREADS
        facts[("lowres", i)] = npix > LOWRES_CAP * THREADS
    return facts


# ------------------------------------------------------------------------------------------------------------------- weight generators

def diagonal_deconv(k):
    """what interp_surgery writes (osvos_layers.py:72-85): [16,16,k,k], block [c][c] the bilinear filter, zero elsewhere"""
    w = np.zeros((SIDE_CH, SIDE_CH, k, k), np.float32)
    f = torch_ref.bilinear_filter(k).astype(np.float32)
    for c in range(SIDE_CH):
        w[c, c] = f
    return w


def apply_weight_kind(wts, kind):
    """A copy of the state dict `wts` (numpy float32; deconvs as oracle.synth.make_weights leaves them) with the deconv weights of `kind`:
    'diagonal'   -- interp_surgery's: the fast, commuted head;
    'dense'      -- the perturbation of test_generic_transposed_conv_head_matches_the_reference_semantics: every tap of every block non-zero;
    'perchannel' -- diagonal, but every channel with a filter of its own: no off-diagonal tap, yet not ONE shared filter -> generic head."""
    out = OrderedDict((k, np.array(v, copy=True)) for k, v in wts.items())
    rng = np.random.RandomState(5)
    for i in range(N_SCALES):
        k = 4 << i
        if kind == "diagonal":
            out["upscale.%d.weight" % i] = diagonal_deconv(k)
            continue
        if kind == "dense":
            out["upscale.%d.weight" % i] = (diagonal_deconv(k) + rng.randn(16, 16, k, k).astype(np.float32) * (0.5 / k)).astype(np.float32)
        elif kind == "perchannel":
            w = diagonal_deconv(k)
            for c in range(SIDE_CH):
                w[c, c] = (w[c, c] * (1.0 + 0.3 * rng.randn(k, k))).astype(np.float32)
            out["upscale.%d.weight" % i] = w
        else:
            raise ValueError(kind)
        out["upscale_.%d.weight" % i] = (out["upscale_.%d.weight" % i] * (1.0 + 0.3 * rng.randn(1, 1, k, k))).astype(np.float32)
    return out


def upstream_gradients(name, N, H, W, seed):
    """five [N,1,H,W] float32 tensors or None, seeded randn: which heads the backward starts from"""
    use = {"all": [0, 1, 2, 3, 4], "fused_only": [4], "sides_only": [0, 1, 2, 3], "side1_and_fused": [1, 4]}[name]
    g = torch.Generator().manual_seed(seed)
    ds = [torch.randn(N, 1, H, W, generator=g) for _ in range(5)]
    return [ds[j] if j in use else None for j in range(5)]


# ------------------------------------------------------------------------------------------------------------------------ the reference

def head_params(wts, dtype=torch.float64):
    """the head's entries of a state dict as float64 leaves"""
    return torch_ref.as_leaf_params(OrderedDict((k, wts[k]) for k in HEAD_PARAM_NAMES), dtype=dtype)


def head_forward(preps, params, H, W):
    """oracle/torch_ref.py forward(), lines 105-111, from the side_prep maps on"""
    side, side_out = [], []
    for i in range(N_SCALES):
        s = 2 ** (i + 1)
        prep = preps[i]
        up = F.conv_transpose2d(prep, params["upscale.%d.weight" % i], stride=s)
        side.append(torch_ref.crop_to(up, H, W))
        score = F.conv2d(prep, params["score_dsn.%d.weight" % i], params["score_dsn.%d.bias" % i])
        up1 = F.conv_transpose2d(score, params["upscale_.%d.weight" % i], stride=s)
        side_out.append(torch_ref.crop_to(up1, H, W))
    fused = F.conv2d(torch.cat(side, dim=1), params["fuse.weight"], params["fuse.bias"])
    return side_out + [fused]


def head_reference(preps, params, H, W, douts):
    """preps: four [N,16,h_i,w_i] leaves; params: {state_dict name: leaf} of the head; douts: five [N,1,H,W] tensors or None.
    Returns (outs, dpreps, grads): the five outputs (detached), d/dprep_i and {name: gradient} after torch.autograd.backward over the heads whose
    dout is not None -- a head without one contributes nothing; a tensor no used head reaches comes back as None."""
    for t in list(preps) + list(params.values()):
        t.grad = None
    outs = head_forward(preps, params, H, W)
    used = [j for j in range(5) if douts[j] is not None]
    if used:
        torch.autograd.backward([outs[j] for j in used], [douts[j].to(outs[j].dtype) for j in used])
    dpreps = [p.grad for p in preps]
    grads = OrderedDict((k, v.grad) for k, v in params.items())
    return [o.detach() for o in outs], dpreps, grads


# ----------------------------------------------------------------------------------------------- the naive restatement (CPU tests only)

def naive_deconv_crop(x, w, s, H, W):
    """ConvTranspose2d(k = 2s, stride s, no padding) + center_crop (osvos_layers.py:51-56) written out: every input pixel stamps its k x k patch
    into the (h + 1) s x (w + 1) s canvas; floor(excess / 2) rows / columns are dropped at the top / left.  numpy float64, [N,Ci,h,w] x [Ci,Co,k,k]."""
    n, ci, h, wd = x.shape
    co, k = w.shape[1], w.shape[2]
    assert k == 2 * s
    full = np.zeros((n, co, (h - 1) * s + k, (wd - 1) * s + k))
    for b in range(n):
        for y in range(h):
            for xx in range(wd):
                for c in range(ci):
                    full[b, :, y * s:y * s + k, xx * s:xx * s + k] += x[b, c, y, xx] * w[c]
    top, left = (full.shape[2] - H) // 2, (full.shape[3] - W) // 2
    return full[:, :, top:top + H, left:left + W]


def naive_head(preps, params, H, W):
    """the five outputs from numpy float64 arrays, loops only"""
    outs, fused = [], np.zeros((preps[0].shape[0], 1, H, W)) + params["fuse.bias"][0]
    for i in range(N_SCALES):
        s = 2 ** (i + 1)
        p = preps[i]
        score = np.zeros((p.shape[0], 1) + p.shape[2:]) + params["score_dsn.%d.bias" % i][0]
        for c in range(SIDE_CH):
            score[:, 0] += params["score_dsn.%d.weight" % i][0, c, 0, 0] * p[:, c]
        outs.append(naive_deconv_crop(score, params["upscale_.%d.weight" % i], s, H, W))
        side = naive_deconv_crop(p, params["upscale.%d.weight" % i], s, H, W)
        for c in range(SIDE_CH):
            fused[:, 0] += params["fuse.weight"][0, 16 * i + c, 0, 0] * side[:, c]
    return outs + [fused]
