"""CPU: tests/head_cases.py -- the float64 head reference the GPU tests of tests/test_gpu_head_in_net.py compare the device with -- against the
oracle it is built on (oracle/torch_ref.py forward, bit for bit), against a naive loop restatement of transposed convolution + centre crop,
against finite differences of that restatement, and the grid-stride arithmetic of `wrap_facts` against the constants in the sources."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as hc
from oracle import synth, torch_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_preps(p, x):
    """the four side_prep outputs of torch_ref.forward, recomputed layer by layer (as test_intermediate_activations_via_ws_query does)"""
    preps, cur = [], x
    for si, names in enumerate(torch_ref.trunk_conv_names()):
        if si > 0:
            cur = F.max_pool2d(cur, 2, 2, ceil_mode=True)
        for nm in names:
            cur = F.relu(F.conv2d(cur, p[nm + ".weight"], p[nm + ".bias"], padding=1))
        if si > 0:
            preps.append(F.conv2d(cur, p["side_prep.%d.weight" % (si - 1)], p["side_prep.%d.bias" % (si - 1)], padding=1))
    return preps


@pytest.mark.parametrize("kind", ["diagonal", "dense"])
@pytest.mark.parametrize("shape", [(1, 9, 7), (2, 37, 53)])
def test_head_reference_reproduces_the_oracle_forward_bit_for_bit(shape, kind):
    n, h, w = shape
    wts = hc.apply_weight_kind(synth.make_weights(1), kind)
    x = torch.from_numpy(synth.make_frame(n, h, w, 3)).double()
    p = torch_ref.as_leaf_params(wts, dtype=torch.float64, requires_grad=False)
    with torch.no_grad():
        want = torch_ref.forward(p, x)
        preps = _oracle_preps(p, x)
    assert [tuple(t.shape[2:]) for t in preps] == hc.side_sizes(h, w)
    outs, dpreps, grads = hc.head_reference([t.clone().requires_grad_() for t in preps], hc.head_params(wts), h, w, [None] * 5)
    for i in range(5):
        assert outs[i].dtype == torch.float64 and torch.equal(outs[i], want[i]), (shape, kind, i)
    assert all(g is None for g in dpreps) and all(g is None for g in grads.values())      # no head used: nothing flows


def _random_case(shape, kind, seed):
    n, h, w = shape
    rng = np.random.RandomState(seed)
    wts = hc.apply_weight_kind(synth.make_weights(1), kind)
    for i in range(4):
        wts["score_dsn.%d.bias" % i] = rng.randn(1).astype(np.float32)
    wts["fuse.bias"] = rng.randn(1).astype(np.float32)
    preps = [rng.randn(n, 16, hh, ww) for hh, ww in hc.side_sizes(h, w)]
    return wts, preps


@pytest.mark.parametrize("kind", hc.WEIGHT_KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 3), (1, 9, 7)])
def test_head_reference_equals_the_naive_loops(shape, kind):
    n, h, w = shape
    wts, preps = _random_case(shape, kind, 11)
    outs, _, _ = hc.head_reference([torch.from_numpy(t).requires_grad_() for t in preps], hc.head_params(wts), h, w, [None] * 5)
    want = hc.naive_head(preps, {k: np.asarray(wts[k], np.float64) for k in hc.HEAD_PARAM_NAMES}, h, w)
    for i in range(5):
        assert outs[i].shape == (n, 1, h, w)
        assert np.abs(outs[i].numpy() - want[i]).max() <= 1e-12 * max(1.0, np.abs(want[i]).max()), (shape, kind, i)


@pytest.mark.parametrize("shape,kind,upstream", [((1, 2, 3), "dense", u) for u in hc.UPSTREAM] +
                         [((1, 9, 7), "perchannel", "all"), ((1, 9, 7), "dense", "side1_and_fused"), ((1, 1, 1), "diagonal", "sides_only")])
def test_head_reference_gradients_equal_finite_differences_of_the_naive_loops(shape, kind, upstream):
    """L = sum over the used heads of <out_j, dout_j> is linear in every single coordinate of every prep and parameter, so a central difference
    of the naive restatement is exact up to rounding, with any step"""
    n, h, w = shape
    wts, preps = _random_case(shape, kind, 12)
    douts = hc.upstream_gradients(upstream, n, h, w, 77)
    params = hc.head_params(wts)
    _, dpreps, grads = hc.head_reference([torch.from_numpy(t).requires_grad_() for t in preps], params, h, w, douts)
    npar = {k: np.asarray(wts[k], np.float64) for k in hc.HEAD_PARAM_NAMES}

    def loss():
        outs = hc.naive_head(preps, npar, h, w)
        return sum(float((outs[j] * douts[j].double().numpy()).sum()) for j in range(5) if douts[j] is not None)

    rng = np.random.RandomState(3)
    tensors = [("prep%d" % i, preps[i], dpreps[i]) for i in range(4)] + [(k, npar[k], grads[k]) for k in hc.HEAD_PARAM_NAMES]
    scale = abs(loss()) + 1.0
    for name, arr, g in tensors:
        flat = arr.reshape(-1)
        for idx in rng.choice(flat.size, size=min(3, flat.size), replace=False):
            keep = flat[idx]
            flat[idx] = keep + 0.5
            up = loss()
            flat[idx] = keep - 0.5
            dn = loss()
            flat[idx] = keep
            fd = up - dn
            got = 0.0 if g is None else float(g.reshape(-1)[idx])
            assert abs(fd - got) <= 1e-9 * (scale + abs(fd)), (name, int(idx), fd, got)      # (g None: no used head reaches it, fd is 0)


def test_a_head_without_upstream_gradient_contributes_nothing():
    n, h, w = 1, 9, 7
    wts, preps = _random_case((n, h, w), "dense", 13)
    params = hc.head_params(wts)
    leaves = [torch.from_numpy(t).requires_grad_() for t in preps]
    _, _, g = hc.head_reference(leaves, params, h, w, hc.upstream_gradients("fused_only", n, h, w, 5))
    assert all(g[k] is None for k in g if k.startswith(("upscale_.", "score_dsn.")))
    assert all(g[k] is not None for k in g if k.startswith(("upscale.", "fuse.")))
    _, _, g = hc.head_reference(leaves, params, h, w, hc.upstream_gradients("side1_and_fused", n, h, w, 5))
    assert [g["upscale_.%d.weight" % i] is None for i in range(4)] == [True, False, True, True]
    assert [g["score_dsn.%d.bias" % i] is None for i in range(4)] == [True, False, True, True]
    _, _, g = hc.head_reference(leaves, params, h, w, hc.upstream_gradients("sides_only", n, h, w, 5))
    assert all(g[k] is None for k in g if k.startswith(("upscale.", "fuse.")))


def test_weight_kinds_are_what_they_claim():
    base = synth.make_weights(1)
    for i in range(4):
        k = 4 << i
        d, e, p = (hc.apply_weight_kind(base, kind)["upscale.%d.weight" % i] for kind in hc.WEIGHT_KINDS)
        assert np.array_equal(d, base["upscale.%d.weight" % i]) and d.shape == (16, 16, k, k)
        off = ~np.eye(16, dtype=bool)
        assert (np.abs(e[off]) > 0).all()
        assert (p[off] == 0).all() and all(not np.array_equal(p[c, c], p[0, 0]) for c in range(1, 16))


def test_wrap_facts_at_the_wrap_shape_and_at_the_small_ones():
    facts = hc.wrap_facts(*hc.WRAP)
    assert facts[("upsample_generic", None)]
    for i in range(4):
        assert facts[("tapsum", i)] and facts[("bwd", i)], i
        assert not facts[("lowres", i)], i                  # (its own op-level case: test_head_lowres_past_its_grid)
    for shape in hc.SMALL:
        assert not any(hc.wrap_facts(*shape).values()), shape
    n, h, w = hc.WRAP
    assert n * h * w == 1052660 and [n * a * b for a, b in hc.side_sizes(h, w)] == [264192, 66048, 16640, 4224]
    assert not any(hc.wrap_facts(1, 725, 725)[("lowres", i)] for i in range(4))      # (725 x 725 is the PREP size of that case, not a frame size)
    assert 725 * 725 > hc.LOWRES_CAP * hc.THREADS


def test_wrap_thresholds_follow_the_constants_in_the_sources():
    """OSVOS_HEAD_MAX_BLOCKS parsed from the header; the literals of the launchers where head_cases.py says they are.  If one of them
    changes, WRAP has to be revisited."""
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    (mb,) = re.findall(r"#define OSVOS_HEAD_MAX_BLOCKS (\d+)", hdr)
    assert int(mb) == hc.HEAD_MAX_BLOCKS
    n, h, w = hc.WRAP
    for i, (hh, ww) in enumerate(hc.side_sizes(h, w)):
        assert hc.wrap_facts(n, h, w, int(mb))[("bwd", i)] == (n * hh * ww * hc.BWD_TPP[i] > int(mb) * 256)
        assert n * hh * ww * hc.BWD_TPP[i] <= 2 * int(mb) * 256      # exactly two trips: the second one is partial
    csrc = os.path.join(REPO, "osvos-pytorch_amd", "csrc")
    head = open(os.path.join(csrc, "head.hip")).read()
    gen = open(os.path.join(csrc, "head_generic.hip")).read()
    assert "grid_for((long)N * H * W, %d)" % hc.UPSAMPLE_GENERIC_CAP in gen
    assert "kk >= 1024 ? %d : (kk >= 256 ? %d : (kk >= 64 ? %d : %d))" % tuple(reversed(hc.TAPSUM_CAPS)) in gen
    assert "grid_for(npix, %d)" % hc.LOWRES_CAP in head
    assert "const int tpp[4] = {%s};" % ", ".join(str(t) for t in hc.BWD_TPP) in head
    assert "grid_for(npix * tpp[scale_idx], OSVOS_HEAD_MAX_BLOCKS)" in head
