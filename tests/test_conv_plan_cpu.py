"""CPU: which kernel every convolution of the network gets is pinned.

osvos_conv3x3_plan (host only) reports what the convolution launchers decide for a call -- family, tile, block order, K split, stream-K, loop
form, separate pool -- through the code the launches themselves go through.  tests/golden/conv_plans.json holds that decision for the
network's 17 forward convolutions and their 16 data gradients (conv1_1's is the dgrad_c3 kernels', not a convolution launch), as
osvos_net_forward / osvos_net_backward build the calls (net.cpp: formats, sign bits, fused pool, pool codes, partial-sum workspaces, masks),
for the four dtype words the network runs with at four frame sizes.  The file was recorded from the launchers as they were BEFORE their tile
switches became tables (a scratch build that wrote down, in front of every switch, what it was about to launch), so a tile or rule change shows
up here as a diff of the golden file.  Nothing touches a GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "conv_plans.json")

F32, BF16MFMA, F32_X3, W2 = 0, 2, 3, 0x4000
DTYPES = {"F32": F32, "F32_X3": F32_X3, "BF16MFMA": BF16MFMA, "BF16MFMA+W2": BF16MFMA | W2}
FRAMES = [(1, 480, 854), (12, 480, 854), (4, 1080, 1920), (2, 37, 53)]
# OSVOS_PLAN_* of include/osvos_hip.h
X_BF16, Y_BF16, Y_F32, RELU, MASK, MASK_BITS, Y_BITS, POOL, POOL_CODE, PART_WS, SK_WS, WPK3 = [1 << k for k in range(12)]
FIELDS = ("family", "tile", "map", "ksplit", "finalize", "sk_grid", "sk_order", "presplit", "pipe", "pool_after")
FAM_F32, FAM_F32X3, FAM_BF16, FAM_BF16_DMA, FAM_BF16_P64, FAM_BF16_W2 = range(6)

STAGE_N, STAGE_C = (2, 2, 3, 3, 3), (64, 128, 256, 512, 512)
TRUNK = []                                     # (name, stage, cin, cin_s, cout)
for _si, _n in enumerate(STAGE_N):
    for _j in range(_n):
        _cin = 3 if not TRUNK else TRUNK[-1][4]
        TRUNK.append(("conv%d_%d" % (_si + 1, _j + 1), _si, _cin, 8 if _cin == 3 else _cin, STAGE_C[_si]))


def _first(l):
    return l == 0 or TRUNK[l - 1][1] != TRUNK[l][1]


def _last(l):
    return l == len(TRUNK) - 1 or TRUNK[l + 1][1] != TRUNK[l][1]


def _has_bits(l, dt):
    """net.cpp use_mask_bits() and act_is_a_mask(): the activation of trunk layer l later masks a data gradient, and its sign bits are kept"""
    is_mask = not _last(l) or l == len(TRUNK) - 1
    if dt == F32_X3:
        return is_mask and l >= 1 and TRUNK[l][1] <= 3
    return is_mask and dt == BF16MFMA


def network_calls(dtype_word, h, w, infer=False, streamk=False):
    """[(name, (H, W, Cin, Cout, y_cs, dtype word, flags))]: the calls of one training step, as net.cpp's conv_of() and its callers fill them.
    infer: the 17 forward calls as osvos_net_forward fills them under OSVOS_FLAG_INFERENCE -- no sign bits, no pool codes, and no partial-sum
    workspace for a layer whose training call carries sign bits (the data gradients are the training step's: no inference call builds them).
    streamk: the main-stream forward convolutions also carry the stream-K workspace, as under OSVOS_X3_STREAMK >= 1 (f32x3 only)"""
    dt = dtype_word & 0xff
    store, x3 = dt == BF16MFMA, dt == F32_X3
    act = (X_BF16, Y_BF16) if store else (0, Y_F32)             # a trunk tensor as an operand / as a result
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append((hs[-1] + 1) // 2)
        ws.append((ws[-1] + 1) // 2)
    calls = []
    for l, (name, si, cin, cin_s, cout) in enumerate(TRUNK):    # forward trunk
        f = act[0] | act[1] | RELU
        if x3 and cin == cin_s:
            f |= WPK3
        if _has_bits(l, dt) and not infer:
            f |= Y_BITS
        if not (_has_bits(l, dt) and infer):
            f |= PART_WS
        if (x3 or store) and si < 4 and _last(l):
            f |= POOL | (POOL_CODE if store and not infer else 0)
        if streamk and x3:
            f |= SK_WS
        calls.append((name, (hs[si], ws[si], cin_s, cout, cout, dtype_word, f)))
    for i in range(4):                                          # forward side branches: fp32 result, cut along K from 256 channels
        c = STAGE_C[i + 1]
        f = act[0] | Y_F32 | (PART_WS if c >= 256 else 0) | (WPK3 if x3 else 0)
        calls.append(("side_prep%d" % (i + 2), (hs[i + 1], ws[i + 1], c, 16, 16, dtype_word, f)))
    bwd = dtype_word & ~W2                                      # the data gradients of 'bf16w2' read single-piece packs
    for i in range(4):                                          # side branches' data gradients: dprep (fp32 + a bf16 copy in the store mode) -> C channels
        c = STAGE_C[i + 1]
        f = act[0] | act[1] | (WPK3 if x3 else 0)
        if i == 3:                                              # stage 5 has no pool behind it: masked by conv5_3's activation right here
            f |= MASK | (MASK_BITS if _has_bits(len(TRUNK) - 1, dt) else 0)
        calls.append(("side_prep%d.dgrad" % (i + 2), (hs[i + 1], ws[i + 1], 16, c, c, bwd, f)))
    for l in range(len(TRUNK) - 1, 0, -1):                      # trunk data gradients (conv1_1's: dgrad_c3.hip, no convolution launch)
        name, si, cin, cin_s, cout = TRUNK[l]
        f = act[0] | act[1] | PART_WS | (WPK3 if x3 else 0)
        if not _first(l):                                       # (first of a stage: through the pool, masked there)
            f |= MASK | (MASK_BITS if _has_bits(l - 1, dt) else 0)
        calls.append((name + ".dgrad", (hs[si], ws[si], cout, cin, cin, bwd, f)))
    return calls


def plan(lib, n, h, w, cin, cout, y_cs, dtype_word, flags, tile=-1, ksplit=0, sk_grid=0):
    out = (C.c_int * len(FIELDS))()
    rc = lib.osvos_conv3x3_plan(n, h, w, cin, cout, y_cs, dtype_word, flags, tile, ksplit, sk_grid, out)
    assert rc == 0, (rc, lib.osvos_last_error())
    return [int(v) for v in out]


def plan_table(lib):
    """{"dtype": {"N x H x W": {"layer": [FIELDS]}}}"""
    return {name: {"%dx%dx%d" % (n, h, w): {layer: plan(lib, n, *args) for layer, args in network_calls(dt, h, w)} for n, h, w in FRAMES}
            for name, dt in DTYPES.items()}


# frames at which a K split is in reach of the f32x3 forward (few tiles per layer), beside FRAMES
SMALL_FRAMES = [(2, 48, 64), (2, 60, 107), (1, 33, 41), (2, 37, 53), (1, 120, 214)]
FORWARD_LAYERS = [t[0] for t in TRUNK] + ["side_prep%d" % (i + 2) for i in range(4)]


def inference_plan_table(lib):
    """{"dtype": {"N x H x W": {"forward layer": [training plan, inference plan, the two with the stream-K workspace]}}}"""
    res = {}
    for name, dt in DTYPES.items():
        for n, h, w in FRAMES + [f for f in SMALL_FRAMES if f not in FRAMES]:
            forms = [dict(network_calls(dt, h, w, infer=infer, streamk=sk)) for sk in (False, True) for infer in (False, True)]
            res.setdefault(name, {})["%dx%dx%d" % (n, h, w)] = {layer: [plan(lib, n, *f[layer]) for f in forms] for layer in FORWARD_LAYERS}
    return res


_TABLE = {}


def _fresh(what):
    """`what`(the library), from a fresh process without any tuning variable (the launchers cache them at first use)"""
    if what not in _TABLE:
        env = {k: v for k, v in os.environ.items() if not k.startswith("OSVOS_") or k == "OSVOS_AUTOBUILD"}
        code = ("import json, sys; sys.path[:0] = [%r, %r]; from osvos_pytorch_amd import _lib; import test_conv_plan_cpu as t; "
                "print('PLANS ' + json.dumps(t.%s(_lib.lib())))" % (REPO, os.path.join(REPO, "tests"), what))
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, out.stderr[-2000:]
        _TABLE[what] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("PLANS ")][-1][6:])
    return _TABLE[what]


def table():
    return _fresh("plan_table")


def test_inference_forward_plans_the_launches_of_the_training_forward():
    """OSVOS_FLAG_INFERENCE promises the training forward's logits bit for bit (include/osvos_hip.h), so every one of its 17 convolutions must
    get the training forward's launch: family, tile, block order, K split, finalize, stream-K grid and order, loop form, separate pool.  The
    f32x3 launcher never cuts a launch that writes sign bits along K; an inference call that merely drops the bits but keeps the partial-sum
    workspace is cut -- conv3_2 / conv4_1 / conv4_2 in 4 / 4 / 8 with a finalize launch at 2x48x64, 2x60x107, 1x33x41, 2x37x53 and 1x120x214 --
    and sums in another order.  Both sides are planned live; with and without the stream-K workspace (OSVOS_X3_STREAMK)."""
    t = _fresh("inference_plan_table")
    assert sorted(t) == sorted(DTYPES)
    bad = []
    for dt in t:
        assert len(t[dt]) == len(FRAMES) + len(SMALL_FRAMES) - 1, dt      # (2x37x53 is in both lists)
        for frame in t[dt]:
            assert sorted(t[dt][frame]) == sorted(FORWARD_LAYERS) and len(FORWARD_LAYERS) == 17
            for layer, (train, infer, train_sk, infer_sk) in t[dt][frame].items():
                assert len(train) == len(FIELDS) == 10
                if infer != train:
                    bad.append((dt, frame, layer, dict(zip(FIELDS, train)), dict(zip(FIELDS, infer))))
                if infer_sk != train_sk:
                    bad.append((dt, frame, layer, "stream-K", dict(zip(FIELDS, train_sk)), dict(zip(FIELDS, infer_sk))))
    assert not bad, bad


def test_plans_equal_the_recorded_ones():
    got, want = table(), json.load(open(GOLDEN))
    assert sorted(got) == sorted(want) == sorted(DTYPES)
    for dt in want:
        assert sorted(got[dt]) == sorted(want[dt]) and len(want[dt]) == len(FRAMES), dt
        for frame in want[dt]:
            assert len(want[dt][frame]) == 33 and sorted(got[dt][frame]) == sorted(want[dt][frame]), (dt, frame)
            for layer in want[dt][frame]:
                assert dict(zip(FIELDS, got[dt][frame][layer])) == dict(zip(FIELDS, want[dt][frame][layer])), (dt, frame, layer)


def test_hand_derived_plans():
    """derived by hand from the rules of conv3x3_f32x3.hip / conv3x3_f32.hip for one 854x480 frame"""
    t = table()
    x3 = {k: dict(zip(FIELDS, v)) for k, v in t["F32_X3"]["1x480x854"].items()}
    # conv1_1 (8 padded input channels) is no f32x3 shape: the exact kernel
    assert x3["conv1_1"]["family"] == FAM_F32 and all(p["family"] == FAM_F32X3 for k, p in x3.items() if k != "conv1_1")
    # conv1_2, 64 -> 64 on 480 x 854: the 64-cout production tile; 410 k pixels against 27 x 64 padded couts: XCD-local
    assert (x3["conv1_2"]["tile"], x3["conv1_2"]["map"]) == (12, 1)
    # conv4_2, 512 -> 512 on 60 x 107: 32-wide tiles pad 107 pixels by 20 % -> the 16 x 16 tile 14; 4 x 7 x 8 = 224 workgroups >= 200: uncut
    assert (x3["conv4_2"]["tile"], x3["conv4_2"]["map"], x3["conv4_2"]["ksplit"]) == (14, 0, 1)
    # conv5_2, 512 -> 512 on 30 x 54: 4 x 2 x 8 = 64 workgroups -> cut in 4 (256 >= 200), a finalize launch behind it
    assert (x3["conv5_2"]["tile"], x3["conv5_2"]["map"], x3["conv5_2"]["ksplit"], x3["conv5_2"]["finalize"]) == (12, 0, 4, 1)
    # the pre-split packs and the pipelined loop of tiles 10, 12, 14 wherever the family runs
    assert all(p["presplit"] == 1 and p["pipe"] == (p["tile"] in (10, 12, 14)) for p in x3.values() if p["family"] == FAM_F32X3)
    assert all(v[:2] == [FAM_F32, 9] for frame in t["F32"].values() for v in frame.values())      # exact fp32: tile 9 everywhere
    # two-piece forward packs run the two-piece tiles and nothing else; their data gradients are single-piece launches
    w2 = t["BF16MFMA+W2"]["12x480x854"]
    assert all((v[0] == FAM_BF16_W2) == (not k.endswith(".dgrad")) for k, v in w2.items())
    assert all(w2[k] == t["BF16MFMA"]["12x480x854"][k] for k in w2 if k.endswith(".dgrad"))


def test_plan_query_rejects_bad_arguments():
    from osvos_pytorch_amd import _lib
    l, out = _lib.lib(), (C.c_int * len(FIELDS))()
    ok = (1, 16, 16, 64, 64, 64, F32_X3, Y_F32 | RELU)
    assert l.osvos_conv3x3_plan(*ok, -1, 0, 0, out) == 0
    assert l.osvos_conv3x3_plan(*ok, -1, 0, 0, None) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_conv3x3_plan(0, 16, 16, 64, 64, 64, F32_X3, Y_F32, -1, 0, 0, out) < 0 and b"bad shape" in l.osvos_last_error()
    assert l.osvos_conv3x3_plan(*ok[:6], 1, Y_F32, -1, 0, 0, out) < 0 and b"not built" in l.osvos_last_error()
    assert l.osvos_conv3x3_plan(*ok[:6], F32 | W2, Y_F32, -1, 0, 0, out) < 0 and b"OSVOS_FLAG_BF16_W2" in l.osvos_last_error()
    assert l.osvos_conv3x3_plan(*ok, 15, 0, 0, out) < 0 and b"unknown tile config 15" in l.osvos_last_error()      # an exact-fp32 tile id
    assert l.osvos_conv3x3_plan(*ok, 200 + 18, 0, 0, out) < 0 and b"f32x3: unknown tile config 18" in l.osvos_last_error()
    assert l.osvos_conv3x3_plan(*ok[:6], BF16MFMA, Y_F32, 42, 0, 0, out) < 0 and b"two-piece" in l.osvos_last_error()
    # the public tile ids: 200 + t = f32x3 tile t (+100: XCD-local) whatever the dtype; the bf16 family's 30-37 and 38 name its other kernels
    assert plan(l, *ok[:6], F32, Y_F32, tile=200 + 103)[:3] == [FAM_F32X3, 3, 1]
    assert plan(l, *ok[:6], F32_X3, Y_F32, tile=3)[:3] == [FAM_F32, 3, 0]
    assert plan(l, *ok[:6], BF16MFMA, X_BF16 | Y_BF16, tile=35)[:3] == [FAM_BF16_DMA, 5, 0]
    assert plan(l, *ok[:6], BF16MFMA, X_BF16 | Y_BF16 | RELU | POOL, tile=138)[:3] == [FAM_BF16_P64, 1, 2]
    p45 = plan(l, *ok[:6], BF16MFMA | W2, X_BF16 | Y_BF16 | RELU | POOL, tile=45)      # (its waves hold no whole pooling windows)
    assert p45[:2] == [FAM_BF16_W2, 5] and p45[FIELDS.index("pool_after")] == 1
