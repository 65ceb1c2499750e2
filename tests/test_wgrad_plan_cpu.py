"""CPU: which kernel every weight gradient of the network gets, and how it cuts the pixels, is pinned.

osvos_wgrad_plan (host only) reports what the weight-gradient launchers decide for a call -- family, kernel row, patches, splits, channel
tiles, grid, block order, reduce, slab sizes -- through the code the launches themselves go through.  tests/golden/wgrad_plans.json holds
that decision for the 17 weight-gradient launches of one backward (13 trunk, 4 side_prep), as osvos_net_backward's `wgrad` lambda fills the
call (net.cpp: x bf16 in the bf16-store mode except conv1_1's, dy bf16 in that mode, Cout_s = Cout, the bias gradient wanted), for the six
arithmetics at four frame sizes.  The file was recorded from the launchers as they were BEFORE each family decided in a choose() and launched
from a table (a scratch build whose every launch wrote down kernel, template arguments, grid, workgroup, LDS bytes and kernel arguments
instead of launching), so a rule or constant change shows up here as a diff of the golden file.  Nothing touches a GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "wgrad_plans.json")

F32, BF16MFMA, F32_X3, X3_TWO, X3_HALF = 0, 2, 3, 0x800, 0x1000
X_BF16, DY_BF16, NO_BIAS = 1, 2, 4                               # OSVOS_WGRAD_PLAN_* of include/osvos_hip.h
# mode -> (dtype word, bf16 tensors): the network's precisions, and 'bf16' with OSVOS_BF16_STORE=0 (fp32 tensors, rounded while staged)
MODES = {"fp32": (F32, False), "fp32x3": (F32_X3, False), "fp32x2": (F32_X3 | X3_TWO, False), "fp32h2": (F32_X3 | X3_HALF, False),
         "bf16": (BF16MFMA, True), "bf16_f32tensors": (BF16MFMA, False)}
FRAMES = [(1, 480, 854), (12, 480, 854), (4, 1080, 1920), (2, 37, 53)]
FIELDS = ("family", "kernel", "pw", "ph", "npx", "npy", "npatches", "per_split", "nsplit", "nco_t", "nci_t", "blocks", "map", "reduce",
          "slab_floats", "bslab_floats")
FAM_F32, FAM_C3_F32, FAM_C3_BF16, FAM_CO16_F32, FAM_F32X3, FAM_BF16 = range(6)
RED_T16, RED_T4, RED_GENERIC, RED_OIHW, RED_C3 = range(5)

STAGE_N, STAGE_C = (2, 2, 3, 3, 3), (64, 128, 256, 512, 512)
LAYERS = []                                    # (name, stage, cin, cin_s, cout): net.cpp's conv_table()
for _si, _n in enumerate(STAGE_N):
    for _j in range(_n):
        _cin = 3 if not LAYERS else LAYERS[-1][4]
        LAYERS.append(("conv%d_%d" % (_si + 1, _j + 1), _si, _cin, 8 if _cin == 3 else _cin, STAGE_C[_si]))
for _i in range(4):
    LAYERS.append(("side_prep%d" % (_i + 2), _i + 1, STAGE_C[_i + 1], STAGE_C[_i + 1], 16))


def network_calls(mode, h, w):
    """[(name, (H, W, Cin, Cin_s, Cout, Cout_s, dtype word, flags))]: the weight-gradient calls of one backward"""
    dtype_word, store = MODES[mode]
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append((hs[-1] + 1) // 2)
        ws.append((ws[-1] + 1) // 2)
    calls = []
    for l, (name, si, cin, cin_s, cout) in enumerate(LAYERS):
        flags = (X_BF16 if store and l != 0 else 0) | (DY_BF16 if store else 0)
        calls.append((name, (hs[si], ws[si], cin, cin_s, cout, cout, dtype_word, flags)))
    return calls


def plan(lib, n, h, w, cin, cin_s, cout, cout_s, dtype_word, flags):
    out = (C.c_int * len(FIELDS))()
    rc = lib.osvos_wgrad_plan(n, h, w, cin, cin_s, cout, cout_s, dtype_word, flags, out)
    assert rc == 0, (rc, lib.osvos_last_error())
    return [int(v) for v in out]


def plan_table(lib):
    """{"mode": {"N x H x W": {"layer": [FIELDS]}}}"""
    return {mode: {"%dx%dx%d" % (n, h, w): {layer: plan(lib, n, *args) for layer, args in network_calls(mode, h, w)} for n, h, w in FRAMES}
            for mode in MODES}


def ws_table(lib):
    """osvos_wgrad_ws_bytes of the same calls"""
    return {mode: {"%dx%dx%d" % (n, h, w): {layer: int(lib.osvos_wgrad_ws_bytes(n, a[0], a[1], a[3], a[4], a[6] & 0xff))
                                           for layer, a in network_calls(mode, h, w)} for n, h, w in FRAMES} for mode in MODES}


def child(expr, **env_extra):
    """`expr` (over `lib` and this module `t`) as JSON, from a fresh process without any tuning variable but env_extra (the launchers cache
    their knobs at first use)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("OSVOS_") or k == "OSVOS_AUTOBUILD"}
    env.update(env_extra)
    code = ("import json, sys; sys.path[:0] = [%r, %r]; from osvos_pytorch_amd import _lib; import test_wgrad_plan_cpu as t; lib = _lib.lib(); "
            "print('RESULT ' + json.dumps(%s))" % (REPO, os.path.join(REPO, "tests"), expr))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


_TABLE = []


def tables():
    """[plan_table, ws_table] of the library, computed once"""
    if not _TABLE:
        _TABLE.append(child("[t.plan_table(lib), t.ws_table(lib)]"))
    return _TABLE[0]


def table():
    return tables()[0]


def named(v):
    return dict(zip(FIELDS, v))


def test_plans_equal_the_recorded_ones():
    got, want = table(), json.load(open(GOLDEN))
    assert sorted(got) == sorted(want) == sorted(MODES)
    for mode in want:
        assert sorted(got[mode]) == sorted(want[mode]) and len(want[mode]) == len(FRAMES), mode
        for frame in want[mode]:
            assert len(want[mode][frame]) == 17 and sorted(got[mode][frame]) == sorted(want[mode][frame]), (mode, frame)
            for layer in want[mode][frame]:
                assert named(got[mode][frame][layer]) == named(want[mode][frame][layer]), (mode, frame, layer)


def test_hand_derived_plans():
    """derived by hand from the rules of the wgrad_*.hip launchers for one 854x480 frame (the last case: a batch of 12)"""
    t = table()
    x3 = {k: named(v) for k, v in t["fp32x3"]["1x480x854"].items()}
    # conv3_2, 256 -> 256 at 120 x 214: 16 x 6 patches (120 = 20 x 6), 14 x 20 = 280 of them; 4 x 4 = 16 channel tiles -> want 256 / 16 = 16 splits
    # of ceil(280 / 16) = 18 patches, 16 splits; 256 workgroups divide among the XCDs; three bf16 pieces, 6-row patches: row 3 * 4 + 1; 16 splits < 32
    # -> the transposing reduce with 4 waves
    p = x3["conv3_2"]
    assert (p["family"], p["pw"], p["ph"], p["npx"], p["npy"], p["npatches"]) == (FAM_F32X3, 16, 6, 14, 20, 280)
    assert (p["nco_t"], p["nci_t"], p["per_split"], p["nsplit"], p["blocks"], p["map"]) == (4, 4, 18, 16, 256, 1)
    assert (p["kernel"], p["reduce"]) == (13, RED_T4)             # wgrad_f32x3_kernel<6,4,0,1,3,0,0>
    assert p["slab_floats"] == 16 * 9 * 256 * 256 and p["bslab_floats"] == 16 * 256
    # conv5_2, 512 -> 512 at 30 x 54: ph 6 (30 <= 32), 4 x 5 = 20 patches; 64 tiles -> want 4, per_split 5, 4 splits, 256 workgroups
    p = x3["conv5_2"]
    assert (p["ph"], p["npx"], p["npy"], p["npatches"], p["nco_t"] * p["nci_t"], p["per_split"], p["nsplit"], p["blocks"], p["map"]) == (6, 4, 5, 20, 64, 5, 4, 256, 1)
    # side_prep of stage 2, 128 -> 16 at 240 x 427: the S16 form, 16 x 4 patches, 27 x 60 = 1620; one 128-cin tile -> want 256, per_split 7, 232
    # splits = 232 workgroups; 1 x 16 <= 1024 reduce workgroups and 232 >= 32 splits -> 16 waves
    p = x3["side_prep2"]
    assert (p["family"], p["kernel"], p["ph"], p["npx"], p["npy"], p["npatches"]) == (FAM_F32X3, 12, 4, 27, 60, 1620)
    assert (p["nco_t"], p["nci_t"], p["per_split"], p["nsplit"], p["blocks"], p["map"], p["reduce"]) == (1, 1, 7, 232, 232, 1, RED_T16)
    # conv1_1 (Cin 3 in 8 padded channels) is no f32x3 shape: conv1_1's exact kernel, 32 x 8 patches, 27 x 60 = 1620, 256 splits wanted -> 7 each
    p = x3["conv1_1"]
    assert (p["family"], p["kernel"], p["pw"], p["ph"], p["npx"], p["npy"], p["npatches"], p["per_split"], p["nsplit"], p["reduce"]) == \
        (FAM_C3_F32, 0, 32, 8, 27, 60, 1620, 7, 232, RED_C3)
    assert all(p["family"] == FAM_F32X3 for k, p in x3.items() if k != "conv1_1")
    # bf16 store, conv1_1: the bf16-pipe kernel, 16 x 8 patches, 54 x 60 = 3240; 1024 splits wanted -> 4 patches each, 810 splits
    p = named(t["bf16"]["1x480x854"]["conv1_1"])
    assert (p["family"], p["kernel"], p["pw"], p["ph"], p["npx"], p["npy"], p["npatches"], p["per_split"], p["nsplit"], p["blocks"], p["reduce"]) == \
        (FAM_C3_BF16, 1, 16, 8, 54, 60, 3240, 4, 810, 810, RED_C3)
    # bf16 store, conv3_2 at batch 12, 256 -> 256 at 120 x 214: 32 x 8 patches, 7 x 15 x 12 = 1260; the 128-cout form: 2 x 4 tiles, want
    # 192 / 8 = 24 splits of ceil(1260 / 24) = 53 patches; 192 workgroups; 4 x 256 reduce workgroups <= 1024 but 24 splits < 32 -> 4 waves
    p = named(t["bf16"]["12x480x854"]["conv3_2"])
    assert (p["family"], p["kernel"], p["pw"], p["ph"], p["npx"], p["npy"], p["npatches"]) == (FAM_BF16, 3, 32, 8, 7, 15, 1260)      # wgrad_bf16pm_kernel<8>
    assert (p["nco_t"], p["nci_t"], p["per_split"], p["nsplit"], p["blocks"], p["map"], p["reduce"]) == (2, 4, 53, 24, 192, 1, RED_T4)
    # the pieces of an f32x3 launch change the kernel row and nothing else
    for frame in t["fp32x3"]:
        for layer, v in t["fp32x3"][frame].items():
            v2, vh = t["fp32x2"][frame][layer], t["fp32h2"][frame][layer]
            assert v2[2:] == v[2:] == vh[2:] and v2[0] == v[0] == vh[0], (frame, layer)
            assert (v2[1], vh[1]) == ((v[1] - 3, v[1] - 6) if v[0] == FAM_F32X3 else (v[1], v[1])), (frame, layer)


def test_plan_query_rejects_bad_arguments():
    from osvos_pytorch_amd import _lib
    l, out = _lib.lib(), (C.c_int * len(FIELDS))()
    ok = (1, 16, 16, 64, 64, 64, 64)
    assert l.osvos_wgrad_plan(*ok, F32_X3, 0, out) == 0
    assert l.osvos_wgrad_plan(*ok, F32_X3, 0, None) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_wgrad_plan(0, 16, 16, 64, 64, 64, 64, F32_X3, 0, out) < 0 and b"bad shape" in l.osvos_last_error()        # empty shape
    assert l.osvos_wgrad_plan(*ok, 1, 0, out) < 0 and b"not built" in l.osvos_last_error()
    # a bf16 tensor hands the call to the bf16 family whatever the dtype, and that family takes both operands in one format
    assert l.osvos_wgrad_plan(*ok, F32_X3, X_BF16, out) < 0 and b"x and dy must both be fp32 or both be bf16" in l.osvos_last_error()      # bf16 x with f32x3
    assert l.osvos_wgrad_plan(*ok, BF16MFMA, DY_BF16, out) < 0 and b"x and dy must both be fp32 or both be bf16" in l.osvos_last_error()   # mixed formats, wide layer
    assert l.osvos_wgrad_plan(1, 16, 16, 32, 32, 16, 16, BF16MFMA, DY_BF16, out) < 0 and b"dy (16 channels) must be fp32" in l.osvos_last_error()   # Cout 16 with bf16 dy
    assert l.osvos_wgrad_plan(1, 16, 16, 24, 24, 64, 64, BF16MFMA, X_BF16 | DY_BF16, out) < 0 and b"no bf16-store weight-gradient kernel" in l.osvos_last_error()


def test_workspace_covers_every_pinned_plan():
    plans, ws = tables()
    for mode in plans:
        for frame in plans[mode]:
            for layer, v in plans[mode][frame].items():
                p = named(v)
                assert ws[mode][frame][layer] >= (p["slab_floats"] + p["bslab_floats"]) * 4, (mode, frame, layer)
                assert p["blocks"] == p["nsplit"] * p["nco_t"] * p["nci_t"] and (p["nsplit"] - 1) * p["per_split"] < p["npatches"] <= p["nsplit"] * p["per_split"]


# (variable, value, mode, frame, layer, the fields it governs as they are with it set; every other field stays as recorded unless listed)
OVERRIDES = [
    ("OSVOS_WGRAD_MAP", "0", "fp32x3", "1x480x854", "conv3_2", {"map": 0}),
    ("OSVOS_WGRAD_MAP", "0", "bf16", "12x480x854", "conv3_2", {"map": 0}),
    ("OSVOS_WGRAD_FORM", "0", "bf16", "12x480x854", "conv3_2",      # wgrad_bf16_kernel<1>: 64-cout tiles -> 4 x 4 tiles, want 512 / 16 = 32 splits of 40
     {"kernel": 1, "nco_t": 4, "per_split": 40, "nsplit": 32, "blocks": 512, "reduce": RED_T16, "slab_floats": 32 * 9 * 256 * 256, "bslab_floats": 32 * 256}),
    ("OSVOS_WGRAD_VARIANT", "2", "fp32", "1x480x854", "conv1_2", {"kernel": 7}),                   # <2,2,0,1,1>
    ("OSVOS_WGRAD_VARIANT", "13", "fp32", "1x480x854", "conv1_2", {"reduce": RED_OIHW}),          # bit 3: reference-order slabs; & 7 = 5: the default row
    ("OSVOS_WGRAD_PW", "32", "fp32", "1x480x854", "conv4_2",        # 107 columns: 16 x 4 patches by default; 32 x 2: 4 x 30 = 120 patches, 64 tiles, 8 splits of 15
     {"kernel": 10, "pw": 32, "ph": 2, "npx": 4, "npy": 30, "npatches": 120, "per_split": 15}),
    ("OSVOS_WGRAD_BLOCKS", "64", "fp32", "1x480x854", "conv1_2",    # one channel tile: 64 splits of ceil(6480 / 64) = 102 patches
     {"per_split": 102, "nsplit": 64, "blocks": 64, "slab_floats": 64 * 9 * 64 * 64, "bslab_floats": 64 * 64}),
    ("OSVOS_WGRAD_GENERIC", "1", "fp32", "1x480x854", "side_prep2", {"family": FAM_F32, "kernel": 1}),      # <1,4,1,0,1>, which cuts this layer as the skinny kernel does
    ("OSVOS_WGRAD_REDUCE_T", "0", "fp32x3", "1x480x854", "conv3_2", {"reduce": RED_GENERIC}),
    ("OSVOS_WGRAD_X3_OLDADDR", "1", "fp32x3", "1x480x854", "conv3_2", {"kernel": 4}),             # <6,4,0,1,3,0,1>
    ("OSVOS_WGRAD_X3_OLDADDR", "1", "fp32h2", "1x480x854", "conv3_2", {}),                        # (bf16 pieces only)
    ("OSVOS_WGRAD_DBG", "1", "bf16", "12x480x854", "conv3_2", {}),                                # probe builds only: no plan field
]


@pytest.mark.parametrize("var,value,mode,frame,layer,changed", OVERRIDES, ids=["%s=%s-%s" % (o[0], o[1], o[2]) for o in OVERRIDES])
def test_environment_overrides(var, value, mode, frame, layer, changed):
    n, h, w = (int(v) for v in frame.split("x"))
    got = named(child("t.plan(lib, %d, *dict(t.network_calls(%r, %d, %d))[%r])" % (n, mode, h, w, layer), **{var: value}))
    want = named(json.load(open(GOLDEN))[mode][frame][layer])
    assert all(want[k] != v for k, v in changed.items()), "the override must change what it governs"
    want.update(changed)
    assert got == want
