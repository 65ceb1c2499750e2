"""GPU: the memory bank of appearance matching -- osvos_match_bank_update (csrc/match_bank.hip) against the numpy restatement in
tests/match_bank_cases.py, bit for bit (the rule is integer arithmetic, copies and single fp32 comparisons: every comparison is an equality);
the bank is pre-filled with a known pattern, so that "no other byte changes" is checked, state with a valid non-zero state and ws with
garbage, with a guard band behind it.  Then the unchanged osvos_match_nearest on a bank the update wrote, the wrappers of
osvos_pytorch_amd.match, AppearanceMatcher(memory=..) around a stand-in network, and train_online.py --match-memory."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import match_bank_cases as mb
import match_cases as mc
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE_BYTE = 0xa5
GUARD = 256
FRAME = ("q", "rinv_q", "label_q", "sim")
BANK = ("R", "rinv_r", "label_r", "state")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t.contiguous()).view(np.uint32)


def _bytes_equal(got, want):
    """a tuple of device tensors against a tuple of numpy arrays, byte for byte (NaNs and signed zeros included)"""
    return all(_np(g).dtype == w.dtype and _np(g).shape == w.shape and np.array_equal(_np(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
               for g, w in zip(got, want))


def _update(frames, banks, protected, max_new, tau, margin, fill=GARBAGE_BYTE, ws=None):
    """one osvos_match_bank_update on N = len(frames) frames and banks (dicts of numpy arrays without the leading N) -> the four bank tensors
    [N, ..] after the call; ws is garbage, and the guard band behind osvos_match_bank_ws_bytes is checked"""
    from osvos_pytorch_amd import _lib
    n = len(frames)
    f = [_dev(np.stack([fr[k] for fr in frames])) for k in FRAME]
    b = [_dev(np.stack([bk[k] for bk in banks])) for k in BANK]
    p, c, cap = int(f[0].shape[1]), int(f[0].shape[2]), int(b[0].shape[1])
    need = int(_lib.lib().osvos_match_bank_ws_bytes(n, p))
    assert need > 0
    own = ws is None
    if own:
        ws = torch.full((need + GUARD,), fill, device="cuda", dtype=torch.uint8)
    assert ws.numel() >= need + GUARD
    rc = _lib.lib().osvos_match_bank_update(*(C.c_void_p(t.data_ptr()) for t in f + b), C.c_void_p(ws.data_ptr()), n, p, c, cap, protected, max_new, tau,
                                            margin, _stream())
    _lib.check(rc, "match_bank_update")
    if own:
        assert bool((ws[need:] == fill).all()), "the call wrote past osvos_match_bank_ws_bytes"
    for t, fr_key in zip(f, FRAME):                                       # the frame's arrays are inputs
        assert np.array_equal(_np(t).view(np.uint8), np.stack([fr[fr_key] for fr in frames]).view(np.uint8))
    return b


# ------------------------------------------------------------------------------------------------------------------ the kernels


@pytest.mark.parametrize("name", sorted(mb.CASES))
def test_update_bit_for_bit(name):
    """one row, a partial wave, one wave, a wave and one row, several workgroups, a tail; C = 64, 128 and 1024; nothing selected (n = 0) and
    EVERY row selected (n = P at P = 1, 64, 256 and 4099: full ballots, workgroup counts of 256, with and without subsampling); max_new
    below, equal to and above n, and 0; a ring smaller than m, of one row, of none; nothing protected; sim with -2
    and NaNs, rows with rinv_q = 0, labels that are neither class"""
    p = mb.problem(name)
    a = p["args"]
    got = _update([p], [p], a["protected"], a["max_new"], a["tau"], a["margin"])
    want = p["out"]
    m = int(want[3][3])
    print("bank update %s: n %d, m %d, state %s (want %s)" % (name, p["n"], m, _np(got[3])[0].tolist(), want[3].tolist()))
    assert _bytes_equal(got, [w[None] for w in want])
    if name in ("nothing_novel", "max_new_zero", "no_ring"):               # m = 0: the bank is the pattern still; only calls and added_last change
        assert m == 0 and _bytes_equal(got[:3], [p[k][None] for k in BANK[:3]])
        assert _np(got[3])[0].tolist() == [int(p["state"][0]), int(p["state"][1]), int(p["state"][2]) + 1, 0]


def test_a_chain_of_five_updates_wraps_the_cursor_twice():
    c = mb.CHAIN
    b = mb.bank(c["cap"], c["C"], c["protected"], 5)
    cur = dict(R=b["R"], rinv_r=b["rinv_r"], label_r=b["label_r"], state=np.array([90, 10, 0, 0], np.int32))
    dev = None
    for t in range(c["frames"]):
        f = mb.frame(c["P"], c["C"], 20 + t)
        want = mb.update(f["q"], f["rinv_q"], f["label_q"], f["sim"], cur["R"], cur["rinv_r"], cur["label_r"], cur["state"], c["protected"], c["max_new"],
                         c["tau"], c["margin"])
        # the device continues from its OWN bank and state
        dev = _update([f], [cur if dev is None else {k: _np(v)[0] for k, v in zip(BANK, dev)}], c["protected"], c["max_new"], c["tau"], c["margin"])
        assert _bytes_equal(dev, [w[None] for w in want]), "call %d" % t
        cur = dict(zip(BANK, want))
    ring = c["cap"] - c["protected"]
    assert cur["state"].tolist() == [(90 + 5 * c["max_new"]) % ring, ring, 5, c["max_new"]] and 90 + 5 * c["max_new"] >= 3 * ring


def test_two_banks_in_one_call_and_identical_calls():
    """N = 2 with different frames, banks and states: each image equals its own N = 1 call, and a repeated call gives the same bytes;
    a reused workspace that holds what another call left changes nothing"""
    from osvos_pytorch_amd import _lib
    p, c, cap, protected = 1000, 128, 1400, 1000
    frames = [mb.frame(p, c, 3), mb.frame(p, c, 4)]
    banks = [mb.bank(cap, c, protected, 3), mb.bank(cap, c, protected, 4, calls=9)]
    args = (protected, 137, 0.4, -0.3)
    both = _update(frames, banks, *args)
    for i in range(2):
        want = mb.update(*(frames[i][k] for k in FRAME), *(banks[i][k] for k in BANK), *args)
        assert 0 < want[3][3] == 137 and _bytes_equal([t[i] for t in both], want)
        alone = _update(frames[i:i + 1], banks[i:i + 1], *args)
        assert _bytes_equal([t[0] for t in alone], want)
    again = _update(frames, banks, *args, fill=0xff)
    assert all(torch.equal(u, v) for u, v in zip(both, again))
    need = int(_lib.lib().osvos_match_bank_ws_bytes(2, p))
    ws = torch.full((need + GUARD,), 0x3c, device="cuda", dtype=torch.uint8)
    for _ in range(2):
        assert all(torch.equal(u, v) for u, v in zip(both, _update(frames, banks, *args, ws=ws)))
    assert bool((ws[need:] == 0x3c).all())


def test_a_row_that_was_added_is_found():
    """after an update that admits every labelled row, the unchanged osvos_match_nearest of the same queries against the bank returns, for
    every labelled row with rinv_q > 0, exactly the row's cosine to itself for its own class"""
    from osvos_pytorch_amd import match
    p, c, protected = 300, 128, 40
    cap = protected + p
    f = mb.frame(p, c, 6, awkward=False)
    b = dict(mb.bank(cap, c, protected, 6))
    b["label_r"] = np.full(cap, mb.VOID, np.uint8)                       # (the pattern's rinv_r are no norms: its rows stay out of both classes)
    got = _update([f], [b], protected, p, 2.0, -4.0)
    labelled = (f["label_q"] <= 1) & (f["rinv_q"] > 0)
    assert int(_np(got[3])[0, 3]) == int(labelled.sum()) > 100
    sim = _np(match.nearest(_dev(f["q"][None]), _dev(f["rinv_q"][None]), got[0], got[1], got[2]))[0]
    dot = (f["q"].astype(np.int64) ** 2).sum(axis=1)
    want = ((dot.astype(np.float32) * f["rinv_q"]).astype(np.float32) * f["rinv_q"]).astype(np.float32)
    own = np.where(f["label_q"] == 1, sim[0], sim[1])
    print("added rows found: %d labelled rows, %d differ" % (int(labelled.sum()), int((own.view(np.uint32) != want.view(np.uint32))[labelled].sum())))
    assert np.array_equal(own.view(np.uint32)[labelled], want.view(np.uint32)[labelled])
    assert (want[labelled] > 0.999).all()


def test_bad_arguments_return_an_error_and_write_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    p = mb.problem("several_workgroups")
    a = p["args"]
    vp = C.c_void_p
    for what, kw in [("C", dict(C=96)), ("cap", dict(cap=0)), ("protected_rows", dict(protected=a["cap"] + 1)), ("max_new", dict(max_new=-1)),
                     ("tau", dict(tau=float("nan"))), ("margin", dict(margin=float("inf"))), ("P", dict(P=0)), ("N", dict(N=0))]:
        f = [_dev(p[k][None]) for k in FRAME]
        b = [_dev(p[k][None]) for k in BANK]
        ws = torch.full((1 << 16,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
        v = dict(N=1, P=a["P"], C=a["C"], cap=a["cap"], protected=a["protected"], max_new=a["max_new"], tau=a["tau"], margin=a["margin"])
        v.update(kw)
        rc = l.osvos_match_bank_update(*(vp(t.data_ptr()) for t in f + b), vp(ws.data_ptr()), v["N"], v["P"], v["C"], v["cap"], v["protected"], v["max_new"],
                                       v["tau"], v["margin"], _stream())
        assert rc < 0 and what.encode() + b" " in l.osvos_last_error(), (what, l.osvos_last_error())
        torch.cuda.synchronize()
        assert _bytes_equal(b, [p[k][None] for k in BANK]) and bool((ws == GARBAGE_BYTE).all())


def test_the_wrappers_match_the_direct_call():
    from osvos_pytorch_amd import match
    p = mb.problem("several_workgroups")
    a = p["args"]
    f = [_dev(p[k][None]) for k in FRAME]
    b = [_dev(p[k][None]) for k in BANK]
    ws = match.bank_update(*f, *b, max_new=a["max_new"], tau=a["tau"], margin=a["margin"], protected=a["protected"])
    assert ws.numel() == match.lib().osvos_match_bank_ws_bytes(1, a["P"]) and _bytes_equal(b, [w[None] for w in p["out"]])
    with pytest.raises(ValueError):
        match.bank_update(*f, *b, max_new=-1, tau=0.5, margin=0.0, protected=0)
    with pytest.raises(ValueError):
        match.bank_update(*f, *b, max_new=4, tau=0.5, margin=0.0, protected=a["cap"] + 1)
    with pytest.raises(ValueError):
        match.bank_update(f[0], f[1], f[2], f[3][:, :1], *b, max_new=4, tau=0.5, margin=0.0, protected=0)
    with pytest.raises(ValueError, match="contiguous"):
        match.bank_update(*f, b[0], b[1], torch.zeros((1, 2 * a["cap"]), device="cuda", dtype=torch.uint8)[:, ::2], b[3], max_new=4, tau=0.5, margin=0.0, protected=0)
    # MemoryBank: seed, two updates, the bound and the narrowed operands
    c = mb.CHAIN
    r0 = mb.frame(c["protected"], c["C"], 9)
    bank = match.MemoryBank(c["cap"] - c["protected"], tau=c["tau"], max_new=c["max_new"], margin=c["margin"])
    bank.seed(_dev(r0["q"][None]), _dev(r0["rinv_q"][None]), _dev(r0["label_q"][None]))
    cap = c["cap"]
    want = (np.concatenate([r0["q"], np.zeros((cap - c["protected"], c["C"]), np.int8)]), np.concatenate([r0["rinv_q"], np.zeros(cap - c["protected"], np.float32)]),
            np.concatenate([r0["label_q"], np.full(cap - c["protected"], 255, np.uint8)]), np.zeros(4, np.int32))
    assert bank.rows == bank.protected == c["protected"] and _bytes_equal((bank.r, bank.rinv_r, bank.label_r, bank.state), [w[None] for w in want])
    assert [tuple(t.shape) for t in bank.operands()] == [(1, c["protected"], c["C"]), (1, c["protected"]), (1, c["protected"])]
    for t in range(3):
        fr = mb.frame(c["P"], c["C"], 20 + t)
        bank.update(*(_dev(fr[k][None]) for k in FRAME))
        want = mb.update(*(fr[k] for k in FRAME), *want, c["protected"], c["max_new"], c["tau"], c["margin"])
        assert _bytes_equal((bank.r, bank.rinv_r, bank.label_r, bank.state), [w[None] for w in want])
        assert bank.rows == mb.bound_rows(c["protected"], cap - c["protected"], c["max_new"], t + 1) == int(bank.operands()[0].shape[1])
        assert bank.rows >= c["protected"] + int(want[3][1]) and all(t.is_contiguous() for t in bank.operands())
    assert bank.rows == cap


# ------------------------------------------------------------------------------------------------------------------ the matcher


class _Planted(object):
    """stands in for the network: ``forward_features`` returns the planted logit maps and features of the frame whose number x carries"""

    def __init__(self, s):
        self.outs = [[_dev(o) for o in outs] for outs in s["outs"]]
        self.feats = [_dev(f[None]) for f in s["feats"]]

    def forward_features(self, x, layer):
        t = int(x[0, 0, 0, 0].item())
        return self.outs[t], self.feats[t], None


def _frame_input(t):
    return torch.full((1, 3, mb.SEQ["H"], mb.SEQ["W"]), float(t), device="cuda")


def _run(matcher, s):
    """the annotated frame 0, then frames 1 .. with the mask of the frame before handed over from frame 2 on -> the fused maps of frames 1 .."""
    matcher.set_reference(_frame_input(0), _dev(s["masks"][0]))
    fused = []
    for t in range(1, mb.SEQ["frames"]):
        outs = matcher(_frame_input(t), None if t == 1 else _dev(s["masks"][t - 1]))
        assert all(torch.equal(u, v) for u, v in zip(outs[:4], matcher.net.outs[t][:4]))
        fused.append(outs[-1])
    return fused


def test_the_matcher_with_a_stand_in_network():
    """memory=0 is today's path (nearest against the first frame's bank, fused by tta.fuse_views); memory > 0 with nothing novel (tau = -3)
    gives the same bytes, the ring's void rows change no bit; with rows admitted the fused output is the restatement of the update composed
    with match_cases' restatement of nearest"""
    from osvos_pytorch_amd import match, tta
    s, q = mb.sequence(), mb.SEQ
    net = _Planted(s)
    size = (q["H"], q["W"])

    def fuse(t, mp):
        return tta.fuse_views([net.outs[t][-1], _dev(mp)], [False, False], size, weights=[1.0, q["gain"]])

    plain = _run(match.AppearanceMatcher(net, 9, q["gain"]), s)
    for t, got in enumerate(plain, 1):
        assert np.array_equal(_bits(got), _bits(fuse(t, mc.match_map(s["sims_first"][t]).reshape(1, s["h"], s["w"]))))
    m = match.AppearanceMatcher(net, 9, q["gain"], memory=q["memory"], memory_tau=-3.0, memory_new=q["memory_new"], memory_margin=q["margin"])
    idle = _run(m, s)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(plain, idle))
    assert _np(m._memory.state)[0].tolist() == [0, 0, q["frames"] - 2, 0] and m._memory.rows == s["p"] + min(q["memory"], 2 * q["memory_new"])
    for kw in (dict(), dict(previous=True), dict(topk=3)):
        m = match.AppearanceMatcher(net, 9, q["gain"], memory=q["memory"], memory_tau=q["tau"], memory_new=q["memory_new"], memory_margin=q["margin"], **kw)
        assert m.needs_previous
        got = _run(m, s)
        assert _np(m._memory.state)[0, 2] == q["frames"] - 2
        if "topk" not in kw:                                                 # (the previous-frame bank is combined in AFTER the sim the update reads)
            assert _bytes_equal((m._memory.r, m._memory.rinv_r, m._memory.label_r, m._memory.state), [w[None] for w in s["bank"]])
        if not kw:
            for t, g in enumerate(got, 1):
                assert np.array_equal(_bits(g), _bits(fuse(t, s["maps"][t]))), "frame %d" % t
            assert not np.array_equal(_bits(got[-1]), _bits(plain[-1]))      # the memory changes the last frame's map
            assert _np(m._memory.state)[0, 3] == s["added"][-1] > 0
    net.feats[1] = torch.cat([net.feats[1], net.feats[1]])                   # two frames in one call: the bank is one image's
    with pytest.raises(ValueError, match="one at a time"):
        m(torch.cat([_frame_input(1), _frame_input(1)]), None)


# ------------------------------------------------------------------------------------------------------------------ the script


def _parent(tmp_path, name):
    import networks.vgg_osvos as vo
    torch.manual_seed(0)
    os.makedirs(str(tmp_path / name))
    torch.save(vo.OSVOS(pretrained=0).state_dict(), str(tmp_path / name / "parent_epoch-239.pth"))


def test_train_online_with_a_memory_bank(tmp_path):
    out = script_runner.train_online(tmp_path / "mem", "--device-augment", "--match-gain", "4", "--match-memory", "256", frames=1).stdout
    assert "Online training time" in out and "J&F on blackswan:" in out, out[-2000:]


def test_train_online_with_a_memory_bank_over_four_frames(tmp_path):
    """frames 2 and 3 are searched against a bank that frames 1 and 2 were written into"""
    out = script_runner.train_online(tmp_path / "mem4", "--device-augment", "--synthetic-frames", "4", "--match-gain", "4", "--match-memory", "256,2,64,-4",
                                     frames=4).stdout
    assert "J&F on blackswan:" in out, out[-2000:]


def test_train_online_multi_object_with_a_memory_bank(tmp_path):
    out = script_runner.train_online(tmp_path / "mo", "--multi-object", "--match-gain", "2", "--match-memory", "64,0.8,16,-0.1").stdout
    assert "J&F on blackswan (2 objects):" in out and "J&F on blackswan object 2:" in out, out[-2000:]


def test_train_online_memory_of_zero_changes_no_byte(tmp_path):
    """--match-memory 0 builds the matcher of --match-gain alone: the PNGs are byte-identical.  Both runs start from the same seeded parent
    checkpoint, for the reason tests/test_gpu_match_ext.py gives."""
    def run(name, *extra):
        _parent(tmp_path, name)
        return script_runner.train_online(tmp_path / name, "--device-augment", "--synthetic-frames", "3", "--match-gain", "2", *extra, frames=3).masks
    assert run("zero", "--match-memory", "0") == run("plain")
