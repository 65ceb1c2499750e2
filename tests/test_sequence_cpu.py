"""osvos_pytorch_amd.sequence -- the test phase of train_online.py -- driven on the CPU with recording stand-ins for the stages: 3 frames of
6 x 8 pixels.  Every stand-in appends (stage, frame) to one log and returns 2 * x + c with a c of its own, so the log proves the order and
the final value proves that each stage ran once, on the output of the one before it."""
import pytest
import torch

from osvos_pytorch_amd import sequence

H, W, F = 6, 8, 3
CPU = torch.device("cpu")
C_MATCH, C_ADAPT, C_TTA, C_CRF, C_SNAP, C_TRACK = 1.0, 3.0, 5.0, 7.0, 11.0, 13.0


class Rec(object):
    """the shared log, and the frame the loader handed out last"""

    def __init__(self):
        self.log, self.f = [], None

    def add(self, stage, *more):
        self.log.append((stage, self.f) + more)

    def of(self, f):
        return [e[0] for e in self.log if e[1] == f]


class Net(object):
    def __init__(self, rec):
        self.rec = rec

    def forward(self, image):
        self.rec.add("net")
        self.out = [None] * 4 + [image[:, :1]]
        return self.out


class Matcher(object):
    def __init__(self, rec, previous=True, c=C_MATCH):
        self.rec, self.previous, self.c, self.has_reference, self.prevs = rec, previous, c, False, []

    def set_reference(self, image, mask):
        self.rec.add("set_reference")
        self.reference, self.has_reference = (image, mask), True

    def __call__(self, image, prev):
        self.rec.add("matcher")
        self.prevs.append(prev)
        return [None] * 4 + [2 * image[:, :1] + self.c]


class Adapter(object):
    """like adapt.OnlineAdapter: two plain forwards through ``forward``, the second one returned"""

    def __init__(self, rec):
        self.rec, self.forward, self.prevs = rec, None, []

    def __call__(self, image, prev_mask):
        self.rec.add("adapter")
        self.prevs.append(prev_mask)
        self.forward(image)
        return 2 * self.forward(image)[-1] + C_ADAPT


class Tta(object):
    def __init__(self, rec):
        self.rec, self.frames = rec, []

    def __call__(self, frame_u8):
        self.rec.add("tta")
        self.frames.append(frame_u8)
        return 2 * frame_u8[None, None, :, :, 0].float() + C_TTA


class Crf(object):
    def __init__(self, rec):
        self.rec, self.frames = rec, []

    def __call__(self, fused, frames_u8):
        self.rec.add("crf")
        self.frames.append(frames_u8)
        return 2 * fused + C_CRF


class Snap(object):
    def __init__(self, rec):
        self.rec, self.calls, self.made = rec, [], []

    def labels(self, frames_u8):
        self.rec.add("labels")
        self.made.append((frames_u8, torch.zeros(frames_u8.shape[:3], dtype=torch.int32)))
        return self.made[-1][1]

    def __call__(self, fused, frames_u8=None, labels=None):
        self.rec.add("snap")
        self.calls.append((frames_u8, labels))
        return 2 * fused + C_SNAP


class Tracker(object):
    def __init__(self, rec, first_mask):
        rec.add("tracker.build")
        self.rec, self.first_mask, self.seed, self.sizes = rec, first_mask, first_mask.to(torch.uint8)[None], []

    def __call__(self, fused):
        self.rec.add("tracker")
        self.sizes.append(int(fused.shape[0]))
        return 2 * fused + C_TRACK


class Flow(object):
    def __init__(self, rec):
        self.rec, self.frames, self.warped = rec, [], []

    def update(self, frame_u8):
        self.rec.add("flow.update")
        self.frames.append(frame_u8)

    def warp(self, x):
        self.rec.add("flow.warp.mask" if x.dtype == torch.bool else "flow.warp.seed")
        self.warped.append(x)
        return torch.roll(x, 1, -1)


def samples(rec, gt_all=False, gt_first=True, with_image=True):
    g = torch.Generator().manual_seed(5)
    out = []
    for f in range(F):
        s = {"fname": ["%05d" % f], "frame_u8": torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)}
        if with_image or f == 0:
            s["image"] = torch.randn(1, 3, H, W, generator=g)
        if (f == 0 and gt_first) or gt_all:
            s["gt"] = (torch.rand(1, 1, H, W, generator=g) > 0.5).float()
        out.append(s)

    def loader():
        for f, s in enumerate(out):
            rec.f = f
            yield s
    return out, loader()


def chain(x):
    return 2 * (2 * (2 * x + C_CRF) + C_SNAP) + C_TRACK


@pytest.mark.parametrize("gt_all", [False, True], ids=["gt_on_frame_0", "gt_on_every_frame"])
def test_single_object_every_stage_but_tta_runs_in_the_order_of_the_recipe(gt_all):
    rec = Rec()
    net, matcher, adapter, crf, snap, flow = Net(rec), Matcher(rec), Adapter(rec), Crf(rec), Snap(rec), Flow(rec)
    trackers = []
    data, loader = samples(rec, gt_all)
    forward = sequence.FrameForward(net, None, adapter, matcher)
    seq = sequence.SingleObjectSequence(loader, forward, CPU, "blackswan", flow=flow, crf=crf, snap=snap,
                                        make_tracker=lambda m: trackers.append(Tracker(rec, m)) or trackers[-1])
    got = list(seq)

    assert rec.of(0) == ["flow.update", "set_reference", "matcher", "crf", "snap", "tracker.build", "tracker"]
    later = ["flow.update", "flow.warp.mask", "flow.warp.seed", "adapter", "matcher", "matcher", "crf", "snap", "tracker"]
    assert rec.of(1) == later and rec.of(2) == later and len(rec.log) == 7 + 2 * 9
    assert len(trackers) == 1 and seq.tracker is trackers[0]

    x = [s["image"][:, :1] for s in data]
    want = [chain(2 * x[0] + C_MATCH)] + [chain(2 * (2 * x[f] + C_MATCH) + C_ADAPT) for f in (1, 2)]
    for f in range(F):
        fname, fused, gt = got[f]
        assert fname == data[f]["fname"] and torch.equal(fused, want[f])
        assert gt is data[f]["gt"] if (gt_all or f == 0) else gt is None
        assert flow.frames[f] is data[f]["frame_u8"] and crf.frames[f] is data[f]["frame_u8"] and snap.calls[f] == (data[f]["frame_u8"], None)

    gt0 = data[0]["gt"]
    assert matcher.reference[0] is data[0]["image"] and torch.equal(matcher.reference[1], gt0[:, 0] > 0.5)
    assert torch.equal(trackers[0].first_mask, gt0[0, 0] > 0.5)
    # what frame f + 1 is handed: the annotation of frame 0, then the FINAL mask of frame f -- moved by the flow before the adapter sees it
    masks, seeds = flow.warped[0::2], flow.warped[1::2]
    assert torch.equal(masks[0], gt0 > 0.5) and torch.equal(masks[1], want[1] > 0)
    assert [torch.equal(p, torch.roll(m, 1, -1)) for p, m in zip(adapter.prevs, masks)] == [True, True]
    assert torch.equal(seeds[0], (gt0[0, 0] > 0.5).to(torch.uint8)[None]) and torch.equal(seeds[1], torch.roll(seeds[0], 1, -1))
    assert torch.equal(trackers[0].seed, torch.roll(seeds[0], 2, -1))
    # the matcher: frame 0 without a previous mask; both of the adapter's forwards of frame f + 1 with the final mask of frame f
    assert matcher.prevs[0] is None and len(matcher.prevs) == 5
    for f in (0, 1):
        assert torch.equal(matcher.prevs[1 + 2 * f], want[f] > 0) and torch.equal(matcher.prevs[2 + 2 * f], want[f] > 0)
    assert torch.equal(forward.match_prev, want[2] > 0) and torch.equal(seq.prev_mask, want[2] > 0)
    assert any(not torch.equal(want[f] > 0, 2 * x[f] + C_MATCH > 0) for f in range(F))      # (final and raw masks differ: the check means something)


def test_the_adapter_hook_calls_the_matcher_with_the_current_previous_mask():
    rec = Rec()
    matcher, adapter = Matcher(rec), Adapter(rec)
    forward = sequence.FrameForward(Net(rec), None, adapter, matcher)
    image = torch.randn(1, 3, H, W)
    for prev in (None, torch.ones(1, 1, H, W) > 0, torch.zeros(1, 1, H, W) > 0):
        forward.match_prev = prev
        out = adapter.forward(image)
        assert matcher.prevs[-1] is prev and torch.equal(out[-1], 2 * image[:, :1] + C_MATCH)
    assert sequence.FrameForward(Net(rec), None, Adapter(rec), None).adapter.forward is None      # no matcher: the adapter's own forwards


def test_without_motion_compensation_frame_1_sees_the_annotation_of_frame_0():
    rec = Rec()
    adapter = Adapter(rec)
    adapter.forward = Net(rec).forward
    data, loader = samples(rec)
    seq = sequence.SingleObjectSequence(loader, sequence.FrameForward(Net(rec), None, adapter, None), CPU, "blackswan")
    got = list(seq)
    assert [rec.of(f) for f in range(F)] == [["net"], ["adapter", "net", "net"], ["adapter", "net", "net"]]
    assert torch.equal(adapter.prevs[0], data[0]["gt"] > 0.5) and torch.equal(adapter.prevs[1], got[1][1] > 0)


def test_test_time_augmentation_takes_the_decoded_frame_and_replaces_every_other_forward():
    rec = Rec()
    tta, matcher = Tta(rec), Matcher(rec)
    data, loader = samples(rec, with_image=False)          # (DeviceTestFrames raw_only: no 'image' for a frame without annotation)
    forward = sequence.FrameForward(Net(rec), tta, Adapter(rec), matcher)
    got = list(sequence.SingleObjectSequence(loader, forward, CPU, "blackswan", crf=Crf(rec)))
    assert not {"adapter", "matcher", "net"} & {e[0] for e in rec.log}
    assert [rec.of(f)[-2:] for f in range(F)] == [["tta", "crf"]] * F
    for f in range(F):
        assert tta.frames[f] is data[f]["frame_u8"]
        assert torch.equal(got[f][1], 2 * (2 * data[f]["frame_u8"][None, None, :, :, 0].float() + C_TTA) + C_CRF)
    assert not forward.needs_image


def test_with_every_stage_off_the_result_is_the_network_output_untouched():
    rec = Rec()
    net = Net(rec)
    data, loader = samples(rec)
    seq = sequence.SingleObjectSequence(loader, sequence.FrameForward(net), CPU, "blackswan")
    for f, (fname, fused, gt) in enumerate(seq):
        assert fused is net.out[-1] and torch.equal(fused, data[f]["image"][:, :1])
    assert rec.log == [("net", 0), ("net", 1), ("net", 2)]
    assert seq.prev_mask is None and seq.tracker is None and seq.forward.match_prev is None


def _refusal(message, gt_first=True, **stages):
    rec = Rec()
    data, loader = samples(rec, gt_first=gt_first)
    if "flow" in stages:
        data[0]["frame_u8"] = torch.stack([data[0]["frame_u8"]] * 2)
    stages = {k: v(rec) for k, v in stages.items()}
    forward = sequence.FrameForward(Net(rec), None, stages.pop("adapter", None), stages.pop("matcher", None))
    with pytest.raises(SystemExit) as e:
        list(sequence.SingleObjectSequence(loader, forward, CPU, "blackswan", **stages))
    assert str(e.value) == message


def test_refusals_keep_their_messages():
    _refusal("--match-gain: sequence blackswan has no first annotation to build the bank from", gt_first=False, matcher=Matcher)
    _refusal("--track-components: sequence blackswan has no first annotation to seed the tracker", gt_first=False,
             make_tracker=lambda rec: lambda m: Tracker(rec, m))
    _refusal("--adapt-steps: sequence blackswan has no first annotation to start from", gt_first=False, adapter=Adapter)
    _refusal("--flow-search: the test loader delivered 2 frames in one batch; it takes one", flow=Flow)


def test_post_chain_serves_one_frame_and_a_chunk_and_takes_shared_labels():
    rec = Rec()
    crf, snap = Crf(rec), Snap(rec)
    tracker = Tracker(rec, torch.ones(H, W) > 0)
    one, frame = torch.randn(1, 1, H, W), torch.zeros(H, W, 3, dtype=torch.uint8)
    assert torch.equal(sequence.post_chain(one, frame, crf, snap, tracker), chain(one))
    many, frames = torch.randn(2, H, W), torch.zeros(2, H, W, 3, dtype=torch.uint8)
    labels = snap.labels(frames)
    assert torch.equal(sequence.post_chain(many, frames, crf, snap, tracker, labels=labels), chain(many))
    assert [e[0] for e in rec.log] == ["tracker.build", "crf", "snap", "tracker", "labels", "crf", "snap", "tracker"]
    assert snap.calls[0] == (frame, None) and snap.calls[1][0] is None and snap.calls[1][1] is labels
    assert sequence.post_chain(one, frame) is one


def test_multi_object_forwards_first_then_the_post_chain_stage_by_stage_over_chunks():
    K, rec = 2, Rec()
    g = torch.Generator().manual_seed(9)
    frames = [torch.full((H, W, 3), f, dtype=torch.uint8) for f in range(F)]
    images = [torch.randn(1, 3, H, W, generator=g) for f in range(F)]
    first = torch.zeros(H, W, dtype=torch.uint8)
    first[1:3, 1:4], first[3:5, 4:7] = 1, 2
    gts = [first, None, None]
    crf, snap, matchers, trackers = Crf(rec), Snap(rec), [], []

    def fine_tuned(k):
        rec.f = None
        rec.add("fine_tune", k)
        return Net(rec)

    def forward_of(net):
        matchers.append(Matcher(rec, previous=True, c=float(len(matchers) + 1)))
        return sequence.FrameForward(net, None, None, matchers[-1])

    def image_of(frame):
        rec.f = int(frame[0, 0, 0])
        return images[rec.f]

    logits, got_trackers, started = sequence.multi_object_sequence(
        frames, gts, K, fine_tuned, forward_of, image_of, crf=crf, snap=snap, make_tracker=lambda m: trackers.append(Tracker(rec, m)) or trackers[-1],
        chunk=2)

    per_object = ["set_reference", "matcher", "matcher", "matcher"]
    stages = [e[0] for e in rec.log]
    assert stages == (["fine_tune"] + per_object) * 2 + ["crf"] * 4 + ["labels", "snap", "snap"] * 2 + ["tracker.build", "tracker", "tracker"] * 2
    assert [e[2] for e in rec.log if e[0] == "fine_tune"] == [1, 2]
    assert [e[1] for e in rec.log if e[0] in per_object] == [0, 0, 1, 2] * 2
    # crf: chunk (0, 1) for both objects, then chunk (2,) for both; one labelling per chunk, handed to both objects
    assert [f[:, 0, 0, 0].tolist() for f in crf.frames] == [[0, 1], [0, 1], [2], [2]]
    assert [f[:, 0, 0, 0].tolist() for f, _ in snap.made] == [[0, 1], [2]]
    assert [c[0] for c in snap.calls] == [None] * 4 and [c[1] is snap.made[i // 2][1] for i, c in enumerate(snap.calls)] == [True] * 4
    # one tracker per object, seeded with its own first mask, walking its chunks in order
    assert got_trackers == trackers and len(trackers) == K
    for k in range(K):
        assert torch.equal(trackers[k].first_mask, first == k + 1) and trackers[k].sizes == [2, 1]
        assert torch.equal(matchers[k].reference[1], first == k + 1) and matchers[k].reference[0] is images[0]
        raw = [2 * images[f][0, 0] + (k + 1.0) for f in range(F)]
        # --match-previous: the RAW output of the matched forward, not the final mask
        assert matchers[k].prevs[0] is None and all(torch.equal(matchers[k].prevs[f + 1], (raw[f] > 0)[None, None]) for f in range(F - 1))
        assert any(not torch.equal(raw[f] > 0, chain(raw[f]) > 0) for f in range(F - 1))
        assert torch.equal(logits[k], torch.stack([chain(r) for r in raw]))
    assert tuple(logits.shape) == (K, F, H, W) and isinstance(started, float)
