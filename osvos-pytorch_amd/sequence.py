"""The test phase of train_online.py: everything between "the network is fine-tuned" and "the masks are scored", for both recipes.

The stages arrive built (results.ComponentTracker as a factory ``first_mask -> tracker``, because its seed is the first annotation), or as
None for an option that is off.  THE ORDER OF THE STAGES LIVES HERE, and tests/test_sequence_cpu.py asserts it with recording stand-ins:

  ``FrameForward``          one frame -> fused logits: roi > tta > adapter (once a previous mask exists) > matcher > net.forward
  ``post_chain``            crf -> snap -> tracker on a logit stack and its decoded frames (one frame or a chunk of frames)
  ``SingleObjectSequence``  per frame: motion compensation of what is carried over, matcher reference, FrameForward, post_chain, then the
                            state of the next frame (SingleObjectSequence.step)
  ``multi_object_sequence`` per object: fine-tuning (the caller's) and FrameForward over every frame into a [K,F,H,W] stack; then post_chain
                            stage by stage over chunks of frames; ``score_objects`` merges, scores and writes
  ``interactive_sequence``  per round: annotate (the first interaction, then the simulated annotator on the worst frame of the previous
                            round's prediction), fit, FrameForward and post_chain over every frame, score

The two recipes differ in ONE rule.  The mask that --match-previous (and --match-local) hands to the next frame (FrameForward.remember) is the FINAL mask in
the single-object recipe -- after crf, snap and tracker -- and the RAW output of the matched forward in the multi-object recipe, whose post
chain runs only after every forward of every object is done.  The mask the object-centred zoom takes its box from (FrameForward.roi_prev)
is remembered by the same call, so it follows the same rule."""
import timeit

import torch

from .results import MultiObjectEvaluator, merge_objects, save_label_maps


class FrameForward(object):
    """``forward(frame_u8, image, prev_mask)`` -> the fused logits [1,1,H,W] of one frame, from the first of: ``roi(frame_u8, roi_prev)``
    (roi.RoiZoom: the network on a crop around the mask ``remember`` was handed last; None on frame 0: the full frame); ``tta(frame_u8)``;
    ``adapter(image, prev_mask)`` once there is a previous mask (so never on frame 0); ``matcher(image, match_prev)[-1]``;
    ``net.forward(image)[-1]``.  With an adapter and a matcher both of the adapter's plain forwards are matched ones that read the current
    ``match_prev``.  One per network: the multi-object recipe builds one per object, without adapter."""

    def __init__(self, net, tta=None, adapter=None, matcher=None, roi=None):
        self.net, self.tta, self.adapter, self.matcher, self.roi = net, tta, adapter, matcher, roi
        self.match_prev = None               # --match-previous / --match-local: the previous frame's mask (which one: see the module docstring)
        self.roi_prev = None                 # --zoom: the previous frame's mask, by the same rule
        if matcher is not None and adapter is not None:
            adapter.forward = lambda image: matcher(image, self.match_prev)

    @property
    def needs_reference(self):
        return self.matcher is not None and not self.matcher.has_reference

    @property
    def needs_image(self):
        """False under test-time augmentation and under the zoom, which make their own views from frame_u8"""
        return self.tta is None and self.roi is None

    def set_reference(self, image, mask):
        if self.needs_reference:
            self.matcher.set_reference(image, mask)

    def __call__(self, frame_u8, image, prev_mask=None):
        if self.roi is not None:
            return self.roi(frame_u8, self.roi_prev)
        if self.tta is not None:
            return self.tta(frame_u8)
        if self.adapter is not None and prev_mask is not None:
            return self.adapter(image, prev_mask)           # (turns gradients on for its own training steps)
        if self.matcher is not None:
            return self.matcher(image, self.match_prev)[-1]
        return self.net.forward(image)[-1]

    def remember(self, logits):
        # (needs_previous: the local view wants the mask too, with or without --match-previous; a matcher without the attribute has .previous)
        if self.matcher is not None and getattr(self.matcher, 'needs_previous', self.matcher.previous):
            self.match_prev = logits > 0
        if self.roi is not None:
            self.roi_prev = logits > 0


def post_chain(fused, frames_u8, crf=None, snap=None, tracker=None, labels=None):
    """crf -> snap -> tracker on ``fused`` ([1,1,H,W] with the frame [H,W,3], or [n,H,W] with n consecutive frames [n,H,W,3]); a stage that
    is None is left out.  ``labels``: ``snap.labels(frames_u8)`` made by the caller, for several objects over the same frames."""
    if crf is not None:
        fused = crf(fused, frames_u8)
    if snap is not None:
        fused = snap(fused, frames_u8) if labels is None else snap(fused, labels=labels)
    if tracker is not None:
        fused = tracker(fused)
    return fused


class SingleObjectSequence(object):
    """Iterating yields ``(fname, fused, gt or None)`` for every sample of ``loader``, in order; the caller writes and scores.  ``prev_mask``
    (--adapt-steps: the previous frame's final mask; for frame 1 the annotation of frame 0), ``tracker`` and ``forward.match_prev`` are the
    state carried from frame to frame, and so is ``forward.roi_prev``; ``flow`` (flow.MotionCompensator) moves the first two and the last to
    where the object is now."""

    def __init__(self, loader, forward, device, seq_name, flow=None, crf=None, snap=None, make_tracker=None):
        self.loader, self.forward, self.device, self.seq_name = loader, forward, device, seq_name
        self.flow, self.crf, self.snap, self.make_tracker = flow, crf, snap, make_tracker
        self.prev_mask = self.tracker = None

    def __iter__(self):
        for sample in self.loader:
            yield self.step(sample)

    @torch.no_grad()
    def step(self, sample):
        forward, seq_name = self.forward, self.seq_name
        frame_u8, gt = sample.get('frame_u8'), sample.get('gt')
        image = sample['image'].to(self.device) if 'image' in sample else None
        if self.flow is not None:                # the field from the previous frame to this one moves what is carried over
            if frame_u8.dim() != 3:
                raise SystemExit('--flow-search: the test loader delivered %d frames in one batch; it takes one' % int(frame_u8.shape[0]))
            self.flow.update(frame_u8)
            if self.prev_mask is not None:
                self.prev_mask = self.flow.warp(self.prev_mask)
            if self.tracker is not None:
                self.tracker.seed = self.flow.warp(self.tracker.seed)
            if forward.roi_prev is not None:
                forward.roi_prev = self.flow.warp(forward.roi_prev)
        if forward.needs_reference:
            if gt is None:
                raise SystemExit('--match-gain: sequence %s has no first annotation to build the bank from' % seq_name)
            forward.set_reference(image, gt.to(self.device)[:, 0] > 0.5)
        fused = forward(frame_u8, image, self.prev_mask)
        fused = post_chain(fused, frame_u8, self.crf, self.snap)
        if self.make_tracker is not None:
            if self.tracker is None:             # (built here, after crf and snap of frame 0, as it always was)
                if gt is None:
                    raise SystemExit('--track-components: sequence %s has no first annotation to seed the tracker' % seq_name)
                self.tracker = self.make_tracker(gt.to(self.device)[0, 0] > 0.5)
            fused = self.tracker(fused)
        if forward.adapter is not None:
            if self.prev_mask is None and gt is None:
                raise SystemExit('--adapt-steps: sequence %s has no first annotation to start from' % seq_name)
            self.prev_mask = gt.to(self.device) > 0.5 if self.prev_mask is None else fused > 0
        forward.remember(fused)                  # the FINAL mask
        return sample['fname'], fused, gt


def multi_object_sequence(frames, gts, K, fine_tuned, forward_of, image_of, crf=None, snap=None, make_tracker=None, chunk=64):
    """The DAVIS 2017 recipe on the decoded frames [H,W,3] and the indexed annotations ``gts`` (gts[0] holds ids 1..K) of one sequence.

    Per object k: ``fine_tuned(k)`` -> its network, ``forward_of(net)`` -> its FrameForward, the matcher's reference from frame 0 under
    ``gts[0] == k``, then every frame (``image_of(frame)``: the network's input) into row k - 1 of the logit stack; the RAW output is what
    --match-previous remembers.  Then, over chunks of ``chunk`` consecutive frames, stage by stage as post_chain orders them: crf for every
    object; one superpixel labelling per chunk, shared by the objects; one tracker per object, seeded with ``gts[0] == k``, walking its
    chunks in order.  Everything is enqueued; nothing is read back.  -> (logits [K,F,H,W], trackers, the timer value the test phase would
    have started at had its parts run back to back)."""
    h, w = int(frames[0].shape[0]), int(frames[0].shape[1])
    logits = torch.empty((K, len(frames), h, w), device=frames[0].device, dtype=torch.float32)
    test_time = 0.0
    for k in range(1, K + 1):
        net = fine_tuned(k)
        start_time = timeit.default_timer()
        forward = forward_of(net)                # one matcher per object's network: its own first-frame bank
        with torch.no_grad():
            if forward.needs_reference:
                forward.set_reference(image_of(frames[0]), gts[0] == k)
            for f, img in enumerate(frames):
                out = forward(img, image_of(img) if forward.needs_image else None)
                logits[k - 1, f].copy_(out[0, 0])
                forward.remember(out)            # the RAW output
        if logits.is_cuda:
            torch.cuda.synchronize()
        test_time += timeit.default_timer() - start_time
        del net, forward

    print('Testing Network')
    started = timeit.default_timer() - test_time
    chunks = [slice(s0, s0 + chunk) for s0 in range(0, len(frames), chunk)]
    if crf is not None:
        for c in chunks:
            stacked = torch.stack(frames[c])
            for k in range(K):
                logits[k, c] = post_chain(logits[k, c], stacked, crf=crf)
    if snap is not None:
        for c in chunks:
            spx = snap.labels(torch.stack(frames[c]))
            for k in range(K):
                logits[k, c] = post_chain(logits[k, c], None, snap=snap, labels=spx)
    trackers = []
    for k in range(K if make_tracker is not None else 0):
        trackers.append(make_tracker(gts[0] == k + 1))
        for c in chunks:
            logits[k, c] = post_chain(logits[k, c], None, tracker=trackers[k])
    return logits, trackers, started


def score_objects(logits, gts, paths):
    """merge the K logit stacks into label maps, score the annotated frames per object, write the indexed PNGs -> the evaluator's summary;
    one read-back for the PNGs, one for the counts"""
    K = int(logits.shape[0])
    labels = merge_objects(logits)
    evaluator = MultiObjectEvaluator(K)
    scored = [f for f, g in enumerate(gts) if g is not None]
    step = max(1, min(64, 65535 // K))
    for s0 in range(0, len(scored), step):
        at = scored[s0:s0 + step]
        evaluator.add(labels[at], torch.stack([gts[f] for f in at]))      # (enqueued: nothing is read back here)
    save_label_maps(labels, paths)
    return evaluator.summary()


def interactive_sequence(session, forward, post, rounds, steps0, steps, gts, robot, first=None, make_evaluator=None, on_round=None):
    """The interactive loop (Scribble-OSVOS) over one sequence.  session: scribble.InteractiveSession (the strokes, the training, the decoded
    frames); forward: the network's FrameForward; post: the keyword arguments of ``post_chain`` (crf, snap); gts: the uint8 annotation
    [H,W] of EVERY frame (the annotator needs the truth of the frame it looks at; the object is ``session.object_id``); robot:
    ``robot(None, gt)`` -> the first interaction's map, ``robot(pred_labels, gt)`` -> the strokes through the errors of a prediction
    (scribble.Robot).  first: [(frame, map), ..] to open with in place of the robot's first interaction (a person's strokes).  on_round:
    ``on_round(r, dict)`` is called as each round's report is complete.

    Round 0 annotates with the first interaction on frame 0 and fits ``steps0`` optimizer steps.  Every later round takes the annotated-truth
    frame with the lowest J of the previous round's prediction (the first of several), runs the robot on it, adds the result and fits
    ``steps`` steps.  Every round then predicts all frames (``forward``, then ``post_chain``) and scores them (``make_evaluator()``, default
    results.SequenceEvaluator).  The network keeps training from round to round.  A round's annotation comes from the round before, so
    nothing is trained after the last prediction: that prediction is the result.

    -> (per round a dict: 'frame' annotated (a list in round 0 with ``first``), 'labelled' pixels of all strokes so far, 'J', 'F' means,
    'fit_s', 'predict_s' seconds; the fused logits of the last round, a list of [1,1,H,W])"""
    if rounds < 1 or steps0 < 0 or steps < 0:
        raise ValueError("interactive_sequence: rounds >= 1 and steps >= 0, got %r, %r, %r" % (rounds, steps0, steps))
    n = len(session.frames_u8)
    if len(gts) != n or any(gt is None for gt in gts):
        raise ValueError("interactive_sequence: the annotator needs the annotation of every one of the %d frames" % n)
    if make_evaluator is None:
        from .results import SequenceEvaluator as make_evaluator
    sync = torch.cuda.synchronize if session.frames_u8[0].is_cuda else (lambda: None)
    report, fused, js = [], None, None
    for r in range(rounds):
        if r == 0 and first is not None:
            frame = [f for f, _ in first]
            for f, m in first:
                session.add(f, m)
        elif r == 0:
            frame = 0
            session.add(0, robot(None, gts[0]))
        else:
            frame = min(range(n), key=lambda f: js[f])
            pred = (fused[frame][0, 0] > 0).to(torch.uint8) * session.object_id
            session.add(frame, robot(pred, gts[frame]))
        sync()
        t0 = timeit.default_timer()
        session.fit(steps0 if r == 0 else steps)
        sync()
        t1 = timeit.default_timer()
        evaluator, fused = make_evaluator(), []
        with torch.no_grad():
            for f in range(n):
                out = forward(session.frames_u8[f], session.image(f) if forward.needs_image else None)
                out = post_chain(out, session.frames_u8[f], **post)
                forward.remember(out)
                evaluator.add(out, (gts[f] == session.object_id).float()[None, None])
                fused.append(out)
        session.set_previous([o[0, 0] > 0 for o in fused])
        js, fs = evaluator.per_frame()          # (the round's one read-back of scores)
        t2 = timeit.default_timer()
        report.append({'frame': frame, 'labelled': session.labelled_pixels(), 'J': sum(js) / len(js), 'F': sum(fs) / len(fs), 'fit_s': t1 - t0,
                       'predict_s': t2 - t1})
        if on_round is not None:
            on_round(r, report[-1])
    return report, fused
