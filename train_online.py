"""Online fine-tuning on the first frame of a sequence, then inference on every frame.

Same entry point, knobs and file naming as the reference's train_online.py (SEQ_NAME env var,
parent checkpoint ``<save_dir>/parent_epoch-239.pth``, result PNGs under ``<save_dir>/Results/<seq>``),
running on the MI355X-native OSVOS path.  Differences by design:
  * the dataset / augmentation layer of the reference needs OpenCV (``cv2``), which this image
    lacks: ``--device-augment`` replaces it (Pillow decode -> pinned uint8 staging -> one HIP kernel
    for flip / scale+rotate / mean / CHW, osvos_pytorch_amd.augment; the first frame is decoded once
    and re-augmented on the GPU every iteration); ``--synthetic`` runs the identical loop on a seeded
    synthetic frame (benchmarking); with the reference's dataloaders package + cv2 installed next to
    this file the original transform chain is used
  * the loss is accumulated on the device and read back only when it is printed
  * ``--multi-object`` (DAVIS 2017): one fine-tuning per object id of the first annotation, the K logit stacks merged into one label map
    per frame on the device, indexed PNGs, J and F per object (osvos_pytorch_amd.results.merge_objects / MultiObjectEvaluator)
  * ``--track-components R``: connected-component clean-up of every test frame on the device -- a component of the thresholded mask is kept
    when it lies within R pixels of what was kept of the previous frame, starting from the first annotation (results.ComponentTracker)
  * ``--tta-scales S1,S2,..`` / ``--tta-flip``: test-time augmentation of the test forwards -- every frame at each scale and (flip) mirrored,
    the views' logit maps resampled onto the frame's grid and averaged on the device (osvos_pytorch_amd.tta.TestTimeAugment)
  * ``--adapt-steps N``: online adaptation over the sequence (OnAVOS-style) -- before a frame after the first is segmented, N optimizer steps
    interleave the annotated first frame with the frame itself, trained against targets made on the device from the network's own confident
    output and the previous frame's mask, the rest void (osvos_pytorch_amd.adapt.OnlineAdapter)
  * ``--crf-iters N``: edge-aware refinement of every test frame's logit map against the decoded frame -- N mean-field steps of a local
    dense CRF on the device (osvos_pytorch_amd.refine.CrfRefiner); parameters --crf-radius, --crf-dilation, --crf-weights, --crf-thetas (starting values, not tuned on DAVIS)
  * ``--flow-search R``: motion compensation of what the test loop carries from frame to frame -- a block-matching motion field from the
    previous decoded frame to the current one on the device (osvos_pytorch_amd.flow.MotionCompensator) moves the previous mask of
    --adapt-steps and the seed of --track-components to where the object is now; parameters --flow-block, --flow-step, --flow-penalty,
    --flow-median (starting values, not tuned on DAVIS)
  * ``--snap-cell S``: superpixel snapping of every test frame's logit map, as in the OSVOS paper -- an integer grid-SLIC of cell S on the
    decoded frame and the mean of the logits over each superpixel, on the device (osvos_pytorch_amd.superpixels.SuperpixelSnapper); parameters --snap-compactness, --snap-iters (starting values, not tuned on DAVIS)
  * ``--match-gain G``: appearance matching to the annotated first frame -- every test frame's trunk features (``--match-layer`` 3, 6, 9 or
    12: conv2_2 .. conv5_3) are quantised to int8 and searched against the first frame's on the integer matrix pipe; G times (cosine to the
    nearest foreground feature minus cosine to the nearest background feature) is added to the fused logits on the device
    (osvos_pytorch_amd.match.AppearanceMatcher), in the test forward itself.  ``--match-previous`` also searches the previous frame's features under its final mask.  Not with --tta-*.
    ``--match-topk K`` scores a class by the mean cosine to its K best bank rows (VideoMatch), ``--match-local R[,GAIN]`` adds GAIN times a
    map searched only within R feature cells of each pixel in the previous frame (FEELVOS); both need --match-gain, off they change no byte.
    ``--match-memory ROWS[,TAU[,NEW[,MARGIN]]]`` searches a memory bank in place of the first frame's alone: the first frame's rows plus a ring
    of ROWS rows into which every frame writes, on the device, at most NEW of its rows that the bank does not hold yet (own-class cosine
    below TAU) and that the bank does not contradict (own minus other at least MARGIN), oldest rows first (osvos_pytorch_amd.match.MemoryBank);
    needs --match-gain, not with --adapt-steps, 0 = off changes no byte; TAU 0.9, NEW 512, MARGIN 0 are starting values, not tuned on DAVIS.
    ``--match-soft BETA[,balance]`` reads the bank with a softmax over all its rows (STM, STCN, XMem): a class scores 1 + ln(sum over its
    rows of exp(BETA (cosine - 1))) / BETA in place of its largest cosine (osvos_pytorch_amd.match.soft), ``balance`` subtracts
    ln(rows) / BETA per class; needs --match-gain, not with --match-topk above 1, off it changes no byte; BETA 10 is a starting value, not
    tuned on DAVIS.
    Starting values, not tuned on DAVIS; with G = 0 nothing is built and not one byte changes
  * ``--lucid P``: lucid first-frame synthesis -- with probability P a training sample is not the flipped / rotated / scaled frame but a
    re-composition of it: the object cut out, the hole inpainted once per sequence, object and background moved by affines of their own,
    re-lit and composited again on the device (osvos_pytorch_amd.lucid.LucidDream); parameters --lucid-grow, --lucid-smooth, --lucid-shift,
    --lucid-tone (starting values, not tuned on DAVIS).  With P = 0 not one random draw and not one byte changes.  ``--lucid-deform A[,CELL]``
    bends the object by a smooth displacement field, ``--lucid-occlude P`` hides part of it behind an ellipse of displaced background,
    ``--lucid-band R`` labels the pixels within R of a label edge void (-1: no count, no loss, no gradient; not with --window-fused); all
    three are off by default, and off they change no draw and no byte
  * ``--zoom MAXZOOM``: object-centred zoom of the test forwards -- on the device, a box around the previous frame's mask (a margin, at most
    MAXZOOM-fold enlargement, the canvas's aspect), the box's window of the decoded frame resampled onto one fixed canvas (``--zoom-canvas``,
    default the frame's size: the network keeps one input shape), the network on that, and its logits pasted back into the frame with
    ``--zoom-outside`` around them (osvos_pytorch_amd.roi.RoiZoom); frame 0 runs on the full frame.  Before --crf-iters, --snap-cell and
    --track-components, which keep running on the frame's grid.  Not with --tta-*, --match-gain or --adapt-steps.  ``--zoom-margin PCT,PX``.
    Starting values, not tuned on DAVIS; with MAXZOOM = 0 nothing is built and not one byte changes
  * ``--interactive ROUNDS[,STEPS0[,STEPS]]``: interactive segmentation from scribbles (Scribble-OSVOS, the baseline of the DAVIS interactive
    track) in place of the first-frame fine-tune -- strokes are rastered into a label map on the device, the network trains on the labelled
    pixels only (the rest void), a simulated annotator draws the skeleton of the largest error regions of the worst frame, and the rounds
    repeat (osvos_pytorch_amd.scribble, sequence.interactive_sequence); ``--scribbles FILE`` runs one round on a person's strokes in the
    DAVIS interactive JSON layout; --scribble-radius, --scribble-min-area, --scribble-prior.  Starting values, not tuned on DAVIS; without
    either option the script makes the calls it made and writes the bytes it wrote
  * the test phase -- which stage runs when, and what is carried from frame to frame -- is osvos_pytorch_amd.sequence for both recipes: the
    order is stated there, once, and asserted by tests/test_sequence_cpu.py; this file parses the options, fine-tunes, builds the stages
    (build_forward, build_post) and prints
  * launched under torchrun with N processes, rank r fine-tunes sequences r, r+N, ... of the
    comma-separated SEQ_NAME list (independent replicas: online training has no exchange step)
"""
from __future__ import division

import argparse
import os
import sys
import timeit

# ROCm maps HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  The backward uses three streams (data gradients / weight
# gradients / slab reduces); once a RCCL communicator adds its own, two of ours share a hardware queue and serialise (bench.py
# --force-dist: 217 vs 224 frames/s; this script with OSVOS_DP_FORCE=1: 2.169 vs 2.143 s per 512-frame epoch).  Eight queues restore it;
# without a communicator 4 and 8 measure the same.  A WARNING that cost this script 39 % for most of round 4: a stream that carries only
# H2D copies must not get a hardware queue of its own next to these -- with the input pipeline's former copy stream on a 5th queue every
# step stretched from 4.3 to 6.2 ms (profiles/r04_scripts_e2e.txt); the pipeline now copies on the consumer's stream (davis_io.py).
# Must be set before the HIP runtime initialises, i.e. before the first CUDA call of the process.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch

import networks.vgg_osvos as vo
from layers.osvos_layers import sigmoid_np  # noqa: F401  (kept importable like the reference)
from osvos_pytorch_amd import sequence
from osvos_pytorch_amd.autograd import PRECISIONS, TEST_PRECISIONS
from osvos_pytorch_amd.results import ComponentTracker, SequenceEvaluator, save_masks
from mypath import Path
from osvos_pytorch_amd.parallel import shard_indices
from osvos_pytorch_amd.train_common import TrainLoop, init_distributed, make_sgd


def synthetic_loader(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(1, 3, h, w, generator=g) * 40.0
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    gt = ((((yy - 0.5 * h) / (0.25 * h)) ** 2 + ((xx - 0.5 * w) / (0.25 * w)) ** 2) <= 1).float()[None, None]
    return [{'image': img, 'gt': gt, 'fname': ['00000']}]


def davis_loaders(db_root_dir, seq_name):
    try:
        from torchvision import transforms
        from torch.utils.data import DataLoader
        from dataloaders import davis_2016 as db
        from dataloaders import custom_transforms as tr
    except ImportError as e:
        raise SystemExit("DAVIS loading needs the reference's dataloaders package + cv2 + torchvision (%s); "
                         "use --synthetic to run without data" % e)
    composed = transforms.Compose([tr.RandomHorizontalFlip(), tr.ScaleNRotate(rots=(-30, 30), scales=(.75, 1.25)), tr.ToTensor()])
    db_train = db.DAVIS2016(train=True, db_root_dir=db_root_dir, transform=composed, seq_name=seq_name)
    db_test = db.DAVIS2016(train=False, db_root_dir=db_root_dir, transform=tr.ToTensor(), seq_name=seq_name)
    return DataLoader(db_train, batch_size=1, shuffle=True, num_workers=1), DataLoader(db_test, batch_size=1, shuffle=False, num_workers=1)


class DeviceTrainFrame(object):
    """train_online.py:92-97 on the device: the sequence's first frame + annotation live on the GPU as uint8; every pass through
    the 'loader' draws the reference's random flip / rotation / scale (same order, Python's random module) and runs one HIP kernel."""

    def __init__(self, img_u8, lab_u8, device, lucid=None):
        """lucid: None, or the keyword arguments of lucid.LucidDream plus 'p' (--lucid): per pass random.random() is drawn first, and below p
        the sample is a lucid one; with None nothing new is drawn and nothing new is built"""
        from osvos_pytorch_amd.augment import DeviceAugment
        self.img, self.lab = torch.as_tensor(img_u8).to(device), torch.as_tensor(lab_u8).to(device)
        self.aug = DeviceAugment(rots=(-30, 30), scales=(.75, 1.25))
        self.lucid_p, self.dream = 0.0, None
        if lucid:
            from osvos_pytorch_amd.lucid import LucidDream
            kw = dict(lucid)
            self.lucid_p = kw.pop('p')
            self.dream = LucidDream(self.img, self.lab, rots=self.aug.rots, scales=self.aug.scales, **kw)

    def __len__(self):
        return 1

    def __iter__(self):
        if self.dream is not None:
            import random
            s = self.dream() if random.random() < self.lucid_p else self.aug(self.img, self.lab)
        else:
            s = self.aug(self.img, self.lab)
        yield {'image': s['image'][None], 'gt': s['gt'][None]}


class DeviceTestFrames(object):
    """train_online.py:98-100 on the device: every frame of the sequence, decoded on the host a few frames ahead, mean-subtracted and
    laid out CHW by the augmentation kernel with the identity transform (the reference's test transform is ToTensor only)."""

    def __init__(self, frames, device, depth, raw_only=False):
        # raw_only (test-time augmentation makes its own views from 'frame_u8'): no identity pass, and no 'image', for a frame without annotation
        self.frames, self.device, self.depth, self.raw_only = frames, device, depth, raw_only

    def __len__(self):
        return len(self.frames)

    def __iter__(self):
        from osvos_pytorch_amd.augment import augment_frame
        from osvos_pytorch_amd.davis_io import DevicePrefetcher
        for idx, img, lab in DevicePrefetcher(self.frames, range(len(self.frames)), self.device, depth=self.depth):
            out = {'fname': [self.frames.fname(idx)], 'frame_u8': img}      # (the decoded frame: test-time augmentation)
            if lab is None and self.raw_only:
                yield out
                continue
            image, gt = augment_frame(img, lab, flip=False, rot=None)
            out['image'] = image[None]
            if lab is not None:
                out['gt'] = gt[None]
            yield out


def device_loaders(args, seq_name, device, seed):
    import random
    from osvos_pytorch_amd.davis_io import ArrayFrames, DavisFrames
    random.seed(seed)
    if args.synthetic:
        s = synthetic_loader(args.height, args.width, seed)[0]
        img = (s['image'][0].permute(1, 2, 0) + 116.0).clamp(0, 255).to(torch.uint8).numpy()
        lab = (s['gt'][0, 0] * 255).to(torch.uint8).numpy()
        # --synthetic-frames K: frame f is the seeded frame with image and ellipse moved right by 4 f pixels (columns wrap), annotated on every frame
        moved = [(np.roll(img, 4 * f, axis=1), np.roll(lab, 4 * f, axis=1)) for f in range(args.synthetic_frames)]
        train, test = ArrayFrames(moved[:1]), ArrayFrames(moved)
    else:
        train, test = DavisFrames(True, Path.db_root_dir(), seq_name=seq_name), DavisFrames(False, Path.db_root_dir(), seq_name=seq_name)
    img, lab = train[0]
    return DeviceTrainFrame(img, lab, device, args.lucid), DeviceTestFrames(test, device, args.prefetch, raw_only=bool(args.tta or args.roi))


def synthetic_objects(h, w):
    """uint8 [H,W] indexed annotation of the --synthetic --multi-object frame: two disjoint ellipses, ids 1 and 2"""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    lab = torch.zeros(h, w, dtype=torch.uint8)
    for k, cx in ((1, 0.28), (2, 0.72)):
        lab[(((yy - 0.5 * h) / (0.3 * h)) ** 2 + ((xx - cx * w) / (0.18 * w)) ** 2) <= 1] = k
    return lab.numpy()


def load_parent(args, save_dir, parentEpoch, device):
    net = vo.OSVOS(pretrained=0)
    parent = os.path.join(save_dir, 'parent_epoch-' + str(parentEpoch - 1) + '.pth')
    if os.path.exists(parent):
        net.load_state_dict(torch.load(parent, map_location=lambda storage, loc: storage))
    elif not args.synthetic:
        raise SystemExit('parent model %s not found' % parent)
    net.to(device)
    net.set_precision(args.precision)
    return net, make_sgd(net, 'online')


def fine_tune(args, net, optimizer, trainloader, device, nEpochs, nAveGrad, seed, snapshot_prefix):
    """train_online.py:129-170 of the reference: nEpochs passes over the (augmented) first frame, an optimizer step every nAveGrad of them"""
    snapshot = nEpochs
    loop = TrainLoop(net, optimizer, mode='online', n_ave_grad=nAveGrad)
    num_img_tr = len(trainloader)
    start_time = timeit.default_timer()
    window = []                      # --window-fused: the micro-batches of the open optimizer-step window
    for epoch in range(0, nEpochs):
        np.random.seed(seed + epoch)
        for ii, sample in enumerate(trainloader):
            inputs, gts = sample['image'], sample['gt']
            inputs, gts = inputs.to(device), gts.to(device)
            if args.window_fused:
                window.append((inputs, gts))
                if len(window) == nAveGrad:
                    loop.window_batch(torch.cat([w[0] for w in window]).requires_grad_(), torch.cat([w[1] for w in window]))
                    window = []
                continue
            inputs = inputs.detach().requires_grad_()      # (a fresh leaf: a frame the loader hands out again must not accumulate a .grad)
            if args.lucid_void:      # --lucid with --lucid-band: labels below 0 are void
                loop.micro_batch(inputs, gts, void_labels=True)
            else:
                loop.micro_batch(inputs, gts)
        if epoch % max(1, nEpochs // 20) == max(1, nEpochs // 20) - 1:
            running = loop.pop_running()[0] / (num_img_tr * max(1, nEpochs // 20))
            print('[Epoch: %d, numImages: %5d]' % (epoch + 1, num_img_tr))
            print('Loss: %f' % running)
        if (epoch % snapshot) == snapshot - 1 and epoch != 0:
            torch.save(net.state_dict(), snapshot_prefix + '_epoch-' + str(epoch) + '.pth')
    if device.type == 'cuda':
        torch.cuda.synchronize()
    print('Online training time: ' + str(timeit.default_timer() - start_time))


def need_decoded_frames(args, what, why):
    """the rule of every option that reads 'frame_u8': only the device input pipeline and the synthetic multi-object recipe deliver it"""
    if not (args.device_augment or (args.multi_object and args.synthetic)):
        raise SystemExit('%s --device-augment (or --multi-object --synthetic): %s' % (what, why))


def check_adapt_args(args):
    """the --adapt-* / --synthetic-frames rules; SystemExit on a combination the script does not run -- checked before any GPU work"""
    if args.synthetic_frames < 1:
        raise SystemExit('--synthetic-frames takes a frame count >= 1, got %d' % args.synthetic_frames)
    if args.synthetic_frames > 1 and not (args.synthetic and args.device_augment and not args.multi_object):
        raise SystemExit('--synthetic-frames needs --synthetic --device-augment (single-object loop): the moved frames are made for the device input pipeline')
    if args.adapt_steps < 0:
        raise SystemExit('--adapt-steps takes a step count >= 0, got %d' % args.adapt_steps)
    if not args.adapt_steps:
        return
    if args.multi_object:
        raise SystemExit('--adapt-steps runs in the single-object loop only: --multi-object fine-tunes one network per object and runs them pass '
                         'by pass, online adaptation needs each frame\'s final mask before the next frame')
    if not args.device_augment:
        raise SystemExit('--adapt-steps needs --device-augment: the first-frame steps re-augment the annotated frame on the device')
    if args.tta:
        raise SystemExit('--adapt-steps does not combine with --tta-scales / --tta-flip: the adapter returns its own final forward')
    if args.adapt_mix < 1:
        raise SystemExit('--adapt-mix takes a period >= 1, got %d' % args.adapt_mix)
    if not 0.0 < args.adapt_prob < 1.0:
        raise SystemExit('--adapt-prob takes a probability in (0, 1), got %r' % args.adapt_prob)
    if args.adapt_erosion < 0 or args.adapt_distance < 0:
        raise SystemExit('--adapt-erosion and --adapt-distance take pixel counts >= 0, got %d and %d' % (args.adapt_erosion, args.adapt_distance))
    if args.adapt_lr is not None and not args.adapt_lr > 0:
        raise SystemExit('--adapt-lr takes a learning rate > 0, got %r' % args.adapt_lr)


def tta_scales(args):
    """the scales of --tta-scales / --tta-flip (() = test-time augmentation off); SystemExit on a bad list -- checked before any GPU work"""
    from osvos_pytorch_amd import tta
    try:
        scales = tta.parse_scales(args.tta_scales)
        if not scales and not args.tta_flip:
            return ()
        scales = scales or (1.0,)
        tta.plan(args.height, args.width, scales, args.tta_flip)      # (duplicates and the view count; the real frame size is checked per frame)
    except ValueError as e:
        raise SystemExit('--tta-scales: %s' % e)
    return scales


def check_zoom_args(args):
    """the --zoom* rules; SystemExit on values or combinations the zoom does not take -- checked before any GPU work.  Sets args.roi to the
    keyword arguments of roi.RoiZoom, or None with --zoom 0"""
    from osvos_pytorch_amd import roi
    from osvos_pytorch_amd._glue import parse_numbers
    args.roi = None
    try:
        pct, px = parse_numbers(args.zoom_margin, (int, int), '--zoom-margin', expect='PCT,PX, two integers >= 0')
        canvas = None
        if args.zoom_canvas:
            sides = 'HxW with sides of 1..%d' % roi.MAX_SIDE
            canvas = parse_numbers(args.zoom_canvas, (int, int), '--zoom-canvas', sep='x', expect=sides)
            if not all(1 <= v <= roi.MAX_SIDE for v in canvas):
                raise ValueError('--zoom-canvas takes %s, got %r' % (sides, args.zoom_canvas))
        if args.zoom != 0 and not args.zoom >= 1:
            raise ValueError('--zoom takes the largest enlargement, a number >= 1 (0 = off), got %r' % args.zoom)
        roi.check_zoom(pct, px, args.zoom or 1.0)
        if args.zoom_outside != args.zoom_outside:
            raise ValueError('--zoom-outside takes a logit, got %r' % args.zoom_outside)
    except ValueError as e:
        raise SystemExit('--zoom*: %s' % e)
    if not args.zoom:
        return
    if args.tta:
        raise SystemExit('--zoom is not run together with --tta-scales / --tta-flip: the views of a crop are not built')
    if args.match_gain:
        raise SystemExit('--zoom is not run together with --match-gain: matching needs the crop of the trunk features, which is not built')
    if args.adapt_steps:
        raise SystemExit('--zoom is not run together with --adapt-steps: the adapter trains on the whole frame and returns its own final forward')
    need_decoded_frames(args, '--zoom needs', 'the crop is made from the decoded uint8 frame on the device')
    args.roi = dict(canvas=canvas, margin_pct=pct, margin_px=px, max_zoom=args.zoom, outside=args.zoom_outside)


def check_crf_args(args):
    """the --crf-* rules; SystemExit on values the refinement does not take -- checked before any GPU work.  Sets args.crf to the
    keyword arguments of refine.CrfRefiner, or None with --crf-iters 0"""
    from osvos_pytorch_amd import refine
    args.crf = None
    try:
        refine.check_window(args.crf_radius, args.crf_dilation, max(args.crf_iters, 0))
        if args.crf_iters < 0:
            raise ValueError('--crf-iters takes an iteration count >= 0 (0 = off), got %d' % args.crf_iters)
        w_a, w_s = refine.parse_pair(args.crf_weights, 2, '--crf-weights WA,WS')
        t_a, t_b, t_g = refine.parse_pair(args.crf_thetas, 3, '--crf-thetas A,B,G')
        refine.crf_coefficients(args.crf_radius, args.crf_dilation, w_a, w_s, t_a, t_b, t_g)
    except ValueError as e:
        raise SystemExit('--crf-*: %s' % e)
    if not args.crf_iters:
        return
    need_decoded_frames(args, '--crf-iters needs', 'the refinement reads the decoded uint8 frame on the device')
    args.crf = dict(iters=args.crf_iters, radius=args.crf_radius, dilation=args.crf_dilation, w_appearance=w_a, w_smooth=w_s, theta_alpha=t_a,
                    theta_beta=t_b, theta_gamma=t_g)


def check_flow_args(args):
    """the --flow-* rules; SystemExit on values or combinations the motion compensation does not take -- checked before any GPU work.  Sets
    args.flow to the keyword arguments of flow.MotionCompensator, or None with --flow-search 0"""
    from osvos_pytorch_amd import flow
    args.flow = None
    try:
        flow.check_flow(args.flow_search, args.flow_block, args.flow_step, args.flow_penalty, args.flow_median)
    except ValueError as e:
        raise SystemExit('--flow-*: %s' % e)
    if not args.flow_search:
        return
    if args.multi_object:
        raise SystemExit('--flow-search runs in the single-object loop only: the per-object trackers of --multi-object run over 64-frame chunks, '
                         'the motion field moves one frame\'s state to the next')
    if not args.device_augment:
        raise SystemExit('--flow-search needs --device-augment: the motion field is made from the decoded uint8 frames on the device (the other '
                         'loaders deliver no frame_u8, and only this one is known to deliver one frame per batch)')
    if not args.adapt_steps and args.track_components is None and not args.roi:
        raise SystemExit('--flow-search needs --adapt-steps or --track-components: it moves the previous mask of the one and the seed of the other')
    args.flow = dict(search=args.flow_search, block=args.flow_block, step=args.flow_step, penalty=args.flow_penalty, median=args.flow_median)


def check_snap_args(args):
    """the --snap-* rules; SystemExit on values the snapping does not take -- checked before any GPU work.  Sets args.snap to the keyword
    arguments of superpixels.SuperpixelSnapper, or None with --snap-cell 0"""
    from osvos_pytorch_amd import superpixels
    args.snap = None
    try:
        superpixels.check_superpixels(args.snap_cell or 2, args.snap_compactness, args.snap_iters)
    except ValueError as e:
        raise SystemExit('--snap-*: %s' % e)
    if not args.snap_cell:
        return
    need_decoded_frames(args, '--snap-cell needs', 'the superpixels are made from the decoded uint8 frame on the device')
    args.snap = dict(cell=args.snap_cell, compactness=args.snap_compactness, iters=args.snap_iters)


def check_match_args(args):
    """the --match-* rules; SystemExit on values the matching does not take -- checked before any GPU work.  Sets args.match to the keyword
    arguments of match.AppearanceMatcher, or None with --match-gain 0"""
    from osvos_pytorch_amd import match
    from osvos_pytorch_amd._glue import parse_numbers
    args.match = None
    try:
        match.check_match(args.match_layer, args.match_gain)
    except ValueError as e:
        raise SystemExit('--match-*: %s' % e)
    try:
        local_radius, local_gain = 0, 0.0
        if args.match_local:
            local_radius, local_gain = (parse_numbers(args.match_local, (int, float) if ',' in args.match_local else (int,), '--match-local',
                                                      expect='R or R,GAIN', finite=True) + (args.match_gain,))[:2]
        match.check_match_options(args.match_topk, local_radius, local_gain)
        memory = (0, 0.9, 512, 0.0)
        if args.match_memory:
            parts = args.match_memory.count(',') + 1
            memory = parse_numbers(args.match_memory, (int, float, int, float)[:parts] if parts <= 4 else (), '--match-memory',
                                   expect='ROWS[,TAU[,NEW[,MARGIN]]]', finite=True) + memory[parts:]
        match.check_memory(*memory)
        soft_beta, soft_balance = 0.0, False
        if args.match_soft:
            beta_text, comma, word = args.match_soft.partition(',')
            if comma and word.strip().lower() != 'balance':
                raise ValueError('--match-soft takes BETA or BETA,balance, got %r' % args.match_soft)
            soft_beta, soft_balance = parse_numbers(beta_text, (float,), '--match-soft', expect='BETA or BETA,balance', finite=True)[0], bool(comma)
            match.check_soft(soft_beta, soft_balance)
            if soft_beta > 0 and args.match_topk > 1:
                raise ValueError('--match-soft is not run together with --match-topk above 1: a softmax over the top k rows is not built')
    except ValueError as e:
        raise SystemExit('--match-*: %s' % e)
    if not args.match_gain:
        if soft_beta > 0:
            raise SystemExit('--match-soft needs --match-gain: it is an option of the appearance matcher')
        if args.match_topk != 1 or args.match_local:
            raise SystemExit('--match-topk / --match-local need --match-gain: they are options of the appearance matcher')
        if memory[0] > 0:
            raise SystemExit('--match-memory needs --match-gain: it is an option of the appearance matcher')
        return
    if args.tta:
        raise SystemExit('--match-gain is not run together with --tta-scales / --tta-flip: matching under test-time augmentation is not built')
    need_decoded_frames(args, '--match-gain needs', 'the first-frame bank is made on the device input pipeline')
    if args.match_previous and args.adapt_steps:
        raise SystemExit('--match-previous is not run together with --adapt-steps: the adapter forwards every frame twice')
    if local_gain > 0 and args.adapt_steps:
        raise SystemExit('--match-local is not run together with --adapt-steps: the adapter forwards every frame twice')
    if memory[0] > 0 and args.adapt_steps:
        raise SystemExit('--match-memory is not run together with --adapt-steps: the adapter forwards every frame twice, and the network '
                         'changes under the bank')
    args.match = dict(layer=args.match_layer, gain=args.match_gain, previous=args.match_previous)
    if args.match_topk > 1:          # (an option that is off adds nothing: AppearanceMatcher is built exactly as before)
        args.match.update(topk=args.match_topk)
    if local_gain > 0:
        args.match.update(local_radius=local_radius, local_gain=local_gain)
    if memory[0] > 0:
        args.match.update(zip(('memory', 'memory_tau', 'memory_new', 'memory_margin'), memory))
    if soft_beta > 0:
        args.match.update(soft_beta=soft_beta, soft_balance=soft_balance)


def check_lucid_args(args):
    """the --lucid* rules; SystemExit on values the synthesis does not take -- checked before any GPU work.  Sets args.lucid to the keyword
    arguments of DeviceTrainFrame's lucid (those of lucid.LucidDream, and p), or None with --lucid 0"""
    from osvos_pytorch_amd import lucid
    from osvos_pytorch_amd._glue import parse_numbers
    args.lucid = None
    two = 'two comma-separated numbers'
    try:
        radius, passes = parse_numbers(args.lucid_smooth, (int, int), '--lucid-smooth RADIUS,PASSES', expect=two)
        fg_shift, bg_shift = parse_numbers(args.lucid_shift, (float, float), '--lucid-shift FG,BG', expect=two)
        gain, offset = parse_numbers(args.lucid_tone, (float, int), '--lucid-tone GAIN,OFFSET', expect=two)
        deform, cell = (parse_numbers(args.lucid_deform, (float, int) if ',' in args.lucid_deform else (float,), '--lucid-deform',
                                      expect='A or A,CELL') + (128,))[:2]
        lucid.check_lucid(args.lucid_p, args.lucid_grow, radius, passes, fg_shift, bg_shift, gain, offset, deform, args.lucid_occlude,
                          args.lucid_band, cell)
    except ValueError as e:
        raise SystemExit('--lucid*: %s' % e)
    args.lucid_void = False          # fine_tune: the samples carry void labels
    if args.lucid_band > 0 and args.window_fused:
        raise SystemExit('--lucid-band does not combine with --window-fused: window_batch has no void rule')
    if args.lucid_band > 0 and os.environ.get('OSVOS_FUSED_LOSS_STEP', '1') == '0':
        raise SystemExit('--lucid-band needs the fused loss step (OSVOS_FUSED_LOSS_STEP is 0): the void rule lives in the HIP loss kernel')
    if not args.lucid_p:
        return
    if not args.device_augment:
        raise SystemExit('--lucid needs --device-augment: the samples are made from the decoded uint8 frame and its annotation on the device')
    args.lucid = dict(p=args.lucid_p, grow=args.lucid_grow, radius=radius, passes=passes, fg_shift=fg_shift, bg_shift=bg_shift, gain=gain,
                      offset=offset)
    if deform > 0:                   # (an option that is off adds nothing: LucidDream is built exactly as before)
        args.lucid.update(deform=deform, deform_cell=cell)
    if args.lucid_occlude > 0:
        args.lucid.update(occlude=args.lucid_occlude)
    if args.lucid_band > 0:
        args.lucid.update(band=args.lucid_band)
        args.lucid_void = True


def check_scribble_args(args):
    """the --interactive / --scribbles rules; SystemExit on values or combinations the interactive loop does not run -- checked before any GPU
    work.  Sets args.interactive to dict(rounds, steps0, steps, file), or None without either option"""
    from osvos_pytorch_amd import scribble
    from osvos_pytorch_amd._glue import parse_numbers
    args.interactive = None
    try:
        scribble.check_radius(args.scribble_radius)
        if args.scribble_min_area < 0:
            raise ValueError('--scribble-min-area takes a pixel count >= 0, got %d' % args.scribble_min_area)
        if not 0 <= args.scribble_prior <= 8192:
            raise ValueError('--scribble-prior takes a distance of 0..8192 pixels (0 = off), got %d' % args.scribble_prior)
        rounds, steps0, steps = 1, 200, 100          # starting values, not tuned on DAVIS
        if args.interactive_rounds:
            parts = args.interactive_rounds.count(',') + 1
            got = parse_numbers(args.interactive_rounds, (int, int, int)[:parts] if parts <= 3 else (), '--interactive', expect='ROUNDS[,STEPS0[,STEPS]]')
            rounds, steps0, steps = got + (rounds, steps0, steps)[parts:]
            if rounds < 1 or steps0 < 1 or steps < 1:
                raise ValueError('--interactive takes ROUNDS >= 1 and step counts >= 1, got %r' % args.interactive_rounds)
    except ValueError as e:
        raise SystemExit('--interactive / --scribble*: %s' % e)
    if not args.interactive_rounds and not args.scribbles:
        return
    if args.scribbles and args.interactive_rounds and rounds != 1:
        raise SystemExit('--scribbles runs ONE round on the strokes of the file in place of the simulated annotator: --interactive 1[,STEPS0] or none')
    refused = (('--multi-object', args.multi_object, 'the interactive loop trains one network on one object'),
               ('--window-fused', args.window_fused, 'window_batch has no void rule, and strokes label few pixels'),
               ('--lucid', args.lucid_p, 'the synthesis needs a complete first-frame mask'),
               ('--adapt-steps', args.adapt_steps, 'the adapter starts from a complete first-frame mask'),
               ('--match-*', args.match_gain or args.match_previous or args.match_topk != 1 or args.match_local or args.match_memory or args.match_soft,
                'the first-frame bank needs a complete first-frame mask'),
               ('--track-components', args.track_components is not None, 'the tracker is seeded with a complete first-frame mask'),
               ('--zoom', args.zoom, 'out of scope of the interactive loop'),
               ('--flow-search', args.flow_search, 'it moves the state of --adapt-steps and --track-components, which do not run here'),
               ('--test-precision', args.test_precision, 'the network keeps training between the predictions: one precision serves both'))
    for name, on, why in refused:
        if on:
            raise SystemExit('--interactive / --scribbles is not run together with %s: %s' % (name, why))
    if not args.device_augment:
        raise SystemExit('--interactive / --scribbles needs --device-augment: strokes are rastered, and the samples made, from the decoded frames on the device')
    if os.environ.get('OSVOS_FUSED_LOSS_STEP', '1') == '0':
        raise SystemExit('--interactive / --scribbles needs the fused loss step (OSVOS_FUSED_LOSS_STEP is 0): the void rule lives in the HIP loss kernel')
    args.interactive = dict(rounds=rounds, steps0=steps0, steps=steps, file=args.scribbles)


def interactive_sequence(args, seq_name, device, seed, save_dir, parentEpoch, nAveGrad):
    """Scribble-OSVOS on one sequence in place of the first-frame fine-tune: rounds of strokes (the simulated annotator's, or with --scribbles
    one round of a person's), training on the labelled pixels only, prediction and scoring of every frame (sequence.interactive_sequence);
    one line per round, one final line, the masks of the last round"""
    from osvos_pytorch_amd import scribble
    from osvos_pytorch_amd.augment import DeviceAugment
    from osvos_pytorch_amd.davis_io import DevicePrefetcher
    net, optimizer = load_parent(args, save_dir, parentEpoch, device)
    _, testloader = device_loaders(args, seq_name, device, seed)          # (seeds Python's random: the augmentation draws)
    frames, gts, names = [], [], []
    for idx, img, lab in DevicePrefetcher(testloader.frames, range(len(testloader.frames)), device, depth=args.prefetch):
        if lab is None:
            raise SystemExit('--interactive / --scribbles: frame %d of %s has no annotation; the annotator and the scores need the truth of every '
                             'frame (--synthetic-frames K, or a DAVIS sequence with all annotations)' % (idx, seq_name))
        frames.append(img)
        gts.append((lab > 127).to(torch.uint8))                           # the label map: object id 1
        names.append(os.path.basename(testloader.frames.fname(idx)))
    h, w = int(frames[0].shape[0]), int(frames[0].shape[1])
    it = args.interactive
    first = None
    if it['file']:
        try:
            paths, _ = scribble.load_davis_json(it['file'], (h, w))
            maps = scribble.rasterize(paths, (h, w), args.scribble_radius, len(frames), device)
        except (OSError, ValueError) as e:
            raise SystemExit('--scribbles: %s' % e)
        first = [(f, maps[f]) for f in sorted(set(p[0] for p in paths))]
        if not first:
            raise SystemExit('--scribbles: %s holds no stroke' % it['file'])
    print('Start of Interactive Training, sequence: ' + seq_name)
    session = scribble.InteractiveSession(net, optimizer, frames, 1, nAveGrad, DeviceAugment(rots=(-30, 30), scales=(.75, 1.25)), args.scribble_prior)
    robot = scribble.Robot(args.scribble_radius, args.scribble_min_area)
    post = build_post(args)
    assert post.pop('flow') is None and post.pop('make_tracker') is None      # (parse_args refuses both with --interactive)

    def round_line(r, rep):
        print('Interactive round %d on %s: frame %s annotated, %d labelled pixels, J %.4f F %.4f, fit %.3f s, predict %.3f s'
              % (r, seq_name, rep['frame'], rep['labelled'], rep['J'], rep['F'], rep['fit_s'], rep['predict_s']))

    report, fused = sequence.interactive_sequence(session, build_forward(args, net), post, it['rounds'], it['steps0'], it['steps'], gts, robot,
                                                  first=first, on_round=round_line)
    jf = [0.5 * (rep['J'] + rep['F']) for rep in report]
    print('Interactive J&F on %s per round: %s mean %.4f' % (seq_name, ' '.join('%.4f' % v for v in jf), sum(jf) / len(jf)))
    c = session.summary()
    print('Interactive strokes on %s: %d frames annotated, %d in the training rotation, %d left out (one class), %d micro-batches'
          % (seq_name, c['annotated'], c['training'], c['left_out'], c['micro_batches']))
    save_dir_res = os.path.join(save_dir, 'Results', seq_name)
    os.makedirs(save_dir_res, exist_ok=True)
    for out, name in zip(fused, names):
        save_masks(out, [os.path.join(save_dir_res, name + '.png')])


def build_forward(args, net, trainloader=None):
    """the sequence.FrameForward of a fine-tuned network: the --test-precision re-pack, then the stages that belong to one network, each None
    when its option is off -- test-time augmentation, the online adapter (with ``trainloader``: the single-object recipe) on a FRESH optimizer
    (no momentum carried over from the first-frame fine-tuning), the appearance matcher"""
    if args.test_precision:
        net.set_precision(args.test_precision)      # (re-packs the weights once: the FP16-pair packs are another format)
    tta = adapter = matcher = roi = None
    if args.roi:
        from osvos_pytorch_amd.roi import RoiZoom
        roi = RoiZoom(net.forward, **args.roi)
    if args.tta:
        from osvos_pytorch_amd.tta import TestTimeAugment
        tta = TestTimeAugment(net.forward, args.tta, args.tta_flip)
    if args.adapt_steps and trainloader is not None:
        from osvos_pytorch_amd.adapt import OnlineAdapter, first_frame_source
        optimizer = make_sgd(net, 'online', lr=args.adapt_lr) if args.adapt_lr is not None else make_sgd(net, 'online')
        adapter = OnlineAdapter(net, optimizer, first_frame_source(trainloader), steps=args.adapt_steps, mix=args.adapt_mix, weight=args.adapt_weight,
                                prob=args.adapt_prob, erosion=args.adapt_erosion, distance=args.adapt_distance)
    if args.match:
        from osvos_pytorch_amd.match import AppearanceMatcher
        matcher = AppearanceMatcher(net, **args.match)
    return sequence.FrameForward(net, tta, adapter, matcher, roi)


def build_post(args):
    """the stages that belong to no network, as keyword arguments of the sequences, each None when its option is off: flow, crf, snap,
    make_tracker (first_mask -> tracker: the tracker is seeded with the first annotation)"""
    from osvos_pytorch_amd.flow import MotionCompensator
    from osvos_pytorch_amd.refine import CrfRefiner
    from osvos_pytorch_amd.superpixels import SuperpixelSnapper
    return dict(flow=MotionCompensator(**args.flow) if args.flow else None, crf=CrfRefiner(**args.crf) if args.crf else None,
                snap=SuperpixelSnapper(**args.snap) if args.snap else None,
                make_tracker=(lambda first_mask: ComponentTracker(first_mask, args.track_components)) if args.track_components is not None else None)


def multi_object_sequence(args, seq_name, device, seed, save_dir, parentEpoch, nEpochs, nAveGrad):
    """DAVIS 2017 recipe for one sequence: one fine-tuning per object id of the first annotation on that object's binary mask, every frame
    through each network, the K logit stacks merged into label maps, indexed PNGs, J and F per object -- one read-back for the PNGs, one for
    the counts."""
    import random
    from osvos_pytorch_amd._lib import MAX_OBJECTS
    from osvos_pytorch_amd.augment import augment_frame
    from osvos_pytorch_amd.davis_io import ArrayFrames, DavisFrames, DevicePrefetcher, n_objects
    if args.synthetic:
        s = synthetic_loader(args.height, args.width, seed)[0]
        img = (s['image'][0].permute(1, 2, 0) + 116.0).clamp(0, 255).to(torch.uint8).numpy()
        test = ArrayFrames([(img, synthetic_objects(args.height, args.width))])
    else:
        test = DavisFrames(False, Path.db_root_dir(), seq_name=seq_name, indexed=True)
    # the sequence lives on the device as decoded uint8 for the K passes: 3 H W bytes per frame, H W more per annotated frame
    frames, gts, names = [], [], []
    for idx, img, lab in DevicePrefetcher(test, range(len(test)), device, depth=args.prefetch):
        frames.append(img)
        gts.append(lab)
        names.append(os.path.basename(test.fname(idx)))
    if not gts or gts[0] is None:
        raise SystemExit('--multi-object: sequence %s has no first annotation' % seq_name)
    K = n_objects(gts[0].cpu().numpy())
    if not 1 <= K <= MAX_OBJECTS:
        raise SystemExit('--multi-object: the first annotation of %s holds %d object ids (1..%d are supported)' % (seq_name, K, MAX_OBJECTS))
    print('Start of Online Training, sequence: %s (%d objects)' % (seq_name, K))

    def fine_tuned(k):
        net, optimizer = load_parent(args, save_dir, parentEpoch, device)
        random.seed(seed)                      # every object sees the augmentation draws of a single-object run
        trainloader = DeviceTrainFrame(frames[0], (gts[0] == k).to(torch.uint8) * 255, device, args.lucid)
        print('Object %d of %d' % (k, K))
        fine_tune(args, net, optimizer, trainloader, device, nEpochs, nAveGrad, seed, os.path.join(save_dir, '%s_object-%d' % (seq_name, k)))
        return net

    save_dir_res = os.path.join(save_dir, 'Results', seq_name)
    os.makedirs(save_dir_res, exist_ok=True)
    post = build_post(args)
    assert post.pop('flow') is None            # (parse_args refuses --flow-search with --multi-object)
    logits, trackers, started = sequence.multi_object_sequence(
        frames, gts, K, fine_tuned, lambda net: build_forward(args, net), lambda img: augment_frame(img, None, flip=False, rot=None)[0][None], **post)
    res = sequence.score_objects(logits, gts, [os.path.join(save_dir_res, n + '.png') for n in names])
    for k, o in enumerate(res['objects']):
        print('J&F on %s object %d: J %.4f F %.4f' % (seq_name, k + 1, o['J']['mean'], o['F']['mean']))
    print('J&F on %s (%d objects): %.4f' % (seq_name, K, res['J&F']))
    for k, t in enumerate(trackers):
        c = t.summary()
        print('Components kept on %s object %d: %d of %d over %d frames' % (seq_name, k + 1, c['kept'], c['seen'], c['frames']))
    print('Testing time multi-object: ' + str(timeit.default_timer() - started))


def parse_args(argv=None):
    """the command line, with every refusal that needs no GPU (bad lists, combinations the script does not run) raised as SystemExit"""
    ap = argparse.ArgumentParser()
    ap.add_argument('--synthetic', action='store_true', help='seeded synthetic 854x480 frame instead of DAVIS')
    ap.add_argument('--epochs', type=int, default=0, help='0 = reference value 2000 * nAveGrad')
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=854)
    ap.add_argument('--device-augment', action='store_true',
                    help='input pipeline on the GPU: Pillow decode -> pinned uint8 -> osvos_augment_frame (flip, scale+rotate, mean, CHW); '
                         'the first frame is decoded ONCE and re-augmented on the device every iteration')
    ap.add_argument('--prefetch', type=int, default=3, help='--device-augment: test frames decoded / copied ahead of the forward')
    ap.add_argument('--precision', default=os.environ.get('OSVOS_PRECISION', 'fp32x3'), choices=list(PRECISIONS), help="arithmetic of the network calls (OSVOS.set_precision): 'fp32x3' fp32-grade results on the bf16 matrix pipe, 'fp32' the exact fp32 kernels, 'fp32x3b2' / 'fp32x3h2' / 'fp32h2' / 'fp32x2' two pieces per operand, 'bf16' bf16 operands and trunk tensors, 'bf16w2' the same with two-piece forward weights")
    ap.add_argument('--test-precision', default=os.environ.get('OSVOS_TEST_PRECISION', ''), choices=[''] + list(TEST_PRECISIONS), help="precision of the TEST forwards, e.g. 'fp32h2' or 'bf16w2' "
                    "(train_online.py:172-189 of the reference; default: the training precision).  'fp32h2' -- the f32x3 "
                         "convolutions on two FP16 pieces under block exponents -- runs a forward 1.5x as fast as 'fp32x3' with logits closer to float64 "
                         "(DESIGN.md 3.1a); the masks are the same up to pixels within 1e-5 std of the threshold")
    ap.add_argument('--window-fused', action='store_true',
                    help='run the nAveGrad micro-batches of every optimizer step as ONE batch with per-image class counts (TrainLoop.window_batch): '
                         'the same gradient up to fp32 summation order, one set of kernel launches per optimizer step instead of nAveGrad')
    ap.add_argument('--multi-object', action='store_true',
                    help='DAVIS 2017: fine-tune one network per object id of the first (indexed) annotation, run every frame through each, give '
                         'each pixel the object with the highest logit (background when none passes 0.5), write indexed PNGs and report J and F '
                         'per object.  Needs --device-augment or --synthetic.  The fused logits of the whole sequence stay on the device until '
                         'the merge: 4 * K * frames * H * W bytes (under 1 GB for the largest DAVIS 2017 val sequence), next to the decoded '
                         'uint8 frames')
    ap.add_argument('--track-components', type=int, default=None, metavar='R',
                    help='clean every test frame\'s mask on the device before it is written and scored: of the connected components of the '
                         'thresholded mask keep those within R pixels (0..64) of what was kept of the previous frame, seeded with the first '
                         'annotation; when nothing was kept the next frame passes whole.  With --multi-object: one tracker per object')
    ap.add_argument('--tta-scales', default='', metavar='S1,S2,..',
                    help='test-time augmentation: run every test frame at these scales (view size floor(side * s + 0.5)), bring the logit maps '
                         'back to the frame\'s grid and average them on the device, before --track-components, the PNG writer and the evaluator.  '
                         'Costs about the sum of s^2 forwards per frame.  Needs the decoded uint8 frame: --device-augment, or --multi-object '
                         '--synthetic')
    ap.add_argument('--tta-flip', action='store_true',
                    help='test-time augmentation: every scale (scale 1 alone without --tta-scales) also runs mirrored, in the same batch; twice '
                         'the forwards')
    ap.add_argument('--adapt-steps', type=int, default=0, metavar='N',
                    help='online adaptation over the sequence (0 = off): before every frame after the first is segmented, N optimizer steps -- '
                         'every --adapt-mix-th on the frame itself against targets from the network\'s own confident output and the previous '
                         'frame\'s mask (the rest void), the others on the re-augmented annotated first frame.  Needs --device-augment; '
                         'single-object loop only; not with --tta-*')
    ap.add_argument('--adapt-mix', type=int, default=5, metavar='M', help='--adapt-steps: step k trains on the current frame when k %% M == M - 1')
    ap.add_argument('--adapt-prob', type=float, default=0.97, help='--adapt-steps: a pixel is a positive target above this probability')
    ap.add_argument('--adapt-erosion', type=int, default=15, help='--adapt-steps: the previous mask is eroded by this many pixels ...')
    ap.add_argument('--adapt-distance', type=int, default=220, help='... and pixels farther than this from what is left are negative targets')
    ap.add_argument('--adapt-weight', type=float, default=1.0, help='--adapt-steps: factor on the gradient of the current-frame steps')
    ap.add_argument('--adapt-lr', type=float, default=None, help='--adapt-steps: learning rate of the adaptation steps (default: the online rate)')
    ap.add_argument('--synthetic-frames', type=int, default=1, metavar='K',
                    help='--synthetic --device-augment: a sequence of K frames, frame f the seeded frame moved right by 4 f pixels, all annotated')
    ap.add_argument('--crf-iters', type=int, default=0, metavar='N',
                    help='edge-aware mask refinement (0 = off): N mean-field steps of a local dense CRF on every test frame\'s logit map '
                         'against the decoded frame, on the device, after the forward / --tta-* / --adapt-steps and before --track-components '
                         '(so --adapt-steps sees the refined mask as the previous mask).  Needs --device-augment, or --multi-object '
                         '--synthetic.  With --multi-object every object is refined as its own binary problem before the merge.  The '
                         'default parameters are starting values, not tuned on DAVIS')
    ap.add_argument('--crf-radius', type=int, default=5, help='--crf-iters: window radius 0..7 in steps of the dilation: (2 R + 1)^2 - 1 neighbours')
    ap.add_argument('--crf-dilation', type=int, default=3, help='--crf-iters: pixels between window taps; radius x dilation <= 16')
    ap.add_argument('--crf-weights', default='4,1', metavar='WA,WS',
                    help='--crf-iters: weights of the appearance and the smoothness kernel, in logits (each normalised by its kernel\'s mass)')
    ap.add_argument('--crf-thetas', default='8,13,3', metavar='A,B,G',
                    help='--crf-iters: standard deviations -- appearance kernel in pixels, in grey levels, smoothness kernel in pixels')
    ap.add_argument('--flow-search', type=int, default=0, metavar='R',
                    help='motion compensation (0 = off): before every test frame a block-matching motion field from the previous decoded frame '
                         'to this one is made on the device, over +-R pixels (at most 48), and the previous mask of --adapt-steps and the seed '
                         'of --track-components are moved along it.  Needs --device-augment and at least one of those two; single-object loop '
                         'only.  The default parameters are starting values, not tuned on DAVIS')
    ap.add_argument('--flow-block', type=int, default=16, help='--flow-search: side of the matched block, 1..32 pixels, centred on its cell')
    ap.add_argument('--flow-step', type=int, default=4, help='--flow-search: side of a cell, 1..32 pixels: one vector per cell')
    ap.add_argument('--flow-penalty', type=int, default=4, help='--flow-search: cost per pixel of |dx| + |dy|, in grey levels summed over the block')
    ap.add_argument('--flow-median', type=int, default=1, help='--flow-search: 3 x 3 median passes over the vector grid, 0..8')
    ap.add_argument('--snap-cell', type=int, default=0, metavar='S',
                    help='superpixel snapping (0 = off): every test frame\'s logit map is averaged over the superpixels of the decoded frame '
                         '-- an integer grid-SLIC with cells of S pixels (2..64) on the device -- after --crf-iters and before '
                         '--track-components, so that a region the image shows as one piece answers as one piece.  Needs --device-augment, '
                         'or --multi-object --synthetic.  With --multi-object the superpixels of a frame are computed once and shared by '
                         'the objects.  The default parameters are starting values, not tuned on DAVIS')
    ap.add_argument('--snap-compactness', type=int, default=10, help='--snap-cell: weight of the pixel distance against the colour distance, 0..64')
    ap.add_argument('--snap-iters', type=int, default=5, help='--snap-cell: assign / update steps, 0..16 (0: the grid cells themselves)')
    ap.add_argument('--match-gain', type=float, default=0.0, metavar='G',
                    help='appearance matching to the first frame (0 = off): the trunk features of every test frame are quantised to int8 and '
                         'searched against those of the annotated first frame on the device; G times (cosine to the nearest foreground feature '
                         'minus cosine to the nearest background feature) is added to the fused logits of the test forward, before '
                         '--adapt-steps uses them and before --crf-iters, --snap-cell and --track-components.  Needs --device-augment, or '
                         '--multi-object --synthetic; not with --tta-*.  With --multi-object one matcher per object\'s network.  The default '
                         'parameters are starting values, not tuned on DAVIS')
    ap.add_argument('--match-layer', type=int, default=9, help='--match-gain: the trunk tensor matched -- 3, 6, 9 or 12 (conv2_2, conv3_3, conv4_3, conv5_3)')
    ap.add_argument('--match-previous', action='store_true',
                    help='--match-gain: also search the previous frame\'s features under its final mask; each class takes the larger cosine.  '
                         'Not with --adapt-steps')
    ap.add_argument('--match-topk', type=int, default=1, metavar='K',
                    help='--match-gain: a class\'s score is the mean cosine to its K best bank rows (1..16; VideoMatch\'s averaging), so that one '
                         'mislabelled cell of the first frame no longer decides a region.  1 (the default) is the nearest row, as before')
    ap.add_argument('--match-local', default='', metavar='R[,GAIN]',
                    help='--match-gain: a third view (FEELVOS\'s local map) -- GAIN (default: G of --match-gain) times the map of a search '
                         'of the previous frame\'s features under its final mask that looks only R feature cells (0..15) around each '
                         'pixel; a class the window does not hold counts as cosine -1.  Independent of --match-previous.  Not with '
                         '--adapt-steps')
    ap.add_argument('--match-memory', default='', metavar='ROWS[,TAU[,NEW[,MARGIN]]]',
                    help='--match-gain: a memory bank of ROWS rows behind the first frame\'s (0 = off; as in STM and its successors) that '
                         'collects features over the sequence, on the device: after every frame at most NEW (default 512) of its rows are '
                         'written over the oldest memory rows, evenly subsampled from those the frame\'s mask labels object or background, '
                         'whose cosine to their own class in the bank is below TAU (default 0.9: the bank does not hold them yet) and at '
                         'least MARGIN (default 0) above the cosine to the other class (the bank does not contradict the mask).  The first '
                         'frame\'s rows are never overwritten.  The mask is the final one, with --multi-object each network\'s raw output.  '
                         'Not with --adapt-steps.  The defaults are starting values, not tuned on DAVIS')
    ap.add_argument('--match-soft', default='', metavar='BETA[,balance]',
                    help='--match-gain: the softmax readout of the bank (off by default; as STM, STCN and XMem read their memory) -- every '
                         'row of a class votes with weight exp(BETA (cosine - 1)) and the class scores 1 + ln(sum of its weights) / BETA in '
                         'place of its largest cosine, so that a few mislabelled or drifted rows are outvoted by the rows that look the same; '
                         'BETA in 0.0625..40.  With --match-previous the two banks combine as the softmax over their union; with '
                         '--match-memory the bank is still updated from the largest cosines and evolves exactly as without this option.  '
                         '",balance" subtracts ln(rows of the class) / BETA: the mean weight, so that the larger class carries no prior.  '
                         'Not with --match-topk above 1; --match-local is unchanged; runs with --adapt-steps wherever --match-gain alone '
                         'does.  BETA 10 is a starting value, not tuned on DAVIS')
    ap.add_argument('--lucid', dest='lucid_p', type=float, default=0.0, metavar='P',
                    help='lucid first-frame synthesis (0 = off): with probability P (0..1) a training sample is a re-composition of the '
                         'annotated frame -- the object cut out, the hole inpainted once per sequence, object and background moved by affines '
                         'of their own, re-lit and composited again on the device -- and otherwise the flipped / rotated / scaled frame as '
                         'before.  Needs --device-augment.  With --multi-object every object is handled as its own binary mask.  The '
                         'default parameters are starting values, not tuned on DAVIS')
    ap.add_argument('--lucid-grow', type=int, default=5, help='--lucid: the inpainted hole is the mask grown by this many pixels, 0..64')
    ap.add_argument('--lucid-smooth', default='2,3', metavar='RADIUS,PASSES',
                    help='--lucid: box smoothing of the filled hole -- window radius 1..8 and passes 0..8')
    ap.add_argument('--lucid-shift', default='0.25,0.05', metavar='FG,BG',
                    help='--lucid: largest shift of the object as a fraction of its bounding box (0..4) and of the background as a fraction of '
                         'the frame (0..1)')
    ap.add_argument('--lucid-tone', default='0.2,20', metavar='GAIN,OFFSET',
                    help='--lucid: each layer is re-lit with a gain of 1 +- GAIN (0..1) and an offset of +- OFFSET grey levels (0..255)')
    ap.add_argument('--lucid-deform', default='0', metavar='A[,CELL]',
                    help='--lucid: non-rigid deformation of the object (0 = off) -- a displacement field on a lattice of CELL pixels (a power of '
                         'two in 8..256, default 128), bilinear in between, each control point moved by up to A * CELL / 8 pixels (A in 0..1)')
    ap.add_argument('--lucid-occlude', type=float, default=0.0, metavar='P',
                    help='--lucid: with probability P (0..1, 0 = off) a lucid sample hides part of the object behind an ellipse of displaced '
                         'background, labelled background')
    ap.add_argument('--lucid-band', type=int, default=0, metavar='R',
                    help='--lucid: labels within R pixels (0..16, 0 = off) of a label edge of a lucid sample are void -- no count, no loss, '
                         'gradient 0.  Needs the fused loss step; not with --window-fused')
    ap.add_argument('--zoom', type=float, default=0.0, metavar='MAXZOOM',
                    help='object-centred zoom (0 = off): every test frame after the first is segmented on a crop around the previous frame\'s '
                         'mask -- the mask\'s box grown by --zoom-margin and to the canvas\'s aspect, never smaller than the canvas over MAXZOOM '
                         '(>= 1) -- resampled onto the canvas on the device, and the logits are pasted back into the frame, before --crf-iters, '
                         '--snap-cell and --track-components.  The single-object loop takes the box from the final mask, --multi-object from '
                         'each network\'s raw output.  Needs --device-augment, or --multi-object --synthetic; not with --tta-*, --match-gain '
                         'or --adapt-steps.  The default parameters are starting values, not tuned on DAVIS')
    ap.add_argument('--zoom-margin', default='25,8', metavar='PCT,PX',
                    help='--zoom: the tight box grows on every side by PCT percent of its longer side plus PX pixels')
    ap.add_argument('--zoom-canvas', default='', metavar='HxW', help='--zoom: the size of the network\'s input (default: the frame\'s size)')
    ap.add_argument('--zoom-outside', type=float, default=-20.0, metavar='V',
                    help='--zoom: the logit of every pixel outside the box (finite, so that --crf-iters and --snap-cell keep working on it)')
    ap.add_argument('--interactive', dest='interactive_rounds', default='', metavar='ROUNDS[,STEPS0[,STEPS]]',
                    help='interactive segmentation from scribbles (Scribble-OSVOS) in place of the first-frame fine-tune: round 0 trains STEPS0 '
                         '(default 200) optimizer steps on strokes through the first annotation\'s object and background, every later round '
                         'STEPS (default 100) more after a simulated annotator has drawn strokes through the largest errors of the worst frame; '
                         'unlabelled pixels are void.  Every round predicts and scores all frames; the masks of the last round are written.  '
                         'Needs --device-augment, the single-object loop and the truth of every frame (--synthetic-frames K, or a DAVIS '
                         'sequence with all annotations).  With --tta-*, --crf-iters, --snap-cell; not with --multi-object, --window-fused, '
                         '--lucid, --adapt-steps, --match-*, --track-components, --zoom, --flow-search, --test-precision.  The defaults are '
                         'starting values, not tuned on DAVIS')
    ap.add_argument('--scribbles', default='', metavar='FILE',
                    help='one interactive round on a person\'s strokes in place of the simulated annotator\'s: a JSON file in the DAVIS '
                         'interactive layout {"scribbles": [per frame: [{"path": [[x, y], ..], "object_id": k}, ..]]}, x and y in 0..1')
    ap.add_argument('--scribble-radius', type=int, default=3, help='--interactive / --scribbles: half the width of a stroke, 0..64 pixels')
    ap.add_argument('--scribble-min-area', type=int, default=64, help='--interactive: error regions below this many pixels get no stroke')
    ap.add_argument('--scribble-prior', type=int, default=0, metavar='D',
                    help='--interactive: from the second round on, unlabelled pixels farther than D pixels from every stroke are trained towards '
                         'the previous round\'s mask instead of being void (0 = off)')
    args = ap.parse_args(argv)
    check_scribble_args(args)
    args.tta = tta_scales(args)
    check_adapt_args(args)
    check_zoom_args(args)
    check_crf_args(args)
    check_flow_args(args)
    check_snap_args(args)
    check_lucid_args(args)
    check_match_args(args)
    if args.tta:
        need_decoded_frames(args, '--tta-scales / --tta-flip need', 'test-time augmentation makes its views from the decoded uint8 frame on the device')
    if args.track_components is not None and not 0 <= args.track_components <= 64:
        raise SystemExit('--track-components takes a radius of 0..64 pixels, got %d' % args.track_components)
    if args.multi_object and not (args.device_augment or args.synthetic):
        raise SystemExit('--multi-object needs --device-augment or --synthetic: the per-object labels are made on the device input pipeline')
    return args


def main():
    args = parse_args()
    rank, world, device = init_distributed(collectives=False)      # sequences are sharded over the ranks: nothing is exchanged
    seqs = os.environ.get('SEQ_NAME', 'blackswan').split(',')
    save_dir = Path.save_root_dir()
    os.makedirs(save_dir, exist_ok=True)
    nAveGrad = 5
    nEpochs = args.epochs or 2000 * nAveGrad
    parentEpoch = 240
    seed = 0

    for si in shard_indices(len(seqs), rank, world):
        seq_name = seqs[si]
        if args.multi_object:
            multi_object_sequence(args, seq_name, device, seed + si, save_dir, parentEpoch, nEpochs, nAveGrad)
            continue
        if args.interactive:
            interactive_sequence(args, seq_name, device, seed + si, save_dir, parentEpoch, nAveGrad)
            continue
        net, optimizer = load_parent(args, save_dir, parentEpoch, device)
        if args.device_augment:
            trainloader, testloader = device_loaders(args, seq_name, device, seed + si)
        elif args.synthetic:
            trainloader = testloader = synthetic_loader(args.height, args.width, seed + si)
        else:
            trainloader, testloader = davis_loaders(Path.db_root_dir(), seq_name)
        print('Start of Online Training, sequence: ' + seq_name)
        fine_tune(args, net, optimizer, trainloader, device, nEpochs, nAveGrad, seed, os.path.join(save_dir, seq_name))

        save_dir_res = os.path.join(save_dir, 'Results', seq_name)
        os.makedirs(save_dir_res, exist_ok=True)
        print('Testing Network')
        evaluator = SequenceEvaluator()      # J and F counts stay on the device: one read-back after the last frame
        forward = build_forward(args, net, trainloader)
        frames = sequence.SingleObjectSequence(testloader, forward, device, seq_name, **build_post(args))
        for fname, fused, gt in frames:
            # sigmoid + scipy<=1.1 imsave byte scaling on the device, PNG written by osvos_pytorch_amd.results (reference :181-187)
            save_masks(fused, [os.path.join(save_dir_res, os.path.basename(fname[jj]) + '.png') for jj in range(int(fused.size()[0]))])
            if gt is not None:
                evaluator.add(fused, gt.to(device))
        tracker, adapter = frames.tracker, forward.adapter
        if evaluator.frames:
            res = evaluator.summary()
            st = res['J']
            print('J (region similarity) on %s: mean %.4f recall %.4f decay %.4f over %d frames' % (seq_name, st['mean'], st['recall'], st['decay'], res['frames']))
            st = res['F']
            print('F (contour accuracy) on %s: mean %.4f recall %.4f decay %.4f over %d frames' % (seq_name, st['mean'], st['recall'], st['decay'], res['frames']))
            print('J&F on %s: %.4f' % (seq_name, res['J&F']))
        if tracker is not None:
            c = tracker.summary()
            print('Components kept on %s: %d of %d over %d frames' % (seq_name, c['kept'], c['seen'], c['frames']))
        if adapter is not None:
            c = adapter.summary()
            print('Online adaptation on %s: %d frames seen, %d adapted, %d skipped, %d steps' % (seq_name, c['adapted'] + c['skipped'], c['adapted'],
                                                                                                c['skipped'], c['steps']))


if __name__ == '__main__':
    sys.exit(main())
