"""ctypes binding of libosvos_hip.so (C ABI: include/osvos_hip.h).  Fails loudly: there is no
CPU or PyTorch fallback for any compute entry point."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import threading

# (GPU_MAX_HW_QUEUES -- how many hardware queues ROCm maps the process's HIP streams onto -- is the CALLER's choice and must be made before
# the first GPU call: the scripts and bench.py ask for 8; see the note at the top of train_parent.py.)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libosvos_hip.so")
CSRC = os.path.join(_HERE, "csrc")
_lock = threading.Lock()
_lib = None

F32, BF16, F32_BF16MFMA, F32_X3 = 0, 1, 2, 3
DEFER_JOIN = 0x200         # OSVOS_FLAG_DEFER_JOIN: osvos_net_backward leaves the side streams un-joined (autograd.NetRuntime.join_backward)
X3_TWO_PIECES = 0x800       # OSVOS_FLAG_X3_TWO_PIECES: precision 'fp32x2' (two bf16 pieces per operand, three products)
X3_HALF_PIECES = 0x1000     # OSVOS_FLAG_X3_HALF_PIECES: precision 'fp32h2' (two FP16 pieces under block exponents, three products); on net_pack: forward packs
X3_HALF_PIECES_BWD = 0x2000 # OSVOS_FLAG_X3_HALF_PIECES_BWD: net_pack only -- data-gradient packs in the FP16-pair format
BF16_W2 = 0x4000            # OSVOS_FLAG_BF16_W2: precision 'bf16w2' (dtype F32_BF16MFMA only) -- two-piece forward weight packs, two products per product
INFERENCE = 0x400           # OSVOS_FLAG_INFERENCE: osvos_net_forward writes nothing only a backward would read (sign bits, pool codes)
MAX_OBJECTS = 16            # OSVOS_MAX_OBJECTS: object ids per label map (osvos_merge_objects, osvos_labels_jf_counts)
BOUNDARY_MAX_RADIUS = 64    # OSVOS_BOUNDARY_MAX_RADIUS: largest disk radius (osvos_mask_jf_counts, osvos_components_select)
TTA_MAX_VIEWS = 16          # OSVOS_TTA_MAX_VIEWS: logit maps per osvos_tta_fuse call
ROI_BOX_PARTS = 64          # OSVOS_ROI_BOX_PARTS: osvos_roi_box takes 16 * ROI_BOX_PARTS bytes of workspace per frame
CRF_MAX_RADIUS = 7          # OSVOS_CRF_MAX_RADIUS: largest window radius of osvos_crf_refine
CRF_MAX_REACH = 16          # OSVOS_CRF_MAX_REACH: largest radius * dilation
CRF_MAX_ITERS = 64          # OSVOS_CRF_MAX_ITERS: mean-field iterations per osvos_crf_refine call
FLOW_MAX_BLOCK = 32         # OSVOS_FLOW_MAX_BLOCK: largest matching block side of osvos_flow_block_match
FLOW_MAX_STEP = 32          # OSVOS_FLOW_MAX_STEP: largest grid step (osvos_flow_block_match, osvos_flow_warp)
FLOW_MAX_SEARCH = 48        # OSVOS_FLOW_MAX_SEARCH: largest search range, pixels on every side
FLOW_MAX_PENALTY = 65535    # OSVOS_FLOW_MAX_PENALTY: largest cost per pixel of |dx| + |dy|
FLOW_MAX_MEDIAN = 8         # OSVOS_FLOW_MAX_MEDIAN: median passes over the vector grid
FLOW_MAX_SIDE = 16384       # OSVOS_FLOW_MAX_SIDE: largest H / W of the flow calls
SUPERPIXELS_MAX_CELL = 64   # OSVOS_SUPERPIXELS_MAX_CELL: largest cell side of osvos_superpixels_slic (the smallest is 2)
SUPERPIXELS_MAX_COMPACTNESS = 64  # OSVOS_SUPERPIXELS_MAX_COMPACTNESS: largest weight of the pixel distance
SUPERPIXELS_MAX_ITERS = 16  # OSVOS_SUPERPIXELS_MAX_ITERS: assign / update steps per osvos_superpixels_slic call
SUPERPIXELS_MAX_SIDE = 16384  # OSVOS_SUPERPIXELS_MAX_SIDE: largest H / W of the superpixel calls
SUPERPIXELS_MAX_K = 268435456  # OSVOS_SUPERPIXELS_MAX_K: most labels per frame of osvos_superpixels_pool
MATCH_MAX_C = 1024          # osvos_match_*: most channels (a multiple of 64, from 64)
MATCH_MAX_P = 1 << 20       # osvos_match_nearest: most query / reference rows per frame
MATCH_MAX_K = 16            # OSVOS_MATCH_MAX_K: most rows osvos_match_topk averages per class
MATCH_MAX_RADIUS = 15       # OSVOS_MATCH_MAX_RADIUS: largest window radius of osvos_match_local, in cells
MATCH_MIN_BETA = 0.0625     # OSVOS_MATCH_MIN_BETA: smallest temperature of osvos_match_soft
MATCH_MAX_BETA = 40.0       # OSVOS_MATCH_MAX_BETA: largest (no weight exp(beta (cos - 1)) is denormal)
SQDIST_NONE = 2147483647    # OSVOS_SQDIST_NONE: osvos_mask_sqdist's value in an image without a source pixel
SQDIST_MAX_SIDE = 4096      # OSVOS_SQDIST_MAX_SIDE: largest H / W of osvos_mask_sqdist and osvos_adapt_targets
LUCID_MAX_BATCH = 16        # OSVOS_LUCID_MAX_BATCH: samples per osvos_lucid_compose launch
LUCID_MAX_SIDE = 4096       # OSVOS_LUCID_MAX_SIDE: largest H / W of osvos_lucid_compose (osvos_lucid_inpaint: SQDIST_MAX_SIDE)
LUCID_MAX_RADIUS = 8        # OSVOS_LUCID_MAX_RADIUS: largest smoothing window radius of osvos_lucid_inpaint (the smallest is 1)
LUCID_MAX_PASSES = 8        # OSVOS_LUCID_MAX_PASSES: smoothing passes per osvos_lucid_inpaint call
LUCID_MAX_GAIN = 1024       # OSVOS_LUCID_MAX_GAIN: largest Q8 tone gain of osvos_lucid_compose (256 = 1)
LUCID_MAX_BAND = 16         # OSVOS_LUCID_MAX_BAND: widest void band of osvos_lucid_compose_ex, pixels
LUCID_MIN_CELL = 8          # OSVOS_LUCID_MIN_CELL: smallest lattice cell of the deformation field (a power of two)
LUCID_MAX_CELL = 256        # OSVOS_LUCID_MAX_CELL: largest lattice cell
LUCID_MAX_OCC_RADIUS = 4096  # OSVOS_LUCID_MAX_OCC_RADIUS: largest occluder semi-axis
LUCID_MAX_OCC_OFFSET = 8192  # OSVOS_LUCID_MAX_OCC_OFFSET: largest |centre| and |source offset| of an occluder
SCRIBBLE_MAX_SEGMENTS = 65535  # OSVOS_SCRIBBLE_MAX_SEGMENTS: most rows of osvos_scribble_raster's segment table
SCRIBBLE_MAX_RADIUS = 64    # OSVOS_SCRIBBLE_MAX_RADIUS: largest stroke radius
SCRIBBLE_LIST_CAP = 512     # OSVOS_SCRIBBLE_LIST_CAP: rows of a tile's LDS list; more survivors take more passes
THIN_MAX_ITERS = 512        # OSVOS_THIN_MAX_ITERS: most iterations of osvos_mask_thin
THIN_RESIDENT_WORDS = 8000  # OSVOS_THIN_RESIDENT_WORDS: largest 1-bit plane, in 64-bit words, that path 1 keeps in LDS
GENERIC_DECONV = 0x100    # OSVOS_FLAG_GENERIC_DECONV: OR-ed into the dtype of the osvos_net_* calls
NPARAMS = 52
# the slot groups of the 52 parameters / gradients in state_dict order (csrc/common.h, namespace slot, names them for the C side)
SLOTS_UPSCALE = range(0, 4)         # slot::upscale(i): upscale[i].weight, the fused head's deconvolutions
SLOTS_UPSCALE_SIDE = range(4, 8)    # slot::upscale_(i): upscale_[i].weight, the side heads'
SLOTS_CONV = range(8, 42)           # slot::conv_w(l), conv_b(l): (weight, bias) pairs of the 13 trunk convolutions, then of side_prep[0..3]
SLOTS_SCORE_DSN = range(42, 50)     # slot::score_dsn_w(i), score_dsn_b(i)
SLOTS_FUSE = range(50, 52)          # slot::fuse_w, fuse_b

_vp, _i, _l, _sz, _f = C.c_void_p, C.c_int, C.c_long, C.c_size_t, C.c_float

# name -> (restype, argtypes); every symbol declared in include/osvos_hip.h
PROTOTYPES = {
    "osvos_version": (_i, []),
    "osvos_last_error": (C.c_char_p, []),
    "osvos_nchw_to_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_nhwc_to_nchw": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_wpack_bytes": (_sz, [_i, _i, _i]),
    "osvos_pack_conv3x3_fwd": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "osvos_wpack_dgrad_bytes": (_sz, [_i, _i, _i]),
    "osvos_pack_conv3x3_dgrad": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "osvos_conv3x3": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_num_tiles": (_i, []),
    "osvos_conv3x3_f32x3_tiles": (_i, []),
    "osvos_wpack_x3_bytes_abi": (_sz, [_i, _i, _i]),
    "osvos_pack_conv3x3_x3": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "osvos_conv3x3_x3": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_x3_streamk_ws_bytes": (_sz, []),
    "osvos_conv3x3_x3_streamk_ticket_bytes": (_sz, []),
    "osvos_conv3x3_x3_streamk": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "osvos_conv3x3_splitk_ws_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "osvos_conv3x3_splitk": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "osvos_conv3x3_bf16io": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_wgrad_bf16act": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2_bf16act": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2_bwd_bf16act": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2_bf16act_code": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2_bwd_bf16act_code": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_bf16act_fused": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_bf16io_tiles": (_i, [_vp, _i]),
    "osvos_conv3x3_bf16w2_fused": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "osvos_conv3x3_bf16w2_tiles": (_i, [_vp, _i]),
    "osvos_set_x3_pieces": (_i, [_i]),
    "osvos_nchw_to_nhwc_bf16copy": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2_bf16copy": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2_bwd_bf16copy": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_dgrad_c3": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_dgrad_c3_bf16mma": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_wgrad_ws_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "osvos_conv3x3_wgrad": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_wgrad_c3_bf16dy": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_wgrad_c3_plan": (_i, [_i, _i, _i, _i, _vp]),
    "osvos_wgrad_wide_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_wgrad_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_conv3x3_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "osvos_maxpool2x2_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "osvos_head_lowres": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_head_upsample": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "osvos_head_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_deconv_diag_check": (_i, [_vp, _i, _i, _vp, _vp]),
    "osvos_cbce": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _vp]),
    "osvos_cbce_step": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _f, _vp, _vp]),
    "osvos_cbce_step_multi": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp, _vp, _vp]),
    "osvos_cbce_scratch_bytes": (_sz, [_i, _i, _i]),
    "osvos_cbce_step_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "osvos_scale": (_i, [_vp, _vp, _vp, _l, _vp]),
    "osvos_net_wbuf_bytes": (_sz, [_i]),
    "osvos_net_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "osvos_net_ws_bytes_infer": (_sz, [_i, _i, _i, _i]),
    "osvos_net_pack": (_i, [_vp, _vp, _i, _i, _vp]),
    "osvos_net_forward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "osvos_net_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "osvos_net_arm_grad_events": (_i, [_vp, _i]),
    "osvos_net_join": (_i, [_vp, _vp, _vp]),
    "osvos_comm_unique_id": (_i, [_vp]),
    "osvos_comm_init": (_i, [_vp, _i, _i, _vp]),
    "osvos_comm_allreduce_f32": (_i, [_vp, _vp, _sz, _vp]),
    "osvos_comm_allreduce_f64": (_i, [_vp, _vp, _sz, _vp]),
    "osvos_comm_allreduce_chunks_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "osvos_comm_destroy": (_i, [_vp]),
    "osvos_net_ws_query": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "osvos_net_ws_format": (_i, [_i, _i]),
    "osvos_augment_frame": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "osvos_mask_to_bytes": (_i, [_vp, _vp, _vp, _l, _i, _vp]),
    "osvos_mask_iou_counts": (_i, [_vp, _vp, _vp, _l, _i, _f, _vp]),
    "osvos_boundary_ws_bytes": (_sz, [_i, _i, _i]),
    "osvos_mask_jf_counts": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _vp]),
    "osvos_merge_objects": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "osvos_labels_jf_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "osvos_labels_jf_counts": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_components_ws_bytes": (_sz, [_i, _i, _i]),
    "osvos_mask_components": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "osvos_components_select": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "osvos_tta_view": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_tta_fuse": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    "osvos_roi_box": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "osvos_roi_view": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "osvos_roi_paste": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "osvos_crf_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "osvos_crf_refine": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _vp]),
    "osvos_flow_ws_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "osvos_flow_block_match": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_flow_warp": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "osvos_superpixels_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "osvos_superpixels_slic": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_superpixels_pool_ws_bytes": (_sz, [_i, _i]),
    "osvos_superpixels_pool": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "osvos_match_quantize": (_i, [_vp, _i, _vp, _vp, _l, _i, _vp]),
    "osvos_match_cell_labels": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_match_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "osvos_match_nearest": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "osvos_match_topk_ws_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "osvos_match_topk": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_match_local": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_match_bank_ws_bytes": (_sz, [_i, _i]),
    "osvos_match_bank_update": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _vp]),
    "osvos_match_soft_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "osvos_match_soft": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "osvos_lucid_inpaint_ws_bytes": (_sz, [_i, _i, _i]),
    "osvos_lucid_inpaint": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "osvos_lucid_compose": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "osvos_lucid_compose_ex_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "osvos_lucid_compose_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "osvos_mask_sqdist_ws_bytes": (_sz, [_i, _i, _i]),
    "osvos_mask_sqdist": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "osvos_adapt_ws_bytes": (_sz, [_i, _i, _i]),
    "osvos_adapt_targets": (_i, [_vp, _vp, _f, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "osvos_scribble_raster": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "osvos_mask_thin_ws_bytes": (_sz, [_i, _i, _i]),
    "osvos_mask_thin": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "osvos_sgd_step": (_i, [_vp, _vp, _vp, _l, _f, _f, _f, _i, _vp]),
    "osvos_sgd_step_multi": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _i, _vp]),
    "osvos_prof_start": (_i, [_i]),
    "osvos_prof_stop": (_i, [_vp, _vp, _vp]),
    "osvos_prof_pause": (_i, [_i]),
    "osvos_debug_conv3x3_naive": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "osvos_debug_mfma_layout": (_i, [_vp, _vp]),
    "osvos_debug_mfma_peak": (_i, [_vp, _i, _i, _vp]),
    "osvos_debug_mfma_peak_bf16": (_i, [_vp, _vp, _i, _i, _vp]),
    "osvos_debug_set_c3_bf16": (_i, [_i]),
    "osvos_debug_lds_dma": (_i, [_vp, _i, _vp, _vp]),
}


def build(force: bool = False) -> str:
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("libosvos_hip.so is not built and hipcc was not found; run `make -C %s`" % CSRC)
    cmd = ["make", "-C", CSRC, "-j8", "-s", "HIPCC=" + hipcc]
    import fcntl
    with open(os.path.join(CSRC, ".build.lock"), "w") as lk:      # ranks of one torchrun launch must not race in make
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if force:
                subprocess.check_call(cmd + ["clean"])
            subprocess.check_call(cmd)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)
    return SO_PATH


def _stale() -> bool:
    if not os.path.exists(SO_PATH):
        return True
    t = os.path.getmtime(SO_PATH)
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".cpp", ".h")) and os.path.getmtime(os.path.join(CSRC, f)) > t:
            return True
    return os.path.getmtime(os.path.join(_HERE, "..", "include", "osvos_hip.h")) > t


def lib() -> C.CDLL:
    """The loaded library.  Builds it first when it is missing or older than its sources and a
    compiler is available; raises RuntimeError otherwise (never falls back to another path)."""
    global _lib
    with _lock:
        if _lib is None:
            # torch first: the process must end up with ONE HIP runtime (the libamdhip64 torch
            # ships); loading ours before torch's makes hipMemsetAsync & co see no device
            import torch  # noqa: F401
            if _stale() and os.environ.get("OSVOS_AUTOBUILD", "1") != "0":
                build()
            try:
                l = C.CDLL(SO_PATH)
            except OSError as e:  # pragma: no cover
                raise RuntimeError("cannot load %s: %s" % (SO_PATH, e))
            for name, (res, args) in PROTOTYPES.items():
                fn = getattr(l, name)          # AttributeError = ABI mismatch: fail loudly
                fn.restype = res
                fn.argtypes = args
            _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().osvos_last_error().decode(errors="replace")
        raise RuntimeError("libosvos_hip %s failed (rc=%d): %s" % (what, rc, msg))


def ptr_array(ptrs):
    """Host array of device pointers (ints or None)."""
    arr = (C.c_void_p * len(ptrs))(*[C.c_void_p(p) if p else None for p in ptrs])
    return arr
