/* osvos_hip.h -- C ABI of libosvos_hip.so: the MI355X (gfx950) OSVOS forward/backward hot path.
 *
 * The reference (kmaninis/OSVOS-PyTorch) has no FFI boundary of its own: its "operator API" is
 * torch.nn.Module + autograd and every arithmetic op is delegated to ATen.  This header is the
 * boundary a maintainer binds instead (INTEGRATION.md shows the ctypes stub).  Each entry point
 * cites the reference call site whose ATen op(s) it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; the caller (PyTorch) owns all
 *     memory, including workspaces; the library never allocates, frees or synchronises
 *   - every function enqueues on `stream` (a hipStream_t passed as void*) and returns
 *     0 on success, >0 a hipError_t, <0 an argument error; osvos_last_error() has the text
 *   - activations are NHWC ("channels last") float32 (dtype 0) or bfloat16 (dtype 1) unless
 *     a parameter says nchw; parameters arrive in the reference's state_dict layout (OIHW fp32)
 *   - re-entrant: no mutable global state except the per-thread error string
 */
#ifndef OSVOS_HIP_H
#define OSVOS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSVOS_ABI_VERSION 1
#define OSVOS_F32 0
#define OSVOS_BF16 1          /* bf16 tensors in HBM: reserved, not built */
#define OSVOS_F32_BF16MFMA 2  /* fp32 tensors in HBM; conv forward/data-gradient operands rounded to bf16 (RNE) while
                                 staged into LDS, v_mfma_f32_32x32x16_bf16 with fp32 accumulate; everything else fp32 */
#define OSVOS_FLAG_GENERIC_DECONV 0x100  /* OR-ed into the dtype of osvos_net_pack / osvos_net_forward / osvos_net_backward (and the *_bytes queries):
                                            upscale[i].weight is NOT diagonal with one shared filter -> the generic transposed-convolution head
                                            (head_generic.hip) runs instead of the commuted one, and gradients of upscale / upscale_ weights
                                            are written when their grads[] entries (0..7) are non-NULL */
#define OSVOS_FLAG_DEFER_JOIN 0x200      /* OR-ed into the dtype of osvos_net_backward: do NOT make `stream` wait for the weight-gradient work still
                                            running on aux_stream / aux2_stream when the call returns (the data-gradient chain, dx and everything the
                                            caller's next forward needs ARE complete in stream order).  The caller owes one osvos_net_join before it reads
                                            a parameter gradient on `stream` (optimizer step, all-reduce) and must keep `ws` alive until then.  Lets the
                                            tail of the weight gradients run under the next micro-batch's forward (gradient-accumulation loops). */
#define OSVOS_FLAG_INFERENCE 0x400       /* OR-ed into the dtype of osvos_net_forward: NO backward will follow (train_online.py:172-181, torch.no_grad): the
                                            forward skips what only a backward reads -- the one-bit ReLU masks and the pool-code bytes -- so the
                                            convolutions that write them keep their fused pooling epilogue and nothing is stored for nobody (round 6;
                                            the workspace may be the inference-sized one, osvos_net_ws_bytes_infer).  Logits are bit-identical. */
#define OSVOS_FLAG_X3_TWO_PIECES 0x800   /* OR-ed into the dtype OSVOS_F32_X3 of osvos_net_forward / osvos_net_backward: precision 'fp32x2' -- the f32x3
                                            kernels take TWO bf16 pieces per operand and form three products (ah*bh + ah*bm + am*bh) instead of three
                                            pieces / six products: operands carry 16 significand bits (TF32, cuDNN's default for fp32 convolutions on
                                            the reference's GPUs, carries 11), accumulation is fp32, half the matrix work.  Tensors, packs and workspaces
                                            are those of OSVOS_F32_X3.  NOT fp32-grade: see profiles/r06_fp32x2.txt for where it lands. */
#define OSVOS_FLAG_X3_HALF_PIECES 0x1000 /* OR-ed into the dtype OSVOS_F32_X3: precision 'fp32h2' -- the f32x3 kernels take TWO FP16 pieces per operand under
                                            block exponents (csrc/h2split.h): 22-23 significand bits per operand, three products on
                                            v_mfma_f32_32x32x16_f16, fp32 accumulation; measured against float64 the error is the exact fp32 kernels'
                                            (tests/test_gpu_ops.py::test_f32x3_kernels_with_fp16_pairs).  osvos_net_forward / osvos_net_backward: the
                                            call's kernels run in that form.  osvos_net_pack: the FORWARD packs are written in the FP16-pair format
                                            (same buffers; a pack and the calls that read it must agree -- a forward with the flag needs forward packs
                                            with it, a backward with the flag needs data-gradient packs with OSVOS_FLAG_X3_HALF_PIECES_BWD). */
#define OSVOS_FLAG_X3_HALF_PIECES_BWD 0x2000 /* osvos_net_pack only: the DATA-GRADIENT packs are written in the FP16-pair format (for backward calls that
                                            carry OSVOS_FLAG_X3_HALF_PIECES) */
#define OSVOS_FLAG_BF16_W2 0x4000        /* OR-ed into the dtype OSVOS_F32_BF16MFMA only (any other dtype: argument error): precision 'bf16w2' -- bf16 activations
                                            times TWO-PIECE weights.  w_hi = RNE_bf16(w), w_lo = RNE_bf16(w - w_hi) (|w - w_hi - w_lo| <= 2^-16 |w|); every
                                            forward 3x3 convolution (13 trunk + 4 side_prep) forms sum a*w_hi + sum a*w_lo on v_mfma_f32_32x32x16_bf16 into one
                                            fp32 accumulator, a = the bf16 activation of the bf16 mode.  Backward, head, loss: those of the bf16 mode.
                                              osvos_wpack_bytes / osvos_pack_conv3x3_fwd: the two-piece forward pack [plane][9][CinP/8][CoutP][8]: plane 0 is
                                            the single-piece pack byte for byte, plane 1 (the lo pieces) follows at + osvos_wpack_bytes(.., OSVOS_F32_BF16MFMA).
                                              osvos_net_wbuf_bytes / osvos_net_pack: the single-piece layout plus the 17 forward lo planes appended behind it in
                                            layer order (13 trunk, then the 4 side_prep filters; each a multiple of 256 bytes); osvos_net_forward (also with
                                            OSVOS_FLAG_INFERENCE): reads them -- a forward with the flag needs a pack with it.  osvos_net_backward accepts the
                                            flag and ignores it (its packs are the single-piece ones at the same offsets). */
#define OSVOS_F32_X3 3        /* fp32 tensors, fp32 parameters and fp32 weight packs exactly as OSVOS_F32; the wide 3x3 convolutions
                                 (forward, data gradient) run on the bf16 matrix pipe with three-way split operands (six bf16
                                 products per fp32 product, fp32 accumulate): fp32-grade results, see osvos_conv3x3 below */
#define OSVOS_NPARAMS 52 /* tensors of OSVOS.state_dict(), reference order */

int osvos_version(void);
const char* osvos_last_error(void);

/* ---- layout helpers -------------------------------------------------------------------- */
/* NCHW fp32 [N,C,H,W] -> NHWC with `cpad` channels (zero filled), replaces the implicit layout
 * of the tensor handed to OSVOS.forward (vgg_osvos.py:59). */
int osvos_nchw_to_nhwc(const float* src, void* dst, int N, int C, int H, int W, int cpad, int dtype, void* stream);
/* NHWC (channel stride cs) -> NCHW fp32 [N,C,H,W] */
int osvos_nhwc_to_nchw(const void* src, float* dst, int N, int C, int H, int W, int cs, int dtype, void* stream);

/* OIHW fp32 [Cout,Cin,3,3] -> forward pack [9][CinP/G][CoutP][G] (G = 4 fp32 / 8 bf16 channels per
 * 16-byte group; CinP = Cin rounded up to 2G, CoutP = Cout rounded up to 32; zero filled). */
size_t osvos_wpack_bytes(int Cout, int Cin, int dtype);
int osvos_pack_conv3x3_fwd(const float* w_oihw, void* wpk, int Cout, int Cin, int dtype, void* stream);
/* same weights packed for the data-gradient: a 3x3 conv of dY with the 180-degree rotated,
 * channel-transposed filter; pack is [9][CoutP'/G][CinP'][G] with roles swapped. */
size_t osvos_wpack_dgrad_bytes(int Cout, int Cin, int dtype);
int osvos_pack_conv3x3_dgrad(const float* w_oihw, void* wpk, int Cout, int Cin, int dtype, void* stream);

/* ---- 3x3 convolution (replaces aten::convolution for nn.Conv2d(k=3,p=1): vgg_osvos.py:41,142
 *      and, with the dgrad pack, the input-gradient half of aten::convolution_backward) ------
 * y[n,h,w,co] = epi( bias[co] + sum_{r,s,ci} x[n,h+r-1,w+s-1,ci] * W[co,ci,r,s] )
 *   x: NHWC, channel stride Cin (multiple of 2G);  y: NHWC, channel stride y_cs, Cout written
 *   bias: fp32 [Cout] or NULL;  relu != 0: epi = max(.,0)  (vgg_osvos.py:143)
 *   mask: NHWC like y or NULL: epi zeroes the result where mask <= 0 (ReLU backward of the
 *         producer layer fused into this layer's data-gradient: aten::threshold_backward)
 *   tile: -1 = automatic, otherwise a tile-config index, +100 for the XCD-local spatial
 *         block mapping (tuning / tests) */
int osvos_conv3x3(const void* x, const void* wpk, const float* bias, const void* mask, void* y,
                  int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int dtype, int tile, void* stream);
int osvos_conv3x3_num_tiles(void);
/* f32x3: the SAME fp32 convolution (fp32 tensors, fp32 packs, dtype OSVOS_F32) evaluated on the bf16 matrix pipe with
 * three-way split operands -- v = hi + mid + lo exactly (three bf16 pieces), a*b ~ six bf16 products accumulated in fp32,
 * dropped terms <= 2^-24 |a b| each: fp32-grade results at up to 2.67x the fp32-MFMA rate.  Needs Cin % 16 == 0,
 * Cout % 4 == 0 and >= 32, y_cs % 4 == 0; other shapes (conv1_1, side_prep) stay on the exact kernel.
 *   The arithmetic is chosen PER CALL: dtype OSVOS_F32_X3 with tile = -1 takes f32x3 wherever it applies, dtype OSVOS_F32 the exact
 *   kernels; tile 200 + k (k < osvos_conv3x3_f32x3_tiles(), +100 for the XCD-local map) forces an f32x3 tile config.  (Rounds 2-3 also had
 *   a process-wide osvos_set_fp32_conv_mode / OSVOS_FP32_CONV switch: removed in round 4 -- no mutable global state behind the ABI.) */
int osvos_conv3x3_f32x3_tiles(void);
/* f32x3 with PRE-SPLIT weights: the three bf16 piece planes of the filter are formed once (osvos_pack_conv3x3_x3; dgrad != 0 packs the
 * rotated / transposed filter of the data gradient) instead of by every workgroup while staging -- same pieces, bit-identical results,
 * less work between the two barriers of a K chunk.  osvos_net_* do this internally for dtype OSVOS_F32_X3 (OSVOS_X3_PRESPLIT=0: don't).
 * osvos_conv3x3_x3: arguments as osvos_conv3x3 with dtype OSVOS_F32_X3; tile -1 or one of the eight-wave f32x3 tiles (10, 12, 14, 15). */
size_t osvos_wpack_x3_bytes_abi(int Cout, int Cin, int dgrad);
int osvos_pack_conv3x3_x3(const float* w_oihw, void* wpk3, int Cout, int Cin, int dgrad, void* stream);
/* Stream-K form of osvos_conv3x3_x3 (round 4): one persistent workgroup per CU walks an even share of the launch's (tile, 16-channel K chunk)
 * units; tiles whose K range is shared are summed by the last arriver in a fixed order (deterministic; no workgroup ever waits for another).
 * sk_ws: caller-owned workspace of osvos_conv3x3_x3_streamk_ws_bytes(); its first osvos_conv3x3_x3_streamk_ticket_bytes() bytes must be ZERO
 * before the first launch that uses the buffer (every launch leaves them zero); launches sharing one workspace must be stream-ordered.
 * grid: 0 = automatic (stream-K only when a plain grid would leave CUs without a tile), > 0 = forced with that many workgroups (<= 256).
 * pooled (optional): maxpool2x2_ceil(y) written next to y (needs relu, y_cs == Cout).  Tiles 10, 12, 14 (or -1); other tiles run plain. */
size_t osvos_conv3x3_x3_streamk_ws_bytes(void);
size_t osvos_conv3x3_x3_streamk_ticket_bytes(void);
int osvos_conv3x3_x3_streamk(const void* x, const void* wpk3, const float* bias, const void* mask, void* y, void* pooled, int N, int H, int W, int Cin,
                             int Cout, int y_cs, int relu, int tile, int grid, void* sk_ws, void* stream);
int osvos_conv3x3_x3(const void* x, const void* wpk3, const float* bias, const void* mask, void* y,
                     int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int tile, void* stream);
/* host only, launches nothing: what the convolution launchers decide for a call -- the kernel family, its tile, the block order, the K split,
 * stream-K and the loop form -- through the same code the launches go through (osvos_net_forward / osvos_net_backward build their calls the
 * same way).  dtype: as osvos_conv3x3, with OSVOS_FLAG_BF16_W2 (two-piece weights) and, for OSVOS_F32_X3, the piece flags OSVOS_FLAG_X3_TWO_PIECES /
 * OSVOS_FLAG_X3_HALF_PIECES.  flags: what the call carries (OSVOS_PLAN_*; a tensor mask is in the format of x).  tile: -1 = automatic, else a
 * public tile id; ksplit: 0 = automatic; sk_grid: 0 = automatic.  out[OSVOS_CONV_PLAN_INTS] = {family (OSVOS_CONV_FAMILY_*), tile (row of the
 * family's table: its tile id; two-piece: id - 40; LDS-DMA: id - 30; p64: epilogue mode 0 plain / 1 fused pool / 2 one-bit mask), block order
 * (1: XCD-local; p64: 2 = banded), ksplit, 1 if a finalize launch follows, stream-K workgroups (0: plain grid), stream-K tile order, f32x3: 1 if
 * the pre-split pack is read, f32x3: 1 if the pipelined K loop runs, 1 if the pooling kernel is a separate launch behind the convolution}.
 * A call no launcher takes is the launcher's argument error. */
#define OSVOS_PLAN_X_BF16 0x1
#define OSVOS_PLAN_Y_BF16 0x2
#define OSVOS_PLAN_Y_F32 0x4
#define OSVOS_PLAN_RELU 0x8
#define OSVOS_PLAN_MASK 0x10        /* a ReLU mask as a tensor */
#define OSVOS_PLAN_MASK_BITS 0x20   /* ... as one bit per element */
#define OSVOS_PLAN_Y_BITS 0x40      /* the result's sign bits are written */
#define OSVOS_PLAN_POOL 0x80        /* the max-pool of the result is asked of the same call */
#define OSVOS_PLAN_POOL_CODE 0x100
#define OSVOS_PLAN_PART_WS 0x200    /* a partial-sum workspace: the launch may be cut along K */
#define OSVOS_PLAN_SK_WS 0x400      /* a stream-K workspace */
#define OSVOS_PLAN_WPK3 0x800       /* f32x3: the pre-split pack (beside the fp32 pack) */
#define OSVOS_CONV_FAMILY_F32 0
#define OSVOS_CONV_FAMILY_F32X3 1
#define OSVOS_CONV_FAMILY_BF16 2
#define OSVOS_CONV_FAMILY_BF16_DMA 3
#define OSVOS_CONV_FAMILY_BF16_P64 4
#define OSVOS_CONV_FAMILY_BF16_W2 5
#define OSVOS_CONV_PLAN_INTS 10
int osvos_conv3x3_plan(int N, int H, int W, int Cin, int Cout, int y_cs, int dtype, int flags, int tile, int ksplit, int sk_grid, int* out);
/* same convolution cut into `ksplit` parts along K = 9*Cin (0 = automatic, 1..8): layers too small to balance over
 * 256 CUs (conv4_x, conv5_x at batch 1) get more, shorter workgroups; partial sums go to part_ws
 * (osvos_conv3x3_splitk_ws_bytes) and a second kernel applies bias / ReLU / mask.  fp32 only. */
size_t osvos_conv3x3_splitk_ws_bytes(int N, int H, int W, int Cout, int dtype);
int osvos_conv3x3_splitk(const void* x, const void* wpk, const float* bias, const void* mask, void* y,
                         int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int dtype, int tile, int ksplit,
                         void* part_ws, void* stream);

/* Input gradient of the FIRST convolution (Cin = 3; train_online.py:121 makes the input require grad): dy NHWC fp32 [N][H][W][Cout]
 * (Cout % 16 == 0), wpk_dgrad = osvos_pack_conv3x3_dgrad(w, .., Cout, 3, OSVOS_F32) -> dx_nchw fp32 [N][3][H][W] directly.  A bandwidth
 * kernel (fp32 FMAs, filter through scalar loads) in place of a 32-cout MFMA tile that would waste 10x the matrix work. */
int osvos_conv3x3_dgrad_c3(const float* dy, const float* wpk_dgrad, float* dx_nchw, int N, int H, int W, int Cout, void* stream);
/* the same from a bf16 dy (NHWC bf16: the bf16-store mode) on the matrix pipe, in the arithmetic of the bf16 mode (bf16 dy x bf16 filter, fp32
 * accumulation; the whole 64-channel halo tile goes through LDS once, the filter is the MFMA's row operand): Cout = 64 only; wpk_bf16_dgrad =
 * osvos_pack_conv3x3_dgrad(w, .., 64, 3, OSVOS_F32_BF16MFMA).  What the network's bf16-store mode runs for train_parent.py:136's input gradient. */
int osvos_conv3x3_dgrad_c3_bf16mma(const void* dy_bf16, const void* wpk_bf16_dgrad, float* dx_nchw, int N, int H, int W, int Cout, void* stream);


/* ---- bf16 operand storage for the bf16-MFMA path (dtype OSVOS_F32_BF16MFMA) ------------------------------------------
 * The convolutions of that path round their operands to bf16 anyway; producers can hand the rounded tensor over
 * directly so that the consumer reads half the bytes and skips the conversion (same numbers, RNE either way).
 *   osvos_conv3x3_bf16io: x fp32 (x_is_bf16 = 0) or bf16 NHWC; mask fp32 or (mask_is_bf16) bf16; y fp32 and/or y_bf16
 *     (either may be NULL; y_bf16 has the same channel stride and needs Cout % 8 == 0, y_cs % 8 == 0).  Other
 *     arguments as osvos_conv3x3.  With x_is_bf16 only the tile ids osvos_conv3x3_bf16io_tiles() reports are built.
 *   *_bf16copy: the fp32 kernel plus a bf16 copy of its output (NULL = none).
 *   *_bf16act: pooling on bf16 tensors (C % 8 == 0); the backward adds in fp32 and rounds once (RNE). */
int osvos_conv3x3_bf16io(const void* x, int x_is_bf16, const void* wpk, const float* bias, const void* mask, int mask_is_bf16, float* y,
                         void* y_bf16, int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int tile, void* stream);
int osvos_maxpool2x2_bf16act(const void* x_bf16, void* y_bf16, int N, int H, int W, int C, void* stream);
/* weight gradient of the wide layers (Cin_s and Cout multiples of 64, Cin == Cin_s) from bf16 x AND dy; workspace of
 * osvos_wgrad_ws_bytes(.., OSVOS_F32_BF16MFMA); dw/db fp32 as osvos_conv3x3_wgrad (db = fp32 sums of the bf16 dy) */
int osvos_conv3x3_wgrad_bf16act(const void* x_bf16, const void* dy_bf16, void* ws, float* dw, float* db, int N, int H, int W, int Cin, int Cin_s,
                                int Cout, int Cout_s, int accumulate, void* stream);
int osvos_maxpool2x2_bwd_bf16act(const void* x_bf16, const void* dy_bf16, const void* dside_bf16, void* dx_bf16, int N, int H, int W, int C,
                                 void* stream);
/* pool-code bytes (round 5): the forward pooling also writes ONE byte per pooled element ([N][ceil(H/2)][ceil(W/2)][C]: bits 1:0 = window
 * position of the first maximum in scan order (0,0) (0,1) (1,0) (1,1), bits 5:2 = "input at position q > 0"), and the backward reads that byte
 * instead of the pool's four inputs (vgg_osvos.py:140 ceil-mode max-pool + the ReLU backward of the producing convolution + the side-branch
 * add, as osvos_maxpool2x2_bwd_bf16act): same results bit for bit, 1 byte instead of 8 read per pooled element. */
int osvos_maxpool2x2_bf16act_code(const void* x_bf16, void* y_bf16, void* code, int N, int H, int W, int C, void* stream);
int osvos_maxpool2x2_bwd_bf16act_code(const void* code, const void* dy_bf16, const void* dside_bf16, void* dx_bf16, int N, int H, int W, int C,
                                      void* stream);
/* The trunk convolution of the bf16-store mode WITH its fused epilogues, as osvos_net_forward / osvos_net_backward launch it (round 6: op-level
 * access for the parity tests of every tile, vgg_osvos.py:136-145 conv -> ReLU [-> MaxPool2d(2, stride=2, ceil_mode=True)] and its autograd):
 *   x_bf16, y_bf16: bf16 NHWC, dense (channel stride = channel count); wpk from osvos_pack_fwd / osvos_pack_dgrad with OSVOS_F32_BF16MFMA
 *   mask_bits (optional): ReLU mask of a data gradient as ONE bit per element, [N][H][W][Cout/32] 32-bit words, bit b of word g = channel 32 g + b
 *   y_bits (optional): the same for the result (what a later data gradient is masked with)
 *   pooled_bf16 + pool_code (optional; need relu, no mask): the 2x2 ceil-mode max-pool of the result and its code bytes (see above)
 *   tile: osvos_conv3x3_bf16io_tiles() ids (+100: XCD-local block order) or -1 = automatic; 36 / 37 need Cin == 64. */
int osvos_conv3x3_bf16act_fused(const void* x_bf16, const void* wpk, const float* bias, const void* mask_bits, void* y_bf16, void* y_bits,
                                void* pooled_bf16, void* pool_code, int N, int H, int W, int Cin, int Cout, int relu, int tile, void* stream);
int osvos_conv3x3_bf16io_tiles(int* tiles, int max);
/* precision 'bf16w2' (OSVOS_FLAG_BF16_W2) at op level: the FORWARD convolution of osvos_conv3x3_bf16act_fused (same arguments and fused epilogues,
 * vgg_osvos.py:136-145 conv -> ReLU [-> MaxPool2d(2, stride=2, ceil_mode=True)]) with a two-piece pack (osvos_pack_conv3x3_fwd(.., OSVOS_F32_BF16MFMA |
 * OSVOS_FLAG_BF16_W2, ..)) -- two MFMA products per product.  x_is_f32 != 0: x is fp32 NHWC (channel stride Cin), rounded to bf16 (RNE) while staged
 * (conv1_1's input).  mask_bits must be NULL (the data gradients stay single-piece).  tile: osvos_conv3x3_bf16w2_tiles() ids (+100: XCD-local block
 * order) or -1 = automatic; a single-piece tile id is an argument error, as is a two-piece id in osvos_conv3x3_bf16act_fused.  y_f32 (optional): the
 * fp32 result before its bf16 rounding (then y_bf16 may be NULL unless pooled_bf16 is given) -- what the accuracy tests compare. */
int osvos_conv3x3_bf16w2_fused(const void* x, const void* wpk_w2, const float* bias, const void* mask_bits, void* y_bf16, void* y_bits,
                               void* pooled_bf16, void* pool_code, int N, int H, int W, int Cin, int Cout, int relu, int x_is_f32, float* y_f32, int tile,
                               void* stream);
int osvos_conv3x3_bf16w2_tiles(int* tiles, int max);
/* pieces per operand of the OSVOS_F32_X3 kernels called from THIS host thread through the op-level entry points (osvos_conv3x3,
 * osvos_conv3x3_x3*, osvos_conv3x3_wgrad, osvos_pack_conv3x3_x3 with that dtype): 3 (default: three bf16 pieces, six products, fp32-grade),
 * 2 (two bf16 pieces, three products; what OSVOS_FLAG_X3_TWO_PIECES selects for the osvos_net_* calls, which set and restore it themselves)
 * or 22 (two FP16 pieces under block exponents, three products; OSVOS_FLAG_X3_HALF_PIECES -- a pack made under 22 is in the FP16-pair
 * format and must be read under 22). */
int osvos_set_x3_pieces(int pieces);
int osvos_nchw_to_nhwc_bf16copy(const float* src, void* dst, void* dst_bf16, int N, int C, int H, int W, int cpad, void* stream);
int osvos_maxpool2x2_bf16copy(const float* x, float* y, void* y_bf16, int N, int H, int W, int C, void* stream);
int osvos_maxpool2x2_bwd_bf16copy(const float* x, const float* dy, const float* dside, float* dx, void* dx_bf16,
                                  int N, int H, int W, int C, void* stream);

/* ---- 3x3 weight gradient (weight/bias half of aten::convolution_backward) -----------------
 * dW[co,ci,r,s] = sum_{n,h,w} dY[n,h,w,co] * x[n,h+r-1,w+s-1,ci];  db[co] = sum dY
 *   x: NHWC stride Cin_s (only ci < Cin used); dy: NHWC stride Cout_s (already ReLU-masked)
 *   ws: workspace of osvos_wgrad_ws_bytes(); dw: fp32 OIHW [Cout,Cin,3,3]; db: fp32 [Cout] or NULL
 *   accumulate != 0: dw/db += result (gradient accumulation) else overwritten */
size_t osvos_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int dtype);
int osvos_conv3x3_wgrad(const void* x, const void* dy, void* ws, float* dw, float* db,
                        int N, int H, int W, int Cin, int Cin_s, int Cout, int Cout_s,
                        int accumulate, int dtype, void* stream);
/* conv1_1's weight gradient as the bf16-store mode runs it: x the 3-channel input as fp32 NHWC8 (channels 3..7 zero), dy bf16 NHWC with
 * channel stride Cout_s; Cout <= 64, Cout % 4 == 0, Cout_s % 4 == 0.  Cout == 64 with Cout_s % 8 == 0 runs on the bf16 matrix pipe (x rounded
 * to bf16 while staged) unless osvos_debug_set_c3_bf16(0), everything else on the exact fp32 kernel reading the bf16 dy.  ws: workspace of
 * osvos_wgrad_ws_bytes(N, H, W, 8, Cout, OSVOS_F32_BF16MFMA); dw fp32 [Cout,3,3,3]; db fp32 [Cout] or NULL; accumulate as above */
int osvos_conv3x3_wgrad_c3_bf16dy(const float* x_nhwc8, const void* dy_bf16, void* ws, float* dw, float* db, int N, int H, int W, int Cout,
                                  int Cout_s, int accumulate, void* stream);
/* host only, launches nothing: how conv1_1's weight gradient cuts N x H x W into patches and splits (one workgroup walks the per_split
 * consecutive patches of a split; patches are numbered x fastest, then y, then image).  bf16_dy = 0: the fp32 kernel (32 x 8 pixel patches),
 * 1: the bf16-pipe kernel (16 x 8).  out[5] = {npx, npy, npatches, per_split, nsplit} */
int osvos_wgrad_c3_plan(int N, int H, int W, int bf16_dy, int* out);
/* host only, launches nothing: what the launcher of the WIDE weight-gradient kernels does with a shape (dense dY) -- dtype OSVOS_F32_X3: the
 * f32x3 kernels (Cin_s, Cout multiples of 64, or Cout 16 with Cin_s % 128 == 0: the skinny form); OSVOS_F32_BF16MFMA: the bf16 kernels on fp32
 * tensors (bf16_tensors = 0; Cout % 64 == 0) or on bf16 tensors (1; also Cout 16).  out[12] = {patch width, patch height, npx, npy, npatches,
 * per_split, nsplit, nco_t, nci_t, workgroups, 1 if the XCD-local block map is taken, 1 if the 128-cout eight-wave bf16 form runs}; the
 * workgroup of split s walks patches [s per_split, min((s + 1) per_split, npatches)), numbered x fastest, then y, then image.  Any other
 * shape / dtype is an argument error. */
int osvos_wgrad_wide_plan(int N, int H, int W, int Cin_s, int Cout, int dtype, int bf16_tensors, int* out);
/* host only, launches nothing: what the weight-gradient launchers decide for a call -- which kernel family takes it, which of the family's kernels,
 * how the pixels are cut into patches and splits, the grid and the reduce behind it -- through the same code the launches go through
 * (osvos_net_backward builds its calls the same way: Cout_s = Cout, x bf16 in the bf16-store mode except conv1_1's, dy bf16 in that mode).
 * dtype: as osvos_conv3x3_wgrad, for OSVOS_F32_X3 with the piece flags OSVOS_FLAG_X3_TWO_PIECES / OSVOS_FLAG_X3_HALF_PIECES.  flags: what the call
 * carries (OSVOS_WGRAD_PLAN_*).  out[OSVOS_WGRAD_PLAN_INTS] = {family (OSVOS_WGRAD_FAMILY_*), kernel (row of the family's kernel table, see below),
 * patch width, patch height, npx, npy, npatches, per_split, nsplit, nco_t, nci_t, workgroups, 1 if the XCD-local block map is taken, reduce
 * (OSVOS_WGRAD_REDUCE_*), floats of the weight slabs, floats of the bias partials (the workspace holds both; saturating at 2^31 - 1)}; the
 * workgroups of split s walk patches [s per_split, min((s + 1) per_split, npatches)), numbered x fastest, then y, then image.
 * Kernel rows.  F32: 0-3 = wgrad_f32_kernel<1,4,PIPE,DBUF,1> and 5-8 = <2,2,PIPE,DBUF,1> with PIPE + 2 DBUF = row / row - 5; 4 = <2,2,1,0,2,16>
 * (16 x 4 patches); 9, 10 = <2,2,PIPE,0,2> (two workgroups per CU).  C3_F32 / C3_BF16 / CO16_F32: 0 / 1 / 2, the three skinny kernels.  F32X3:
 * 3 * form + geometry, form 0 / 1 = two / three bf16 pieces with the staging addresses of OSVOS_WGRAD_X3_OLDADDR=1, 2 = two FP16 pieces, 3 = two
 * bf16 pieces, 4 = three bf16 pieces; geometry 0 = the Cout 16 form, 1 = 16 x 6 patches, 2 = 16 x 4 patches.  BF16: 0 / 1 = wgrad_bf16_kernel<0 / 1>
 * (fp32 / bf16 tensors), 2 / 3 = wgrad_bf16pm_kernel<4 / 8> (64- / 128-cout tiles).  A call no launcher takes is the launcher's argument error. */
#define OSVOS_WGRAD_PLAN_X_BF16 0x1
#define OSVOS_WGRAD_PLAN_DY_BF16 0x2
#define OSVOS_WGRAD_PLAN_NO_BIAS 0x4   /* db = NULL */
#define OSVOS_WGRAD_FAMILY_F32 0        /* exact fp32, the generic kernel */
#define OSVOS_WGRAD_FAMILY_C3_F32 1     /* conv1_1, exact fp32 (wgrad_c3_f32_kernel) */
#define OSVOS_WGRAD_FAMILY_C3_BF16 2    /* conv1_1 on the bf16 pipe (wgrad_c3_bf16_kernel) */
#define OSVOS_WGRAD_FAMILY_CO16_F32 3   /* Cout = 16, exact fp32 (wgrad_co16_f32_kernel) */
#define OSVOS_WGRAD_FAMILY_F32X3 4
#define OSVOS_WGRAD_FAMILY_BF16 5
#define OSVOS_WGRAD_REDUCE_T16 0        /* the transposing reduce, 16 waves per workgroup */
#define OSVOS_WGRAD_REDUCE_T4 1         /* ... 4 waves */
#define OSVOS_WGRAD_REDUCE_GENERIC 2    /* the generic reduce */
#define OSVOS_WGRAD_REDUCE_OIHW 3       /* ... over reference-order slabs (OSVOS_WGRAD_VARIANT bit 3) */
#define OSVOS_WGRAD_REDUCE_C3 4         /* conv1_1's own */
#define OSVOS_WGRAD_PLAN_INTS 16
int osvos_wgrad_plan(int N, int H, int W, int Cin, int Cin_s, int Cout, int Cout_s, int dtype, int flags, int* out);

/* ---- 2x2/2 max-pool, ceil_mode (aten::max_pool2d_with_indices, vgg_osvos.py:140) ---------- */
int osvos_maxpool2x2(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);
/* fused backward: dx = relu_mask(x) * ( route(dy, first max of the window in scan order) + dside )
 * x is the (post-ReLU) pool input, dside (NULL ok) the gradient from the side branch. */
int osvos_maxpool2x2_bwd(const void* x, const void* dy, const void* dside, void* dx,
                         int N, int H, int W, int C, int dtype, void* stream);

/* ---- side-output / fuse head (vgg_osvos.py:68-72: score_dsn 1x1, upscale_/upscale transposed
 *      convs, center_crop (osvos_layers.py:51-56), torch.cat, fuse 1x1) ----------------------
 * Commuted form: valid when upscale[i].weight is diagonal with one shared
 * k x k filter; the caller checks that with osvos_deconv_diag_check and must refuse otherwise.
 *   prep:   NHWC [N,h,w,16] output of side_prep[i]
 *   wd/bd:  score_dsn[i] weight[16] / bias[1];  wf: fuse.weight[16*i .. 16*i+15]
 *   score, fpart: fp32 [N,h,w] low-resolution maps */
int osvos_head_lowres(const void* prep, const float* wd, const float* bd, const float* wf,
                      float* score, float* fpart, int N, int h, int w, int dtype, void* stream);
/* outs[0..3] = crop(upscale_[i](score_i)), outs[4] = fuse.bias + sum_i crop(up_i(fpart_i)); all
 * fp32 NCHW [N,1,H,W].  score/fpart/f1/f16: host arrays of 4 device pointers (filters k x k,
 * k = 4,8,16,32; f1 = upscale_[i].weight[0,0], f16 = upscale[i].weight[0,0]); hs/ws: host int[4]. */
int osvos_head_upsample(const float* const* score, const float* const* fpart,
                        const float* const* f1, const float* const* f16, const float* fuse_bias,
                        float* const* outs, int N, int H, int W, const int* hs, const int* ws, void* stream);
/* backward of both, per scale: dprep[N,h,w,16] (NHWC, dtype) = wf*up^T(dfused) + wd*up_^T(dside);
 * writes per-workgroup partial sums of the weight/bias gradients to acc (double[OSVOS_HEAD_MAX_BLOCKS][34] at most:
 * {dwf[16], dwd[16], dbd, spare} per launched workgroup; the whole-network call sums them).
 * dside / dfused: fp32 NCHW [N,1,H,W] or NULL (treated as zero). */
#define OSVOS_HEAD_MAX_BLOCKS 1024
int osvos_head_bwd(const void* prep, const float* dside, const float* dfused,
                   const float* f1, const float* f16, const float* wd, const float* wf,
                   void* dprep, double* acc, int N, int H, int W, int h, int w, int scale_idx,
                   int dtype, void* stream);
/* max |off-diagonal| and max |w[c,c]-w[0,0]| of a [16,16,k,k] deconv weight -> out[2] (device) */
int osvos_deconv_diag_check(const float* w, int C, int k, float* out2, void* stream);

/* ---- class-balanced BCE with logits (osvos_layers.py:19-48) ------------------------------
 * out/label fp32, `count` elements over N images.  mode 0: size_average, 1: batch_average,
 * 2: neither.  loss: fp32[1]; grad: fp32[count] = dLoss/dOut (upstream 1) or NULL;
 * scratch: 32 bytes, zeroed by this call.  Tensors that are not 16-byte aligned (offset views) are swept element-wise: slower, same numbers. */
int osvos_cbce(const float* out, const float* label, float* loss, float* grad, void* scratch,
               long count, int N, int mode, void* stream);
/* The same loss as one step of the training loops sees it (train_online.py:127-141, train_parent.py:143-163): `loss` is the plain
 * loss (what the reference adds to running_loss), `running` (device fp32[1] or NULL) += loss inside the final kernel, and
 * grad = grad_scale * dLoss/dOut with grad_scale = the upstream gradient the reference's `loss /= nAveGrad; loss.backward()` hands the
 * loss (1/nAveGrad, times (1 - epoch/nEpochs) for the parent loop's side heads) -- rounded like osvos_cbce followed by osvos_scale,
 * but without the separate scale / add / divide launches between the loss and the head's backward. */
int osvos_cbce_step(const float* out, const float* label, float* loss, float* grad, void* scratch,
                    long count, int N, int mode, float grad_scale, float* running, void* stream);
/* Several heads against ONE label (train_parent.py:143-147: the five losses of a micro-batch) in three launches instead of 3 per head: the class
 * counts of the label are formed once.  outs / losses / grads / running: arrays of n_heads (1..8) device pointers (grads, running and their entries
 * may be NULL); grad_scales: n_heads HOST floats; scratch: 32 x n_heads bytes, zeroed by this call.  Per head identical to osvos_cbce_step. */
int osvos_cbce_step_multi(const float* const* outs, const float* label, float* const* losses, float* const* grads, void* scratch,
                          long count, int N, int mode, int n_heads, const float* grad_scales, float* const* running, void* stream);
/* General form (the three calls above forward to it with flags = 0, counts = NULL).
 *   flags & OSVOS_CBCE_PER_IMAGE: each of the N images is its own reference batch of ONE -- class weights from its own label, size_average
 *     divides by the elements of one image, batch_average by 1 -- and `loss` receives the SUM of the N losses: the nAveGrad micro-batches of
 *     an accumulation window (train_online.py:116-149: cbce(..., batch of 1); loss /= nAveGrad; backward(); running_loss += loss) in ONE call
 *     on a batch-N forward, with grad_scale = 1 / nAveGrad.
 *   counts != NULL: device fp32[3] = {n_pos, n_total, n_images} of the GLOBAL batch these tensors are a shard of (the count exchange of a
 *     batch sharded over ranks; layers/osvos_layers.py:28-34,43-46 count over the whole input tensor): weights and divisors come
 *     from them, no count sweep runs.  Summed over the shards the losses / gradients are those of the whole batch.  Not with PER_IMAGE.
 *   scratch: osvos_cbce_scratch_bytes(n_heads, N, flags) bytes, zeroed by the call -- or, with flags & OSVOS_CBCE_SCRATCH_ZEROED, already zero by
 *     the caller's promise (no memset is enqueued).  Every call LEAVES the scratch zero (its last workgroup forms the losses and clears what it
 *     read), so a buffer that was zeroed once can be handed to call after call on one stream.
 *   flags & OSVOS_CBCE_VOID: a pixel whose label is < 0 is VOID (online adaptation: "don't know").  It is in neither class count and in
 *     neither loss sum, and its gradient is WRITTEN as +0.0f.  Per count group n_total is the number of non-void pixels; size_average divides
 *     by it, batch_average is unchanged: for one group the loss is the reference's function on the non-void pixels as a flat one-image tensor,
 *     the gradient on those pixels that call's gradient.  A group without a non-void pixel contributes loss 0 and gradient 0 (no NaN is
 *     formed).  The scratch holds a void count per group more (the size query takes the flag).  Not with counts != NULL.  Without the flag a
 *     negative label is a negative-class pixel, as ever. */
#define OSVOS_CBCE_PER_IMAGE 1
#define OSVOS_CBCE_SCRATCH_ZEROED 2
#define OSVOS_CBCE_VOID 4
size_t osvos_cbce_scratch_bytes(int n_heads, int N, int flags);
int osvos_cbce_step_ex(const float* const* outs, const float* label, float* const* losses, float* const* grads, void* scratch, long count,
                       int N, int mode, int flags, const float* counts, int n_heads, const float* grad_scales, float* const* running,
                       void* stream);
/* y[i] = x[i] * (*scalar)   (loss.backward() chain rule with a device-resident upstream grad) */
int osvos_scale(const float* x, const float* scalar, float* y, long count, void* stream);

/* ---- whole network ------------------------------------------------------------------------
 * One call = OSVOS.forward (vgg_osvos.py:59-74) / its autograd backward.
 *   params: host array of 52 device pointers, state_dict order, fp32, contiguous
 *   wbuf:   persistent buffer of osvos_net_wbuf_bytes(): packed weights (refresh with
 *           osvos_net_pack whenever a parameter changed, e.g. after optimizer.step())
 *   ws:     per-call workspace of osvos_net_ws_bytes(); forward leaves the activations the
 *           backward needs in it (and, in the bf16-store and f32x3 modes, the SIGN BITS of the activations that mask a later data
 *           gradient -- one 32-bit word per pixel and 32 channels, csrc/maskbits.h -- so the same ws must go to the backward untouched)
 *   outs:   host array of 5 device pointers, fp32 [N,1,H,W] */
size_t osvos_net_wbuf_bytes(int dtype);
size_t osvos_net_ws_bytes(int N, int H, int W, int dtype);
/* workspace of a forward that will never be followed by osvos_net_backward (inference): a prefix of ws */
size_t osvos_net_ws_bytes_infer(int N, int H, int W, int dtype);
int osvos_net_pack(const float* const* params, void* wbuf, int dtype, int with_dgrad, void* stream);
int osvos_net_forward(const float* x_nchw, const void* wbuf, void* ws, float* const* outs,
                      int N, int H, int W, int dtype, void* stream, void* aux_stream /* NULL ok: see backward */);
/* douts: host array of 5 device pointers (NULL = no gradient for that head).
 * grads: host array of 52 device pointers (NULL entries are skipped; deconv weights are frozen in
 *        both reference scripts -- train_online.py:84-85 -- and are never written).
 * dx_nchw: fp32 [N,3,H,W] or NULL.  accumulate != 0: grads += instead of overwrite.
 * aux_stream: NULL, or a second stream owned by the caller: the weight-gradient kernels are then
 *   enqueued on it, concurrently with the data-gradient kernel of the same layer (fork/join with
 *   events; everything has joined `stream` again when the call returns).
 * aux2_stream: NULL, or a third stream for the bandwidth-bound slab reduces of the weight gradients, so they
 *   do not sit between two MFMA weight-gradient kernels on aux_stream. */
int osvos_net_backward(const void* wbuf, void* ws, const float* const* douts, float* const* grads,
                       float* dx_nchw, int N, int H, int W, int dtype, int accumulate, void* stream, void* aux_stream,
                       void* aux2_stream);
/* makes `stream` wait for everything enqueued so far on aux_stream / aux2_stream (NULL = skip): the join a backward with
 * OSVOS_FLAG_DEFER_JOIN left out */
int osvos_net_join(void* stream, void* aux_stream, void* aux2_stream);
/* Gradient-ready events for overlapping the data-parallel all-reduce with the rest of the backward (extends
 * train_parent.py:163-172; SURVEY 8e "overlap with the last micro-batch's backward, bucket order = reverse layer order").
 * Arms the NEXT osvos_net_backward call made by THIS host thread: events[k] (hipEvent_t handles owned by the caller, k < 7) is
 * recorded on whichever stream writes the last gradient of group k, right after that write:
 *   0 = score_dsn + fuse, 1 = side_prep (all four), 2 = stages.4, 3 = stages.3, 4 = stages.2, 5 = stages.1, 6 = stages.0
 * -- the order in which a backward completes them.  A communication stream that waits on events[k] may reduce group k's gradients
 * while the shallower layers are still being computed.  n = 0 disarms.  Entries may be NULL. */
#define OSVOS_NGRAD_GROUPS 7
int osvos_net_arm_grad_events(void* const* events, int n);
/* ---- RCCL through the C ABI: the gradient exchange of the data-parallel loop (one sum of the flat gradient buffer per
 *      optimizer step; extends train_parent.py:163-172) without torch.distributed.  librccl is bound with dlopen at the first call.
 *   osvos_comm_unique_id: on ONE rank; ship the 128 bytes to the others by any means (file, socket, torch.distributed broadcast).
 *   osvos_comm_init: collective over all `world` ranks, on the calling process's current HIP device; *comm is the only library-owned
 *     handle of this ABI (opaque; osvos_comm_destroy releases it).
 *   osvos_comm_allreduce_f32: in-place sum of buf[0..count) over the ranks, enqueued on `stream` (no host synchronisation).
 *   osvos_comm_allreduce_chunks_f32: the same as n chunks buf[first[k] .. first[k] + count[k]), chunk k enqueued on comm_stream behind
 *     ready_events[k] (hipEvent_t, NULL = no wait): with the events of osvos_net_arm_grad_events and the chunks in the backward's
 *     completion order, the deep layers' gradients travel while the shallow ones are still being computed.
 *   Return: 0, < 0 argument / loader error, hipError_t, or 1000 + ncclResult_t. */
#define OSVOS_COMM_ID_BYTES 128
int osvos_comm_unique_id(void* id128);
int osvos_comm_init(void** comm, int rank, int world, const void* id128);
int osvos_comm_allreduce_f32(void* comm, float* buf, size_t count, void* stream);
int osvos_comm_allreduce_f64(void* comm, double* buf, size_t count, void* stream);   /* sum of doubles: class counts, loss statistics (exact) */
int osvos_comm_allreduce_chunks_f32(void* comm, float* buf, const size_t* first, const size_t* count, void* const* ready_events, int n,
                                    void* comm_stream);
int osvos_comm_destroy(void* comm);
/* byte offset / element count of a saved activation inside ws (tests): which = 0..12 trunk conv
 * outputs, 13..16 pooled inputs of stages 1-4, 17..20 side_prep outputs, 21 NHWC input.  (fp32 elements; with dtype
 * OSVOS_F32_BF16MFMA the trunk tensors 0..16 are bf16 unless OSVOS_BF16_STORE=0.) */
int osvos_net_ws_query(int N, int H, int W, int dtype, int which, size_t* offset, size_t* elems, int* channels, int* h, int* w);
/* storage format of trunk tensor `which` (0..16) for `dtype`: 0 fp32 NHWC, 1 bf16 NHWC (OSVOS_F32_BF16MFMA store mode) */
int osvos_net_ws_format(int dtype, int which);

/* ---- training-time input pipeline (dataloaders/davis_2016.py:99-106 + custom_transforms.py: flip, ScaleNRotate, ToTensor) ------
 * One frame: uint8 BGR [H][W][3] (+ uint8 label [H][W] or NULL) -> float32 image [3][H][W] = (flipped, warped) frame minus mean3,
 * float32 gt [1][H][W] = label / max(label.max(), 1e-8) (nearest warp for 0/1 masks, bicubic for soft ones, decided on the device).
 * Minv: HOST pointer to the dst->src affine cv::warpAffine derives from getRotationMatrix2D (6 doubles), NULL = no warp.
 * scratch: 2 unsigned on the device.  OpenCV's fixed-point coordinate / 5-bit cubic table algorithm, border value 0. */
int osvos_augment_frame(const unsigned char* img_bgr, const unsigned char* label, const float* mean3, int flip, const double* Minv,
                        float* out_img, float* out_gt, void* scratch, int H, int W, void* stream);

/* ---- result writer / evaluator (train_online.py:181-189) -----------------------------------
 * osvos_mask_to_bytes: per image p = sigmoid(logit), then scipy<=1.1 imsave's min-max byte scaling
 *   uint8((p - min) * 255/(max - min) clipped + 0.5); scratch = 2 N unsigned.  The host side writes the PNG.
 * osvos_mask_iou_counts: per image {|P & G|, |P | G|} with P = logit > logit_threshold, G = gt > 0.5 (DAVIS region measure J);
 *   counts = 2 N unsigned long long. */
int osvos_mask_to_bytes(const float* logits, unsigned char* out, void* scratch, long count, int N, void* stream);
int osvos_mask_iou_counts(const float* logits, const float* gt, void* counts, long count, int N, float logit_threshold, void* stream);
/* DAVIS J and F in one call (train_online.py:181-189 writes PNGs and leaves both measures to the external DAVIS toolkit; this stands in
 * for its db_eval_iou + db_eval_boundary).  logits, gt: N frames of H x W floats, read once; P = logit > logit_threshold, G = gt > 0.5.
 * Boundary map B(M): a pixel is set when M differs from its right, lower or lower-right neighbour (last row: right only, last column:
 * lower only, corner never); a pixel of one boundary map is matched when the other has a pixel with dy*dy + dx*dx <= radius*radius.
 * counts: 6 unsigned long long per frame {|P & G|, |P | G|, |B(P)|, |B(G)|, matched of B(P), matched of B(G)} -- the first two are
 *   osvos_mask_iou_counts' -- accumulate == 0: overwritten; != 0: added to (the caller zeroed it once).
 * ws: osvos_boundary_ws_bytes(N, H, W) bytes (two one-bit-per-pixel maps per frame), contents irrelevant on entry.  ws and counts 8-byte
 *   aligned.  radius: 1..OSVOS_BOUNDARY_MAX_RADIUS pixels (DAVIS: ceil(0.008 * image diagonal); 8 at 854x480, 36 at 3840x2160); N <= 65535. */
#define OSVOS_BOUNDARY_MAX_RADIUS 64
size_t osvos_boundary_ws_bytes(int N, int H, int W);
int osvos_mask_jf_counts(const float* logits, const float* gt, void* ws, void* counts, int N, int H, int W, float logit_threshold, int radius,
                         int accumulate, void* stream);

/* ---- multi-object results (DAVIS 2017: one network per object, one indexed label map per frame, J and F per object) ----------
 * osvos_merge_objects: logits [K][N][H][W] fp32 (the fused outputs of K per-object networks for N frames) -> labels [N][H][W] uint8.
 *   Per pixel m = max_k logits[k] (fmax: a NaN logit never wins); label = 0 when `m > logit_threshold` is false (all NaN included), else
 *   1 + the lowest k with logits[k] == m.  Decided on the logits, never on a sigmoid.  Every logit is read once; no workspace.
 * osvos_labels_jf_counts: pred, gt [N][H][W] uint8 label maps, read once.  For frame n and object id k = 1..K row n K + (k - 1) of counts
 *   [N][K][6] unsigned long long receives the six counts of osvos_mask_jf_counts with P = (pred == k), G = (gt == k); label 0 and labels
 *   above K belong to no object.  accumulate, radius, alignment: as osvos_mask_jf_counts.  ws: osvos_labels_jf_ws_bytes(N, K, H, W) bytes
 *   (two one-bit-per-pixel maps per frame and object), contents irrelevant on entry.  1 <= K <= OSVOS_MAX_OBJECTS, N K <= 65535. */
#define OSVOS_MAX_OBJECTS 16
int osvos_merge_objects(const float* logits, unsigned char* labels, int N, int K, int H, int W, float logit_threshold, void* stream);
size_t osvos_labels_jf_ws_bytes(int N, int K, int H, int W);
int osvos_labels_jf_counts(const unsigned char* pred, const unsigned char* gt, void* ws, void* counts, int N, int K, int H, int W, int radius,
                           int accumulate, void* stream);

/* ---- connected components of the thresholded mask, and their selection (the clean-up step between the logits and the result writers) ----
 * Definitions.  Foreground of a frame: P = logit > logit_threshold (osvos_mask_jf_counts' test: a NaN is background).  connectivity: 4
 *   (edge neighbours) or 8 (edge and corner neighbours); a component is a maximal connected subset of P inside ONE frame.
 *   labels [N][H][W] int: 0 off P, else 1 + min(y W + x) over the component's pixels -- independent of algorithm, tiling and scheduling.
 *   area [N][H][W] int: the component's pixel count at its root pixel (flat index label - 1), 0 everywhere else.
 *   stats [N][4] long long: {components, |P|, largest area, label of the largest component -- the lowest label on a tie, 0 when none}.
 * osvos_mask_components: logits read once; area and stats may be NULL; labels, area, stats and ws may hold anything on entry.
 *   N 1..65535, H W < 2^31 - 1, stats and ws 8-byte aligned.
 * osvos_components_select: labels, area, stats as osvos_mask_components wrote them for these logits (stats may be NULL when keep_largest
 *   is 0).  A component of frame n is kept when  area >= min_area  AND  (keep_largest == 0 OR its label is stats[n][3])  AND  the seed
 *   test passes: seed == NULL, or the seed map of frame n has no non-zero pixel (the object was lost: everything passes, so tracking can
 *   recover), or some pixel of the component lies within dy*dy + dx*dx <= seed_radius^2 of a non-zero seed pixel (seed_radius
 *   0..OSVOS_BOUNDARY_MAX_RADIUS, 0 = plain overlap).  chain == 0: seed is [N][H][W] uint8, one map per frame.  chain != 0: seed is
 *   [1][H][W] and seeds frame 0, frame n > 0 is seeded by kept[n - 1] (kept is required; hand kept[N - 1] back as the next call's seed).
 *   kept [N][H][W] uint8: 1 at the foreground pixels of kept components, else 0.  out_logits (may be logits itself): logits, except
 *   `fill` at the foreground pixels of dropped components; fill must not be NaN and must be <= logit_threshold (-inf is allowed).
 *   Either output may be NULL, not both.
 * ws: osvos_components_ws_bytes(N, H, W) bytes serve both calls -- sized for the larger need, the selection's: one flag word per pixel
 *   and a one-bit-per-pixel seed map per frame, plus 16 N bytes -- contents irrelevant on entry.  0 for sizes the calls refuse. */
size_t osvos_components_ws_bytes(int N, int H, int W);
int osvos_mask_components(const float* logits, int* labels, int* area, void* stats, void* ws, int N, int H, int W, float logit_threshold,
                          int connectivity, void* stream);
int osvos_components_select(const float* logits, const int* labels, const int* area, const void* stats, const unsigned char* seed, int chain,
                            int seed_radius, int min_area, int keep_largest, float fill, float* out_logits, unsigned char* kept, void* ws, int N,
                            int H, int W, float logit_threshold, void* stream);

/* ---- test-time augmentation: resized / mirrored network inputs from the decoded frame, and the views' logit maps fused on one grid ----
 * Sampling rule of both calls: separable bilinear with half-pixel centres (the geometry of F.interpolate(mode='bilinear',
 *   align_corners=False)), taps in integers: for destination index i of n_dst over a source of n_src
 *     num = max((2 i + 1) n_src - n_dst, 0), den = 2 n_dst, i0 = min(num / den, n_src - 1), i1 = min(i0 + 1, n_src - 1),
 *     f = float(num % den) / float(den) is the weight of i1, 1 - f that of i0;  value = f == 0 ? s[i0] : (1 - f) s[i0] + f s[i1]
 *   along x first, then along y, without fused multiply-adds.  A tap of weight zero is not read into the sum, so a source of the
 *   destination's own size passes through bit for bit (inf and NaN included).  Every side 1..16384 (num stays inside int32), N 1..65535.
 * osvos_tta_view: bgr [N][H][W][3] uint8 (device) -> out [N][3][Hv][Wv] fp32 = sample of channel c minus mean3[c] (mean3: HOST pointer,
 *   as in osvos_augment_frame).  flip != 0: destination column x holds exactly what the unflipped view holds at column Wv - 1 - x.
 *   Hv == H, Wv == W, flip == 0 is bit-identical to osvos_augment_frame's image output for the identity transform.
 * osvos_tta_fuse: views[v] [N][Hv[v]][Wv[v]] fp32 (device pointers, 4-byte aligned) -> out [N][H][W] = sum_v weight[v] * sample_v(y, x),
 *   summed in the order of v starting from the first product; sample_v reads view v through column Wv[v] - 1 - c where flip[v] != 0.
 *   views, Hv, Wv, flip and weight are HOST arrays of length V, 1 <= V <= OSVOS_TTA_MAX_VIEWS; weight == NULL means 1 / V each.  The maps
 *   are logits: a mean of logits, never of sigmoids.  One launch each on `stream`, no workspace, nothing uploaded. */
#define OSVOS_TTA_MAX_VIEWS 16
int osvos_tta_view(const unsigned char* bgr, const float* mean3, float* out, int N, int H, int W, int Hv, int Wv, int flip, void* stream);
int osvos_tta_fuse(const float* const* views, const int* Hv, const int* Wv, const int* flip, const float* weight, int V, float* out, int N,
                   int H, int W, void* stream);

/* ---- object-centred zoom: a box from a mask, the box's window as a network input of fixed size, the canvas's logits pasted back ----
 * A box is int32 (x0, y0, bw, bh) in DEVICE memory, one per frame: the window of columns x0 .. x0 + bw - 1 and rows y0 .. y0 + bh - 1.
 * osvos_roi_box: mask [N][H][W] bytes (device; non-zero = object) -> box [N][4].  Per frame, in signed 64-bit integers, `/` rounding down
 *   (every operand it meets is >= 0):
 *     1. xa, xb, ya, yb = the smallest and largest column and row of a set pixel; no set pixel: box = (0, 0, W, H), done
 *     2. bw = xb - xa + 1, bh = yb - ya + 1, pad = (max(bw, bh) * margin_pct + 99) / 100 + margin_px;
 *        x0 = xa - pad, y0 = ya - pad, bw += 2 pad, bh += 2 pad
 *     3. bw < min_w: x0 -= (min_w - bw) / 2, bw = min_w;  bh < min_h: y0 -= (min_h - bh) / 2, bh = min_h
 *     4. bw * Hc < bh * Wc: nw = (bh * Wc + Hc - 1) / Hc, x0 -= (nw - bw) / 2, bw = nw;
 *        else bh * Wc < bw * Hc: nh = (bw * Hc + Wc - 1) / Wc, y0 -= (nh - bh) / 2, bh = nh          (the canvas's aspect)
 *     5. bw = min(bw, W), x0 = min(max(x0, 0), W - bw);  bh = min(bh, H), y0 = min(max(y0, 0), H - bh)
 *   The box lies in the frame and holds the tight box; one capped by the frame loses the aspect.  margin_pct, margin_px >= 0,
 *   0 <= min_w <= W, 0 <= min_h <= H.  ws: OSVOS_ROI_BOX_WS_BYTES(N) bytes, 16-byte aligned, contents irrelevant on entry and worthless
 *   afterwards: the call keeps no state in it.  Two launches on `stream`; frames are independent.
 * osvos_roi_view: bgr [N][H][W][3] uint8 -> out [N][3][Hc][Wc] fp32 = the sampling rule above (test-time augmentation) with n_src = bw
 *   (bh), n_dst = Wc (Hc), source indices offset by x0 (y0) and clamped to the box, minus mean3[c] (HOST pointer): osvos_tta_view of the
 *   cropped frame.  The box (0, 0, W, H) with Hc == H, Wc == W gives osvos_tta_view's same-size unflipped output bit for bit.
 * osvos_roi_paste: logits [N][Hc][Wc] fp32 -> out [N][H][W] fp32: inside the box the same rule with n_src = Wc (Hc), n_dst = bw (bh) at
 *   destination index x - x0 (y - y0); `outside` everywhere else.  A canvas of the box's size passes through bit for bit, inf and NaN
 *   included.  out must not be logits.
 * Both read the box from device memory -- only sizes are arguments, nothing is read back -- and force it into the frame first
 *   (1 <= bw <= W, 0 <= x0 <= W - bw, likewise y), which leaves a box of osvos_roi_box as it is.  One launch each on `stream`.
 * Every side 1..16384, N 1..65535; pointers to floats and ints 4-byte aligned.  A refused call returns a negative code, sets
 *   osvos_last_error and launches nothing. */
#define OSVOS_ROI_BOX_PARTS 64
#define OSVOS_ROI_BOX_WS_BYTES(N) ((size_t)(N) * OSVOS_ROI_BOX_PARTS * 16)
int osvos_roi_box(const unsigned char* mask, int* box, int N, int H, int W, int Hc, int Wc, int margin_pct, int margin_px, int min_w, int min_h,
                  void* ws, void* stream);
int osvos_roi_view(const unsigned char* bgr, const int* box, const float* mean3, float* out, int N, int H, int W, int Hc, int Wc, void* stream);
int osvos_roi_paste(const float* logits, const int* box, float* out, int N, int Hc, int Wc, int H, int W, float outside, void* stream);

/* ---- mask refinement: mean field of a local two-label dense CRF (Potts compatibility, ConvCRF-style window), logits in, logits out ----
 * Per image: unary [H][W] fp32 logits u, bgr [H][W][3] uint8 (the decoded frame I), a start state z^0 = init (NULL: unary).  For t = 0..iters-1
 *     s_j       = 2 sigmoid(z_j^t) - 1
 *     k(i, j)   = w_a exp(-(a_s ds + a_c dc)) + w_s exp(-g_s ds)
 *     z_i^(t+1) = u_i + sum over j in W(i), j != i, j inside the image, of k(i, j) s_j
 *   W(i): the offsets (dy * dilation, dx * dilation), |dy|, |dx| <= radius;  ds = (dy dilation)^2 + (dx dilation)^2;
 *   dc = sum_c (I_i,c - I_j,c)^2 (an integer, at most 195075).  No other normalisation; a neighbour outside the image contributes nothing.
 *   out [N][H][W] = z^iters.  iters == 0: out is the start state, copied bit for bit.  A pixel whose messages sum to zero (no neighbour
 *   inside the image, radius 0, zero weights) leaves as u bit for bit.  Images of a batch are independent.
 * Arithmetic: fp32.  The spatial factors w_a exp(-a_s ds) and w_s exp(-g_s ds) are made once per call on the host (float64, rounded once),
 *   dc is exact, the colour factor is one hardware exp2 per neighbour, the sum runs over the window row by row (dy, then dx, ascending) with
 *   one fused multiply-add per neighbour: no atomics, a fixed order per pixel -- identical calls give identical bits.
 * One launch per iteration on `stream`; the states alternate between ws and out so that the last iteration writes out.
 *   ws: osvos_crf_ws_bytes(N, H, W, iters) bytes (one state; 0 below two iterations and for sizes the call refuses), contents irrelevant on
 *   entry; may be NULL when iters < 2.  out must not be unary or init (each iteration reads a neighbourhood of its source).
 * Limits: radius 0..OSVOS_CRF_MAX_RADIUS (0: no neighbours), dilation >= 1, radius * dilation <= OSVOS_CRF_MAX_REACH, iters
 *   0..OSVOS_CRF_MAX_ITERS, sides 1..16384, N 1..65535; the five coefficients finite and >= 0; float pointers 4-byte aligned.  Every
 *   argument error returns < 0 before any device call. */
#define OSVOS_CRF_MAX_RADIUS 7
#define OSVOS_CRF_MAX_REACH 16
#define OSVOS_CRF_MAX_ITERS 64
size_t osvos_crf_ws_bytes(int N, int H, int W, int iters);
int osvos_crf_refine(const float* unary, const float* init, const unsigned char* bgr, float* out, void* ws, int N, int H, int W, int iters,
                     int radius, int dilation, float w_a, float w_s, float a_s, float a_c, float g_s, void* stream);

/* ---- motion compensation: a block-matching motion field between two decoded frames, and the integer warp that applies it ----
 * Integer arithmetic throughout; division is floor division; results are exact (tests compare bit for bit).
 * Luma of a BGR byte triple: Y = (29 B + 150 G + 77 R + 128) >> 8, in 0..255.
 * Grid: step S, block B, search R.  GH = ceil(H / S) by GW = ceil(W / S) cells; cell (i, j) owns the pixels y in [i S, min((i + 1) S, H)),
 *   x in [j S, min((j + 1) S, W)).  Its matching block is the B x B square with top-left corner (i S + floor((S - B) / 2),
 *   j S + floor((S - B) / 2)): for B > S the blocks overlap and are centred on their cells.
 * Cost of a candidate d = (dx, dy), |dx|, |dy| <= R:
 *     cost(d) = sum over the block's B * B pixels p of |Ycur(clamp(p)) - Yprev(clamp(p + d))| + penalty * (|dx| + |dy|)
 *   clamp brings each coordinate into the frame (edge replication), applied to p and to p + d separately.
 * Choice: the cell's vector is the candidate that minimises (cost, dx * dx + dy * dy, dy, dx) lexicographically -- every tie is decided; a
 *   constant frame gives all-zero vectors.  The vector points from a pixel of the CURRENT frame to where it was in the PREVIOUS frame (a
 *   backward field).
 * Median: `median` passes over the vector grid, each replacing each component by the median of its 3 x 3 grid neighbourhood (grid indices
 *   clamped).  cost stays the pre-median minimum of the cell.
 * osvos_flow_block_match: prev_bgr, cur_bgr [N][H][W][3] uint8 -> vec [N][GH][GW][2] int32 = (dx, dy), cost [N][GH][GW] int32 (may be NULL).
 *   Frames of a batch are independent.  2 + median launches on `stream` (luma planes; one workgroup per tile of cells with the tile's luma
 *   staged in LDS, candidates walked four at a time with v_qsad_pk_u16_u8, the minimum taken as an integer min of packed keys; the median passes), no atomics on
 *   global memory, every element of vec and cost written.  ws: osvos_flow_ws_bytes(...) bytes, 4-byte aligned, contents irrelevant on entry
 *   (0 for arguments the call refuses).
 * osvos_flow_warp: out(n, y, x) = src(n, y + dy, x + dx) with (dx, dy) the vector of cell (min(y / S, GH - 1), min(x / S, GW - 1)), `fill`
 *   where the source coordinate leaves the frame.  src, out [N][H][W] of dtype 0 = uint8 or 1 = float32 (moved as 32-bit words: NaN payloads
 *   and -0 survive); vec [N][GH][GW][2] int32 with any values.  With dtype 0, fill must be an integer in 0..255.  out must not be src.  One
 *   launch.  Zero vectors (search = 0) make the warp the identity.
 * Limits: block 1..32, step 1..32, search 0..48, penalty 0..65535, median 0..8, sides 1..16384, N 1..65535.  The largest cost,
 *   255 * 1024 + 65535 * 96, fits int.  Every argument error returns < 0 before any device call. */
#define OSVOS_FLOW_MAX_BLOCK 32
#define OSVOS_FLOW_MAX_STEP 32
#define OSVOS_FLOW_MAX_SEARCH 48
#define OSVOS_FLOW_MAX_PENALTY 65535
#define OSVOS_FLOW_MAX_MEDIAN 8
#define OSVOS_FLOW_MAX_SIDE 16384
size_t osvos_flow_ws_bytes(int N, int H, int W, int block, int step, int search, int median);
int osvos_flow_block_match(const unsigned char* prev_bgr, const unsigned char* cur_bgr, int* vec, int* cost, void* ws, int N, int H, int W,
                           int block, int step, int search, int penalty, int median, void* stream);
int osvos_flow_warp(const void* src, int dtype, const int* vec, void* out, int N, int H, int W, int step, float fill, void* stream);

/* ---- superpixel snapping: an integer grid-SLIC on the decoded frame, and logit pooling over a labelling ----
 * Integer arithmetic throughout; division is floor division; results are exact and do not depend on tile shape, schedule or the order in
 *   which atomics arrive (tests compare bit for bit).
 * Superpixels (osvos_superpixels_slic): frames [N][H][W][3] uint8 BGR, cell S, compactness m, iters T.
 *   Grid: GH = ceil(H / S), GW = ceil(W / S), K = GH * GW clusters per frame, cluster k = gy * GW + gx; a pixel's home cell is (y / S, x / S).
 *   update(labels, prev), per cluster, with count the number of pixels that carry label k: each of the five centre components (x, y, b, g, r)
 *     becomes floor((2 sum + count) / (2 count)) over those pixels; a cluster with count == 0 keeps prev.
 *   assign(centres), per pixel: of the clusters of the 3 x 3 cells around its home cell that lie inside the grid, the minimiser of (D, k),
 *     D = S * S * dc + m * m * ds, dc the squared BGR distance to the centre colour, ds the squared pixel distance to the centre position.
 *   labels_0 = home cell; centres_0 = update(labels_0, -); for t = 1..T: labels_t = assign(centres_(t-1)), centres_t = update(labels_t,
 *     centres_(t-1)).  Out: labels [N][H][W] int32 = labels_T; centres [N][K][6] int32 = (x, y, b, g, r, count) of centres_T (may be NULL).
 *   32 bits suffice: a cluster's pixels lie in the 3 x 3 cells around it, so does its centre; hence |dx|, |dy| < 3 S and
 *     D < 4096 * 195075 + 4096 * 73728 < 2^31; a cluster has at most 9 S S = 36864 pixels and its x or y sum is below 16384 * 36864 < 2^32.
 *   Deliberately left out: there is NO connectivity enforcement (a superpixel may be disconnected; pooling does not mind), and colour is
 *     plain BGR, not CIELAB.  Frames of a batch are independent.
 *   Launches on `stream`: one memset, then 2 (T + 1) kernels -- per step one tile kernel (labels_0, or assign from the tile's ring of
 *     centres in LDS, fused with the sums of the next update: LDS integer atomics, at most one global atomic per non-zero accumulator and
 *     workgroup) and one per-cluster update that divides and re-zeroes the sums.  No workgroup waits for another.
 *   ws: osvos_superpixels_ws_bytes(N, H, W, cell) bytes (the sums and the working centres), 4-byte aligned, contents irrelevant on entry;
 *     0 for arguments the call refuses.  frames, labels, centres and ws must not overlap.
 * Pooling (osvos_superpixels_pool): logits [N][H][W] float32, labels [N][H][W] int32 (ANY labelling, not only SLIC's), K.
 *   Per pixel q = (int) rint(clamp(x, -16384, 16384) * 65536), half to even; NaN maps to the lower clamp (a NaN is background).  Per frame
 *   and label: the int64 sum of q and the int32 count; mean_q = floor((2 sum + count) / (2 count)) -- floor, not C truncation: sums are
 *   negative; out = (float) mean_q * 2^-16.  A pixel whose label is outside [0, K) passes its logit through bit for bit and contributes
 *   to nothing.  One memset and two launches: an accumulate pass (per workgroup an LDS table over the 2048 labels from the tile's smallest
 *   one, 64-bit integer global atomics for its non-empty slots and for labels beyond it) and an apply pass (one gather per pixel).
 *   ws: osvos_superpixels_pool_ws_bytes(N, K) bytes, 8-byte aligned, contents irrelevant on entry; 0 for arguments the call refuses.
 *   out must not overlap logits or labels; ws must not overlap any of the three.
 * Limits: cell 2..64, compactness 0..64, iters 0..16, K 1..2^28, sides 1..16384, N 1..65535, N * H * W <= 2^38.  Every argument error
 *   returns < 0 before any device call, with a text that names the bad parameter. */
#define OSVOS_SUPERPIXELS_MAX_CELL 64
#define OSVOS_SUPERPIXELS_MAX_COMPACTNESS 64
#define OSVOS_SUPERPIXELS_MAX_ITERS 16
#define OSVOS_SUPERPIXELS_MAX_SIDE 16384
#define OSVOS_SUPERPIXELS_MAX_K 268435456
size_t osvos_superpixels_ws_bytes(int N, int H, int W, int cell);
int osvos_superpixels_slic(const unsigned char* frames, int* labels, int* centres, void* ws, int N, int H, int W, int cell, int compactness,
                           int iters, void* stream);
size_t osvos_superpixels_pool_ws_bytes(int N, int K);
int osvos_superpixels_pool(const float* logits, const int* labels, float* out, void* ws, int N, int H, int W, int K, void* stream);

/* ---- online adaptation: exact squared Euclidean distance maps and the adaptation targets made from them ----
 * osvos_mask_sqdist: mask [N][H][W] uint8 -> sqdist [N][H][W] int32.  A pixel q is a SOURCE when (mask[q] != 0) != (invert != 0);
 *   sqdist[n][y][x] = min over the sources q of image n of |p - q|^2, an exact integer, OSVOS_SQDIST_NONE everywhere in an image without a
 *   source.  Sides 1..OSVOS_SQDIST_MAX_SIDE (the largest distance, 2 * 4095^2, stays inside int32), N 1..65535.  Two launches: a column
 *   pass (one lane per column: the vertical distance to the column's nearest source, or "none") and a row pass (one workgroup per row and
 *   image with the row of column distances in LDS; each output pixel walks outwards from its own column and stops once dx^2 >= best, which
 *   is exact because every later candidate is at least dx^2; columns without a source are skipped, never squared).
 *   ws: osvos_mask_sqdist_ws_bytes(N, H, W) bytes (the column distances), contents irrelevant on entry; 0 for sizes the call refuses.
 * osvos_adapt_targets: the label map of one online-adaptation step (OnAVOS) from the network's own fused logits [N][H][W] fp32 and the
 *   previous frame's final mask prev_mask [N][H][W] uint8 (non-zero = object).  Per image:
 *     E        = { p in prev_mask : sqdist(p, background of prev_mask) > erosion^2 }; the image border is not background (a mask that
 *                fills the image erodes to itself); erosion = 0 gives E = prev_mask
 *     negative   label 0.0f:  sqdist(p, E) > distance^2 (OSVOS_SQDIST_NONE counts as far: an empty E makes every pixel negative)
 *     positive   label 1.0f:  not negative and logits[p] > pos_logit (strict; a NaN logit is not positive); pos_logit = log(a / (1 - a))
 *     void       label -1.0f: everything else (the loss ignores it under OSVOS_CBCE_VOID)
 *   counts [N][3] unsigned long long = {n_pos, n_neg, n_void}, overwritten.  erosion, distance >= 0.  Integer and raw-float comparisons
 *   only: the label map is exact.  Sizes as osvos_mask_sqdist; ws: osvos_adapt_ws_bytes(N, H, W) bytes, contents irrelevant on entry.
 *   Four launches (two distance maps; E is decided inside the second one's column pass, the labels inside its row pass) and one small memset
 *   on `stream`. */
#define OSVOS_SQDIST_NONE 2147483647
#define OSVOS_SQDIST_MAX_SIDE 4096
size_t osvos_mask_sqdist_ws_bytes(int N, int H, int W);
int osvos_mask_sqdist(const unsigned char* mask, int invert, int* sqdist, int N, int H, int W, void* ws, void* stream);
size_t osvos_adapt_ws_bytes(int N, int H, int W);
int osvos_adapt_targets(const float* logits, const unsigned char* prev_mask, float pos_logit, int erosion, int distance, float* label,
                        void* counts, int N, int H, int W, void* ws, void* stream);

/* ---- lucid first-frame synthesis: inpaint the background once, then move, re-light and re-composite object and background ----
 * Integer arithmetic throughout; division is floor division; results are exact (tests compare bit for bit).  Colours are BGR bytes.
 * osvos_lucid_inpaint (once per sequence): bgr [H][W][3] uint8, hole [H][W] uint8 (non-zero = to be filled) -> out_bgr [H][W][3].
 *   Fill: a hole pixel p takes the colour of the non-hole pixel q that minimises the key (|p - q|^2, qy, qx) lexicographically -- every tie
 *     is decided; a non-hole pixel keeps its colour; a frame without a non-hole pixel is copied unchanged (the call still returns 0).
 *   Smooth, `passes` times: every hole pixel becomes floor((2 sum + n) / (2 n)) per channel, the sum over the (2 radius + 1)^2 window around
 *     it clipped to the image, n the number of pixels in the clipped window; the window is read from the previous pass's state (hole and
 *     non-hole pixels alike); non-hole pixels never change.  passes = 0 gives the pure fill.
 *   Launches on `stream`: a column pass (one lane per column: the row of the column's nearest non-hole pixel, the smaller row on a tie), a
 *     row pass (one workgroup per row with the row of column answers in LDS; a hole pixel walks outwards from its own column and stops once
 *     dx^2 > best -- strictly, so that an equally distant candidate with a smaller (qy, qx) is still seen; exact, because within a column the
 *     key is monotone in |dy|), and one launch per smoothing pass, alternating between ws and out_bgr so that the last writes out_bgr.  No
 *     atomics; no workgroup waits for another.
 *   ws: osvos_lucid_inpaint_ws_bytes(H, W, passes) bytes, 4-byte aligned, contents irrelevant on entry; 0 for arguments the call refuses.
 *     out_bgr must not overlap bgr or hole; ws must not overlap any of the three.
 *   Limits: sides 1..OSVOS_SQDIST_MAX_SIDE (the largest distance stays inside int32), radius 1..8, passes 0..8.
 * osvos_lucid_compose (once per training sample): N samples out of one source frame in one launch.  bgr [H][W][3], mask [H][W] (non-zero =
 *   object), bg [H][W][3] (the inpainted frame) are device pointers; M [N][2][6] doubles, tone [N][2][6] ints and mean3 are HOST pointers and
 *   travel as kernel arguments: nothing is uploaded and there is no workspace.  Layer 0 is the foreground (colours from bgr, alpha from
 *   mask != 0), layer 1 the background (colours from bg).  Per sample n, layer L and destination pixel (x, y):
 *   Coordinates: M[n][L] is a dst -> src affine; exactly as osvos_augment_frame forms them (doubles, no fused multiply-add, rn = round half to
 *     even): Xb = rn((M1 y + M2) 1024), adelta = rn(M0 x 1024), X = (Xb + adelta + 16) >> 5, ix = X >> 5 (arithmetic), fx = X & 31; Y, iy, fy
 *     the same with M3, M4, M5.  A flip is just an affine.
 *   Sample: the four taps (iy + j, ix + i), i, j in {0, 1}, with integer weights (32 - fx, fx) x (32 - fy, fy), which sum to 1024.  A colour
 *     sample S is the weighted sum of bytes, 0..255 * 1024; a colour tap outside the frame reads the clamped index (edge replication) in BOTH
 *     layers.  a = the weighted sum of (mask != 0) over the taps, 0..1024; a foreground tap outside the frame has alpha 0.
 *   Tone: tone[n][L] = (g_b, g_g, g_r, o_b, o_g, o_r), gains Q8 in 0..1024 (256 = 1), offsets -255..255:
 *     S' = clamp(((S g + 128) >> 8) + (o << 10), 0, 255 << 10).
 *   Composite: C = a F' + (1024 - a) B' (at most 1024 * 261120 < 2^31); out_img[n][c][y][x] = (float) C * 2^-20 - mean3[c], channel order BGR
 *     as osvos_augment_frame; out_gt[n][0][y][x] = a >= 512 ? 1.0f : 0.0f.  (Foreground colours are not premultiplied.)
 *   With identity matrices, gain 256 and offset 0: S' = 1024 v, so wherever mask is set or bg equals bgr the image is (float) v - mean, what
 *     osvos_augment_frame gives for the identity transform, and the label is the mask.
 *   Refused (< 0) before any device call: N outside 1..OSVOS_LUCID_MAX_BATCH; sides outside 1..OSVOS_LUCID_MAX_SIDE; a non-finite matrix
 *     entry; |M0|, |M1|, |M3|, |M4| > 64 or |M2|, |M5| > 2^18 (this keeps every fixed-point coordinate inside int32); gains or offsets out of
 *     range; a null pointer.
 * osvos_lucid_compose_ex: osvos_lucid_compose with a non-rigid deformation of the foreground, an occluder and a void band around the label's
 *   edges.  Everything not named here (coordinates, taps, tone, composite, the limits on M and tone) is osvos_lucid_compose's rule unchanged.
 *   Deformation: D is a DEVICE pointer, null = none: short [N][GH][GW][2] = (dx, dy) in 1/32 pixel on a lattice of `cell` pixels, 4-byte
 *     aligned (a pair is loaded as one 32-bit word).  cell is a power of two in OSVOS_LUCID_MIN_CELL..OSVOS_LUCID_MAX_CELL, s = log2(cell),
 *     GW = ((W - 1) >> s) + 2, GH = ((H - 1) >> s) + 2.  For the destination pixel (x, y): gx = x >> s, tx = x & (cell - 1), gy and ty alike,
 *     dX = ((cell - tx)(cell - ty) D00.x + tx (cell - ty) D01.x + (cell - tx) ty D10.x + tx ty D11.x + (1 << (2 s - 1))) >> 2 s (arithmetic
 *     shift), D00 = D[n][gy][gx], D01 = D[n][gy][gx + 1], D10 = D[n][gy + 1][gx], D11 = D[n][gy + 1][gx + 1]; dY the same from the .y
 *     components.  The weights are >= 0 and sum to 2^(2 s) <= 2^16, so every partial sum lies in -2^31 .. 2^31 - 2^15: inside int32.  The
 *     FOREGROUND layer only uses X = ((Xb + adelta + 16) >> 5) + dX, and Y alike; the background layer is untouched.  The field is indexed
 *     by the destination pixel and added to the source coordinate; it is bilinear in the lattice (C0).  No bound on D beyond short (every
 *     coordinate stays inside int32); that the map does not fold is the caller's business.
 *   Occluder: occ is a HOST pointer, null = none: int [N][6] = (cx, cy, rx, ry, sx, sy), carried in the kernel arguments like M and tone.
 *     rx == 0 or ry == 0: no occluder in that sample.  Pixel (x, y) is covered iff, in 64-bit integers,
 *     (x - cx)^2 ry^2 + (y - cy)^2 rx^2 <= rx^2 ry^2.  A covered pixel shows the inpainted background at an integer offset through the
 *     background's tone: S = 1024 bg[clamp(y + sy, 0, H - 1)][clamp(x + sx, 0, W - 1)][c], S' = tone[n][1] applied to S, C = 1024 S'.
 *   Label and void band: L(p) = (a >= 512) && !covered.  band in 0..OSVOS_LUCID_MAX_BAND.  p is void iff some pixel q INSIDE the image has
 *     |p - q|^2 <= band^2 and L(q) != L(p) (the image border is not an edge).  out_gt is -1.0f at a void pixel and (float) L elsewhere;
 *     out_img does not depend on band.  band == 0: nothing is void, there is no second launch and ws may be null.
 *   Launches on `stream`: the composition (with band >= 1 each wave also stores the ballot of its 64 labels as one word of a 1-bit label
 *     plane [N][H][ceil(W / 64)] in ws -- an ordinary vector store), then with band >= 1 one launch that reads only that plane: per row
 *     offset dy the row's word and its two neighbours, the columns x - hw .. x + hw, hw = isqrt(band^2 - dy^2), clipped to the image, XOR-ed
 *     with the pixel's own bit; it overwrites out_gt with -1.0f where any bit is left.  No atomics; no workgroup waits for another.
 *   ws: osvos_lucid_compose_ex_ws_bytes(N, H, W, band) = 8 N H ceil(W / 64) bytes with band >= 1; 0 with band == 0 and for arguments the
 *     call refuses.  8-byte aligned, contents irrelevant on entry; it must not overlap an input or an output.
 *   Refused (< 0) before any device call: everything osvos_lucid_compose refuses; with D given, a cell that is not a power of two in
 *     range or a misaligned D; band out of range; band > 0 with a null, misaligned or overlapping ws; rx or ry outside 0..4096; |cx|, |cy|,
 *     |sx| or |sy| above 8192.
 *   With D null (or all zero), occ null and band 0 out_img and out_gt are osvos_lucid_compose's bit for bit (the same kernel is launched). */
#define OSVOS_LUCID_MAX_BATCH 16
#define OSVOS_LUCID_MAX_SIDE 4096
#define OSVOS_LUCID_MAX_RADIUS 8
#define OSVOS_LUCID_MAX_PASSES 8
#define OSVOS_LUCID_MAX_GAIN 1024
size_t osvos_lucid_inpaint_ws_bytes(int H, int W, int passes);
int osvos_lucid_inpaint(const unsigned char* bgr, const unsigned char* hole, unsigned char* out_bgr, int H, int W, int radius, int passes,
                        void* ws, void* stream);
int osvos_lucid_compose(const unsigned char* bgr, const unsigned char* mask, const unsigned char* bg, const double* M, const int* tone,
                        const float* mean3, float* out_img, float* out_gt, int N, int H, int W, void* stream);
#define OSVOS_LUCID_MAX_BAND        16
#define OSVOS_LUCID_MIN_CELL        8
#define OSVOS_LUCID_MAX_CELL        256
#define OSVOS_LUCID_MAX_OCC_RADIUS  4096
#define OSVOS_LUCID_MAX_OCC_OFFSET  8192
size_t osvos_lucid_compose_ex_ws_bytes(int N, int H, int W, int band);
int osvos_lucid_compose_ex(const unsigned char* bgr, const unsigned char* mask, const unsigned char* bg, const double* M, const int* tone,
                           const int* occ, const short* D, int cell, int band, const float* mean3, float* out_img, float* out_gt, int N, int H,
                           int W, void* ws, void* stream);

/* ---- appearance matching to the first frame: int8 features and a labelled nearest-neighbour search on the integer matrix pipe ----
 * Every float operation below is ONE IEEE fp32 operation (no fused multiply-add); the dot products are integers.  Results are exact and do
 *   not depend on tiling, slicing or schedule (tests compare bit for bit against a numpy restatement).
 * Quantise (osvos_match_quantize): feat [P][C], format 0 = fp32 or 1 = bf16 (the value of osvos_net_ws_format; bf16 widens exactly).
 *   Per pixel: m = max_c |f_c|.  If m is zero, or any f_c is not finite, q_c = 0 for every c and rinv = 0.  Otherwise s = 127.0f / m and
 *   q_c = (int8) clamp(rintf(f_c * s), -127, 127), half to even, a NaN product (0 * inf, when s overflows) counting as 0;
 *   n = sum_c q_c^2 (int32, at most 127^2 * 1024 < 2^24, so (float) n is exact); rinv = n ? 1.0f / sqrtf((float) n) : 0.  The two quotients
 *   and the square root are correctly rounded: the kernel forms them in double and rounds once more, which is the correctly rounded fp32
 *   result because 53 >= 2 * 24 + 2.  Out: q int8 [P][C], rinv fp32 [P].  One launch, one wave per pixel.
 * Cell labels (osvos_match_cell_labels): mask uint8 [N][H][W], nonzero = object; the feature grid h x w = ceil(H / S) x ceil(W / S), S the
 *   stride (2^stage under ceil-mode pooling).  Cell (i, j) covers rows S i .. min(S i + S, H) - 1 and the same for columns; a = its area,
 *   k = its object pixels.  label = 1 if 4 k >= 3 a, 0 if 4 k <= a, 255 (void: in neither bank) otherwise.  Out: uint8 [N][h][w].  One launch.
 * Nearest (osvos_match_nearest): query Q int8 [N][Pq][C] with rinv_q [N][Pq]; reference R int8 [NR][Pr][C] with rinv_r and label_r [NR][Pr];
 *   NR is N, or 1 (every frame searches the same bank).  For class c in {1 foreground, 0 background}:
 *     t_ab = (float) dot(Q_a, R_b) * rinv_r[b]                  (|dot| <= 127^2 C < 2^24 for C <= 1024: the conversion is exact)
 *     best_c[a] = max of t_ab over the b with label_r[b] == c;  idx_c[a] = the smallest such b that attains it;  sim_c[a] = best_c[a] * rinv_q[a]
 *   a class without a reference row gives sim = -2.0f and idx = -1; rows with any other label are in neither class.
 *   Out: sim fp32 [N][2][Pq] (foreground first), idx int32 [N][2][Pq] (may be NULL).  Two launches: a tile kernel on
 *   v_mfma_i32_32x32x32_i8 (a workgroup owns 128 query rows, staged once in LDS, and walks a slice of R through LDS; the scores are reduced
 *   in registers and never stored; per-slice partial (value, index) pairs go to ws) and a small kernel that merges the slices.  Rows past
 *   Pq / Pr are masked by the kernel, not padded by the caller.  No atomics; deterministic.
 *   ws: osvos_match_ws_bytes(N, Pq, Pr, C) bytes, 8-byte aligned, contents irrelevant on entry; 0 for arguments the call refuses.
 * Top-K (osvos_match_topk; VideoMatch's averaging): the operands, the scores t_ab and the classes of nearest; K in 1..OSVOS_MATCH_MAX_K.
 *   Per query row a and class c: T = the multiset of t_ab over the b with label_r[b] == c, n = |T|, k = min(K, n).  n = 0 gives sim = -2.0f.
 *   Otherwise v_1 >= .. >= v_k are the k largest members of T (duplicated rows are separate members; which of several equal rows is taken
 *   cannot matter, so no index is kept);  s = v_1, then s = fl32(s + v_i) for i = 2 .. k in that order;  m = s / (float) k, correctly
 *   rounded (formed in double and rounded once more, as in quantise);  sim_c[a] = fl32(m * rinv_q[a]).  K = 1 is nearest's sim bit for bit.
 *   For operands made by osvos_match_quantize every t is finite and never -0; the kernels mark an empty slot with -inf.
 *   Out: sim fp32 [N][2][Pq].  Two launches: nearest's tile kernel with, per lane and class, a descending list of the 4, 8 or 16 best
 *   values in registers (the smallest length that holds K) in place of the (value, index) pair, and a kernel that merges the slices' lists.
 *   ws: osvos_match_topk_ws_bytes(N, Pq, Pr, C, K) bytes (K floats per slice, class and query), 8-byte aligned, contents irrelevant on
 *   entry and meaningless after the call; 0 for arguments the call refuses.
 * Local window (osvos_match_local; FEELVOS's local map): queries and references live on the SAME h x w grid, row-major, P = h w <= 2^20 rows
 *   each; radius in 0..OSVOS_MATCH_MAX_RADIUS.  For query cell (i, j) and class c the candidates are the reference cells (i + di, j + dj)
 *   inside the grid with |di| <= radius, |dj| <= radius and label c.  best = the largest t over them, idx = the smallest reference row
 *   (i + di) w + (j + dj) that attains it, sim = best * rinv_q; (-2.0f, -1) when the window holds no row of the class.  A window that covers
 *   the grid is nearest.  Out: sim fp32 [N][2][P], idx int32 [N][2][P] (may be NULL).  One launch, no workspace: four lanes per query cell
 *   walk the window in ascending row with the 4-byte integer dot instruction.
 *   The local map a caller forms from it is max(sim_fg, -1) - max(sim_bg, -1), three fp32 operations: an empty class counts as the smallest
 *   possible cosine.
 * Memory bank (osvos_match_bank_update; the bank of STM and its successors, kept by age): a bank has cap rows -- R int8 [cap][C], rinv_r fp32
 *   [cap], label_r uint8 [cap] -- and is searched by nearest / topk as it is (Pr <= cap; an unused row carries label 255, so it is in
 *   neither class).  Rows [0, protected_rows) are the first frame's and are never written by an update; rows [protected_rows, cap) form a
 *   ring of ring = cap - protected_rows rows.  state int32 [4] in device memory = {cursor, filled, calls, added_last}, all zero for a new
 *   bank; a state that is neither that nor written by this function is outside the contract (the kernel reduces cursor mod ring before it
 *   uses it, so even then nothing outside the ring is written).
 *   The call takes the rows of ONE frame that has already been searched against THIS bank: q int8 [P][C] with rinv_q fp32 [P], label_q uint8
 *   [P] (osvos_match_cell_labels of that frame's mask) and sim fp32 [2][P], that search's output, foreground first.
 *   Selection: row a is selected iff all four hold -- label_q[a] is 0 or 1;  rinv_q[a] > 0;  own < tau (the row is novel), where
 *     own = sim[label_q[a] == 1 ? 0 : 1][a] and other is the other class's value;  fl32(own - other) >= margin (the bank as it stands does not
 *     contradict the mask's label: the guard against drift).  Each comparison is one fp32 comparison, so a NaN selects nothing.
 *   Subsampling: n = the number of selected rows, m = min(n, max_new, ring).  The selected rows are ranked r = 0 .. n - 1 in ascending row
 *     order; rank r is kept iff floor((r + 1) m / n) > floor(r m / n), in 64-bit integers, and is then kept row j = floor(r m / n): an even
 *     subsample in which every j in 0 .. m - 1 occurs exactly once.
 *   Write: kept row j goes to slot protected_rows + (cursor + j) mod ring -- its C bytes, its rinv_q and its label.  No other byte of the
 *     bank changes.  m <= ring, so one call writes no slot twice; the oldest rows are overwritten first.
 *   State after the call: cursor = (cursor + m) mod ring, filled = min(filled + m, ring), calls += 1, added_last = m.  With ring == 0 or
 *     n == 0, m = 0 and only calls and added_last change.
 *   N frames each update their own bank: every array above, state included, carries a leading [N].  Three launches on the stream: flags and
 *   per-workgroup counts;  one workgroup per bank that scans the counts, reads state, leaves n, m and the old cursor in ws and writes the
 *   new state;  the ranks (wave ballots and population counts) and the copies (16-byte vector loads and stores).  No atomics, no workgroup
 *   waits on another, no read-back; identical calls give identical bytes.
 *   ws: osvos_match_bank_ws_bytes(N, P) bytes, 8-byte aligned, contents irrelevant on entry; 0 for arguments the call refuses.
 *   tau and margin are finite, max_new >= 0, 0 <= protected_rows <= cap, cap in 1..2^20; the bank, state and ws overlap neither the frame's
 *   arrays nor each other.
 * Softmax readout (osvos_match_soft; the memory read of STM, STCN and XMem): the operands, limits, alignment, aliasing rules and the NR = N
 *   or 1 rule of nearest; beta, the temperature, a finite float in OSVOS_MATCH_MIN_BETA..OSVOS_MATCH_MAX_BETA.  Every row of a class votes
 *   with weight exp(beta (cosine - 1)), and the class's evidence is the mass of its votes.  For query row a and reference row b:
 *     t_ab = (float) dot(Q_a, R_b) * rinv_r[b], exactly as in nearest;   cos_ab = fl32(t_ab * rinv_q[a]);
 *     k = (float) ((double) beta * log2(e)), formed once on the host;     e_ab = fl32(fl32(cos_ab - 1.0f) * k)
 *   -- single fp32 operations, no fused multiply-add -- and w_ab = 2^e_ab, for which the hardware exponential is allowed (so lse is compared
 *   within a bar, not bit for bit).  beta <= 40 keeps e >= -116: no weight is denormal or zero; Pr <= 2^20 keeps every sum finite.
 *     S_c[a] = the sum of w_ab over the b with label_r[b] == c, in fp32, in an order the sizes alone fix;
 *     lse_c[a] = (float) (1.0 + log((double) S_c[a]) / (double) beta), formed in double by the finish kernel.
 *   Rows with any other label contribute nothing, and neither do the rows past Pr that a tile loads as zeros: they are masked by their
 *   label, not relied on to be small (a zero row has cosine 0 and weight exp(-beta)).  max_b cos <= lse <= max_b cos + ln(n_c) / beta, n_c
 *   the rows of the class; the attention log-odds of the object are beta (lse_fg - lse_bg).  A class without a row gives -2.0f.
 *   best_c[a], when requested, is nearest's sim BIT FOR BIT, the -2.0f of an empty class included: a caller that feeds the memory bank's
 *   novelty and margin tests with it keeps their meaning under the soft readout.
 *   Out: lse fp32 [N][2][Pq] (foreground first), best fp32 [N][2][Pq] (may be NULL).  Two launches: nearest's tile kernel with, per lane,
 *   the query's rinv_q and a running sum (and, with best, a running maximum) per class in place of the (value, index) pairs -- the two lane
 *   halves merged with one shuffle, low half plus high half; per-slice partial sums and maxima go to ws -- and a kernel with one lane per
 *   (frame, class, query) that adds the slices in ascending order and forms lse.  No atomics, no workgroup waits on another; identical
 *   calls give identical bytes whatever ws held on entry.
 *   ws: osvos_match_soft_ws_bytes(N, Pq, Pr, C) bytes, 8-byte aligned, contents irrelevant on entry; 0 for arguments the call refuses.
 *   Left out: a softmax over the top k rows only; a value read-out richer than the label; a soft readout inside the local window; a
 *   learned temperature.
 * Limits: C a multiple of 64 in 64..1024, Pq and Pr 1..2^20, P 1..2^30 (1..2^20 for the bank update), N 1..65535, sides 1..16384, stride a
 *   power of two 1..64.  q, Q and R are 16-byte aligned.  Outputs (and ws) must not overlap inputs or each other.  Every argument error
 *   returns < 0 before any device call, with a text that names the bad parameter. */
int osvos_match_quantize(const void* feat, int format, signed char* q, float* rinv, long P, int C, void* stream);
int osvos_match_cell_labels(const unsigned char* mask, unsigned char* label, int N, int H, int W, int h, int w, int stride, void* stream);
size_t osvos_match_ws_bytes(int N, int Pq, int Pr, int C);
int osvos_match_nearest(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r, float* sim,
                        int* idx, void* ws, int N, int NR, int Pq, int Pr, int C, void* stream);
#define OSVOS_MATCH_MAX_K       16
#define OSVOS_MATCH_MAX_RADIUS  15
size_t osvos_match_topk_ws_bytes(int N, int Pq, int Pr, int C, int K);
int osvos_match_topk(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r, float* sim,
                     void* ws, int N, int NR, int Pq, int Pr, int C, int K, void* stream);
int osvos_match_local(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r, float* sim,
                      int* idx /* may be NULL */, int N, int NR, int h, int w, int C, int radius, void* stream);
size_t osvos_match_bank_ws_bytes(int N, int P);
int osvos_match_bank_update(const signed char* q, const float* rinv_q, const unsigned char* label_q, const float* sim, signed char* R,
                            float* rinv_r, unsigned char* label_r, int* state, void* ws, int N, int P, int C, int cap, int protected_rows,
                            int max_new, float tau, float margin, void* stream);
#define OSVOS_MATCH_MIN_BETA 0.0625f
#define OSVOS_MATCH_MAX_BETA 40.0f
size_t osvos_match_soft_ws_bytes(int N, int Pq, int Pr, int C);
int osvos_match_soft(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r,
                     float* lse, float* best /* may be NULL */, void* ws, int N, int NR, int Pq, int Pr, int C, float beta, void* stream);

/* ---- fused SGD (torch.optim.SGD semantics, train_online.py:79-88,147) ----------------------
 * for each i: d = g + wd*p; buf = first ? d : momentum*buf + d; p -= lr*buf      (flat tensors) */
int osvos_sgd_step(float* p, const float* g, float* buf, long count, float lr, float momentum,
                   float weight_decay, int first, void* stream);
/* the same update for a whole list of tensors in one launch (per-tensor lr / weight decay = the reference's 8 SGD
 * parameter groups); host arrays of n device pointers / counts / rates; tensors whose group has lr = 0 and no
 * weight decay can simply be left out.  `first` != 0: the momentum buffers are initialised (buf = d). */
#define OSVOS_SGD_MAX_TENSORS 64
int osvos_sgd_step_multi(float* const* params, const float* const* grads, float* const* bufs, const long* counts,
                         const float* lrs, const float* wds, int n, float momentum, int first, void* stream);

/* ---- interactive scribbles: strokes to a label map, an error region to a stroke (its skeleton) ----
 * The raster call: segs int32 [M][6] on the device, a row = (x0, y0, x1, y1, value, frame) -> out uint8 [N][H][W], every byte written.  A
 *   row with frame < 0 (or >= N) is padding.  out[n][y][x] = 255 when no row of frame n covers the pixel p = (x, y), else the `value` of the
 *   covering row with the HIGHEST index.  Coverage of p by the segment a -> b with radius r, exact in signed 64-bit integers:
 *     d = b - a, L = d.d, w = p - a, t = w.d;   L == 0 or t <= 0: w.w <= r^2;   t >= L: |p - b|^2 <= r^2;   else (w x d)^2 <= r^2 L.
 *   The caller keeps coordinates in [0, 16384) and value in 0..254 (the kernel does not check them; with such coordinates nothing
 *   overflows: (w x d)^2 < 2^58, r^2 L < 2^42).  M 0..OSVOS_SCRIBBLE_MAX_SEGMENTS (segs may be null when M is 0), radius
 *   0..OSVOS_SCRIBBLE_MAX_RADIUS.  One launch, no atomics, no workspace: a workgroup per 64 x 16 tile and frame gathers the rows that can
 *   touch its tile into an LDS list of OSVOS_SCRIBBLE_LIST_CAP rows, highest index first, and empties the list in as many passes as it takes.
 * The thinning call: mask bytes [N][H][W] (non-zero = set) -> out bytes in {0, 1}: the Guo-Hall skeleton; info int32 [N][2] on the device =
 *   (iterations run, 1 if the last of them deleted nothing else 0).  Neighbours of a pixel clockwise from north: P2 N, P3 NE, P4 E, P5 SE,
 *   P6 S, P7 SW, P8 W, P9 NW; pixels outside the frame are 0.
 *     C  = (!P2 & (P3 | P4)) + (!P4 & (P5 | P6)) + (!P6 & (P7 | P8)) + (!P8 & (P9 | P2))
 *     N1 = (P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8),  N2 = (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9),  Nm = min(N1, N2)
 *   Sub-step 0 deletes every set pixel with C == 1, 2 <= Nm <= 3 and ((P2 | P3 | !P5) & P4) == 0; sub-step 1 likewise with
 *   ((P6 | P7 | !P9) & P8) == 0; each sub-step is evaluated for all pixels on the plane as it was before it.  An iteration is sub-step 0
 *   then sub-step 1; a frame stops after its first iteration that deletes nothing or after max_iters (1..OSVOS_THIN_MAX_ITERS), and never
 *   changes again whatever the other frames do.  path: 1 = one workgroup per frame keeps the frame's 1-bit plane in LDS and iterates behind
 *   barriers (H * ceil(W / 64) <= OSVOS_THIN_RESIDENT_WORDS, an argument error otherwise), 2 = two planes ping-pong in ws, one launch per
 *   iteration, max_iters launches enqueued whatever the masks hold, 0 = path 1 when the plane fits, else path 2.  Both paths write the same
 *   bytes.  Nothing is read back.  out may be mask.  ws: the size query's bytes for (N, H, W), 8-byte aligned, contents irrelevant on entry;
 *   0 for sizes the call refuses.  Sides 1..16384, N 1..65535. */
#define OSVOS_SCRIBBLE_MAX_SEGMENTS 65535
#define OSVOS_SCRIBBLE_MAX_RADIUS 64
#define OSVOS_SCRIBBLE_LIST_CAP 512
#define OSVOS_THIN_MAX_ITERS 512
#define OSVOS_THIN_RESIDENT_WORDS 8000
int osvos_scribble_raster(const int* segs, int M, unsigned char* out, int N, int H, int W, int radius, void* stream);
size_t osvos_mask_thin_ws_bytes(int N, int H, int W);
int osvos_mask_thin(const unsigned char* mask, unsigned char* out, int* info, int N, int H, int W, int max_iters, int path, void* ws, void* stream);

/* ---- opt-in launch profiler (bench.py only): hipEvent pairs around every kernel family that
 * osvos_net_forward/backward launches, recorded on the caller's stream.  Families: 0 conv3x3
 * forward launches, 1 backward conv regions (data-gradient kernel || weight-gradient kernel +
 * slab reduce of one layer, fork to join), 2-3 spare.
 * osvos_prof_stop fills ms[4] (sum of launch durations), flops[4] (algorithmic FLOPs of those
 * launches: 2*N*H*W*Cout*9*Cin) and count[4]; synchronise the stream before calling it. */
int osvos_prof_start(int max_records);
int osvos_prof_stop(double* ms, double* flops, long* count);
/* between start and stop: paused != 0 suspends recording (no events are enqueued), 0 resumes it; returns the previous state */
int osvos_prof_pause(int paused);

/* ---- debug references (plain one-thread-per-output kernels, used only by tests) ----------- */
int osvos_debug_conv3x3_naive(const float* x, const float* w_oihw, const float* bias, float* y,
                              int N, int H, int W, int Cin, int Cin_s, int Cout, int relu, void* stream);
int osvos_debug_mfma_layout(float* out /* 4*64*16 floats */, void* stream);
int osvos_debug_mfma_peak(float* out /* blocks*256 floats */, int blocks, int iters, void* stream);
/* register-only loop of v_mfma_f32_32x32x16_bf16 (blocks x 8 waves x iters x 8 MFMAs) on the caller's operand bits (seed: 2048 bytes of bf16):
 * the rate the bf16 matrix pipe SUSTAINS on this chip -- 2.48 PFLOP/s at 2.37 GHz on zeros, 1.83 at 1.81 GHz on noise (bench.py reports it live) */
int osvos_debug_mfma_peak_bf16(const void* seed, float* out /* blocks*512 floats */, int blocks, int iters, void* stream);
/* bf16-store mode: conv1_1's weight gradient on the bf16 matrix pipe (1, default) or on the exact fp32 skinny kernel fed with the bf16 dY
 * (0); returns the previous setting.  Tests compare the two. */
int osvos_debug_set_c3_bf16(int on);
/* LDS-DMA layout probe (buffer_load_dwordx4 ... lds): out[8*64*4] = LDS image after 4 waves x 2 DMA instructions; the test
 * pins "lane l of instruction j lands in 16-byte slot 64 j + l, out-of-range lanes land as zeros" (tests/test_gpu_ops.py) */
int osvos_debug_lds_dma(const float* src, int ngroups, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
