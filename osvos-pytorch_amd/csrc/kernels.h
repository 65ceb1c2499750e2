// Internal (non-ABI) launchers implemented by the .hip translation units.
#pragma once
#include "common.h"
#include "epi.h"

// One 3x3 convolution launch (stride 1, zero padding 1, NHWC), as every launcher below takes it.  Host only: each launcher translates it
// into the argument struct of its kernels.  A launcher reads the fields its family has and ignores the others (the exact fp32 kernels
// have no fused epilogue, the bf16 ones no K split); a caller fills, by name, only what it uses.
struct ConvCall {
  const void* x = nullptr;             // input, channel stride Cin: fp32, or bf16 when x_bf16 (bf16 family only)
  int x_bf16 = 0;
  // weights, one form per family: fp32 pack (osvos_pack_{fwd,dgrad}_f32) / bf16 pack (osvos_pack_bf16_multi) in wpk; f32x3 also takes the
  // pre-split pack (osvos_pack_x3) in wpk3 -- wpk is then not read and may be NULL
  const void* wpk = nullptr;
  const void* wpk3 = nullptr;
  int w_pieces = 1;                    // bf16 family: 2 = two-piece weights (precision 'bf16w2'): wpk is the hi plane (= the single-piece pack), the lo
  size_t w_lo = 0;                     // plane lies w_lo bytes behind it; only the two-piece tiles 40-45 read such packs, and they read nothing else
  const float* bias = nullptr;
  // ReLU mask of a data gradient (y = 0 where mask <= 0), laid out like y: fp32, or bf16 when mask_bf16 (bf16 family only); mask_bits: the same as
  // one bit per element (maskbits.h; dense results with Cout % 32 == 0), takes precedence -- except in the finalize kernel of a launch cut along
  // K, which reads `mask`: the fp32 families take both
  const void* mask = nullptr;
  int mask_bf16 = 0;
  const unsigned* mask_bits = nullptr;
  float* y = nullptr;                  // fp32 result, channel stride y_cs (bf16 family: may be NULL when y_bf16 is given)
  void* y_bf16 = nullptr;              // bf16 family: bf16 result / copy of y with the same stride
  unsigned* y_bits = nullptr;          // sign bits of the result, written next to it (maskbits.h; f32x3: the launch is then never cut along K)
  int y_cs = 0;
  // max-pool 2x2 (ceil mode) of the result by the same call, [N][ceil(H/2)][ceil(W/2)][Cout]; needs ReLU and a dense result.  f32x3: `pooled`
  // (fp32; tiles 10, 12, 14 only, never cut along K by partial-sum launches).  bf16 family: pooled_bf16 (needs y_bf16, no mask, Cout % 8 == 0; a
  // tile whose waves do not hold whole windows launches the pooling kernel behind the convolution) and, optionally with it, pool_code: one byte
  // per pooled element for osvos_maxpool2x2_bwd_bf16_code, written whichever kernel runs
  float* pooled = nullptr;
  void* pooled_bf16 = nullptr;
  void* pool_code = nullptr;
  int N = 0, H = 0, W = 0, Cin = 0, Cout = 0, relu = 0;
  int pieces = 3;                      // f32x3 family, per operand: 3 bf16 pieces, 2 bf16 ('fp32x2') or 22 = two FP16 under block exponents ('fp32h2'; such a wpk3)
  int tile = -1;                       // -1: automatic; else the family's tile id (+100: XCD-local block map)
  int ksplit = 0;                      // fp32 families: K parts (<= 8) of a launch cut along K; 0 = automatic.  Taken only with part_ws
  void* part_ws = nullptr;             // NULL (never cut) or osvos_conv3x3_splitk_ws_bytes_f32() bytes for the partial sums
  // f32x3 stream-K: workspace of osvos_conv3x3_f32x3_streamk_ws_bytes(), tickets zeroed once by the caller (NULL = plain grids only); sk_grid 0 =
  // automatic (taken when the plain grid would idle CUs), > 0 = forced, that many workgroups (tests)
  void* sk_ws = nullptr;
  int sk_grid = 0;
  hipStream_t stream = nullptr;
};

// What a launcher decides about one ConvCall before it launches: written by the family's choose() (argument checks, measured rules, environment
// overrides; host only, no launch, no device memory), read by the launcher, which fills its kernel arguments and calls the tile's table row.
// osvos_conv3x3_plan reports it without launching (tests/test_conv_plan_cpu.py pins it for every layer of the network)
enum ConvFamily {
  CONV_F32 = OSVOS_CONV_FAMILY_F32, CONV_F32X3 = OSVOS_CONV_FAMILY_F32X3, CONV_BF16 = OSVOS_CONV_FAMILY_BF16, CONV_BF16_DMA = OSVOS_CONV_FAMILY_BF16_DMA,
  CONV_BF16_P64 = OSVOS_CONV_FAMILY_BF16_P64, CONV_BF16_W2 = OSVOS_CONV_FAMILY_BF16_W2
};
struct ConvPlan {
  int family = CONV_F32;
  int tile = 0;                        // row of the family's tile table (two-piece: public id - 40; LDS-DMA: the variant, public id - 30; p64: the epilogue mode)
  int map = 0;                         // 1: XCD-local block order (p64: 2 = its banded form)
  int ksplit = 1;                      // fp32 families: K parts; > 1: partial sums into part_ws and a finalize launch behind the convolution
  int sk_grid = 0, sk_order = 0;       // f32x3 stream-K: persistent workgroups (0 = plain grid) and their tile order
  int presplit = 0, pipe = 0;          // f32x3 loop form: reads the pre-split pack (else splits the fp32 pack itself); the pipelined K loop (OSVOS_X3_PIPE)
  int pool_after = 0;                  // bf16 family: the tile cannot pool in its epilogue -- the pooling kernel is a separate launch behind the convolution
};
// chooses the family by dtype and by what the call carries, and launches (the rule: api.cpp)
int osvos_conv3x3_dispatch(const ConvCall& c, int dtype);
// f32x3: weights pre-split once per pack (default) or re-split by every workgroup from the fp32 pack (OSVOS_X3_PRESPLIT=0; bit-identical).  Read by
// the network's pack and by its convolutions' dispatch, nowhere below them: an op-level call uses the pack it is handed
inline bool osvos_x3_presplit() {
  static const bool on = [] { const char* e = getenv("OSVOS_X3_PRESPLIT"); return !(e && e[0] == '0'); }();
  return on;
}

// One 3x3 weight-gradient launch (dw[co][ci][tap] = sum over pixels of dy[co] * x[ci] shifted by the tap; db = sum of dy), as every launcher below
// takes it.  Host only, like ConvCall.  Each launcher states which operand formats it takes and rejects the others with an argument error.
enum WgradPhase { WGRAD_BOTH = 0, WGRAD_PARTIALS = 1, WGRAD_REDUCE = 2 };
struct WgradCall {
  const void* x = nullptr;             // the layer's input, NHWC with channel stride Cin_s: fp32, or bf16 when x_bf16
  const void* dy = nullptr;            // gradient of the layer's output, NHWC with channel stride Cout_s: fp32, or bf16 when dy_bf16
  int x_bf16 = 0, dy_bf16 = 0;
  void* ws = nullptr;                  // partial slabs [split][...] + bias partials: osvos_wgrad_ws_bytes() of the dtype (the family's *_ws_bytes)
  float *dw = nullptr, *db = nullptr;  // results: OIHW fp32 [Cout][Cin][3][3]; [Cout] or NULL (no bias gradient)
  int N = 0, H = 0, W = 0, Cin = 0, Cin_s = 0, Cout = 0, Cout_s = 0;
  int accumulate = 0;                  // != 0: dw / db += instead of =
  // both: partial slabs, then their reduce into dw / db.  osvos_net_backward enqueues the two halves on different streams (the bandwidth-bound
  // reduces off the critical path of the MFMA weight-gradient chain): partials only, then -- same descriptor, stream-ordered behind it -- reduce only
  WgradPhase phase = WGRAD_BOTH;
  int pieces = 3;                      // f32x3 family: pieces per operand, as ConvCall::pieces
  hipStream_t stream = nullptr;
};
// What a launcher decides about one WgradCall before it launches, as ConvPlan above: written by the family's choose() (argument checks, measured
// rules, environment overrides; host only, no HIP call, no device memory), read by the launcher, which fills its kernel arguments, launches
// the family's table row `kernel` and then the reduce `reduce`.  osvos_wgrad_plan reports it without launching (tests/test_wgrad_plan_cpu.py pins
// it for every layer of the network)
enum WgradFamily {
  WGRAD_F32 = OSVOS_WGRAD_FAMILY_F32, WGRAD_C3_F32 = OSVOS_WGRAD_FAMILY_C3_F32, WGRAD_C3_BF16 = OSVOS_WGRAD_FAMILY_C3_BF16,
  WGRAD_CO16_F32 = OSVOS_WGRAD_FAMILY_CO16_F32, WGRAD_F32X3 = OSVOS_WGRAD_FAMILY_F32X3, WGRAD_BF16 = OSVOS_WGRAD_FAMILY_BF16
};
// which kernel sums the slabs: the shared transposing reduce with 16 or 4 waves, the shared generic reduce, the same over reference-order (OIHW)
// slabs (OSVOS_WGRAD_VARIANT bit 3), conv1_1's own
enum WgradReduce {
  WGRAD_REDUCE_T16 = OSVOS_WGRAD_REDUCE_T16, WGRAD_REDUCE_T4 = OSVOS_WGRAD_REDUCE_T4, WGRAD_REDUCE_GENERIC = OSVOS_WGRAD_REDUCE_GENERIC,
  WGRAD_REDUCE_OIHW = OSVOS_WGRAD_REDUCE_OIHW, WGRAD_REDUCE_C3 = OSVOS_WGRAD_REDUCE_C3
};
struct WgradPlan {
  int family = WGRAD_F32;
  int kernel = 0;                      // row of the family's kernel table
  int pw = 0, ph = 0;                  // pixel patch
  int npx = 0, npy = 0, npatches = 0;  // patches along x, along y, in all (x fastest, then y, then image)
  int per_split = 0, nsplit = 0;       // the workgroups of split s walk patches [s per_split, min((s + 1) per_split, npatches)) and write slab s
  int nco_t = 1, nci_t = 1;            // channel tiles
  long blocks = 0;                     // workgroups: nsplit * nco_t * nci_t
  int map = 0;                         // 1: XCD-local block order
  size_t slab_floats = 0, bslab_floats = 0;      // the workspace: weight slabs, then the bias partials
  int reduce = WGRAD_REDUCE_GENERIC;
};
// The arithmetic every family's plan shares.  Patches: pw x ph pixels over N frames.
static inline void wgrad_patches(WgradPlan* p, int N, int H, int W, int pw, int ph) {
  p->pw = pw; p->ph = ph;
  p->npx = ceil_div(W, pw);
  p->npy = ceil_div(H, ph);
  p->npatches = N * p->npx * p->npy;
}
// Splits, from the patches and channel tiles already in the plan: aim at `target_workgroups` workgroups, keep at least `min_patches_per_split`
// patches in a split and at most `max_splits` splits, then even the splits out.  A split writes slab_per_split + bslab_per_split floats.
static inline void wgrad_split(WgradPlan* p, int target_workgroups, int min_patches_per_split, int max_splits, size_t slab_per_split,
                               size_t bslab_per_split) {
  int want = ceil_div(target_workgroups, p->nco_t * p->nci_t);
  const int most = p->npatches / min_patches_per_split > 0 ? p->npatches / min_patches_per_split : 1;
  if (want > most) want = most;
  if (want > max_splits) want = max_splits;
  if (want < 1) want = 1;
  p->per_split = ceil_div(p->npatches, want);
  p->nsplit = ceil_div(p->npatches, p->per_split);
  p->blocks = (long)p->nsplit * p->nco_t * p->nci_t;
  p->slab_floats = (size_t)p->nsplit * slab_per_split;
  p->bslab_floats = (size_t)p->nsplit * bslab_per_split;
}
static inline size_t wgrad_plan_ws_bytes(const WgradPlan& p) { return align_up((p.slab_floats + p.bslab_floats) * sizeof(float), 256); }
// a dense call of a shape, for the workspace queries (which know no tensors): Cin_s = 8 is conv1_1's padded 3-channel input
static inline WgradCall wgrad_shape_call(int N, int H, int W, int Cin_s, int Cout) {
  WgradCall c;
  c.N = N; c.H = H; c.W = W; c.Cin = Cin_s == 8 ? 3 : Cin_s; c.Cin_s = Cin_s; c.Cout = c.Cout_s = Cout;
  return c;
}
// chooses the family by dtype and by what the tensors are (the rule: api.cpp), and launches / only plans
int osvos_wgrad_dispatch(const WgradCall& c, int dtype);
int osvos_wgrad_dispatch_plan(const WgradCall& c, int dtype, WgradPlan* p);
// the slab reduces the families share (wgrad_f32.hip): slab [split][tap][co][ci] -> dw, bslab [split][co] -> db.  *_kind: which of them takes a
// layer (OSVOS_WGRAD_REDUCE_T); *_launch: launches `kind`
int osvos_wgrad_reduce_kind(int nsplit, int Cout, int Cin, int Cin_s);
int osvos_wgrad_reduce_launch(int kind, const float* slab, const float* bslab, float* dw, float* db, int nsplit, int Cout, int Cin, int Cin_s,
                              int accumulate, hipStream_t stream);

// exact fp32 (conv3x3_f32.hip): fp32 tensors and fp32 pack, Cin % 8 == 0
int osvos_conv3x3_f32(const ConvCall& c);
int osvos_conv3x3_f32_plan(const ConvCall& c, ConvPlan* p);
size_t osvos_conv3x3_splitk_ws_bytes_f32(int N, int H, int W, int Cout);
int osvos_conv3x3_splitk_finalize_f32(const float* part, const float* bias, const float* mask, float* y, long npix, int Cout, int y_cs,
                                      int ksplit, int relu, hipStream_t stream);
// f32x3 (conv3x3_f32x3.hip): fp32 tensors, three-way bf16 split operands on the bf16 matrix pipe; tile ids 0..num_tiles-1.  Cout may be ragged
// (the 3-channel input gradient) as long as y has room for the rounded-up channel quad
bool osvos_conv3x3_f32x3_applicable(int Cin, int Cout, int y_cs);
int osvos_conv3x3_f32x3_num_tiles(void);
size_t osvos_conv3x3_f32x3_streamk_ws_bytes(void);
size_t osvos_conv3x3_f32x3_streamk_ticket_bytes(void);
int osvos_conv3x3_f32x3(const ConvCall& c);
int osvos_conv3x3_f32x3_plan(const ConvCall& c, ConvPlan* p);
// f32x3 weight gradient (wgrad_f32x3.hip): fp32 x / dy, three-way bf16 split, fp32 slabs + the shared reduce
// (the wide trunk layers, or side_prep's Cout = 16: the S16 form)
bool osvos_wgrad_f32x3_wide_applicable(const WgradCall& c);
bool osvos_wgrad_f32x3_skinny_applicable(const WgradCall& c);
static inline bool osvos_wgrad_f32x3_applicable(const WgradCall& c) { return osvos_wgrad_f32x3_wide_applicable(c) || osvos_wgrad_f32x3_skinny_applicable(c); }
size_t osvos_wgrad_f32x3_ws_bytes(int N, int H, int W, int Cin_s, int Cout);
int osvos_conv3x3_wgrad_f32x3(const WgradCall& c);
int osvos_wgrad_f32x3_plan(const WgradCall& c, WgradPlan* p);
size_t osvos_wpack_x3_bytes(int M, int K);
#define OSVOS_PACK_MAX 40
// One weight pack to write: w OIHW fp32 [Cout][Cin][3][3] -> dst; dgrad != 0: data-gradient form.  The two multi-pack launchers write n of them
// (n <= OSVOS_PACK_MAX) in one launch
struct PackEntry {
  const float* w = nullptr;
  void* dst = nullptr;
  void* lo_dst = nullptr;              // bf16 only: also the lo plane of a two-piece forward pack, there (the hi plane, at dst, is the single-piece pack byte for byte)
  int Cout = 0, Cin = 0, dgrad = 0;
  int half = 0;                        // f32x3 only: != 0 the two-piece FP16 format (h2split.h; three launches instead of one), else three bf16 planes
};
int osvos_pack_bf16_multi(const PackEntry* e, int n, hipStream_t stream);
int osvos_pack_x3_multi(const PackEntry* e, int n, hipStream_t stream);      // (pre-split f32x3 packs)
int osvos_pack_x3(const float* w, void* wpk3, int Cout, int Cin, int dgrad, int half, hipStream_t stream);
bool osvos_dgrad_c3_applicable(int Cin, int Cout);
int osvos_conv3x3_dgrad_c3_f32(const float* dy, const float* wpk_dgrad, float* dx_nchw, int N, int H, int W, int Cout, hipStream_t stream);
int osvos_conv3x3_dgrad_c3_bf16mfma(const void* dy_bf16, const void* wpk_bf16_dgrad, float* dx_nchw, int N, int H, int W, int Cout, hipStream_t stream);
// exact fp32 weight gradient, the generic kernel (wgrad_f32.hip): fp32 x and dy.  *_check: the argument checks every fp32-tensor call of the
// exact kernels meets (the skinny launcher's too)
size_t osvos_wgrad_ws_bytes_f32(int N, int H, int W, int Cin_s, int Cout);
int osvos_wgrad_f32_check(const WgradCall& c);
int osvos_conv3x3_wgrad_f32(const WgradCall& c);
int osvos_wgrad_f32_plan(const WgradCall& c, WgradPlan* p);
int osvos_nchw_to_nhwc_f32(const float* src, float* dst, void* dstbf, int N, int C, int H, int W, int cpad, hipStream_t stream);
int osvos_nhwc_to_nchw_f32(const float* src, float* dst, int N, int C, int H, int W, int cs, hipStream_t stream);
int osvos_pack_fwd_f32(const float* w, float* wpk, int Cout, int Cin, hipStream_t stream);
int osvos_pack_dgrad_f32(const float* w, float* wpk, int Cout, int Cin, hipStream_t stream);
int osvos_maxpool2x2_f32(const float* x, float* y, void* ybf, int N, int H, int W, int C, hipStream_t stream);
int osvos_maxpool2x2_bwd_f32(const float* x, const float* dy, const float* dside, float* dx, void* dxbf,
                             int N, int H, int W, int C, hipStream_t stream);
int osvos_maxpool2x2_bf16(const void* x, void* y, int N, int H, int W, int C, hipStream_t stream);
int osvos_maxpool2x2_bf16_code(const void* x, void* y, void* code, int N, int H, int W, int C, hipStream_t stream);
int osvos_maxpool2x2_bwd_bf16_code(const void* code, const void* dy, const void* dside, void* dx, int N, int H, int W, int C, hipStream_t stream);
int osvos_maxpool2x2_bwd_bf16(const void* x, const void* dy, const void* dside, void* dx, int N, int H, int W, int C, hipStream_t stream);
int osvos_head_lowres_f32(const float* prep, const float* wd, const float* bd, const float* wf,
                          float* score, float* fpart, int N, int h, int w, hipStream_t stream);
int osvos_head_bwd_f32(const float* prep, const float* dside, const float* dfused, const float* f1, const float* f16,
                       const float* wd, const float* wf, float* dprep, void* dprep_bf16, double* acc, int N, int H, int W, int h, int w,
                       int scale_idx, hipStream_t stream);
int osvos_head_bwd4_f32(const float* const* prep, const float* const* dside, const float* dfused, const float* const* f1, const float* const* f16,
                        const float* const* wd, const float* wf, float* const* dprep, void* const* dprep_bf16, double* const* acc,
                        int N, int H, int W, const int* hs, const int* ws, hipStream_t stream);      // the four scales in one launch
int osvos_head_bwd_blocks(int N, int h, int w, int scale_idx);   // workgroups (= partial rows of 34 doubles) head_bwd launches
int osvos_sum_partials(const float* x, long count, double* part, int* nblocks, hipStream_t stream);
// generic (non-diagonal upscale weights) head: head_generic.hip
int osvos_head_weff(const float* wup, const float* wf16, float* weff, int k, hipStream_t stream);
int osvos_head_upsample_generic(const float* const* score, const float* const* prep, const float* const* f1, const float* const* weff,
                                const float* fuse_bias, float* const* outs, int N, int H, int W, const int* hs, const int* ws, hipStream_t stream);
int osvos_head_bwd_generic(const float* prep, const float* dside, const float* dfused, const float* f1, const float* weff, const float* wd,
                           float* dprep, void* dprep_bf16, double* acc, int N, int H, int W, int h, int w, int scale_idx, hipStream_t stream);
int osvos_head_tapsum(const float* P, int channels, const float* d, double* G, int N, int H, int W, int h, int w, int scale_idx, hipStream_t stream);
int osvos_head_generic_param_grads(const float* wup, const float* wf16, const double* G, float* dwf16, float* dwup, int k, int accumulate, hipStream_t stream);
int osvos_head_dw1(const double* G1, float* dw, int k, int accumulate, hipStream_t stream);

// bf16-operand MFMA convolution (conv3x3_bf16.hip): x fp32 or bf16, bf16 pack, fp32 and / or bf16 result.  Tile ids: 0-11 register-staged,
// 30-37 LDS-DMA staged and 38 persistent (bf16 x only; its plan hands them to the two launchers below), 40-45 two-piece weights
int osvos_pack_fwd_bf16(const float* w, void* wpk, int Cout, int Cin, hipStream_t stream);
int osvos_pack_dgrad_bf16(const float* w, void* wpk, int Cout, int Cin, hipStream_t stream);
int osvos_conv3x3_bf16mfma(const ConvCall& c);
int osvos_conv3x3_bf16mfma_plan(const ConvCall& c, ConvPlan* p);
int osvos_conv3x3_bf16mfma_num_tiles(void);
int osvos_conv3x3_bf16w2_tiles_impl(int* tiles, int max);
int osvos_conv3x3_bf16mfma_xb_tiles(int* tiles, int max);
// LDS-DMA staged variant (conv3x3_bf16_dma.hip; bf16 x, single-piece pack): variant = tile id - 30 (0-3: 256 px x 128 / 64 co with 4 waves,
// 512 px x 128 / 64 co with 8 waves; 4, 5: persistent forms; 6, 7: resident-filter persistent forms for Cin = 64).  The bf16 family's choose()
// names the variant and the map in the plan; *_plan checks the call against them and completes the plan, the launcher takes it as it is
bool osvos_conv3x3_bf16_dma_applicable(int Cin, int Cout, int y_cs);
int osvos_conv3x3_bf16_dma_num_variants(void);
int osvos_conv3x3_bf16_dma_plan(const ConvCall& c, ConvPlan* p);
int osvos_conv3x3_bf16_dma(const ConvCall& c, const ConvPlan& p);
// Cin = 64, bf16 in / out: persistent, resident filter, deferred + skewed packed epilogue (conv3x3_bf16_p64.hip; tile id 38); plan as above
bool osvos_conv3x3_bf16_p64_applicable(const ConvCall& c);
int osvos_conv3x3_bf16_p64_plan(const ConvCall& c, ConvPlan* p);
int osvos_conv3x3_bf16_p64(const ConvCall& c, const ConvPlan& p);

// bf16-operand weight gradient (wgrad_bf16.hip): x and dy both fp32 or both bf16 (the bf16-store mode of the network)
bool osvos_wgrad_bf16_applicable(const WgradCall& c);
size_t osvos_wgrad_bf16_ws_bytes(int N, int H, int W, int Cin_s, int Cout);
int osvos_conv3x3_wgrad_bf16mfma(const WgradCall& c);
int osvos_wgrad_bf16_plan(const WgradCall& c, WgradPlan* p);
// the skinny fp32 kernels (wgrad_small_f32.hip): Cin = 3 (conv1_1: x fp32, dy fp32 or bf16) and Cout = 16 (side_prep: dy fp32, x fp32 or bf16).
// *_applicable: the shape is one of the two (and OSVOS_WGRAD_GENERIC does not hand an fp32-tensor call to the generic kernel)
bool osvos_wgrad_small_applicable(const WgradCall& c);
size_t osvos_wgrad_small_ws_bytes(int N, int H, int W, int Cin_s, int Cout);
int osvos_conv3x3_wgrad_small_f32(const WgradCall& c);
int osvos_wgrad_small_plan(const WgradCall& c, WgradPlan* p);
void osvos_wgrad_c3_split(int N, int H, int W, int bf16_pipe, WgradPlan* p);      // how either conv1_1 kernel cuts a frame (no checks; osvos_wgrad_c3_plan)
