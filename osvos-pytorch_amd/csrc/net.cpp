// Whole-network orchestration: OSVOS.forward (reference vgg_osvos.py:59-74) and its backward as
// two C calls that only enqueue kernels on the caller's stream (no allocation, no sync, so both
// are hipGraph-capturable).  The caller owns `wbuf` (packed parameters) and `ws` (activations +
// gradient scratch); their layouts are defined here and nowhere else.
#include <stdlib.h>
#include <string.h>

#include "kernels.h"
#include "prof.h"

namespace {
inline int streamk_mode();      // (defined with the other process-cached switches below)

constexpr int kStageN[5] = {2, 2, 3, 3, 3};
constexpr int kStageC[5] = {64, 128, 256, 512, 512};
constexpr int kNumTrunk = 13;
constexpr int kNumConv = 17;          // 13 trunk + 4 side_prep
constexpr int kInPad = 8;             // conv1_1 input channels padded 3 -> 8 (one K chunk)

// the 17 3x3 convolutions: 13 of the trunk in order (kStageN[stage] per stage, kStageC[stage] output channels), then side_prep[0..3], which read
// the last activation of stages 1-4.  cin_s: channel stride of the input tensor (conv1_1's 3 channels are padded to kInPad)
struct ConvDesc {
  int stage, cin, cin_s, cout, w_param, b_param;
};
constexpr ConvDesc conv_row(int l, int stage, int cin, int cout) { return ConvDesc{stage, cin, cin == 3 ? kInPad : cin, cout, slot::conv_w(l), slot::conv_b(l)}; }
constexpr ConvDesc kConv[kNumConv] = {
    conv_row(0, 0, 3, 64),     conv_row(1, 0, 64, 64),                                                             // conv1_x
    conv_row(2, 1, 64, 128),   conv_row(3, 1, 128, 128),                                                           // conv2_x
    conv_row(4, 2, 128, 256),  conv_row(5, 2, 256, 256),   conv_row(6, 2, 256, 256),                               // conv3_x
    conv_row(7, 3, 256, 512),  conv_row(8, 3, 512, 512),   conv_row(9, 3, 512, 512),                               // conv4_x
    conv_row(10, 4, 512, 512), conv_row(11, 4, 512, 512),  conv_row(12, 4, 512, 512),                              // conv5_x
    conv_row(13, 1, 128, 16),  conv_row(14, 2, 256, 16),   conv_row(15, 3, 512, 16),   conv_row(16, 4, 512, 16)};  // side_prep[0..3]

// (the rows restate kStageN / kStageC, which the stage loops and the layouts still walk: an edit of one without the other does not compile)
constexpr bool conv_table_agrees() {
  int l = 0;
  for (int si = 0; si < 5; ++si)
    for (int j = 0; j < kStageN[si]; ++j, ++l)
      if (l >= kNumTrunk || kConv[l].stage != si || kConv[l].cout != kStageC[si] || kConv[l].cin != (j > 0 ? kStageC[si] : si > 0 ? kStageC[si - 1] : 3)) return false;
  for (int i = 0; i < 4; ++i)
    if (kConv[kNumTrunk + i].stage != i + 1 || kConv[kNumTrunk + i].cin != kStageC[i + 1] || kConv[kNumTrunk + i].cout != 16) return false;
  return l == kNumTrunk;
}
static_assert(conv_table_agrees(), "kConv disagrees with kStageN / kStageC");

int last_of_stage(int si) {
  int l = -1;
  for (int s = 0; s <= si; ++s) l += kStageN[s];
  return l;
}

struct WbufLayout {
  size_t fwd[kNumConv], dgrad[kNumConv], bias[kNumConv];
  size_t fwd3[kNumConv], dgrad3[kNumConv];      // OSVOS_F32_X3: pre-split bf16x3 packs of the layers the f32x3 kernels take ((size_t)-1: none)
  size_t fwd_lo[kNumConv];   // OSVOS_FLAG_BF16_W2: lo planes of the forward packs, BEHIND everything else ((size_t)-1: none)
  size_t wd[4], bd[4], wf, bf, f1[4], f16[4];
  size_t weff[4];            // generic head only: Weff_i[16][k*k] (head_generic.hip)
  size_t wup[4];             // generic head only: copy of upscale[i].weight [16][16][k][k] (the backward forms fuse / upscale gradients from it)
  size_t total;
};

// With OSVOS_FLAG_BF16_W2 (dw.w2) the layout is the single-piece one plus the 17 forward lo planes appended in layer order (trunk 0-12, side_prep
// 13-16): every other offset is unchanged, so the hi planes ARE the bf16 packs and a backward finds its packs with or without the flag
WbufLayout wbuf_layout(const DtypeWord& dw) {
  const int dtype = dw.dtype;
  WbufLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  for (int l = 0; l < kNumConv; ++l) {
    L.fwd[l] = take(osvos_wpack_bytes(kConv[l].cout, kConv[l].cin_s, dtype));
    L.dgrad[l] = take(osvos_wpack_dgrad_bytes(kConv[l].cout, kConv[l].cin, dtype));
    L.bias[l] = take(sizeof(float) * kConv[l].cout);
    L.fwd3[l] = L.dgrad3[l] = (size_t)-1;
    if (dtype == OSVOS_F32_X3) {
      if (kConv[l].cin_s % 16 == 0 && kConv[l].cin == kConv[l].cin_s) L.fwd3[l] = take(osvos_wpack_x3_bytes(kConv[l].cout, kConv[l].cin));
      if (kConv[l].cout % 16 == 0) L.dgrad3[l] = take(osvos_wpack_x3_bytes(kConv[l].cin, kConv[l].cout));
    }
  }
  for (int i = 0; i < 4; ++i) { L.wd[i] = take(16 * sizeof(float)); L.bd[i] = take(sizeof(float)); }
  L.wf = take(64 * sizeof(float));
  L.bf = take(sizeof(float));
  for (int i = 0; i < 4; ++i) { const int k = 4 << i; L.f1[i] = take(sizeof(float) * k * k); L.f16[i] = take(sizeof(float) * k * k); }
  for (int i = 0; i < 4; ++i) { const int k = 4 << i; L.weff[i] = take(sizeof(float) * 16 * k * k); }
  for (int i = 0; i < 4; ++i) { const int k = 4 << i; L.wup[i] = take(sizeof(float) * 256 * k * k); }
  for (int l = 0; l < kNumConv; ++l) L.fwd_lo[l] = dw.w2 ? take(osvos_wpack_bytes(kConv[l].cout, kConv[l].cin_s, dtype)) : (size_t)-1;
  L.total = off;
  return L;
}

// bf16-ONLY trunk tensors: in the bf16-MFMA mode activations, pooled tensors and their gradients are stored as bf16 and nothing
// fp32 is written for them (default; OSVOS_BF16_STORE=0 keeps fp32 tensors and rounds while staging).  Producers write half the
// bytes, consumers read half the bytes; pooling and its backward run on bf16; bias / skinny weight gradients are formed from the
// bf16 tensors.  Measured: 666 -> 746 frames/s (batch 12), 374 -> 415 (batch 1).
inline bool use_store(int dtype) {
  static const bool on = [] { const char* e = getenv("OSVOS_BF16_STORE"); return !(e && e[0] == '0'); }();
  return dtype == OSVOS_F32_BF16MFMA && on;
}

inline char* at(void* base, size_t off) { return reinterpret_cast<char*>(base) + off; }
inline const char* at(const void* base, size_t off) { return reinterpret_cast<const char*>(base) + off; }

// the two views a workspace tensor can have (WsLayout::view); NULL = the tensor does not exist in that format
struct Tensor {
  void* f;      // fp32
  void* b;      // bf16
};

struct WsLayout {
  int hs[5], ws[5];
  size_t xin, act[kNumTrunk], pooled[5], prep[4], score[4], fpart[4];
  size_t conv_part;          // split-K partial sums of the small deep layers (forward prefix: inference uses it too)
  size_t sk_ws;              // f32x3: stream-K workspace of the main-stream convolutions (tickets + partial slots; (size_t)-1 = none)
  size_t side_part[4];       // the same for the side_prep convolutions, which run on the aux stream beside the trunk (own buffers)
  size_t dy[kNumTrunk], dpool[5], dside[4], dprep[4], wgrad[kNumConv], acc, dxin;
  size_t gbuf[4];            // generic head only: tap-indexed reductions G_i[16][k*k] + G1_i[k*k], doubles
  // bf16-store mode (dtype OSVOS_F32_BF16MFMA, OSVOS_BF16_STORE=1): the trunk tensors (act, pooled, dy, dpool, dside) ARE bf16, at the offsets
  // above, and nothing fp32 is written for them; xin and dprep stay fp32 and get a bf16 copy here (0 / unused otherwise)
  bool store;
  size_t xin_b, dprep_b[4];
  // sign bits of the activations that later serve as ReLU masks (maskbits.h; (size_t)-1 = none): [N][h][w][cout / 32] words
  size_t bits[kNumTrunk];
  // bf16-store mode: one code byte per pooled element, written by the forward's pooling (fused epilogue or kernel), read by maxpool_bwd
  // instead of the pool's input (pool.hip; (size_t)-1 = none)
  size_t pool_code[5];
  size_t fwd_total, total;

  // a tensor of the workspace `ws` as a launcher takes it: trunk tensors have ONE view (bf16 in the store mode, else fp32); with `off_b` (xin,
  // dprep) the fp32 view always and the bf16 copy in the store mode
  Tensor view(void* ws, size_t off) const { return store ? Tensor{nullptr, at(ws, off)} : Tensor{at(ws, off), nullptr}; }
  Tensor view(void* ws, size_t off, size_t off_b) const { return Tensor{at(ws, off), store ? at(ws, off_b) : nullptr}; }
};

// One-bit ReLU masks (maskbits.h): the forward writes the sign bits of every activation a data gradient is later masked with, the data
// gradient reads one word per (pixel, 32 channels) instead of the activation itself.  bf16-store mode (OSVOS_MASK_BITS=0: the activation).
inline bool use_mask_bits(int dtype) {
  static const bool on = [] { const char* e = getenv("OSVOS_MASK_BITS"); return !(e && e[0] == '0'); }();
  return on && (use_store(dtype) || dtype == OSVOS_F32_X3);
}
// act[l] masks the data gradient of layer l + 1 when both are in the same stage; stage 4's last activation masks its side branch's.
// f32x3 (fp32 tensors): only where the f32x3 kernel produces the activation in ONE launch -- not conv1_1
// (exact kernel) and not stage 4, whose forward launches are cut along K (bits would pin them to one K range)
inline bool act_is_a_mask(int l, int dtype) {
  const bool is = (l + 1 < kNumTrunk && kConv[l + 1].stage == kConv[l].stage) || l == kNumTrunk - 1;
  if (dtype == OSVOS_F32_X3) return is && l >= 1 && kConv[l].stage <= 3;
  return is;
}

// A/B switch of the round-5 pool-code bytes (OSVOS_POOL_CODE=0: maxpool_bwd recomputes the argmax from the pool's input, as in rounds 1-4)
inline bool use_pool_code() {
  static const bool on = [] { const char* e = getenv("OSVOS_POOL_CODE"); return !(e && e[0] == '0'); }();
  return on;
}

WsLayout ws_layout(int N, int H, int W, int dtype) {
  WsLayout L;
  memset(&L, 0, sizeof(L));
  for (int l = 0; l < kNumTrunk; ++l) L.bits[l] = (size_t)-1;
  for (int si = 0; si < 5; ++si) L.pool_code[si] = (size_t)-1;
  const size_t es = osvos_elem(dtype);
  L.hs[0] = H; L.ws[0] = W;
  for (int i = 1; i < 5; ++i) { L.hs[i] = (L.hs[i - 1] + 1) / 2; L.ws[i] = (L.ws[i - 1] + 1) / 2; }
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  const bool store = L.store = use_store(dtype);
  const size_t te = store ? 2 : es;          // element size of the trunk tensors
  L.xin = take(es * N * H * W * kInPad);
  if (store) L.xin_b = take((size_t)2 * N * H * W * kInPad);
  for (int l = 0; l < kNumTrunk; ++l) {
    const int si = kConv[l].stage;
    const size_t e = (size_t)N * L.hs[si] * L.ws[si] * kConv[l].cout;
    L.act[l] = take(te * e);
    L.bits[l] = (use_mask_bits(dtype) && act_is_a_mask(l, dtype)) ? take(e / 8) : (size_t)-1;
  }
  for (int si = 1; si < 5; ++si) {
    const size_t e = (size_t)N * L.hs[si] * L.ws[si] * kStageC[si - 1];
    L.pooled[si] = take(te * e);
    L.pool_code[si] = (store && use_pool_code()) ? take(e) : (size_t)-1;
  }
  for (int i = 0; i < 4; ++i) {
    const size_t npix = (size_t)N * L.hs[i + 1] * L.ws[i + 1];
    L.prep[i] = take(es * npix * 16);
    L.score[i] = take(sizeof(float) * npix);
    L.fpart[i] = take(sizeof(float) * npix);
  }
  {
    size_t mx = 0;
    for (int l = 0; l < kNumTrunk; ++l)
      if (kConv[l].cin >= 256) {
        const size_t b = osvos_conv3x3_splitk_ws_bytes_f32(N, L.hs[kConv[l].stage], L.ws[kConv[l].stage], kConv[l].cout > kConv[l].cin ? kConv[l].cout : kConv[l].cin);
        if (b > mx) mx = b;
      }
    L.conv_part = take(mx);
    // stream-K is opt-in (OSVOS_X3_STREAMK, read once per process): its 64 MiB of tickets + partial tiles exist only in layouts that use them
    L.sk_ws = (dtype == OSVOS_F32_X3 && streamk_mode() >= 1) ? take(osvos_conv3x3_f32x3_streamk_ws_bytes()) : (size_t)-1;
    // side_prep[i]: Cout = 16 on a small frame is a handful of workgroups walking K = 9 Cin serially (88 us for 0.24 GFLOP at
    // 30 x 54) -- and the last one sits exposed between conv5_3 and the head.  K splits turn it into a full-chip launch.
    for (int i = 0; i < 4; ++i)
      L.side_part[i] = kStageC[i + 1] >= 256 ? take(osvos_conv3x3_splitk_ws_bytes_f32(N, L.hs[i + 1], L.ws[i + 1], 16)) : (size_t)-1;
  }
  L.fwd_total = off;          // everything above is all an inference-only forward touches
  for (int i = 0; i < 4; ++i) {
    const size_t npix = (size_t)N * L.hs[i + 1] * L.ws[i + 1];
    L.dprep[i] = take(es * npix * 16);
    L.dprep_b[i] = store ? take((size_t)2 * npix * 16) : 0;
    L.dside[i] = take(te * npix * kStageC[i + 1]);
  }
  // one gradient buffer per trunk conv output (dLoss/d act[l], ReLU mask applied) and per pooled
  // tensor: no buffer is ever rewritten inside one backward, so the weight-gradient stream can trail
  // the data-gradient stream by any number of layers without write-after-read hazards
  for (int l = 0; l < kNumTrunk; ++l) {
    const size_t e = (size_t)N * L.hs[kConv[l].stage] * L.ws[kConv[l].stage] * kConv[l].cout;
    L.dy[l] = take(te * e);
  }
  for (int si = 1; si < 5; ++si) L.dpool[si] = take(te * N * L.hs[si] * L.ws[si] * kStageC[si - 1]);
  // one slab workspace per layer: the slab reduce of layer l runs on its own stream while the partial
  // kernel of the next layer already refills another buffer
  for (int l = 0; l < kNumConv; ++l) {
    const int si = kConv[l].stage;
    L.wgrad[l] = take(osvos_wgrad_ws_bytes(N, L.hs[si], L.ws[si], kConv[l].cin_s, kConv[l].cout, dtype));
  }
  L.acc = take(sizeof(double) * (5 * OSVOS_HEAD_MAX_BLOCKS * 34));   // head_bwd partials: 4 scales + fuse bias
  L.dxin = take(es * N * H * W * 4);
  for (int i = 0; i < 4; ++i) { const int k = 4 << i; L.gbuf[i] = take(sizeof(double) * 17 * k * k); }
  L.total = off;
  return L;
}

// events for the fork/join of the two-stream backward: created once per host thread, reused round-robin
struct EventPool {
  hipEvent_t ev[128];      // (round-robin: an event recorded early in a backward and waited for late must not come around in between -- ~45 per call)
  int n = 0, cur = 0;
  hipEvent_t next() {
    if (n < 128) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
        osvos_set_error("net_backward: hipEventCreate failed");
        return nullptr;
      }
      ev[n++] = e;
      return e;
    }
    hipEvent_t e = ev[cur];
    cur = (cur + 1) % 128;
    return e;
  }
};
EventPool& event_pool() {
  static thread_local EventPool p;
  return p;
}

// `waiter` waits for everything enqueued on `on` so far
int stream_wait(hipStream_t waiter, hipStream_t on) {
  hipEvent_t e = event_pool().next();
  if (!e) return -1;
  OSVOS_HIP_CHECK(hipEventRecord(e, on));
  OSVOS_HIP_CHECK(hipStreamWaitEvent(waiter, e, 0));
  return 0;
}

// The convolution of layer l (forward) or its data gradient (dgrad: Cin and Cout swap roles) on an h x w map, as far as the layer table and the
// packed parameters and the call's f32x3 `pieces` decide it; the caller adds operands, results and workspaces by name.  Precision 'bf16w2':
// forward packs have two pieces
ConvCall conv_of(const ConvDesc& dl, int l, bool dgrad, const void* wbuf, const WbufLayout& P, int pieces, int N, int h, int w, hipStream_t stream) {
  ConvCall c;
  c.pieces = pieces;
  const size_t w3 = dgrad ? P.dgrad3[l] : P.fwd3[l];
  c.wpk = at(wbuf, dgrad ? P.dgrad[l] : P.fwd[l]);
  if (w3 != (size_t)-1) c.wpk3 = at(wbuf, w3);
  if (!dgrad) c.bias = reinterpret_cast<const float*>(at(wbuf, P.bias[l]));
  if (!dgrad && P.fwd_lo[l] != (size_t)-1) { c.w_pieces = 2; c.w_lo = P.fwd_lo[l] - P.fwd[l]; }
  c.N = N; c.H = h; c.W = w;
  c.Cin = dgrad ? dl.cout : dl.cin_s;
  c.Cout = c.y_cs = dgrad ? dl.cin : dl.cout;
  c.stream = stream;
  return c;
}
inline void set_x(ConvCall& c, Tensor t) { c.x = t.b ? t.b : t.f; c.x_bf16 = t.b != nullptr; }                // (the bf16 view is preferred when present)
inline void set_mask(ConvCall& c, Tensor t) { c.mask = t.b ? t.b : t.f; c.mask_bf16 = t.b != nullptr; }
inline void set_y(ConvCall& c, Tensor t) { c.y = reinterpret_cast<float*>(t.f); c.y_bf16 = t.b; }

// f32x3 and the bf16-store mode: the forward max-pool of a stage boundary runs as an epilogue of the stage's last convolution (epi.h).
// Measured at 854x480 batch 1 (profiles/r03_ab_fusions.txt): saves its launch and 20 us (1.473 -> 1.451 ms of forward convolutions +
// pools).  OSVOS_FUSE_POOL=0 (tests: bit-identity against the separate launches) turns it off.
inline bool fuse_pool(int dtype) {
  static const bool on = [] { const char* e = getenv("OSVOS_FUSE_POOL"); return !(e && e[0] == '0'); }();
  return on && (dtype == OSVOS_F32_X3 || use_store(dtype));
}

// f32x3 stream-K (conv3x3_f32x3.hip): OSVOS_X3_STREAMK = 0 (default) off, 1 the forward's main-stream convolutions, 2 also the data-gradient
// chain.  Built and measured in round 4 (profiles/r04_tune_streamk.txt, docs/DESIGN_rounds_1-4.md 3.9): op level the 64-cout tiles gain 4-7 % (conv1_2, conv4_x)
// and the 128-cout tile loses 1-12 % (conv2_x, conv3_x); in the network, with the automatic choice restricted to the winners, the headline
// loop reads 234.8-235.9 frames/s against 235.2-236.2 without it (three alternating runs on one box) and configs[4] 157.2-157.3 against
// 157.3-157.5 -- the CUs a plain grid leaves without a tile are not idle in the step: the side-branch convolutions of the second stream run
// there.  Mode 2 costs 3.6 % (the weight-gradient stream already fills the data-gradient chain's idle CUs).  Hence opt-in.
inline int streamk_mode() {
  static const int v = [] { const char* e = getenv("OSVOS_X3_STREAMK"); return e ? atoi(e) : 0; }();
  return v;
}

// TIMING ABLATIONS (wrong results; tools/ablate_step.sh) exist only in probe builds (make EXTRA=-DOSVOS_DBG_ABLATIONS): OSVOS_DBG_SKIP bit
// 1 = no slab reduces, 2 = no pool backward kernels, 8 = no side_prep data gradients, 16 = no side_prep weight gradients, 32 = no input
// gradient, 64 = no conv1_1 weight gradient.  The shipped library never skips work.
#ifdef OSVOS_DBG_ABLATIONS
inline int dbg_skip() {
  static const int v = [] { const char* e = getenv("OSVOS_DBG_SKIP"); return e ? atoi(e) : 0; }();
  return v;
}
#else
constexpr int dbg_skip() { return 0; }
#endif

// What the head launchers take per scale i = 0..3 (stage i + 1), typed, gathered once per call: the head's parameters in wbuf and its tensors in ws.
// The forward touches the first two rows only (the backward's tensors lie behind an inference workspace's end: addresses, never read)
struct HeadPtrs {
  const float *wd[4], *bd[4], *f1[4], *f16[4], *weff[4], *wup[4], *wf, *bf;      // score_dsn, the deconvolution filters, (generic) Weff and upscale; fuse
  float *prep[4], *score[4], *fpart[4];
  float* dprep[4];
  void* dprep_b[4];           // (bf16 copy of dprep: store mode, else NULL)
  double *acc[4], *fb_acc;    // head_bwd partials per scale, then the fuse bias's
};
HeadPtrs head_ptrs(const void* wbuf, const WbufLayout& P, void* ws, const WsLayout& L) {
  HeadPtrs h;
  auto par = [&](size_t off) { return reinterpret_cast<const float*>(at(wbuf, off)); };
  auto ten = [&](size_t off) { return reinterpret_cast<float*>(at(ws, off)); };
  double* const acc = reinterpret_cast<double*>(at(ws, L.acc));
  for (int i = 0; i < 4; ++i) {
    h.wd[i] = par(P.wd[i]); h.bd[i] = par(P.bd[i]); h.f1[i] = par(P.f1[i]); h.f16[i] = par(P.f16[i]); h.weff[i] = par(P.weff[i]); h.wup[i] = par(P.wup[i]);
    h.prep[i] = ten(L.prep[i]); h.score[i] = ten(L.score[i]); h.fpart[i] = ten(L.fpart[i]);
    const Tensor dprep = L.view(ws, L.dprep[i], L.dprep_b[i]);
    h.dprep[i] = reinterpret_cast<float*>(dprep.f);
    h.dprep_b[i] = dprep.b;
    h.acc[i] = acc + (size_t)i * OSVOS_HEAD_MAX_BLOCKS * 34;
  }
  h.wf = par(P.wf); h.bf = par(P.bf);
  h.fb_acc = acc + (size_t)4 * OSVOS_HEAD_MAX_BLOCKS * 34;
  return h;
}

// gradient-ready events armed for the next backward of this host thread (osvos_net_arm_grad_events)
struct GradEvents { hipEvent_t ev[OSVOS_NGRAD_GROUPS]; int n = 0; };
GradEvents& grad_events() {
  static thread_local GradEvents g;
  return g;
}

inline double conv_flops(int N, int h, int w, int cin, int cout) { return 2.0 * N * h * w * (double)cout * 9.0 * cin; }

}  // namespace

// device-side helpers implemented in net_kernels.hip
int osvos_gather_small(const float* const* srcs, const size_t* dst_off, const int* counts, int n, void* wbuf, hipStream_t stream);
int osvos_head_grads_finalize(const double* const* part, const int* nblk, const double* fb_part, int fb_nblk,
                              float* const* grads, int accumulate, int have_side, hipStream_t stream);

extern "C" {

// (every entry decodes its dtype word with osvos_dtype_word, common.h: an unbuilt dtype or OSVOS_FLAG_BF16_W2 on another dtype than
// OSVOS_F32_BF16MFMA is an argument error in all of them -- 0 bytes from the size queries)
size_t osvos_net_wbuf_bytes(int dtype_) {
  DtypeWord dw;
  return osvos_dtype_word(dtype_, "net_wbuf_bytes", &dw) ? wbuf_layout(dw).total : 0;
}
size_t osvos_net_ws_bytes(int N, int H, int W, int dtype_) {
  DtypeWord dw;
  return osvos_dtype_word(dtype_, "net_ws_bytes", &dw) ? ws_layout(N, H, W, dw.dtype).total : 0;
}
size_t osvos_net_ws_bytes_infer(int N, int H, int W, int dtype_) {
  DtypeWord dw;
  return osvos_dtype_word(dtype_, "net_ws_bytes_infer", &dw) ? ws_layout(N, H, W, dw.dtype).fwd_total : 0;
}

int osvos_net_ws_query(int N, int H, int W, int dtype_, int which, size_t* offset, size_t* elems, int* channels, int* h, int* w) {
  OSVOS_ARG_CHECK(which >= 0 && which < ws_which::count && offset && elems && channels && h && w, "ws_query: bad arguments");
  DtypeWord dw;
  if (!osvos_dtype_word(dtype_, "ws_query", &dw)) return -1;
  WsLayout L = ws_layout(N, H, W, dw.dtype);
  int si, c;
  size_t off;
  if (which < ws_which::pooled) { si = kConv[which].stage; c = kConv[which].cout; off = L.act[which]; }
  else if (which < ws_which::prep) { si = which - ws_which::pooled + 1; c = kStageC[si - 1]; off = L.pooled[si]; }
  else if (which < ws_which::input) { si = which - ws_which::prep + 1; c = 16; off = L.prep[which - ws_which::prep]; }
  else { si = 0; c = kInPad; off = L.xin; }
  *offset = off; *channels = c; *h = L.hs[si]; *w = L.ws[si];
  *elems = (size_t)N * L.hs[si] * L.ws[si] * c;
  return 0;
}

// storage format of trunk tensor `which` (osvos_net_ws_query 0..16): 0 fp32 NHWC, 1 bf16 NHWC
int osvos_net_ws_format(int dtype_, int which) {
  (void)which;
  DtypeWord dw;
  if (!osvos_dtype_word(dtype_, "ws_format", &dw)) return -1;
  return use_store(dw.dtype) ? 1 : 0;
}

int osvos_net_pack(const float* const* params, void* wbuf, int dtype_, int with_dgrad, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(params && wbuf, "net_pack: null pointer");
  DtypeWord dw;
  if (!osvos_dtype_word(dtype_, "net_pack", &dw)) return -1;
  const int dtype = dw.dtype;
  for (int i = 0; i < OSVOS_NPARAMS; ++i) OSVOS_ARG_CHECK(params[i] != nullptr, "net_pack: params[%d] is null", i);
  WbufLayout L = wbuf_layout(dw);
  // the small parameters (biases, head weights, deconvolution filters): one gather launch
  const float* srcs[64];
  size_t dsts[64];
  int counts[64];
  int ns = 0;
  auto small = [&](int param, size_t dst, int count) { srcs[ns] = params[param]; dsts[ns] = dst; counts[ns] = count; ++ns; };
  // f32x3 with pre-split weights: the fp32 packs are read only where no pre-split pack exists (conv1_1 forward: the exact kernel) and by
  // the input-gradient kernel (layer 0's data-gradient pack); all pre-split packs are formed by ONE launch
  const bool x3ps = dtype == OSVOS_F32_X3 && osvos_x3_presplit();
  // precision 'fp32h2' (dw.half_fwd / half_bwd): forward and / or data-gradient packs in the FP16-pair format (h2split.h) -- same buffers, other contents
  OSVOS_ARG_CHECK(!(dw.half_fwd || dw.half_bwd) || x3ps, "net_pack: the FP16-pair packs exist for dtype OSVOS_F32_X3 with pre-split weights only");
  const bool b16 = dtype == OSVOS_F32_BF16MFMA;      // all bf16 packs (17 filters x 2 forms) in ONE launch too (round 5 prep)
  PackEntry packs[OSVOS_PACK_MAX];
  int nx = 0;
  // layer l's filter -> wbuf + dst in the multi-pack launch; lo: the lo plane of a two-piece forward pack ('bf16w2'; (size_t)-1: single piece)
  auto pack = [&](int l, size_t dst, size_t lo, int dgrad, bool half) {
    PackEntry& e = packs[nx++];
    e.w = params[kConv[l].w_param]; e.dst = at(wbuf, dst); e.lo_dst = lo != (size_t)-1 ? at(wbuf, lo) : nullptr;
    e.Cout = kConv[l].cout; e.Cin = kConv[l].cin; e.dgrad = dgrad; e.half = half;
  };
  for (int l = 0; l < kNumConv; ++l) {
    const ConvDesc& c = kConv[l];
    small(c.b_param, L.bias[l], c.cout);
    if (b16) {
      pack(l, L.fwd[l], L.fwd_lo[l], 0, false);
      if (with_dgrad) pack(l, L.dgrad[l], (size_t)-1, 1, false);
      continue;
    }
    int rc;
    if (!(x3ps && L.fwd3[l] != (size_t)-1) && (rc = osvos_pack_conv3x3_fwd(params[c.w_param], at(wbuf, L.fwd[l]), c.cout, c.cin, dtype, stream))) return rc;
    if (with_dgrad && !(x3ps && L.dgrad3[l] != (size_t)-1 && l != 0) &&
        (rc = osvos_pack_conv3x3_dgrad(params[c.w_param], at(wbuf, L.dgrad[l]), c.cout, c.cin, dtype, stream))) return rc;
    if (L.fwd3[l] != (size_t)-1) pack(l, L.fwd3[l], (size_t)-1, 0, dw.half_fwd);
    if (with_dgrad && L.dgrad3[l] != (size_t)-1) pack(l, L.dgrad3[l], (size_t)-1, 1, dw.half_bwd);
  }
  if (nx > 0) {
    const int rc = b16 ? osvos_pack_bf16_multi(packs, nx, stream) : osvos_pack_x3_multi(packs, nx, stream);
    if (rc) return rc;
  }

  for (int i = 0; i < 4; ++i) {
    const int k = 4 << i;
    small(slot::score_dsn_w(i), L.wd[i], 16);
    small(slot::score_dsn_b(i), L.bd[i], 1);
    small(slot::upscale_(i), L.f1[i], k * k);      // upscale_[i].weight[0,0]
    small(slot::upscale(i), L.f16[i], k * k);      // upscale[i].weight[0,0]
  }
  small(slot::fuse_w, L.wf, 64);
  small(slot::fuse_b, L.bf, 1);
  int rc = osvos_gather_small(srcs, dsts, counts, ns, wbuf, stream);
  if (rc || !dw.generic) return rc;
  for (int i = 0; i < 4; ++i) {      // Weff_i = sum_co wfuse[16 i + co] * upscale[i].weight[:, co]
    const float* wup = params[slot::upscale(i)];
    rc = osvos_head_weff(wup, params[slot::fuse_w] + 16 * i, reinterpret_cast<float*>(at(wbuf, L.weff[i])), 4 << i, stream);
    if (rc) return rc;
    const int k = 4 << i;
    OSVOS_HIP_CHECK(hipMemcpyAsync(at(wbuf, L.wup[i]), wup, sizeof(float) * 256 * k * k, hipMemcpyDeviceToDevice, stream));
  }
  return 0;
}

int osvos_net_forward(const float* x_nchw, const void* wbuf, void* ws, float* const* outs,
                      int N, int H, int W, int dtype_, void* stream_, void* aux_stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  hipStream_t aux_all = aux_stream_ ? (hipStream_t)aux_stream_ : stream;
  const bool two = aux_all != stream;
  OSVOS_ARG_CHECK(x_nchw && wbuf && ws && outs, "net_forward: null pointer");
  DtypeWord dw;
  if (!osvos_dtype_word(dtype_, "net_forward", &dw)) return -1;
  OSVOS_ARG_CHECK(N > 0 && H > 0 && W > 0, "net_forward: bad shape %dx%dx%d", N, H, W);
  for (int i = 0; i < 5; ++i) OSVOS_ARG_CHECK(outs[i] != nullptr, "net_forward: outs[%d] is null", i);
  const int dtype = dw.dtype, pieces = dw.pieces;
  const bool infer = dw.infer;      // no backward will read the sign bits / pool codes: do not write them
  // precision 'bf16w2' (dw.w2): all 17 forward convolutions read two-piece packs (osvos_net_pack with the same flag)
  const WbufLayout P = wbuf_layout(dw);
  const WsLayout L = ws_layout(N, H, W, dtype);
  const HeadPtrs hd = head_ptrs(wbuf, P, ws, L);
  const bool store = L.store;
  Tensor cur = L.view(ws, L.xin, L.xin_b);
  int rc = osvos_nchw_to_nhwc_f32(x_nchw, reinterpret_cast<float*>(cur.f), cur.b, N, 3, H, W, kInPad, stream);
  if (rc) return rc;
  // stream-K workspace of the main-stream convolutions: the tickets must be zero before the first launch (every launch leaves them zero; the
  // workspace itself arrives uninitialised from the caller, so they are cleared once per forward -- a 32 KB memset node, capturable)
  void* const sk_ws = (L.sk_ws != (size_t)-1 && streamk_mode() >= 1) ? at(ws, L.sk_ws) : nullptr;
  if (sk_ws != nullptr) OSVOS_HIP_CHECK(hipMemsetAsync(sk_ws, 0, osvos_conv3x3_f32x3_streamk_ticket_bytes(), stream));
  int l = 0;
  for (int si = 0; si < 5; ++si) {
    const int h = L.hs[si], w = L.ws[si];
    if (si > 0) {
      const Tensor pooled = L.view(ws, L.pooled[si]);
      if (!fuse_pool(dtype)) {      // (else pooled[si] was written by the previous stage's last convolution)
        if (store)
          rc = osvos_maxpool2x2_bf16_code(cur.b, pooled.b, (L.pool_code[si] != (size_t)-1 && !infer) ? at(ws, L.pool_code[si]) : nullptr, N, L.hs[si - 1],
                                          L.ws[si - 1], kStageC[si - 1], stream);
        else
          rc = osvos_maxpool2x2_f32(reinterpret_cast<const float*>(cur.f), reinterpret_cast<float*>(pooled.f), nullptr, N, L.hs[si - 1], L.ws[si - 1],
                                    kStageC[si - 1], stream);
        if (rc) return rc;
      }
      cur = pooled;
    }
    for (int j = 0; j < kStageN[si]; ++j, ++l) {
      {
        ProfScope ps(OSVOS_PROF_CONV_FWD, conv_flops(N, h, w, kConv[l].cin, kConv[l].cout), stream);
        ConvCall c = conv_of(kConv[l], l, false, wbuf, P, pieces, N, h, w, stream);
        c.relu = 1;
        const Tensor act = L.view(ws, L.act[l]);
        set_x(c, cur);
        set_y(c, act);
        const bool has_bits = L.bits[l] != (size_t)-1;
        if (has_bits && !infer) c.y_bits = reinterpret_cast<unsigned*>(at(ws, L.bits[l]));
        if (fuse_pool(dtype) && si < 4 && j == kStageN[si] - 1) {      // last convolution of stages 0-3: + the pooled tensor
          const Tensor pooled = L.view(ws, L.pooled[si + 1]);
          c.pooled = reinterpret_cast<float*>(pooled.f);
          c.pooled_bf16 = pooled.b;
          if (L.pool_code[si + 1] != (size_t)-1 && !infer) c.pool_code = at(ws, L.pool_code[si + 1]);
        }
        // A launch that writes sign bits is never cut along K (f32x3 choose()).  The inference forward writes no bits, so it withholds the
        // partial-sum workspace from those layers instead: same plan, same summation order, the logits of the training forward bit for bit.
        // (Stream-K is decided from the K split alone, so with the split gone sk_ws changes nothing between the two forms.)
        if (!(has_bits && infer)) c.part_ws = at(ws, L.conv_part);
        c.sk_ws = sk_ws;
        rc = osvos_conv3x3_dispatch(c, dtype);
        cur = act;
      }
      if (rc) return rc;
    }
    if (si > 0) {
      // side branch of this stage (skinny Cout=16 conv + the two 1x1 dots): latency-bound launches
      // that run on the aux stream in the shadow of the next stage's big convolutions
      const int i = si - 1, sl = kNumTrunk + i;
      // the LAST stage's side branch has nothing left to hide behind: on the main stream it saves two cross-stream event hops (~12-25 us each)
      hipStream_t aux = (si == 4) ? stream : aux_all;
      if (two && aux != stream && (rc = stream_wait(aux, stream))) return rc;
      {
        ProfScope ps(OSVOS_PROF_OTHER, conv_flops(N, h, w, kConv[sl].cin, 16), aux);
        ConvCall c = conv_of(kConv[sl], sl, false, wbuf, P, pieces, N, h, w, aux);
        set_x(c, cur);
        c.y = hd.prep[i];
        if (L.side_part[i] != (size_t)-1) c.part_ws = at(ws, L.side_part[i]);
        rc = osvos_conv3x3_dispatch(c, dtype);
      }
      if (rc) return rc;
      rc = osvos_head_lowres(hd.prep[i], hd.wd[i], hd.bd[i], hd.wf + 16 * i, hd.score[i], hd.fpart[i], N, h, w, dtype, aux);
      if (rc) return rc;
    }
  }
  if (two && (rc = stream_wait(stream, aux_all))) return rc;
  if (dw.generic)      // non-diagonal upscale weights: fused head from the 16-channel side_prep outputs and Weff (head_generic.hip)
    return osvos_head_upsample_generic(hd.score, hd.prep, hd.f1, hd.weff, hd.bf, outs, N, H, W, &L.hs[1], &L.ws[1], stream);
  return osvos_head_upsample(hd.score, hd.fpart, hd.f1, hd.f16, hd.bf, outs, N, H, W, &L.hs[1], &L.ws[1], stream);
}

int osvos_net_join(void* stream_, void* aux_, void* aux2_) {
  hipStream_t stream = (hipStream_t)stream_;
  for (void* a : {aux_, aux2_}) {
    if (a == nullptr || a == stream_) continue;
    if (const int rc = stream_wait(stream, (hipStream_t)a)) return rc;
  }
  return 0;
}

int osvos_net_arm_grad_events(void* const* events, int n) {
  OSVOS_ARG_CHECK(n >= 0 && n <= OSVOS_NGRAD_GROUPS && (n == 0 || events != nullptr), "arm_grad_events: n = %d (0..%d)", n, OSVOS_NGRAD_GROUPS);
  GradEvents& g = grad_events();
  g.n = n;
  for (int k = 0; k < n; ++k) g.ev[k] = (hipEvent_t)events[k];
  return 0;
}

int osvos_net_backward(const void* wbuf, void* ws, const float* const* douts, float* const* grads,
                       float* dx_nchw, int N, int H, int W, int dtype_, int accumulate, void* stream_, void* aux_stream_,
                       void* aux2_stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  hipStream_t aux = aux_stream_ ? (hipStream_t)aux_stream_ : stream;
  hipStream_t aux2 = aux2_stream_ ? (hipStream_t)aux2_stream_ : aux;
  const GradEvents gev = grad_events();      // armed for this call only
  grad_events().n = 0;
  auto ready = [&](int group, hipStream_t st) -> int {      // group's gradients are complete once `st` gets here
    if (group < gev.n && gev.ev[group] != nullptr) OSVOS_HIP_CHECK(hipEventRecord(gev.ev[group], st));
    return 0;
  };
  const bool two = aux != stream;
  const bool three = aux2 != aux;
  OSVOS_ARG_CHECK(wbuf && ws && douts && grads, "net_backward: null pointer");
  DtypeWord dw;
  if (!osvos_dtype_word(dtype_, "net_backward", &dw)) return -1;      // (OSVOS_FLAG_BF16_W2: the backward of 'bf16w2' is that of 'bf16', on the same packs)
  const int dtype = dw.dtype, pieces = dw.pieces;
  const bool generic = dw.generic;
  // deferred join (OSVOS_FLAG_DEFER_JOIN): not with armed gradient-ready events (their last group is recorded behind the join)
  const bool defer_join = dw.defer_join && gev.n == 0 && aux != stream;
  const WbufLayout P = wbuf_layout(dw);
  const WsLayout L = ws_layout(N, H, W, dtype);
  const HeadPtrs hd = head_ptrs(wbuf, P, ws, L);
  const bool store = L.store;
  // fork: aux waits for everything enqueued on `stream` so far; join: `stream` waits for aux.
  // The weight-gradient kernels run on aux concurrently with the data-gradient kernel of the same
  // layer: both are MFMA kernels with independent stalls (barriers, LDS latency, tails), and
  // together they keep the matrix pipes busier than either does alone.
  auto join = [&]() -> int {
    if (defer_join) return 0;            // the caller joins (osvos_net_join) before it touches a parameter gradient
    int r = two ? stream_wait(stream, aux) : 0;
    if (r == 0 && three) r = stream_wait(stream, aux2);
    return r;
  };
  // Weight gradient of layer l from its input and the gradient of its output: partial slabs on aux (MFMA kernel), then -- the same descriptor --
  // the slab reduce on aux2 (bandwidth kernel).  Without a third stream, and for conv1_1's tail on the main stream (on_main), both halves in one
  // launch sequence.  Store mode: every trunk tensor and dprep's copy are bf16, conv1_1's input stays fp32 (which kernel: osvos_wgrad_dispatch)
  auto wgrad = [&](const void* xin, const void* g, int l, int h, int w, bool on_main) -> int {
    WgradCall c;
    c.x = xin; c.dy = g; c.x_bf16 = store && l != 0; c.dy_bf16 = store;
    c.ws = at(ws, L.wgrad[l]); c.dw = grads[kConv[l].w_param]; c.db = grads[kConv[l].b_param];
    c.N = N; c.H = h; c.W = w; c.Cin = kConv[l].cin; c.Cin_s = kConv[l].cin_s; c.Cout = c.Cout_s = kConv[l].cout; c.accumulate = accumulate; c.pieces = pieces;
    const bool split = three && !on_main;
    c.phase = split ? WGRAD_PARTIALS : WGRAD_BOTH; c.stream = on_main ? stream : aux;
    int r = osvos_wgrad_dispatch(c, dtype);
    if (r || !split || (dbg_skip() & 1)) return r;
    if ((r = stream_wait(aux2, aux))) return r;
    c.phase = WGRAD_REDUCE; c.stream = aux2;
    return osvos_wgrad_dispatch(c, dtype);
  };
  int rc;
  int nblk[4], fb_nblk = 0;
  bool have_side = false;
  for (int i = 0; i < 4; ++i) {
    have_side = have_side || douts[i] != nullptr;
    nblk[i] = osvos_head_bwd_blocks(N, L.hs[i + 1], L.ws[i + 1], i);
  }
  const float* dfused = douts[4];

  // ---- head: upstream full-resolution gradients -> dprep[i] (+ score_dsn / fuse gradients) ----
  if (!generic) {        // the four scales in one launch (as four ~20 us launches they sit back to back on the critical path)
    rc = osvos_head_bwd4_f32(hd.prep, douts, dfused, hd.f1, hd.f16, hd.wd, hd.wf, hd.dprep, hd.dprep_b, hd.acc, N, H, W, &L.hs[1], &L.ws[1], stream);
    if (rc) return rc;
  } else
  for (int i = 0; i < 4; ++i) {
    rc = osvos_head_bwd_generic(hd.prep[i], douts[i], dfused, hd.f1[i], hd.weff[i], hd.wd[i], hd.dprep[i], hd.dprep_b[i], hd.acc[i], N, H, W, L.hs[i + 1],
                                L.ws[i + 1], i, stream);
    if (rc) return rc;
  }
  if (dfused != nullptr) {
    rc = osvos_sum_partials(dfused, (long)N * H * W, hd.fb_acc, &fb_nblk, stream);
    if (rc) return rc;
  }
  // The finalize kernel only feeds PARAMETER gradients (score_dsn, fuse): off the critical path -- on the reduce stream (or the weight-gradient
  // stream) behind an event, so that the data-gradient chain starts one launch earlier (round 6; workspace partials only: nothing of the caller's
  // is read off `stream`; on `stream`, as rounds 1-5 had it, the seam is one launch longer and the step level: 232.1 vs 232.2 frames/s).  The generic
  // head's extra reductions stay on `stream`.
  hipStream_t fin = (!generic && two) ? aux2 : stream;
  if (fin != stream && (rc = stream_wait(fin, stream))) return rc;
  rc = osvos_head_grads_finalize(hd.acc, nblk, hd.fb_acc, fb_nblk, grads, accumulate, have_side ? 1 : 0, fin);
  if (rc) return rc;
  if (generic) {
    // fuse.weight / upscale[i].weight gradients from the tap-indexed sums G_i (the partials above carried zeros for fuse.weight);
    // upscale_[i].weight (the 1 -> 1 side deconv) likewise when asked for.  The upscale weights themselves are read from the copy
    // osvos_net_pack left in wbuf.
    float* const dwf = grads[slot::fuse_w];
    for (int i = 0; i < 4; ++i) {
      const int si = i + 1, k = 4 << i;
      double* G = reinterpret_cast<double*>(at(ws, L.gbuf[i]));
      float* const dwup = grads[slot::upscale(i)];
      float* const dwup1 = grads[slot::upscale_(i)];
      if (dfused != nullptr && (dwf != nullptr || dwup != nullptr)) {
        rc = osvos_head_tapsum(hd.prep[i], 16, dfused, G, N, H, W, L.hs[si], L.ws[si], i, stream);
        if (rc) return rc;
        rc = osvos_head_generic_param_grads(hd.wup[i], hd.wf + 16 * i, G, dwf ? dwf + 16 * i : nullptr, dwup, k, accumulate, stream);
        if (rc) return rc;
      } else if (dwup != nullptr && !accumulate) {
        OSVOS_HIP_CHECK(hipMemsetAsync(dwup, 0, sizeof(float) * 256 * k * k, stream));
      }
      if (dwup1 != nullptr) {
        if (douts[i] != nullptr) {
          rc = osvos_head_tapsum(hd.score[i], 1, douts[i], G + 16 * k * k, N, H, W, L.hs[si], L.ws[si], i, stream);
          if (rc) return rc;
          rc = osvos_head_dw1(G + 16 * k * k, dwup1, k, accumulate, stream);
          if (rc) return rc;
        } else if (!accumulate) {
          OSVOS_HIP_CHECK(hipMemsetAsync(dwup1, 0, sizeof(float) * k * k, stream));
        }
      }
    }
  }
  if ((rc = ready(0, fin))) return rc;      // score_dsn + fuse gradients

  // ---- data-gradient chain on `stream`, weight gradients trailing on `aux` ----------------------
  // ready[k]: event recorded on `stream` when the k-th upstream gradient tensor is complete
  double bwd_flops = 0.0;
  for (int l = 0; l < kNumConv; ++l) bwd_flops += 2.0 * conv_flops(N, L.hs[kConv[l].stage], L.ws[kConv[l].stage], kConv[l].cin, kConv[l].cout);
  if (dx_nchw == nullptr) bwd_flops -= conv_flops(N, H, W, 3, kConv[0].cout);
  ProfScope ps(OSVOS_PROF_CONV_BWD, bwd_flops, stream);
  auto signal = [&]() -> int { return two ? stream_wait(aux, stream) : 0; };      // aux may consume everything `stream` has produced so far
  if ((rc = signal())) return rc;       // dprep[0..3] ready
  // the four skinny side_prep weight gradients head the weight-gradient stream (on the third stream beside the first trunk gradients they
  // measured +0.1-0.25 %, inside the noise: round 3)
  for (int i = 0; i < 4; ++i) {
    const int si = i + 1, sl = kNumTrunk + i, h = L.hs[si], w = L.ws[si];
    const int lx = last_of_stage(si);
    if (grads[kConv[sl].w_param] != nullptr && !(dbg_skip() & 16)) {
      rc = wgrad(at(ws, L.act[lx]), hd.dprep_b[i] ? hd.dprep_b[i] : hd.dprep[i], sl, h, w, false);      // (store mode: bf16 x and bf16 dprep)
      if (rc) return rc;
    }
  }
  if ((rc = ready(1, aux2))) return rc;        // the four side_prep layers (their slab reduces are the last writers, in order, on aux2)
  // The side branches' data gradients (16 -> C channels: one K chunk, all prologue and epilogue, 13-51 us each at batch 1).  Only stage 4's is needed
  // at once (it IS the upstream gradient of conv5_3); dside of stages 3, 2, 1 is consumed three, six and nine trunk layers later, by the pooling
  // backward of the stage boundary.  All four stay on `stream`, in front of the chain.  Those three on the reduce stream beside the head of the
  // chain instead were measured in round 6 and are gone: the backward is bound by the chip's throughput over BOTH chains (the weight-gradient
  // stream ends within 3 us of the data-gradient chain), not by the chain's length -- 238.2 vs 237.4 frames/s at batch 1 (noise), 1147 vs 1157 on
  // configs[2] and 300 vs 306 with the two-piece backward (both slightly worse): same-box alternating rounds.
  for (int i = 3; i >= 0; --i) {
    const int si = i + 1, sl = kNumTrunk + i, h = L.hs[si], w = L.ws[si];
    const int lx = last_of_stage(si);
    // stage 4 has no pool after it: its ReLU mask is applied right here and the result is the
    // upstream gradient of conv5_3; stages 1-3 are merged in maxpool2x2_bwd below
    if (dbg_skip() & 8) continue;
    ConvCall c = conv_of(kConv[sl], sl, true, wbuf, P, pieces, N, h, w, stream);
    set_x(c, L.view(ws, L.dprep[i], L.dprep_b[i]));
    set_y(c, L.view(ws, (i == 3) ? L.dy[lx] : L.dside[i]));
    if (i == 3) {
      set_mask(c, L.view(ws, L.act[lx]));
      if (L.bits[lx] != (size_t)-1) c.mask_bits = reinterpret_cast<const unsigned*>(at(ws, L.bits[lx]));
    }
    rc = osvos_conv3x3_dispatch(c, dtype);
    if (rc) return rc;
  }

  // trunk, deepest layer first; dy[l] = dLoss/d(conv l output), ReLU mask already applied
  // (stream-K for the data-gradient chain only with OSVOS_X3_STREAMK=2; the workspace's tickets are zero: every launch leaves them so)
  void* const sk_bwd = (L.sk_ws != (size_t)-1 && streamk_mode() >= 2) ? at(ws, L.sk_ws) : nullptr;
  for (int l = kNumTrunk - 1; l >= 0; --l) {
    const int si = kConv[l].stage, h = L.hs[si], w = L.ws[si];
    const bool first_of_stage = (l == 0) || kConv[l - 1].stage != si;
    const void* xin = first_of_stage ? (si == 0 ? at(ws, L.xin) : at(ws, L.pooled[si])) : at(ws, L.act[l - 1]);
    const void* g = at(ws, L.dy[l]);
    const Tensor dy = L.view(ws, L.dy[l]);
    // (Measured twice in round 3: conv1_1's weight gradient on the third stream BESIDE the input gradient instead of behind it is neutral at
    //  batch 1 (f32x3) and 0.5-1 % slower at batch 12 (bf16) -- not built in.)
    // conv1_1's weight gradient is the LAST piece of work of the step and the weight-gradient stream is the one that finishes last (conv1_2's
    // gradient is still running when the data-gradient chain ends): it goes on the main stream, behind the input gradient, beside conv1_2's
    const bool tail_on_main = l == 0 && two && !defer_join;      // (deferred join: everything gradient-related stays on the side streams)
    if (grads[kConv[l].w_param] != nullptr && !tail_on_main) {
      if ((rc = signal())) return rc;   // dy[l] ready -> its weight gradient may start on aux
      rc = wgrad(xin, g, l, h, w, false);
      if (rc) return rc;
    }
    if (first_of_stage && !tail_on_main && (rc = ready(2 + (4 - si), aux2))) return rc;      // stage si complete (its first conv is the last one processed)
    if (l == 0) {
      if (dbg_skip() & 32) {
      } else if (dx_nchw != nullptr && (dtype == OSVOS_F32 || dtype == OSVOS_F32_X3)) {
        rc = osvos_conv3x3_dgrad_c3_f32(reinterpret_cast<const float*>(g), reinterpret_cast<const float*>(at(wbuf, P.dgrad[0])), dx_nchw, N, h, w, kConv[0].cout, stream);
        if (rc) return rc;
      } else if (dx_nchw != nullptr && dy.b != nullptr && kConv[0].cout == 64) {
        // bf16 trunk tensors: the whole 64-channel halo tile once through LDS, filter rows on the matrix pipe, straight into NCHW (dgrad_c3.hip;
        // same-box A/B at batch 12, two alternating rounds: 1118.7 / 1114.1 frames/s against 1099.1 / 1106.4 with the 32-cout tile + layout
        // kernel below; the fp32-FMA kernel fed with bf16, a first attempt of the round, read 1073-1081 and is gone)
        rc = osvos_conv3x3_dgrad_c3_bf16mfma(dy.b, at(wbuf, P.dgrad[0]), dx_nchw, N, h, w, kConv[0].cout, stream);
        if (rc) return rc;
      } else if (dx_nchw != nullptr) {
        ConvCall c = conv_of(kConv[0], 0, true, wbuf, P, pieces, N, h, w, stream);
        set_x(c, dy);
        c.y = reinterpret_cast<float*>(at(ws, L.dxin));
        c.y_cs = 4;
        rc = osvos_conv3x3_dispatch(c, dtype);
        if (rc) return rc;
        rc = osvos_nhwc_to_nchw(at(ws, L.dxin), dx_nchw, N, 3, H, W, 4, dtype, stream);
        if (rc) return rc;
      }
      if (tail_on_main) {
        if (grads[kConv[0].w_param] != nullptr && !(dbg_skip() & 64) && (rc = wgrad(xin, g, 0, h, w, true))) return rc;
        if ((rc = join())) return rc;
        return ready(2 + 4, stream);      // stage 0 complete: conv1_2's reduce (aux2, joined) and conv1_1's (main)
      }
      break;
    }
    ConvCall c = conv_of(kConv[l], l, true, wbuf, P, pieces, N, h, w, stream);      // the data gradient of layer l; below: where it goes and what masks it
    set_x(c, dy);
    c.part_ws = at(ws, L.conv_part);
    c.sk_ws = sk_bwd;
    if (first_of_stage) {
      // through the pool into the previous stage's output (+ that stage's side branch, + ReLU mask)
      set_y(c, L.view(ws, L.dpool[si]));
      if ((rc = osvos_conv3x3_dispatch(c, dtype))) return rc;
      const int ps2 = si - 1;
      const void* dside = ps2 >= 1 ? at(ws, L.dside[ps2 - 1]) : nullptr;
      if (dbg_skip() & 2) continue;
      if (store && L.pool_code[si] != (size_t)-1)      // one code byte per pooled element instead of the pool's four inputs
        rc = osvos_maxpool2x2_bwd_bf16_code(at(ws, L.pool_code[si]), at(ws, L.dpool[si]), dside, at(ws, L.dy[l - 1]), N, L.hs[ps2], L.ws[ps2],
                                            kStageC[ps2], stream);
      else if (store)
        rc = osvos_maxpool2x2_bwd_bf16(at(ws, L.act[l - 1]), at(ws, L.dpool[si]), dside, at(ws, L.dy[l - 1]), N, L.hs[ps2], L.ws[ps2],
                                       kStageC[ps2], stream);
      else
        rc = osvos_maxpool2x2_bwd_f32(reinterpret_cast<const float*>(at(ws, L.act[l - 1])), reinterpret_cast<const float*>(at(ws, L.dpool[si])),
                                      reinterpret_cast<const float*>(dside), reinterpret_cast<float*>(at(ws, L.dy[l - 1])), nullptr, N,
                                      L.hs[ps2], L.ws[ps2], kStageC[ps2], stream);
      if (rc) return rc;
    } else {
      set_y(c, L.view(ws, L.dy[l - 1]));
      set_mask(c, L.view(ws, L.act[l - 1]));
      if (L.bits[l - 1] != (size_t)-1) c.mask_bits = reinterpret_cast<const unsigned*>(at(ws, L.bits[l - 1]));
      if ((rc = osvos_conv3x3_dispatch(c, dtype))) return rc;
    }
  }
  if ((rc = join())) return rc;         // everything is back on `stream` when the call returns
  return 0;
}

}  // extern "C"
