// extern "C" surface of libosvos_hip.so: argument checks + dtype dispatch for the per-op entry
// points declared in include/osvos_hip.h.  (The whole-network calls live in net.cpp.)
#include "kernels.h"

// fp32 tensors in HBM for both built dtypes (OSVOS_F32 and OSVOS_F32_BF16MFMA); only the conv / pack entry
// points behave differently for the latter
#define NEED_F32(dtype, what)                                                                     \
  OSVOS_ARG_CHECK(osvos_dtype_built(dtype), "%s: dtype %d not built (fp32 tensors only)", what, (int)(dtype))

// Which weight-gradient family takes the launch (kernels.h): two rules, by what the tensors are.  NULL (and the error set): no kernel takes the call
struct WgradEntry {
  bool (*applicable)(const WgradCall&);
  int (*plan)(const WgradCall&, WgradPlan*);
  int (*launch)(const WgradCall&);
};
static bool wgrad_any(const WgradCall&) { return true; }      // the generic exact kernel: its choose() rejects what it cannot take
static const WgradEntry* wgrad_family(const WgradCall& c, int dtype) {
  static const WgradEntry f32 = {wgrad_any, osvos_wgrad_f32_plan, osvos_conv3x3_wgrad_f32},
                          small = {osvos_wgrad_small_applicable, osvos_wgrad_small_plan, osvos_conv3x3_wgrad_small_f32},
                          f32x3 = {osvos_wgrad_f32x3_applicable, osvos_wgrad_f32x3_plan, osvos_conv3x3_wgrad_f32x3},
                          bf16 = {osvos_wgrad_bf16_applicable, osvos_wgrad_bf16_plan, osvos_conv3x3_wgrad_bf16mfma};
  if (!c.x_bf16 && !c.dy_bf16) {      // fp32 tensors: by dtype
    // the wide trunk layers go through the bf16 MFMA kernel; conv1_1 (Cin 3) and side_prep (Cout 16) keep
    // their exact-fp32 skinny kernels (5 % of the weight-gradient FLOPs)
    if (dtype == OSVOS_F32_BF16MFMA && c.Cout % 64 == 0 && bf16.applicable(c)) return &bf16;
    // f32x3: the wide trunk layers and side_prep (the S16 form) on the bf16 matrix pipe with split operands; conv1_1 keeps its exact skinny kernel
    if (dtype == OSVOS_F32_X3 && f32x3.applicable(c)) return &f32x3;
    return small.applicable(c) ? &small : &f32;
  }
  // a bf16 tensor (the network's bf16-store mode, osvos_conv3x3_wgrad_bf16act): the wide layers AND side_prep (Cout 16: one 64-cout tile with 16
  // live rows, still 2x faster than the skinny kernel -- wgrad_bf16.hip) read both operands as bf16 on the bf16 MFMA kernel; conv1_1 (Cin 3) takes
  // the skinny kernel with its fp32 input and the bf16 dy.  (The skinny Cout = 16 kernel's bf16-x path is reached by no layer of the network.)
  if (bf16.applicable(c)) return &bf16;
  if (small.applicable(c)) return &small;
  osvos_set_error("net_backward: no bf16-store weight-gradient kernel for layer Cin %d/%d Cout %d", c.Cin, c.Cin_s, c.Cout);
  return nullptr;
}
int osvos_wgrad_dispatch(const WgradCall& c, int dtype) {
  const WgradEntry* e = wgrad_family(c, dtype);
  return e ? e->launch(c) : 1;
}
int osvos_wgrad_dispatch_plan(const WgradCall& c, int dtype, WgradPlan* p) {
  const WgradEntry* e = wgrad_family(c, dtype);
  return e ? e->plan(c, p) : 1;
}

// Which convolution family takes the launch (kernels.h): by dtype, by the public tile id and by what the call carries.  Edits the call it is
// handed into the one the family's launcher takes
struct ConvEntry {
  int (*launch)(const ConvCall&);
  int (*plan)(const ConvCall&, ConvPlan*);
};
static const ConvEntry& conv_family(ConvCall& c, int dtype) {
  static const ConvEntry f32 = {osvos_conv3x3_f32, osvos_conv3x3_f32_plan}, f32x3 = {osvos_conv3x3_f32x3, osvos_conv3x3_f32x3_plan},
                         bf16 = {osvos_conv3x3_bf16mfma, osvos_conv3x3_bf16mfma_plan};
  if (dtype == OSVOS_F32_BF16MFMA) return bf16;
  // f32x3: the same fp32 problem on the bf16 matrix pipe with three-way split operands (conv3x3_f32x3.hip).  Public tile ids 200 + t force its
  // tile t whatever the dtype (tests, tuning); dtype OSVOS_F32_X3 without a tile = automatic, in the f32x3 arithmetic where it applies (round 4:
  // the arithmetic is a per-call argument of the ABI, not a process-wide mode) -- also for launches cut along K (part_ws)
  if (c.tile >= 200) {
    c.tile -= 200;
    return f32x3;
  }
  if (dtype == OSVOS_F32_X3 && c.tile < 0 && osvos_conv3x3_f32x3_applicable(c.Cin, c.Cout, c.y_cs)) {
    // (with a pre-split pack the fp32 pack of the layer is not even built -- osvos_net_pack -- so it is not handed over either)
    if (!osvos_x3_presplit()) c.wpk3 = nullptr;
    if (c.wpk3 != nullptr) c.wpk = nullptr;
    return f32x3;
  }
  // exact fp32.  Launches may be cut along K (split-K, partial sums in c.part_ws) when the layer is too small to balance across 256 CUs; fused
  // epilogues, bits and stream-K exist in the f32x3 / bf16 families only (net.cpp's fuse_pool() etc. say when a caller may ask for them) and the
  // exact kernels ignore them
  return f32;
}
int osvos_conv3x3_dispatch(const ConvCall& c0, int dtype) {
  ConvCall c = c0;
  return conv_family(c, dtype).launch(c);
}

extern "C" {

int osvos_nchw_to_nhwc(const float* src, void* dst, int N, int C, int H, int W, int cpad, int dtype, void* stream) {
  NEED_F32(dtype, "nchw_to_nhwc");
  return osvos_nchw_to_nhwc_f32(src, (float*)dst, nullptr, N, C, H, W, cpad, (hipStream_t)stream);
}
int osvos_nchw_to_nhwc_bf16copy(const float* src, void* dst, void* dst_bf16, int N, int C, int H, int W, int cpad, void* stream) {
  return osvos_nchw_to_nhwc_f32(src, (float*)dst, dst_bf16, N, C, H, W, cpad, (hipStream_t)stream);
}
int osvos_nhwc_to_nchw(const void* src, float* dst, int N, int C, int H, int W, int cs, int dtype, void* stream) {
  NEED_F32(dtype, "nhwc_to_nchw");
  return osvos_nhwc_to_nchw_f32((const float*)src, dst, N, C, H, W, cs, (hipStream_t)stream);
}

// the dtype word at op level (common.h): the checks and the message of NEED_F32.  OSVOS_FLAG_BF16_W2 (d->w2) on the two forward-pack entries
// below: the two-piece pack, hi plane then lo plane
static bool op_dtype_word(int word, const char* what, DtypeWord* d) { return osvos_dtype_word(word, what, d, " (fp32 tensors only)"); }

size_t osvos_wpack_bytes(int Cout, int Cin, int dtype_) {
  DtypeWord d;
  if (!op_dtype_word(dtype_, "wpack_bytes", &d)) return 0;
  if (d.dtype == OSVOS_F32_BF16MFMA) return (size_t)9 * ((Cin + 31) / 32 * 32) * osvos_cout_pad(Cout) * 2 * (d.w2 ? 2 : 1);
  return (size_t)9 * osvos_cin_pad(Cin, d.dtype) * osvos_cout_pad(Cout) * osvos_elem(d.dtype);
}
size_t osvos_wpack_dgrad_bytes(int Cout, int Cin, int dtype) {
  if (dtype == OSVOS_F32_BF16MFMA) return (size_t)9 * ((Cout + 31) / 32 * 32) * osvos_cout_pad(Cin) * 2;
  return (size_t)9 * osvos_cin_pad(Cout, dtype) * osvos_cout_pad(Cin) * osvos_elem(dtype);
}
int osvos_pack_conv3x3_fwd(const float* w, void* wpk, int Cout, int Cin, int dtype_, void* stream) {
  DtypeWord d;
  if (!op_dtype_word(dtype_, "pack_conv3x3_fwd", &d)) return -1;
  if (d.w2) {
    OSVOS_ARG_CHECK(w && wpk && Cout > 0 && Cin > 0, "pack_conv3x3_fwd w2: bad arguments");
    PackEntry e;
    e.w = w; e.dst = wpk; e.lo_dst = reinterpret_cast<char*>(wpk) + osvos_wpack_bytes(Cout, Cin, OSVOS_F32_BF16MFMA); e.Cout = Cout; e.Cin = Cin;
    return osvos_pack_bf16_multi(&e, 1, (hipStream_t)stream);
  }
  if (d.dtype == OSVOS_F32_BF16MFMA) return osvos_pack_fwd_bf16(w, wpk, Cout, Cin, (hipStream_t)stream);
  return osvos_pack_fwd_f32(w, (float*)wpk, Cout, Cin, (hipStream_t)stream);
}
int osvos_pack_conv3x3_dgrad(const float* w, void* wpk, int Cout, int Cin, int dtype, void* stream) {
  NEED_F32(dtype, "pack_conv3x3_dgrad");
  if (dtype == OSVOS_F32_BF16MFMA) return osvos_pack_dgrad_bf16(w, wpk, Cout, Cin, (hipStream_t)stream);
  return osvos_pack_dgrad_f32(w, (float*)wpk, Cout, Cin, (hipStream_t)stream);
}

// what every op-level convolution entry passes: fp32 tensors, one pack in `wpk`, this thread's pieces (the entries below add what they have beyond that)
static ConvCall conv_call(const void* x, const void* wpk, const float* bias, const void* mask, void* y, int N, int H, int W, int Cin, int Cout, int y_cs,
                          int relu, int tile, void* stream) {
  ConvCall c;
  c.x = x; c.wpk = wpk; c.bias = bias; c.mask = mask; c.y = (float*)y;
  c.N = N; c.H = H; c.W = W; c.Cin = Cin; c.Cout = Cout; c.y_cs = y_cs; c.relu = relu; c.tile = tile;
  c.pieces = osvos_x3_pieces();
  c.stream = (hipStream_t)stream;
  return c;
}
// the same for the op-level weight-gradient entries
static WgradCall wgrad_call(const void* x, const void* dy, int bf16, void* ws, float* dw, float* db, int N, int H, int W, int Cin, int Cin_s, int Cout,
                            int Cout_s, int accumulate, void* stream) {
  WgradCall c;
  c.x = x; c.dy = dy; c.x_bf16 = c.dy_bf16 = bf16; c.ws = ws; c.dw = dw; c.db = db;
  c.N = N; c.H = H; c.W = W; c.Cin = Cin; c.Cin_s = Cin_s; c.Cout = Cout; c.Cout_s = Cout_s; c.accumulate = accumulate;
  c.pieces = osvos_x3_pieces(); c.stream = (hipStream_t)stream;
  return c;
}

int osvos_conv3x3(const void* x, const void* wpk, const float* bias, const void* mask, void* y,
                  int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int dtype, int tile, void* stream) {
  NEED_F32(dtype, "conv3x3");
  return osvos_conv3x3_dispatch(conv_call(x, wpk, bias, mask, y, N, H, W, Cin, Cout, y_cs, relu, tile, stream), dtype);
}

// host only: what osvos_conv3x3_dispatch decides for a call of this shape that carries what `flags` says (launches nothing, reads no tensor)
int osvos_conv3x3_plan(int N, int H, int W, int Cin, int Cout, int y_cs, int dtype_, int flags, int tile, int ksplit, int sk_grid, int* out) {
  OSVOS_ARG_CHECK(out != nullptr, "conv3x3_plan: null result array");
  DtypeWord d;
  if (!op_dtype_word(dtype_, "conv3x3_plan", &d)) return -1;
  const int dtype = d.dtype;
  static char here[8];      // any non-null address stands for a tensor the call carries: no launcher's choose() reads through one
  void* const some = here;
  ConvCall c;
  c.N = N; c.H = H; c.W = W; c.Cin = Cin; c.Cout = Cout; c.y_cs = y_cs; c.tile = tile; c.ksplit = ksplit; c.sk_grid = sk_grid;
  c.x = some; c.x_bf16 = (flags & OSVOS_PLAN_X_BF16) != 0;
  c.wpk = some;
  if (flags & OSVOS_PLAN_WPK3) c.wpk3 = some;
  if (d.w2) { c.w_pieces = 2; c.w_lo = osvos_wpack_bytes(Cout, Cin, OSVOS_F32_BF16MFMA); }
  c.pieces = d.pieces;
  c.relu = (flags & OSVOS_PLAN_RELU) != 0;
  if (flags & OSVOS_PLAN_Y_F32) c.y = reinterpret_cast<float*>(some);
  if (flags & OSVOS_PLAN_Y_BF16) c.y_bf16 = some;
  if (flags & OSVOS_PLAN_MASK) c.mask = some;
  c.mask_bf16 = (flags & OSVOS_PLAN_MASK) && c.x_bf16;
  if (flags & OSVOS_PLAN_MASK_BITS) c.mask_bits = reinterpret_cast<const unsigned*>(some);
  if (flags & OSVOS_PLAN_Y_BITS) c.y_bits = reinterpret_cast<unsigned*>(some);
  if (flags & OSVOS_PLAN_POOL) { c.pooled = reinterpret_cast<float*>(some); c.pooled_bf16 = some; }
  if (flags & OSVOS_PLAN_POOL_CODE) c.pool_code = some;
  if (flags & OSVOS_PLAN_PART_WS) c.part_ws = some;
  if (flags & OSVOS_PLAN_SK_WS) c.sk_ws = some;
  ConvPlan p;
  if (conv_family(c, dtype).plan(c, &p)) return -1;
  const int v[OSVOS_CONV_PLAN_INTS] = {p.family, p.tile, p.map, p.ksplit, p.ksplit > 1, p.sk_grid, p.sk_order, p.presplit, p.pipe, p.pool_after};
  for (int k = 0; k < OSVOS_CONV_PLAN_INTS; ++k) out[k] = v[k];
  return 0;
}

int osvos_conv3x3_f32x3_tiles(void) { return osvos_conv3x3_f32x3_num_tiles(); }
size_t osvos_wpack_x3_bytes_abi(int Cout, int Cin, int dgrad) { return dgrad ? osvos_wpack_x3_bytes(Cin, Cout) : osvos_wpack_x3_bytes(Cout, Cin); }
int osvos_pack_conv3x3_x3(const float* w, void* wpk3, int Cout, int Cin, int dgrad, void* stream) {
  return osvos_pack_x3(w, wpk3, Cout, Cin, dgrad, osvos_x3_pieces() == 22, (hipStream_t)stream);
}
int osvos_conv3x3_x3(const void* x, const void* wpk3, const float* bias, const void* mask, void* y,
                     int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int tile, void* stream) {
  OSVOS_ARG_CHECK(wpk3 != nullptr, "conv3x3_x3: null pack");
  ConvCall c = conv_call(x, nullptr, bias, mask, y, N, H, W, Cin, Cout, y_cs, relu, tile >= 200 ? tile - 200 : tile, stream);
  c.wpk3 = wpk3;
  return osvos_conv3x3_f32x3(c);
}

// stream-K form of osvos_conv3x3_x3 (conv3x3_f32x3.hip): sk_ws of osvos_conv3x3_x3_streamk_ws_bytes() with its first
// osvos_conv3x3_x3_streamk_ticket_bytes() bytes ZERO before the first use; grid 0 = automatic decision, > 0 = forced with that many workgroups
size_t osvos_conv3x3_x3_streamk_ws_bytes(void) { return osvos_conv3x3_f32x3_streamk_ws_bytes(); }
size_t osvos_conv3x3_x3_streamk_ticket_bytes(void) { return osvos_conv3x3_f32x3_streamk_ticket_bytes(); }
int osvos_conv3x3_x3_streamk(const void* x, const void* wpk3, const float* bias, const void* mask, void* y, void* pooled, int N, int H, int W, int Cin,
                             int Cout, int y_cs, int relu, int tile, int grid, void* sk_ws, void* stream) {
  OSVOS_ARG_CHECK(wpk3 != nullptr && sk_ws != nullptr && grid >= 0, "conv3x3_x3_streamk: null pack / workspace");
  ConvCall c = conv_call(x, nullptr, bias, mask, y, N, H, W, Cin, Cout, y_cs, relu, tile >= 200 ? tile - 200 : tile, stream);
  c.wpk3 = wpk3; c.ksplit = 1; c.sk_ws = sk_ws; c.sk_grid = grid; c.pooled = reinterpret_cast<float*>(pooled);
  return osvos_conv3x3_f32x3(c);
}

// bf16-MFMA convolution with explicit operand / result formats: x fp32 (x_is_bf16 = 0) or bf16 NHWC; y fp32 and,
// when y_bf16 != NULL, a bf16 copy of y with the same channel stride (the operand of the next convolution)
int osvos_conv3x3_bf16io(const void* x, int x_is_bf16, const void* wpk, const float* bias, const void* mask, int mask_is_bf16, float* y,
                         void* y_bf16, int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int tile, void* stream) {
  ConvCall c = conv_call(x, wpk, bias, mask, y, N, H, W, Cin, Cout, y_cs, relu, tile, stream);
  c.x_bf16 = x_is_bf16 ? 1 : 0; c.mask_bf16 = mask_is_bf16; c.y_bf16 = y_bf16;
  return osvos_conv3x3_bf16mfma(c);
}
// weight gradient of the wide layers (Cin_s, Cout multiples of 64) from bf16 x AND dy; dw/db fp32 as osvos_conv3x3_wgrad
int osvos_conv3x3_wgrad_bf16act(const void* x_bf16, const void* dy_bf16, void* ws, float* dw, float* db, int N, int H, int W, int Cin, int Cin_s,
                                int Cout, int Cout_s, int accumulate, void* stream) {
  return osvos_wgrad_dispatch(wgrad_call(x_bf16, dy_bf16, 1, ws, dw, db, N, H, W, Cin, Cin_s, Cout, Cout_s, accumulate, stream), OSVOS_F32_BF16MFMA);
}
// conv1_1's weight gradient of the bf16-store mode at op level: fp32 NHWC8 input, bf16 dy (the skinny launcher picks the kernel)
int osvos_conv3x3_wgrad_c3_bf16dy(const float* x_nhwc8, const void* dy_bf16, void* ws, float* dw, float* db, int N, int H, int W, int Cout,
                                  int Cout_s, int accumulate, void* stream) {
  OSVOS_ARG_CHECK(x_nhwc8 && dy_bf16 && ws && dw, "wgrad_c3_bf16dy: null pointer");
  OSVOS_ARG_CHECK(N > 0 && H > 0 && W > 0, "wgrad_c3_bf16dy: bad shape");
  OSVOS_ARG_CHECK(Cout > 0 && Cout <= 64 && Cout % 4 == 0 && Cout_s % 4 == 0 && Cout <= Cout_s,
                  "wgrad_c3_bf16dy: Cout <= 64, Cout and its stride multiples of 4 (Cout %d/%d)", Cout, Cout_s);
  OSVOS_ARG_CHECK((long)H * W * Cout_s < (1L << 29), "wgrad_c3_bf16dy: image too large for 31-bit byte offsets");
  WgradCall c = wgrad_call(x_nhwc8, dy_bf16, 0, ws, dw, db, N, H, W, 3, 8, Cout, Cout_s, accumulate, stream);
  c.dy_bf16 = 1;
  return osvos_wgrad_dispatch(c, OSVOS_F32_BF16MFMA);
}
int osvos_maxpool2x2_bf16act(const void* x_bf16, void* y_bf16, int N, int H, int W, int C, void* stream) {
  return osvos_maxpool2x2_bf16(x_bf16, y_bf16, N, H, W, C, (hipStream_t)stream);
}
int osvos_maxpool2x2_bwd_bf16act(const void* x_bf16, const void* dy_bf16, const void* dside_bf16, void* dx_bf16, int N, int H, int W, int C,
                                 void* stream) {
  return osvos_maxpool2x2_bwd_bf16(x_bf16, dy_bf16, dside_bf16, dx_bf16, N, H, W, C, (hipStream_t)stream);
}
int osvos_maxpool2x2_bf16act_code(const void* x_bf16, void* y_bf16, void* code, int N, int H, int W, int C, void* stream) {
  return osvos_maxpool2x2_bf16_code(x_bf16, y_bf16, code, N, H, W, C, (hipStream_t)stream);
}
int osvos_maxpool2x2_bwd_bf16act_code(const void* code, const void* dy_bf16, const void* dside_bf16, void* dx_bf16, int N, int H, int W, int C,
                                      void* stream) {
  return osvos_maxpool2x2_bwd_bf16_code(code, dy_bf16, dside_bf16, dx_bf16, N, H, W, C, (hipStream_t)stream);
}
int osvos_conv3x3_bf16act_fused(const void* x_bf16, const void* wpk, const float* bias, const void* mask_bits, void* y_bf16, void* y_bits,
                                void* pooled_bf16, void* pool_code, int N, int H, int W, int Cin, int Cout, int relu, int tile, void* stream) {
  OSVOS_ARG_CHECK(y_bf16 != nullptr, "conv3x3_bf16act_fused: y_bf16 is required");
  ConvCall c = conv_call(x_bf16, wpk, bias, nullptr, nullptr, N, H, W, Cin, Cout, Cout, relu, tile, stream);
  c.x_bf16 = 1; c.mask_bits = reinterpret_cast<const unsigned*>(mask_bits);
  c.y_bf16 = y_bf16; c.y_bits = reinterpret_cast<unsigned*>(y_bits); c.pooled_bf16 = pooled_bf16; c.pool_code = pool_code;
  return osvos_conv3x3_bf16mfma(c);
}
int osvos_conv3x3_bf16io_tiles(int* tiles, int max) { return osvos_conv3x3_bf16mfma_xb_tiles(tiles, max); }
int osvos_conv3x3_bf16w2_fused(const void* x, const void* wpk_w2, const float* bias, const void* mask_bits, void* y_bf16, void* y_bits,
                               void* pooled_bf16, void* pool_code, int N, int H, int W, int Cin, int Cout, int relu, int x_is_f32, float* y_f32, int tile,
                               void* stream) {
  OSVOS_ARG_CHECK(y_bf16 != nullptr || (y_f32 != nullptr && pooled_bf16 == nullptr), "conv3x3_bf16w2_fused: y_bf16 (or y_f32 without a pool) is required");
  OSVOS_ARG_CHECK(mask_bits == nullptr, "conv3x3_bf16w2_fused: forward only (the data gradients of 'bf16w2' are single-piece)");
  OSVOS_ARG_CHECK(Cout > 0 && Cin > 0, "conv3x3_bf16w2_fused: bad shape");
  ConvCall c = conv_call(x, wpk_w2, bias, nullptr, y_f32, N, H, W, Cin, Cout, Cout, relu, tile, stream);
  c.x_bf16 = x_is_f32 ? 0 : 1; c.w_pieces = 2; c.w_lo = osvos_wpack_bytes(Cout, Cin, OSVOS_F32_BF16MFMA);
  c.y_bf16 = y_bf16; c.y_bits = reinterpret_cast<unsigned*>(y_bits); c.pooled_bf16 = pooled_bf16; c.pool_code = pool_code;
  return osvos_conv3x3_bf16mfma(c);
}
int osvos_conv3x3_bf16w2_tiles(int* tiles, int max) { return osvos_conv3x3_bf16w2_tiles_impl(tiles, max); }

size_t osvos_conv3x3_splitk_ws_bytes(int N, int H, int W, int Cout, int dtype) {
  (void)dtype;
  return osvos_conv3x3_splitk_ws_bytes_f32(N, H, W, Cout);
}
int osvos_conv3x3_splitk(const void* x, const void* wpk, const float* bias, const void* mask, void* y,
                         int N, int H, int W, int Cin, int Cout, int y_cs, int relu, int dtype, int tile, int ksplit,
                         void* part_ws, void* stream) {
  OSVOS_ARG_CHECK(dtype == OSVOS_F32 || dtype == OSVOS_F32_X3, "conv3x3_splitk: fp32 only (dtype %d)", dtype);
  OSVOS_ARG_CHECK(part_ws != nullptr && ksplit >= 0 && ksplit <= 8, "conv3x3_splitk: bad ksplit / workspace");
  ConvCall c = conv_call(x, wpk, bias, mask, y, N, H, W, Cin, Cout, y_cs, relu, tile, stream);
  c.ksplit = ksplit; c.part_ws = part_ws;
  return osvos_conv3x3_dispatch(c, dtype);
}

// the most any family that osvos_wgrad_dispatch can hand this shape to under `dtype` asks for (each from the plans its launches make)
size_t osvos_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int dtype) {
  const size_t f = osvos_wgrad_ws_bytes_f32(N, H, W, Cin, Cout);
  const size_t b = dtype == OSVOS_F32_BF16MFMA ? osvos_wgrad_bf16_ws_bytes(N, H, W, Cin, Cout) : osvos_wgrad_f32x3_ws_bytes(N, H, W, Cin, Cout);
  return f > b ? f : b;
}
int osvos_conv3x3_wgrad(const void* x, const void* dy, void* ws, float* dw, float* db,
                        int N, int H, int W, int Cin, int Cin_s, int Cout, int Cout_s,
                        int accumulate, int dtype, void* stream) {
  NEED_F32(dtype, "conv3x3_wgrad");
  return osvos_wgrad_dispatch(wgrad_call(x, dy, 0, ws, dw, db, N, H, W, Cin, Cin_s, Cout, Cout_s, accumulate, stream), dtype);
}

// host only: what osvos_wgrad_dispatch and the family's choose() decide for a call of this shape that carries what `flags` says
static char g_some[8];      // any non-null address stands for a tensor the call carries: no choose() reads through one
static WgradCall wgrad_plan_call(int N, int H, int W, int Cin, int Cin_s, int Cout, int Cout_s, int pieces, int flags) {
  WgradCall c;
  c.x = c.dy = c.ws = g_some; c.dw = reinterpret_cast<float*>(g_some);
  if (!(flags & OSVOS_WGRAD_PLAN_NO_BIAS)) c.db = c.dw;
  c.x_bf16 = (flags & OSVOS_WGRAD_PLAN_X_BF16) != 0; c.dy_bf16 = (flags & OSVOS_WGRAD_PLAN_DY_BF16) != 0;
  c.N = N; c.H = H; c.W = W; c.Cin = Cin; c.Cin_s = Cin_s; c.Cout = Cout; c.Cout_s = Cout_s;
  c.pieces = pieces;
  return c;
}
int osvos_wgrad_plan(int N, int H, int W, int Cin, int Cin_s, int Cout, int Cout_s, int dtype_, int flags, int* out) {
  OSVOS_ARG_CHECK(out != nullptr, "wgrad_plan: null result array");
  OSVOS_ARG_CHECK(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "wgrad_plan: bad shape");
  DtypeWord d;
  if (!op_dtype_word(dtype_, "wgrad_plan", &d)) return -1;
  WgradPlan p;
  if (osvos_wgrad_dispatch_plan(wgrad_plan_call(N, H, W, Cin, Cin_s, Cout, Cout_s, d.pieces, flags), d.dtype, &p)) return -1;
  auto sat = [](size_t v) { return v > 0x7fffffffu ? 0x7fffffff : (int)v; };
  const int v[OSVOS_WGRAD_PLAN_INTS] = {p.family, p.kernel, p.pw, p.ph, p.npx, p.npy, p.npatches, p.per_split, p.nsplit, p.nco_t, p.nci_t,
                                        (int)p.blocks, p.map, p.reduce, sat(p.slab_floats), sat(p.bslab_floats)};
  for (int k = 0; k < OSVOS_WGRAD_PLAN_INTS; ++k) out[k] = v[k];
  return 0;
}
// the two older queries: fields of the same plans
int osvos_wgrad_c3_plan(int N, int H, int W, int bf16_dy, int* out) {
  OSVOS_ARG_CHECK(N > 0 && H > 0 && W > 0 && out != nullptr, "wgrad_c3_plan: bad arguments");
  WgradPlan p;
  osvos_wgrad_c3_split(N, H, W, bf16_dy, &p);
  out[0] = p.npx; out[1] = p.npy; out[2] = p.npatches; out[3] = p.per_split; out[4] = p.nsplit;
  return 0;
}
int osvos_wgrad_wide_plan(int N, int H, int W, int Cin_s, int Cout, int dtype, int bf16_tensors, int* out) {
  OSVOS_ARG_CHECK(N > 0 && H > 0 && W > 0 && Cin_s > 0 && Cout > 0 && out != nullptr, "wgrad_wide_plan: bad arguments");
  OSVOS_ARG_CHECK(!bf16_tensors || dtype == OSVOS_F32_BF16MFMA, "wgrad_wide_plan: bf16 tensors go with dtype OSVOS_F32_BF16MFMA (got %d)", dtype);
  const WgradCall c = wgrad_plan_call(N, H, W, Cin_s, Cin_s, Cout, Cout, 3, bf16_tensors ? OSVOS_WGRAD_PLAN_X_BF16 | OSVOS_WGRAD_PLAN_DY_BF16 : 0);
  WgradPlan p;
  if (osvos_wgrad_dispatch_plan(c, dtype, &p)) return -1;
  OSVOS_ARG_CHECK(p.family == WGRAD_F32X3 || p.family == WGRAD_BF16, "wgrad_wide_plan: no wide weight-gradient kernel for dtype %d Cin %d Cout %d", dtype, Cin_s, Cout);
  const int v[12] = {p.pw, p.ph, p.npx, p.npy, p.npatches, p.per_split, p.nsplit, p.nco_t, p.nci_t, (int)p.blocks, p.map,
                     p.family == WGRAD_BF16 && p.nco_t * 64 < Cout};      // (128-cout tiles)
  for (int k = 0; k < 12; ++k) out[k] = v[k];
  return 0;
}

int osvos_maxpool2x2(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream) {
  NEED_F32(dtype, "maxpool2x2");
  return osvos_maxpool2x2_f32((const float*)x, (float*)y, nullptr, N, H, W, C, (hipStream_t)stream);
}
int osvos_maxpool2x2_bf16copy(const float* x, float* y, void* y_bf16, int N, int H, int W, int C, void* stream) {
  return osvos_maxpool2x2_f32(x, y, y_bf16, N, H, W, C, (hipStream_t)stream);
}
int osvos_maxpool2x2_bwd(const void* x, const void* dy, const void* dside, void* dx,
                         int N, int H, int W, int C, int dtype, void* stream) {
  NEED_F32(dtype, "maxpool2x2_bwd");
  return osvos_maxpool2x2_bwd_f32((const float*)x, (const float*)dy, (const float*)dside, (float*)dx, nullptr, N, H, W, C, (hipStream_t)stream);
}
int osvos_maxpool2x2_bwd_bf16copy(const float* x, const float* dy, const float* dside, float* dx, void* dx_bf16,
                                  int N, int H, int W, int C, void* stream) {
  return osvos_maxpool2x2_bwd_f32(x, dy, dside, dx, dx_bf16, N, H, W, C, (hipStream_t)stream);
}

int osvos_conv3x3_dgrad_c3(const float* dy, const float* wpk_dgrad, float* dx_nchw, int N, int H, int W, int Cout, void* stream) {
  return osvos_conv3x3_dgrad_c3_f32(dy, wpk_dgrad, dx_nchw, N, H, W, Cout, (hipStream_t)stream);
}
int osvos_conv3x3_dgrad_c3_bf16mma(const void* dy_bf16, const void* wpk_bf16_dgrad, float* dx_nchw, int N, int H, int W, int Cout, void* stream) {
  return osvos_conv3x3_dgrad_c3_bf16mfma(dy_bf16, wpk_bf16_dgrad, dx_nchw, N, H, W, Cout, (hipStream_t)stream);
}


int osvos_head_lowres(const void* prep, const float* wd, const float* bd, const float* wf,
                      float* score, float* fpart, int N, int h, int w, int dtype, void* stream) {
  NEED_F32(dtype, "head_lowres");
  return osvos_head_lowres_f32((const float*)prep, wd, bd, wf, score, fpart, N, h, w, (hipStream_t)stream);
}
int osvos_head_bwd(const void* prep, const float* dside, const float* dfused,
                   const float* f1, const float* f16, const float* wd, const float* wf,
                   void* dprep, double* acc, int N, int H, int W, int h, int w, int scale_idx,
                   int dtype, void* stream) {
  NEED_F32(dtype, "head_bwd");
  return osvos_head_bwd_f32((const float*)prep, dside, dfused, f1, f16, wd, wf, (float*)dprep, nullptr, acc, N, H, W, h, w,
                            scale_idx, (hipStream_t)stream);
}

}  // extern "C"
