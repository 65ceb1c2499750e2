// Object-centred zoom around the network: a box from the previous mask, the box's window resampled onto a fixed canvas, the canvas's logit
// map pasted back into the frame -- the box never leaves device memory, the network keeps one input shape.
//
//   osvos_roi_box    mask bytes [N][H][W] (non-zero = object) -> box int32 [N][4] = (x0, y0, bw, bh): the tight box of the set pixels, grown
//                    by a margin, to a minimum size and to the canvas's aspect, then shifted and capped into the frame (the rule, in signed
//                    64-bit integers: roi_rule below and include/osvos_hip.h).  An empty mask gives the full frame (0, 0, W, H).
//   osvos_roi_view   decoded uint8 BGR frames [N][H][W][3] -> one network input [N][3][Hc][Wc] fp32: the bilinear resample of the box's window
//                    minus mean3[c] -- osvos_tta_view of the cropped frame.
//   osvos_roi_paste  logit maps [N][Hc][Wc] -> out [N][H][W]: the map resampled onto the box's bw x bh pixels, `outside` everywhere else.
//
// Sampling is tta_tap's integer rule (tta_tap.h, the one place it is written), unchanged: n_src = bw (bh), n_dst = Wc (Hc) in the view, the
// other way round in the paste; source indices are offset by x0 (y0) and clamp to the BOX, not to the frame.  A tap of weight zero is
// selected away, the x pass comes first, no fused multiply-adds: with the full-frame box on a canvas of the frame's size the view is
// osvos_tta_view's same-size output bit for bit and the paste hands the map through bit for bit, inf and NaN included.
//
// Box: two launches and NO state.  roi_scan_kernel: the rows of a frame are dealt to at most OSVOS_ROI_BOX_PARTS workgroups in contiguous
// runs; a run of rows is one contiguous byte range, read as 16-byte words from its first 16-byte boundary on, with a scalar head before it
// and a scalar tail after it (so neither W % 16 nor the mask's own alignment matters); a word that holds no set byte -- nearly all of them
// -- costs one load and one compare.  Each workgroup reduces its extent through wave shuffles and LDS and STORES it to its own slot of ws;
// roi_rule_kernel (one wave per frame) reduces the slots and applies the rule.  Every slot that is read was written by the same call: ws
// needs no initial contents and keeps nothing a later call depends on -- no counters, no atomics, nothing a failed call could poison.
//
// View and paste: tta.hip's layout -- 64 lanes along x times 4 rows per workgroup, four pixels per thread, one 16-byte store per thread where
// the row length is a multiple of 4 and the output is 16-byte aligned, otherwise pixels 64 apart and 4-byte stores; both forms write the
// same bits.  The box is read from device memory (four wave-uniform loads per workgroup) and clamped into the frame before it is used, so a
// box the caller filled with garbage reads and writes inside the arrays all the same.
#include "common.h"
#include "tta_tap.h"

namespace {

constexpr int PARTS = OSVOS_ROI_BOX_PARTS;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct Extent {
  int xa, xb, ya, yb;      // min / max column and row of the set pixels; xb < 0: none
};

__device__ __forceinline__ void extent_add(Extent& e, int x, int y) {
  e.xa = min(e.xa, x); e.xb = max(e.xb, x); e.ya = min(e.ya, y); e.yb = max(e.yb, y);
}

__device__ __forceinline__ Extent extent_wave(Extent e) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    e.xa = min(e.xa, __shfl_xor(e.xa, o, 64)); e.xb = max(e.xb, __shfl_xor(e.xb, o, 64));
    e.ya = min(e.ya, __shfl_xor(e.ya, o, 64)); e.yb = max(e.yb, __shfl_xor(e.yb, o, 64));
  }
  return e;
}

// grid (parts, N), block 256; ws slot [n][part] = the extent of rows [part * rows, (part + 1) * rows) of frame n
__global__ __launch_bounds__(256) void roi_scan_kernel(const unsigned char* __restrict__ mask, int4* __restrict__ ws, int H, int W, int rows) {
  const int n = blockIdx.y, part = blockIdx.x, t = threadIdx.x;
  const unsigned char* __restrict__ m = mask + (size_t)n * H * W;
  const int lo = part * rows * W, hi = min((part + 1) * rows, H) * W;          // pixel indices of this run (H W <= 2^28)
  Extent e = {INT_MAX, -1, INT_MAX, -1};
  const int head = min(hi, lo + (int)((16 - (uintptr_t)(m + lo) % 16) % 16));    // first 16-byte boundary at or after lo
  const int words = (hi - head) / 16, tail = head + words * 16;
  for (int i = lo + t; i < head; i += 256)
    if (m[i]) extent_add(e, i % W, i / W);
  for (int i = tail + t; i < hi; i += 256)
    if (m[i]) extent_add(e, i % W, i / W);
  const u32x4* __restrict__ wide = reinterpret_cast<const u32x4*>(m + head);
  for (int k = t; k < words; k += 256) {
    const u32x4 v = wide[k];
    if ((v[0] | v[1] | v[2] | v[3]) == 0u) continue;
    const int i = head + k * 16;
    int y = i / W, x = i - y * W;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      if ((v[b / 4] >> (8 * (b % 4))) & 0xffu) extent_add(e, x, y);
      if (++x == W) { x = 0; ++y; }
    }
  }
  e = extent_wave(e);
  __shared__ int4 sh[4];
  if (t % 64 == 0) sh[t / 64] = make_int4(e.xa, e.xb, e.ya, e.yb);
  __syncthreads();
  if (t == 0) {
    int4 r = sh[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) { r.x = min(r.x, sh[w].x); r.y = max(r.y, sh[w].y); r.z = min(r.z, sh[w].z); r.w = max(r.w, sh[w].w); }
    ws[n * PARTS + part] = r;
  }
}

struct BoxRule {
  int H, W, Hc, Wc, margin_pct, margin_px, min_w, min_h;
};

// the rule of include/osvos_hip.h on a non-empty extent; every product fits int64 (sides <= 2^14, margins < 2^31)
__device__ int4 roi_rule(const Extent e, const BoxRule r) {
  typedef long long i64;
  i64 bw = e.xb - e.xa + 1, bh = e.yb - e.ya + 1;
  const i64 pad = ((bw > bh ? bw : bh) * r.margin_pct + 99) / 100 + r.margin_px;
  i64 x0 = e.xa - pad, y0 = e.ya - pad;
  bw += 2 * pad; bh += 2 * pad;
  if (bw < r.min_w) { x0 -= (r.min_w - bw) / 2; bw = r.min_w; }
  if (bh < r.min_h) { y0 -= (r.min_h - bh) / 2; bh = r.min_h; }
  if (bw * r.Hc < bh * r.Wc) {
    const i64 nw = (bh * r.Wc + r.Hc - 1) / r.Hc;
    x0 -= (nw - bw) / 2; bw = nw;
  } else if (bh * r.Wc < bw * r.Hc) {
    const i64 nh = (bw * r.Hc + r.Wc - 1) / r.Wc;
    y0 -= (nh - bh) / 2; bh = nh;
  }
  bw = bw < r.W ? bw : r.W;
  bh = bh < r.H ? bh : r.H;
  x0 = x0 < 0 ? 0 : (x0 > r.W - bw ? r.W - bw : x0);
  y0 = y0 < 0 ? 0 : (y0 > r.H - bh ? r.H - bh : y0);
  return make_int4((int)x0, (int)y0, (int)bw, (int)bh);
}

// grid N, block 64
__global__ __launch_bounds__(64) void roi_rule_kernel(const int4* __restrict__ ws, int* __restrict__ box, int parts, BoxRule r) {
  const int n = blockIdx.x, t = threadIdx.x;
  Extent e = {INT_MAX, -1, INT_MAX, -1};
  for (int p = t; p < parts; p += 64) {
    const int4 s = ws[n * PARTS + p];
    e.xa = min(e.xa, s.x); e.xb = max(e.xb, s.y); e.ya = min(e.ya, s.z); e.yb = max(e.yb, s.w);
  }
  e = extent_wave(e);
  if (t == 0) {
    const int4 b = e.xb < 0 ? make_int4(0, 0, r.W, r.H) : roi_rule(e, r);
    box[4 * n + 0] = b.x; box[4 * n + 1] = b.y; box[4 * n + 2] = b.z; box[4 * n + 3] = b.w;
  }
}

// the box of frame n, forced into the frame: (x0, y0, bw, bh) with 1 <= bw <= W, 0 <= x0 <= W - bw (osvos_roi_box's boxes pass unchanged)
__device__ __forceinline__ int4 roi_load_box(const int* __restrict__ box, int n, int H, int W) {
  int4 b = make_int4(box[4 * n + 0], box[4 * n + 1], box[4 * n + 2], box[4 * n + 3]);
  b.z = min(max(b.z, 1), W); b.w = min(max(b.w, 1), H);
  b.x = min(max(b.x, 0), W - b.z); b.y = min(max(b.y, 0), H - b.w);
  return b;
}

struct RoiViewArgs {
  const unsigned char* bgr;      // [N][H][W][3]
  const int* box;                // [N][4]
  float* out;                    // [N][3][Hc][Wc]
  float mean[3];
  int H, W, Hc, Wc;
};

// grid (ceil(Wc / 256), ceil(Hc / 4), N), block (64, 4)
template <bool VEC>
__global__ __launch_bounds__(256) void roi_view_kernel(RoiViewArgs a) {
#pragma clang fp contract(off)
  const int y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (y >= a.Hc) return;
  const int4 b = roi_load_box(a.box, n, a.H, a.W);
  const Tap ty = tta_tap(y, a.Hc, b.w);
  const unsigned char* __restrict__ r0 = a.bgr + (((size_t)n * a.H + b.y + ty.i0) * a.W + b.x) * 3;
  const unsigned char* __restrict__ r1 = a.bgr + (((size_t)n * a.H + b.y + ty.i1) * a.W + b.x) * 3;
  float v[3][4] = {};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = tta_column<VEC>(j);
    if (x >= a.Wc) continue;
    const Tap tx = tta_tap(x, a.Wc, b.z);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][j] = tta_lerp((float)r0[tx.i0 * 3 + c], (float)r0[tx.i1 * 3 + c], tx.f);
    if (ty.f != 0.f) {                                                                     // (wave-uniform)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][j] = tta_lerp(v[c][j], tta_lerp((float)r1[tx.i0 * 3 + c], (float)r1[tx.i1 * 3 + c], tx.f), ty.f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][j] = v[c][j] - a.mean[c];
  }
  const size_t plane = (size_t)a.Hc * a.Wc;
  float* __restrict__ o = a.out + (size_t)n * 3 * plane + (size_t)y * a.Wc;
#pragma unroll
  for (int c = 0; c < 3; ++c) tta_store4<VEC>(o + c * plane, a.Wc, v[c]);
}

struct RoiPasteArgs {
  const float* logits;           // [N][Hc][Wc]
  const int* box;                // [N][4]
  float* out;                    // [N][H][W]
  float outside;
  int H, W, Hc, Wc;
};

// grid (ceil(W / 256), ceil(H / 4), N), block (64, 4)
template <bool VEC>
__global__ __launch_bounds__(256) void roi_paste_kernel(RoiPasteArgs a) {
#pragma clang fp contract(off)
  const int y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (y >= a.H) return;
  const int4 b = roi_load_box(a.box, n, a.H, a.W);
  float v[4] = {a.outside, a.outside, a.outside, a.outside};
  if (y >= b.y && y < b.y + b.w) {                                                         // (wave-uniform: a wave is one row)
    const Tap ty = tta_tap(y - b.y, b.w, a.Hc);
    const float* __restrict__ r0 = a.logits + ((size_t)n * a.Hc + ty.i0) * a.Wc;
    const float* __restrict__ r1 = a.logits + ((size_t)n * a.Hc + ty.i1) * a.Wc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = tta_column<VEC>(j);
      if (x < b.x || x >= b.x + b.z) continue;
      const Tap tx = tta_tap(x - b.x, b.z, a.Wc);
      float s = tta_lerp(r0[tx.i0], r0[tx.i1], tx.f);
      if (ty.f != 0.f) s = tta_lerp(s, tta_lerp(r1[tx.i0], r1[tx.i1], tx.f), ty.f);        // (wave-uniform)
      v[j] = s;
    }
  }
  tta_store4<VEC>(a.out + ((size_t)n * a.H + y) * a.W, a.W, v);
}

bool size_ok(int v) { return v >= 1 && v <= 16384; }

}  // namespace

// mask: device bytes [N][H][W]; box: device int32 [N][4]; ws: device, OSVOS_ROI_BOX_WS_BYTES(N) bytes, 16-byte aligned, contents irrelevant
extern "C" int osvos_roi_box(const unsigned char* mask, int* box, int N, int H, int W, int Hc, int Wc, int margin_pct, int margin_px, int min_w,
                             int min_h, void* ws, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(mask && box && ws, "roi_box: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "roi_box: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W) && size_ok(Hc) && size_ok(Wc), "roi_box: bad size H %d W %d, canvas Hc %d Wc %d (1..16384 per side)", H, W,
                  Hc, Wc);
  OSVOS_ARG_CHECK(margin_pct >= 0 && margin_px >= 0, "roi_box: negative margin (%d percent, %d pixels)", margin_pct, margin_px);
  OSVOS_ARG_CHECK(min_w >= 0 && min_w <= W && min_h >= 0 && min_h <= H, "roi_box: minimum size %d x %d outside the %d x %d frame", min_w, min_h, W, H);
  OSVOS_ARG_CHECK((uintptr_t)box % 4 == 0 && (uintptr_t)ws % 16 == 0, "roi_box: box must be 4-byte and ws 16-byte aligned");
  const int parts = H < PARTS ? H : PARTS, rows = (H + parts - 1) / parts;
  const int used = (H + rows - 1) / rows;                                                  // runs that hold a row: exactly the slots written and read
  hipLaunchKernelGGL(roi_scan_kernel, dim3((unsigned)used, (unsigned)N), dim3(256), 0, stream, mask, (int4*)ws, H, W, rows);
  OSVOS_LAUNCH_CHECK();
  BoxRule r = {H, W, Hc, Wc, margin_pct, margin_px, min_w, min_h};
  hipLaunchKernelGGL(roi_rule_kernel, dim3((unsigned)N), dim3(64), 0, stream, (const int4*)ws, box, used, r);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

// bgr: device uint8 [N][H][W][3]; box: device int32 [N][4]; mean3: HOST pointer to 3 floats; out: device fp32 [N][3][Hc][Wc]
extern "C" int osvos_roi_view(const unsigned char* bgr, const int* box, const float* mean3, float* out, int N, int H, int W, int Hc, int Wc,
                              void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(bgr && box && mean3 && out, "roi_view: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "roi_view: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W) && size_ok(Hc) && size_ok(Wc), "roi_view: bad size H %d W %d -> Hc %d Wc %d (1..16384 per side)", H, W, Hc,
                  Wc);
  OSVOS_ARG_CHECK((uintptr_t)out % 4 == 0 && (uintptr_t)box % 4 == 0, "roi_view: out and box must be 4-byte aligned");
  RoiViewArgs a;
  a.bgr = bgr; a.box = box; a.out = out; a.H = H; a.W = W; a.Hc = Hc; a.Wc = Wc;
  for (int c = 0; c < 3; ++c) a.mean[c] = mean3[c];
  const dim3 grid((unsigned)((Wc + 255) / 256), (unsigned)((Hc + 3) / 4), (unsigned)N), block(64, 4);
  if (Wc % 4 == 0 && (uintptr_t)out % 16 == 0)
    hipLaunchKernelGGL(roi_view_kernel<true>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(roi_view_kernel<false>, grid, block, 0, stream, a);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

// logits: device fp32 [N][Hc][Wc]; box: device int32 [N][4]; out: device fp32 [N][H][W], not logits
extern "C" int osvos_roi_paste(const float* logits, const int* box, float* out, int N, int Hc, int Wc, int H, int W, float outside, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(logits && box && out, "roi_paste: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "roi_paste: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W) && size_ok(Hc) && size_ok(Wc), "roi_paste: bad size Hc %d Wc %d -> H %d W %d (1..16384 per side)", Hc, Wc, H,
                  W);
  OSVOS_ARG_CHECK((uintptr_t)out % 4 == 0 && (uintptr_t)logits % 4 == 0 && (uintptr_t)box % 4 == 0, "roi_paste: logits, out and box must be 4-byte aligned");
  RoiPasteArgs a;
  a.logits = logits; a.box = box; a.out = out; a.outside = outside; a.H = H; a.W = W; a.Hc = Hc; a.Wc = Wc;
  const dim3 grid((unsigned)((W + 255) / 256), (unsigned)((H + 3) / 4), (unsigned)N), block(64, 4);
  if (W % 4 == 0 && (uintptr_t)out % 16 == 0)
    hipLaunchKernelGGL(roi_paste_kernel<true>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(roi_paste_kernel<false>, grid, block, 0, stream, a);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
