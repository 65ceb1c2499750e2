// Lucid first-frame synthesis (include/osvos_hip.h, "lucid data dreaming"): a second training sample out of the one annotated frame.
//   osvos_lucid_inpaint  once per sequence: the object's hole filled from the nearest pixel outside it, then box-smoothed.
//   osvos_lucid_compose  once per training sample: object and inpainted background moved by affines of their own, re-lit, composited.
// Integers only, so both are exact and tests compare bit for bit.
//
// Inpainting is distance.hip carried one step further, to the arg-min.  Column pass: one lane per column records for every pixel the row of
// the nearest non-hole pixel of its column (a tie between above and below goes to the smaller row).  Row pass: one workgroup per row, the row of
// column answers in LDS; a hole pixel walks outwards from its own column and keeps the minimiser of (d, qy, qx).  Within a column the key is
// monotone in |dy| (and the tie went to the smaller qy), so the column's nearest row is the column's only candidate.  The walk stops once
// dx^2 > best -- strictly: a candidate at equal distance with a smaller (qy, qx) still has to be seen.  The smoothing passes alternate between
// ws and out_bgr so that the last one writes out_bgr (as crf.hip does).  No atomics, no workgroup waits for another.
//
// Composition: one workgroup per 64 x 4 destination tile, a lane is a column, N samples in grid z; the 2 N affines and tone sets travel as
// kernel arguments.  Taps are read through the cache: staging a tile's source footprint in LDS first was timed and lost, other tile shapes
// made no difference (profiles/lucid_timing.txt).
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int kColThreads = 64;
constexpr int kRowThreads = 256;
constexpr int kNone = -1;

// grid ceil(W / kColThreads).  near[y][x] = the row of the non-hole pixel of column x nearest to y (smaller row on a tie), kNone without one
__global__ __launch_bounds__(kColThreads) void lucid_column_kernel(const unsigned char* __restrict__ hole, int* __restrict__ near, int H, int W) {
  const int x = blockIdx.x * kColThreads + threadIdx.x;
  if (x >= W) return;
  int q = kNone;                                             // nearest non-hole row at or above y
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    const size_t i = (size_t)y * W + x;
    q = hole[i] == 0 ? y : q;
    near[i] = q;
  }
  q = kNone;                                                 // ... at or below y
#pragma unroll 8
  for (int y = H - 1; y >= 0; --y) {
    const size_t i = (size_t)y * W + x;
    const int up = near[i];
    q = up == y ? y : q;
    near[i] = up < 0 ? q : (q < 0 ? up : (y - up <= q - y ? up : q));
  }
}

// grid H, dynamic LDS 4 W bytes
__global__ __launch_bounds__(kRowThreads) void lucid_fill_kernel(const unsigned char* __restrict__ bgr, const int* __restrict__ near,
                                                                 unsigned char* __restrict__ out, int H, int W) {
  extern __shared__ int row[];
  const int y = blockIdx.x;
  const size_t base = (size_t)y * W;
  for (int x = threadIdx.x; x < W; x += kRowThreads) row[x] = near[base + x];
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += kRowThreads) {
    int c = row[x];
    int qy = y, qx = x;                                      // (a frame without a non-hole pixel keeps its colours)
    if (c != y) {
      int best = INT_MAX;
      if (c >= 0) { best = (c - y) * (c - y); qy = c; }
      const int left = x, right = W - 1 - x;
      const int reach = left > right ? left : right;
      for (int dx = 1; dx <= reach; ++dx) {
        const int dd = dx * dx;
        if (dd > best) break;
        if (dx <= left) {                                    // the smaller qx first
          c = row[x - dx];
          if (c >= 0) {
            const int v = dd + (c - y) * (c - y);
            if (v < best || (v == best && (c < qy || (c == qy && x - dx < qx)))) { best = v; qy = c; qx = x - dx; }
          }
        }
        if (dx <= right) {
          c = row[x + dx];
          if (c >= 0) {
            const int v = dd + (c - y) * (c - y);
            if (v < best || (v == best && (c < qy || (c == qy && x + dx < qx)))) { best = v; qy = c; qx = x + dx; }
          }
        }
      }
    }
    const size_t s = ((size_t)qy * W + qx) * 3, d = (base + x) * 3;
    out[d] = bgr[s]; out[d + 1] = bgr[s + 1]; out[d + 2] = bgr[s + 2];
  }
}

// grid (ceil(W / 64), ceil(H / 4)), block (64, 4).  A hole pixel becomes the rounded mean of its clipped window of src; the others are copied.
__global__ __launch_bounds__(256) void lucid_smooth_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ hole,
                                                           unsigned char* __restrict__ dst, int H, int W, int radius) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const size_t o = ((size_t)y * W + x) * 3;
  if (hole[(size_t)y * W + x] == 0) {
    dst[o] = src[o]; dst[o + 1] = src[o + 1]; dst[o + 2] = src[o + 2];
    return;
  }
  const int x0 = max(x - radius, 0), x1 = min(x + radius, W - 1), y0 = max(y - radius, 0), y1 = min(y + radius, H - 1);
  int sb = 0, sg = 0, sr = 0;
  for (int yy = y0; yy <= y1; ++yy) {
    const unsigned char* p = src + ((size_t)yy * W + x0) * 3;
    for (int xx = x0; xx <= x1; ++xx, p += 3) { sb += p[0]; sg += p[1]; sr += p[2]; }
  }
  const int n = (x1 - x0 + 1) * (y1 - y0 + 1);              // at most 289: 2 * 289 * 255 + 289 fits easily
  dst[o] = (unsigned char)((2 * sb + n) / (2 * n));
  dst[o + 1] = (unsigned char)((2 * sg + n) / (2 * n));
  dst[o + 2] = (unsigned char)((2 * sr + n) / (2 * n));
}

struct ComposeArgs {
  const unsigned char* bgr;      // [H][W][3] the frame (layer 0: foreground colours)
  const unsigned char* mask;     // [H][W]    layer 0's alpha, != 0
  const unsigned char* bg;       // [H][W][3] the inpainted frame (layer 1)
  float* out_img;                // [N][3][H][W]
  float* out_gt;                 // [N][1][H][W]
  int H, W;
  float mean[3];
  double M[OSVOS_LUCID_MAX_BATCH][2][6];
  int tone[OSVOS_LUCID_MAX_BATCH][2][6];
};

// fixed-point source coordinates exactly as augment_kernel forms them (doubles, no fused multiply-add, round half to even)
__device__ __forceinline__ void lucid_coords(const double* M, int x, int y, int& X, int& Y) {
#pragma clang fp contract(off)
  const int adelta = __double2int_rn(M[0] * (double)x * 1024.0), bdelta = __double2int_rn(M[3] * (double)x * 1024.0);
  const int Xb = __double2int_rn((M[1] * (double)y + M[2]) * 1024.0), Yb = __double2int_rn((M[4] * (double)y + M[5]) * 1024.0);
  X = (Xb + adelta + 16) >> 5;
  Y = (Yb + bdelta + 16) >> 5;
}

// block (64, 4), grid (ceil(W / 64), ceil(H / 4), N): a wave is 64 consecutive columns of one row
__global__ __launch_bounds__(256) void lucid_compose_kernel(const ComposeArgs a) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  const int H = a.H, W = a.W;
  if (x >= W || y >= H) return;
  int alpha = 0;
  int col[2][3];
#pragma unroll
  for (int L = 0; L < 2; ++L) {
    int X, Y;
    lucid_coords(a.M[n][L], x, y, X, Y);
    const int ix = X >> 5, iy = Y >> 5, fx = X & 31, fy = Y & 31;
    const int cx0 = min(max(ix, 0), W - 1), cx1 = min(max(ix + 1, 0), W - 1), cy0 = min(max(iy, 0), H - 1), cy1 = min(max(iy + 1, 0), H - 1);
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    const size_t o00 = (size_t)cy0 * W + cx0, o01 = (size_t)cy0 * W + cx1, o10 = (size_t)cy1 * W + cx0, o11 = (size_t)cy1 * W + cx1;
    const unsigned char* src = L == 0 ? a.bgr : a.bg;
    const int* t = a.tone[n][L];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int S = w00 * src[o00 * 3 + c] + w01 * src[o01 * 3 + c] + w10 * src[o10 * 3 + c] + w11 * src[o11 * 3 + c];
      const int v = ((S * t[c] + 128) >> 8) + t[3 + c] * 1024;
      col[L][c] = min(max(v, 0), 255 << 10);
    }
    if (L == 0) {                                            // taps outside the frame have alpha 0
      const bool x0in = ix >= 0 && ix < W, x1in = ix + 1 >= 0 && ix + 1 < W, y0in = iy >= 0 && iy < H, y1in = iy + 1 >= 0 && iy + 1 < H;
      alpha = (x0in && y0in && a.mask[o00] ? w00 : 0) + (x1in && y0in && a.mask[o01] ? w01 : 0) + (x0in && y1in && a.mask[o10] ? w10 : 0) +
              (x1in && y1in && a.mask[o11] ? w11 : 0);
    }
  }
  const size_t hw = (size_t)H * W, o = (size_t)y * W + x;
  float* img = a.out_img + (size_t)n * 3 * hw;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int C = alpha * col[0][c] + (1024 - alpha) * col[1][c];      // <= 1024 * 261120 < 2^31
    img[c * hw + o] = (float)C * (1.0f / 1048576.0f) - a.mean[c];
  }
  a.out_gt[(size_t)n * hw + o] = alpha >= 512 ? 1.0f : 0.0f;
}

inline bool inpaint_ok(int H, int W, int passes) {
  return H >= 1 && H <= OSVOS_SQDIST_MAX_SIDE && W >= 1 && W <= OSVOS_SQDIST_MAX_SIDE && passes >= 0 && passes <= OSVOS_LUCID_MAX_PASSES;
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char* p = reinterpret_cast<const char*>(a);
  const char* q = reinterpret_cast<const char*>(b);
  return p < q + nb && q < p + na;
}

}  // namespace

// ws: the column answers [H][W] int32, then (passes > 0) the second colour buffer [H][W][3]
extern "C" size_t osvos_lucid_inpaint_ws_bytes(int H, int W, int passes) {
  if (!inpaint_ok(H, W, passes)) return 0;
  const size_t px = (size_t)H * W;
  return sizeof(int) * px + (passes > 0 ? align_up(3 * px, 4) : 0);
}

extern "C" int osvos_lucid_inpaint(const unsigned char* bgr, const unsigned char* hole, unsigned char* out_bgr, int H, int W, int radius, int passes,
                                   void* ws, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(bgr && hole && out_bgr && ws, "lucid_inpaint: null pointer");
  OSVOS_ARG_CHECK(H >= 1 && H <= OSVOS_SQDIST_MAX_SIDE && W >= 1 && W <= OSVOS_SQDIST_MAX_SIDE, "lucid_inpaint: size H %d, W %d (sides 1..%d)", H, W,
                  OSVOS_SQDIST_MAX_SIDE);
  OSVOS_ARG_CHECK(radius >= 1 && radius <= OSVOS_LUCID_MAX_RADIUS, "lucid_inpaint: radius %d (1..%d)", radius, OSVOS_LUCID_MAX_RADIUS);
  OSVOS_ARG_CHECK(passes >= 0 && passes <= OSVOS_LUCID_MAX_PASSES, "lucid_inpaint: passes %d (0..%d)", passes, OSVOS_LUCID_MAX_PASSES);
  OSVOS_ARG_CHECK((reinterpret_cast<size_t>(ws) & 3) == 0, "lucid_inpaint: ws must be 4-byte aligned");
  const size_t px = (size_t)H * W, need = osvos_lucid_inpaint_ws_bytes(H, W, passes);
  OSVOS_ARG_CHECK(!overlap(out_bgr, 3 * px, bgr, 3 * px) && !overlap(out_bgr, 3 * px, hole, px), "lucid_inpaint: out_bgr overlaps an input");
  OSVOS_ARG_CHECK(!overlap(ws, need, bgr, 3 * px) && !overlap(ws, need, hole, px) && !overlap(ws, need, out_bgr, 3 * px),
                  "lucid_inpaint: ws overlaps a frame");
  int* near = reinterpret_cast<int*>(ws);
  unsigned char* other = reinterpret_cast<unsigned char*>(near + px);      // (never touched with passes == 0)
  unsigned char* cur = passes % 2 == 0 ? out_bgr : other;
  hipLaunchKernelGGL(lucid_column_kernel, dim3((unsigned)ceil_div(W, kColThreads)), dim3(kColThreads), 0, stream, hole, near, H, W);
  OSVOS_LAUNCH_CHECK();
  hipLaunchKernelGGL(lucid_fill_kernel, dim3((unsigned)H), dim3(kRowThreads), sizeof(int) * (size_t)W, stream, bgr, near, cur, H, W);
  OSVOS_LAUNCH_CHECK();
  for (int p = 0; p < passes; ++p) {
    unsigned char* nxt = cur == out_bgr ? other : out_bgr;
    hipLaunchKernelGGL(lucid_smooth_kernel, dim3((unsigned)ceil_div(W, 64), (unsigned)ceil_div(H, 4)), dim3(64, 4), 0, stream, cur, hole, nxt, H, W,
                       radius);
    OSVOS_LAUNCH_CHECK();
    cur = nxt;
  }
  return 0;
}

extern "C" int osvos_lucid_compose(const unsigned char* bgr, const unsigned char* mask, const unsigned char* bg, const double* M, const int* tone,
                                   const float* mean3, float* out_img, float* out_gt, int N, int H, int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(bgr && mask && bg && M && tone && mean3 && out_img && out_gt, "lucid_compose: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= OSVOS_LUCID_MAX_BATCH, "lucid_compose: N %d (1..%d)", N, OSVOS_LUCID_MAX_BATCH);
  OSVOS_ARG_CHECK(H >= 1 && H <= OSVOS_LUCID_MAX_SIDE && W >= 1 && W <= OSVOS_LUCID_MAX_SIDE, "lucid_compose: size H %d, W %d (sides 1..%d)", H, W,
                  OSVOS_LUCID_MAX_SIDE);
  OSVOS_ARG_CHECK((reinterpret_cast<size_t>(out_img) & 3) == 0 && (reinterpret_cast<size_t>(out_gt) & 3) == 0,
                  "lucid_compose: float pointers must be 4-byte aligned");
  ComposeArgs args;          // (2.4 KB of kernel arguments: nothing is uploaded)
  for (int i = 0; i < N * 12; ++i) {
    const double v = M[i];
    const int k = i % 6;
    OSVOS_ARG_CHECK(isfinite(v), "lucid_compose: matrix entry %d of sample %d, layer %d is not finite", k, i / 12, (i / 6) % 2);
    const double lim = (k == 2 || k == 5) ? 262144.0 : 64.0;      // every fixed-point coordinate stays inside int32
    OSVOS_ARG_CHECK(fabs(v) <= lim, "lucid_compose: matrix entry %d of sample %d, layer %d is %g (|.| <= %g)", k, i / 12, (i / 6) % 2, v, lim);
    const int t = tone[i];
    if (k < 3)
      OSVOS_ARG_CHECK(t >= 0 && t <= OSVOS_LUCID_MAX_GAIN, "lucid_compose: gain %d of sample %d, layer %d (0..%d, 256 = 1)", t, i / 12, (i / 6) % 2,
                      OSVOS_LUCID_MAX_GAIN);
    else
      OSVOS_ARG_CHECK(t >= -255 && t <= 255, "lucid_compose: offset %d of sample %d, layer %d (-255..255)", t, i / 12, (i / 6) % 2);
    (&args.M[0][0][0])[i] = v;
    (&args.tone[0][0][0])[i] = t;
  }
  for (int i = N * 12; i < OSVOS_LUCID_MAX_BATCH * 12; ++i) { (&args.M[0][0][0])[i] = 0.0; (&args.tone[0][0][0])[i] = 0; }
  args.bgr = bgr; args.mask = mask; args.bg = bg; args.out_img = out_img; args.out_gt = out_gt; args.H = H; args.W = W;
  for (int c = 0; c < 3; ++c) args.mean[c] = mean3[c];
  hipLaunchKernelGGL(lucid_compose_kernel, dim3((unsigned)ceil_div(W, 64), (unsigned)ceil_div(H, 4), (unsigned)N), dim3(64, 4), 0, stream, args);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
