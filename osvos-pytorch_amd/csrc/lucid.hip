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
//
//   osvos_lucid_compose_ex  the same kernel body, templated on three options: a displacement field bilinear in a coarse lattice added to the
// foreground's source coordinate, an ellipse of displaced background over the composite, and a void band around the label's edges.  The band
// needs the neighbours' labels, which no lane has: each wave stores the ballot of its 64 labels -- one word of a 1-bit label plane [N][H][W / 64]
// -- and a second launch reads only that plane (about 54 KB per 854x480 sample): per row of the disc three words (fetched a row per lane, handed
// round as scalars), a funnel shift to the lane's window, an XOR with the lane's own bit and a mask.  No in-place hazard, no atomics
// (profiles/lucid_deform_timing.txt).
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

// osvos_lucid_compose_ex's additions ride behind the plain arguments, so that the plain kernel's argument block stays what it was
struct ComposeExArgs : ComposeArgs {
  const int* D;                  // [N][GH][GW] (dx, dy) shorts in 1/32 pixel, a pair per word; only read with DEFORM
  unsigned long long* plane;     // [N][H][ceil(W / 64)] the 1-bit label plane; only written with BAND
  int shift, GH, GW;             // log2(cell) and the lattice
  int occ[OSVOS_LUCID_MAX_BATCH][6];      // (cx, cy, rx, ry, sx, sy); only read with OCCLUDE
};

// fixed-point source coordinates exactly as augment_kernel forms them (doubles, no fused multiply-add, round half to even)
__device__ __forceinline__ void lucid_coords(const double* M, int x, int y, int& X, int& Y) {
#pragma clang fp contract(off)
  const int adelta = __double2int_rn(M[0] * (double)x * 1024.0), bdelta = __double2int_rn(M[3] * (double)x * 1024.0);
  const int Xb = __double2int_rn((M[1] * (double)y + M[2]) * 1024.0), Yb = __double2int_rn((M[4] * (double)y + M[5]) * 1024.0);
  X = (Xb + adelta + 16) >> 5;
  Y = (Yb + bdelta + 16) >> 5;
}

// block (64, 4), grid (ceil(W / 64), ceil(H / 4), N): a wave is 64 consecutive columns of one row.  One body: osvos_lucid_compose launches
// <false, false, false, ComposeArgs>, which compiles to what it was before the options existed.
template <bool DEFORM, bool OCCLUDE, bool BAND, typename Args>
__global__ __launch_bounds__(256) void lucid_compose_kernel(const Args a) {
  const int xl = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  const int H = a.H, W = a.W;
  // With BAND the wave's ballot is a word of the label plane, so lanes past the row's end must NOT leave before it: they stay active, work on
  // the row's last pixel (every read in bounds), vote 0 and store nothing.  Nothing relies on how inactive lanes vote.  (A row past the
  // frame's end is a whole wave: y is uniform in it.)
  if constexpr (BAND) {
    if (y >= H) return;
  } else {
    if (xl >= W || y >= H) return;
  }
  const bool live = xl < W;
  const int x = BAND ? min(xl, W - 1) : xl;
  int alpha = 0;
  int col[2][3];
#pragma unroll
  for (int L = 0; L < 2; ++L) {
    int X, Y;
    lucid_coords(a.M[n][L], x, y, X, Y);
    if constexpr (DEFORM) {
      if (L == 0) {
        const int s = a.shift, cell = 1 << s, gx = x >> s, gy = y >> s, tx = x & (cell - 1), ty = y & (cell - 1);
        const int* d = a.D + ((size_t)n * a.GH + gy) * a.GW + gx;              // gy + 1 < GH and gx + 1 < GW by the lattice's size
        const int d00 = d[0], d01 = d[1], d10 = d[a.GW], d11 = d[a.GW + 1];
        const int w00 = (cell - tx) * (cell - ty), w01 = tx * (cell - ty), w10 = (cell - tx) * ty, w11 = tx * ty, half = 1 << (2 * s - 1);
        // (short)(d) = .x, d >> 16 = .y; weights >= 0 summing to 2^(2 s) <= 2^16 times shorts: every partial sum inside int32
        X += (w00 * (short)d00 + w01 * (short)d01 + w10 * (short)d10 + w11 * (short)d11 + half) >> (2 * s);
        Y += (w00 * (d00 >> 16) + w01 * (d01 >> 16) + w10 * (d10 >> 16) + w11 * (d11 >> 16) + half) >> (2 * s);
      }
    }
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
  if constexpr (OCCLUDE) {
    const int* e = a.occ[n];
    const long long rx2 = (long long)e[2] * e[2], ry2 = (long long)e[3] * e[3], dx = x - e[0], dy = y - e[1];
    if (rx2 != 0 && ry2 != 0 && dx * dx * ry2 + dy * dy * rx2 <= rx2 * ry2) {      // at most 12288^2 * 4096^2 * 2 < 2^52
      const size_t o = ((size_t)min(max(y + e[5], 0), H - 1) * W + min(max(x + e[4], 0), W - 1)) * 3;
      const int* t = a.tone[n][1];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v = ((a.bg[o + c] * 1024 * t[c] + 128) >> 8) + t[3 + c] * 1024;
        col[1][c] = min(max(v, 0), 255 << 10);
      }
      alpha = 0;                                             // C = 1024 S', label 0
    }
  }
  const size_t hw = (size_t)H * W, o = (size_t)y * W + x;
  const bool label = alpha >= 512;
  if (live) {
    float* img = a.out_img + (size_t)n * 3 * hw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int C = alpha * col[0][c] + (1024 - alpha) * col[1][c];      // <= 1024 * 261120 < 2^31
      img[c * hw + o] = (float)C * (1.0f / 1048576.0f) - a.mean[c];
    }
    a.out_gt[(size_t)n * hw + o] = label ? 1.0f : 0.0f;
  }
  if constexpr (BAND) {
    const unsigned long long word = __ballot(live && label);                 // all 64 lanes are here: bit i = column 64 blockIdx.x + i
    if (threadIdx.x == 0) a.plane[((size_t)n * H + y) * gridDim.x + blockIdx.x] = word;
  }
}

struct BandArgs {
  const unsigned long long* plane;      // [N][H][ceil(W / 64)]
  float* out_gt;                        // [N][1][H][W]
  int H, W, band;
  int hw[OSVOS_LUCID_MAX_BAND + 1];     // isqrt(band^2 - dy^2) by |dy|
};

__device__ __forceinline__ unsigned long long lane_word(unsigned long long v, int lane) {      // lane: uniform
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, lane), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// block (64, 4), grid (ceil(W / 64), ceil(H / 4), N), after the composition on the same stream.  A wave needs the word of its 64 columns
// and the two next to it from the 2 band + 1 <= 33 rows of the disc: lane i fetches those of row y - band + i (three loads per wave, all in
// flight at once; a loop of uniform loads was timed first and waited on every row), and the loop takes row after row out of that lane -- as
// scalars, so that a row of three zero words is skipped by the whole wave.  Every lane stays to the end for that: lanes past the row's end
// work on the last pixel and store nothing.  A lane looks at the 64 columns x - 32 .. x + 31 funnelled out of two of the words; columns
// outside the image are masked, never read as 0.
__global__ __launch_bounds__(256) void lucid_band_kernel(const BandArgs a) {
  const int lane = threadIdx.x, xl = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y), n = blockIdx.z;
  const int H = a.H, W = a.W, band = a.band, words = gridDim.x, wi = blockIdx.x;      // (y: a wave is one row of the block, so the row is scalar)
  if (y >= H) return;                                                        // (the whole wave)
  const int x = min(xl, W - 1);
  const unsigned long long* rows = a.plane + (size_t)n * H * words;
  unsigned long long wl = 0, wm = 0, wh = 0;
  const int fetch = y - band + lane;
  const int half_width = a.hw[min(lane < band ? band - lane : lane - band, OSVOS_LUCID_MAX_BAND)];      // of the row this lane fetches
  if (lane <= 2 * band && fetch >= 0 && fetch < H) {
    const unsigned long long* r = rows + (size_t)fetch * words;
    wm = r[wi];
    if (wi > 0) wl = r[wi - 1];
    if (wi + 1 < words) wh = r[wi + 1];
  }
  const unsigned long long own = (lane_word(wm, band) >> lane) & 1 ? ~0ull : 0ull;      // (for a lane past the row's end: 0, unused)
  const int left = min(band, x), right = min(band, W - 1 - x);               // the disc's columns clipped to the image, for hw = band
  const bool low = lane < 32;
  const int k = low ? lane + 32 : lane - 32;                                 // window bit j = column x - 32 + j
  unsigned long long differ = 0;
  for (int dy = -band; dy <= band; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;                                         // (uniform in the wave)
    const unsigned long long mid = lane_word(wm, dy + band), lo = lane_word(wl, dy + band), hi = lane_word(wh, dy + band);
    if ((lo | mid | hi) == 0) {                                              // (uniform) a row of background: it differs from every set pixel --
      differ |= own;                                                         // the row is inside the image and holds at least column x
      continue;
    }
    const unsigned long long A = low ? lo : mid, B = low ? mid : hi;
    const unsigned long long win = k == 0 ? A : (A >> k) | (B << (64 - k));
    const int h = __builtin_amdgcn_readlane(half_width, dy + band), l = min(h, left), rr = min(h, right);
    const unsigned long long m = ((2ull << (l + rr)) - 1) << (32 - l);       // l + rr + 1 <= 33 bits from bit 32 - l >= 16
    differ |= (win ^ own) & m;
  }
  if (differ && xl < W) a.out_gt[((size_t)n * H + y) * W + x] = -1.0f;
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

// the checks and the argument block that osvos_lucid_compose and osvos_lucid_compose_ex share; 0 or the refusal
static int compose_fill(ComposeArgs& args, const unsigned char* bgr, const unsigned char* mask, const unsigned char* bg, const double* M,
                        const int* tone, const float* mean3, float* out_img, float* out_gt, int N, int H, int W) {
  OSVOS_ARG_CHECK(bgr && mask && bg && M && tone && mean3 && out_img && out_gt, "lucid_compose: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= OSVOS_LUCID_MAX_BATCH, "lucid_compose: N %d (1..%d)", N, OSVOS_LUCID_MAX_BATCH);
  OSVOS_ARG_CHECK(H >= 1 && H <= OSVOS_LUCID_MAX_SIDE && W >= 1 && W <= OSVOS_LUCID_MAX_SIDE, "lucid_compose: size H %d, W %d (sides 1..%d)", H, W,
                  OSVOS_LUCID_MAX_SIDE);
  OSVOS_ARG_CHECK((reinterpret_cast<size_t>(out_img) & 3) == 0 && (reinterpret_cast<size_t>(out_gt) & 3) == 0,
                  "lucid_compose: float pointers must be 4-byte aligned");
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
  return 0;
}

static inline dim3 compose_grid(int N, int H, int W) { return dim3((unsigned)ceil_div(W, 64), (unsigned)ceil_div(H, 4), (unsigned)N); }

extern "C" int osvos_lucid_compose(const unsigned char* bgr, const unsigned char* mask, const unsigned char* bg, const double* M, const int* tone,
                                   const float* mean3, float* out_img, float* out_gt, int N, int H, int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ComposeArgs args;          // (2.4 KB of kernel arguments: nothing is uploaded)
  if (const int rc = compose_fill(args, bgr, mask, bg, M, tone, mean3, out_img, out_gt, N, H, W)) return rc;
  hipLaunchKernelGGL((lucid_compose_kernel<false, false, false, ComposeArgs>), compose_grid(N, H, W), dim3(64, 4), 0, stream, args);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

static inline bool compose_ex_sizes_ok(int N, int H, int W, int band) {
  return N >= 1 && N <= OSVOS_LUCID_MAX_BATCH && H >= 1 && H <= OSVOS_LUCID_MAX_SIDE && W >= 1 && W <= OSVOS_LUCID_MAX_SIDE && band >= 0 &&
         band <= OSVOS_LUCID_MAX_BAND;
}

// ws: the 1-bit label plane [N][H][ceil(W / 64)] of 64-bit words
extern "C" size_t osvos_lucid_compose_ex_ws_bytes(int N, int H, int W, int band) {
  if (!compose_ex_sizes_ok(N, H, W, band) || band == 0) return 0;
  return sizeof(unsigned long long) * (size_t)N * H * ceil_div(W, 64);
}

typedef void (*ComposeExKernel)(const ComposeExArgs);
// [deform][occlude][band]; the entry without any option is never launched from here: that call goes to the plain kernel
static const ComposeExKernel kComposeEx[2][2][2] = {
    {{nullptr, lucid_compose_kernel<false, false, true, ComposeExArgs>},
     {lucid_compose_kernel<false, true, false, ComposeExArgs>, lucid_compose_kernel<false, true, true, ComposeExArgs>}},
    {{lucid_compose_kernel<true, false, false, ComposeExArgs>, lucid_compose_kernel<true, false, true, ComposeExArgs>},
     {lucid_compose_kernel<true, true, false, ComposeExArgs>, lucid_compose_kernel<true, true, true, ComposeExArgs>}}};

extern "C" int osvos_lucid_compose_ex(const unsigned char* bgr, const unsigned char* mask, const unsigned char* bg, const double* M, const int* tone,
                                      const int* occ, const short* D, int cell, int band, const float* mean3, float* out_img, float* out_gt, int N,
                                      int H, int W, void* ws, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ComposeExArgs args;        // (under 3 KB of kernel arguments: only D is read from device memory)
  if (const int rc = compose_fill(args, bgr, mask, bg, M, tone, mean3, out_img, out_gt, N, H, W)) return rc;
  const size_t px = (size_t)H * W;
  int shift = 0;
  if (D) {
    OSVOS_ARG_CHECK(cell >= OSVOS_LUCID_MIN_CELL && cell <= OSVOS_LUCID_MAX_CELL && (cell & (cell - 1)) == 0,
                    "lucid_compose_ex: cell %d (a power of two in %d..%d)", cell, OSVOS_LUCID_MIN_CELL, OSVOS_LUCID_MAX_CELL);
    OSVOS_ARG_CHECK((reinterpret_cast<size_t>(D) & 3) == 0, "lucid_compose_ex: D must be 4-byte aligned");
    while ((1 << shift) < cell) ++shift;
  }
  OSVOS_ARG_CHECK(band >= 0 && band <= OSVOS_LUCID_MAX_BAND, "lucid_compose_ex: band %d (0..%d)", band, OSVOS_LUCID_MAX_BAND);
  const size_t need = osvos_lucid_compose_ex_ws_bytes(N, H, W, band);
  if (band > 0) {
    OSVOS_ARG_CHECK(ws, "lucid_compose_ex: band %d needs ws (null pointer)", band);
    OSVOS_ARG_CHECK((reinterpret_cast<size_t>(ws) & 7) == 0, "lucid_compose_ex: ws must be 8-byte aligned");
    OSVOS_ARG_CHECK(!overlap(ws, need, bgr, 3 * px) && !overlap(ws, need, mask, px) && !overlap(ws, need, bg, 3 * px) &&
                        !overlap(ws, need, out_img, sizeof(float) * 3 * N * px) && !overlap(ws, need, out_gt, sizeof(float) * N * px),
                    "lucid_compose_ex: ws overlaps an input or an output");
  }
  bool occlude = false;
  for (int i = 0; i < OSVOS_LUCID_MAX_BATCH * 6; ++i) (&args.occ[0][0])[i] = 0;
  if (occ) {
    for (int i = 0; i < N * 6; ++i) {
      const int v = occ[i], k = i % 6;
      if (k == 2 || k == 3)
        OSVOS_ARG_CHECK(v >= 0 && v <= OSVOS_LUCID_MAX_OCC_RADIUS, "lucid_compose_ex: occluder radius %d of sample %d (0..%d)", v, i / 6,
                        OSVOS_LUCID_MAX_OCC_RADIUS);
      else
        OSVOS_ARG_CHECK(v >= -OSVOS_LUCID_MAX_OCC_OFFSET && v <= OSVOS_LUCID_MAX_OCC_OFFSET,
                        "lucid_compose_ex: occluder %s %d of sample %d (|.| <= %d)", k < 2 ? "centre" : "offset", v, i / 6, OSVOS_LUCID_MAX_OCC_OFFSET);
      (&args.occ[0][0])[i] = v;
    }
    for (int n = 0; n < N; ++n) occlude = occlude || (args.occ[n][2] != 0 && args.occ[n][3] != 0);
  }
  if (!D && !occlude && band == 0) {                         // nothing asked for: osvos_lucid_compose's own kernel, its bits and its cost
    hipLaunchKernelGGL((lucid_compose_kernel<false, false, false, ComposeArgs>), compose_grid(N, H, W), dim3(64, 4), 0, stream,
                       static_cast<const ComposeArgs&>(args));
    OSVOS_LAUNCH_CHECK();
    return 0;
  }
  args.D = reinterpret_cast<const int*>(D);
  args.plane = reinterpret_cast<unsigned long long*>(ws);
  args.shift = shift;
  args.GH = D ? ((H - 1) >> shift) + 2 : 0;
  args.GW = D ? ((W - 1) >> shift) + 2 : 0;
  hipLaunchKernelGGL(kComposeEx[D != nullptr][occlude][band > 0], compose_grid(N, H, W), dim3(64, 4), 0, stream, args);
  OSVOS_LAUNCH_CHECK();
  if (band > 0) {
    BandArgs b;
    b.plane = args.plane; b.out_gt = out_gt; b.H = H; b.W = W; b.band = band;
    for (int dy = 0; dy <= OSVOS_LUCID_MAX_BAND; ++dy) {
      int h = 0;
      while (dy <= band && (h + 1) * (h + 1) <= band * band - dy * dy) ++h;
      b.hw[dy] = h;
    }
    hipLaunchKernelGGL(lucid_band_kernel, compose_grid(N, H, W), dim3(64, 4), 0, stream, b);
    OSVOS_LAUNCH_CHECK();
  }
  return 0;
}
