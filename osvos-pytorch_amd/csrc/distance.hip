// Exact squared Euclidean distance maps of binary masks, and the online-adaptation targets made from two of them (OnAVOS-style adaptation
// over the sequence: include/osvos_hip.h, "online adaptation").
//
// Separable form.  With g[y][x] = the vertical distance from (y, x) to the nearest source pixel of column x (or "none"),
//   sqdist[y][x] = min over x' with g[y][x'] != none of (x - x')^2 + g[y][x']^2.
// Column pass: one lane per column, a sweep down and a sweep up; consecutive lanes read consecutive bytes / words of a row.
// Row pass: one workgroup per (row, image); the row of g sits in LDS (4 W bytes, at most 16 KB); every lane owns the output pixels
//   x, x + blockDim, ... and walks outwards from x, both sides in the same step, until dx^2 >= best: every later candidate is at least
//   dx^2, so the stop is exact.  Consecutive lanes read consecutive LDS words (no bank conflicts).  A column without a source is SKIPPED
//   (kNoSource is a marker, never a number that gets squared).  Everything is integer: g <= 4095, so (x - x')^2 + g^2 <= 2 * 4095^2 < 2^31.
// Worst case of the walk: an image with one far source pixel (or none) -- every pixel walks its whole row, H W W / 2 steps per side
// (854x480: 0.35 G LDS reads); a blob stops after about its own distance.
#include <limits.h>

#include "common.h"

namespace {

constexpr int kNoSource = -1;
constexpr int kRowThreads = 256;
constexpr int kColThreads = 64;

// What the column pass takes for a source pixel.  kEroded = false: (mask != 0) != invert.  kEroded = true: the eroded mask
// E = mask != 0 and sqdist-to-background > erosion^2 (d_bg is the distance map of the inverted mask; OSVOS_SQDIST_NONE = no background
// in the image = every mask pixel stays) -- the adaptation targets never materialise E.
template <bool kEroded>
__device__ __forceinline__ bool is_source(const unsigned char* __restrict__ mask, int invert, const int* __restrict__ d_bg, long long erosion2, size_t i) {
  const bool m = mask[i] != 0;
  if (!kEroded) return m != (invert != 0);
  const int d = d_bg[i];
  return m && (d == OSVOS_SQDIST_NONE || (long long)d > erosion2);
}

// grid (ceil(W / kColThreads), N)
template <bool kEroded>
__global__ __launch_bounds__(kColThreads) void sqdist_column_kernel(const unsigned char* __restrict__ mask, int invert, const int* __restrict__ d_bg,
                                                                    long long erosion2, int* __restrict__ g, int H, int W) {
  const int x = blockIdx.x * kColThreads + threadIdx.x;
  if (x >= W) return;
  const size_t base = (size_t)blockIdx.y * H * W + x;
  int d = kNoSource;                                         // distance to the nearest source at or above y
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    const size_t i = base + (size_t)y * W;
    d = is_source<kEroded>(mask, invert, d_bg, erosion2, i) ? 0 : (d < 0 ? kNoSource : d + 1);
    g[i] = d;
  }
  d = kNoSource;                                             // ... at or below y
#pragma unroll 8
  for (int y = H - 1; y >= 0; --y) {
    const size_t i = base + (size_t)y * W;
    const int up = g[i];
    d = up == 0 ? 0 : (d < 0 ? kNoSource : d + 1);
    g[i] = up < 0 ? d : (d < 0 ? up : (up < d ? up : d));
  }
}

struct LabelEpilogue {
  const float* logits;
  float pos_logit;
  long long distance2;
  float* label;
  unsigned long long* counts;      // [N][3]: n_pos, n_neg, n_void
};

// grid (H, N), dynamic LDS 4 W bytes.  kLabels = false: out = sqdist.  kLabels = true: the adaptation labels and their counts.
template <bool kLabels>
__global__ __launch_bounds__(kRowThreads) void sqdist_row_kernel(const int* __restrict__ g, int* __restrict__ out, int H, int W, LabelEpilogue ep) {
  extern __shared__ int row[];
  const size_t base = ((size_t)blockIdx.y * H + blockIdx.x) * W;
  for (int x = threadIdx.x; x < W; x += kRowThreads) row[x] = g[base + x];
  __syncthreads();
  unsigned npos = 0, nneg = 0;
  for (int x = threadIdx.x; x < W; x += kRowThreads) {
    int c = row[x];
    int best = c < 0 ? OSVOS_SQDIST_NONE : c * c;
    const int left = x, right = W - 1 - x;
    const int reach = left > right ? left : right;
    for (int dx = 1; dx <= reach; ++dx) {
      const int dd = dx * dx;
      if (dd >= best) break;
      if (dx <= left) {
        c = row[x - dx];
        if (c >= 0) { const int v = dd + c * c; best = v < best ? v : best; }
      }
      if (dx <= right) {
        c = row[x + dx];
        if (c >= 0) { const int v = dd + c * c; best = v < best ? v : best; }
      }
    }
    if (!kLabels) {
      out[base + x] = best;
    } else {
      const bool neg = best == OSVOS_SQDIST_NONE || (long long)best > ep.distance2;
      const bool pos = !neg && ep.logits[base + x] > ep.pos_logit;      // (false for a NaN logit)
      ep.label[base + x] = neg ? 0.f : (pos ? 1.f : -1.f);
      npos += pos ? 1u : 0u;
      nneg += neg ? 1u : 0u;
    }
  }
  if (kLabels) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      npos += __shfl_xor(npos, o, 64);
      nneg += __shfl_xor(nneg, o, 64);
    }
    __shared__ unsigned red[kRowThreads / 64][2];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = npos; red[threadIdx.x >> 6][1] = nneg; }
    __syncthreads();
    if (threadIdx.x == 0) {
      npos = nneg = 0;
      for (int k = 0; k < kRowThreads / 64; ++k) { npos += red[k][0]; nneg += red[k][1]; }
      unsigned long long* cn = ep.counts + 3 * (size_t)blockIdx.y;
      if (npos) atomicAdd(&cn[0], (unsigned long long)npos);
      if (nneg) atomicAdd(&cn[1], (unsigned long long)nneg);
      if ((unsigned)W - npos - nneg) atomicAdd(&cn[2], (unsigned long long)((unsigned)W - npos - nneg));
    }
  }
}

inline bool sides_ok(int N, int H, int W) {
  return N >= 1 && N <= 65535 && H >= 1 && H <= OSVOS_SQDIST_MAX_SIDE && W >= 1 && W <= OSVOS_SQDIST_MAX_SIDE;
}

template <bool kEroded>
inline void launch_columns(const unsigned char* mask, int invert, const int* d_bg, long long erosion2, int* g, int N, int H, int W, hipStream_t stream) {
  hipLaunchKernelGGL(sqdist_column_kernel<kEroded>, dim3((unsigned)ceil_div(W, kColThreads), (unsigned)N), dim3(kColThreads), 0, stream, mask, invert,
                     d_bg, erosion2, g, H, W);
}

}  // namespace

extern "C" size_t osvos_mask_sqdist_ws_bytes(int N, int H, int W) {
  return sides_ok(N, H, W) ? sizeof(int) * (size_t)N * H * W : 0;
}

extern "C" int osvos_mask_sqdist(const unsigned char* mask, int invert, int* sqdist, int N, int H, int W, void* ws, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(mask && sqdist && ws, "mask_sqdist: null pointer");
  OSVOS_ARG_CHECK(sides_ok(N, H, W), "mask_sqdist: N %d, H %d, W %d (N 1..65535, sides 1..%d)", N, H, W, OSVOS_SQDIST_MAX_SIDE);
  int* g = reinterpret_cast<int*>(ws);
  launch_columns<false>(mask, invert, nullptr, 0, g, N, H, W, stream);
  OSVOS_LAUNCH_CHECK();
  hipLaunchKernelGGL(sqdist_row_kernel<false>, dim3((unsigned)H, (unsigned)N), dim3(kRowThreads), sizeof(int) * (size_t)W, stream, g, sqdist, H, W,
                     LabelEpilogue{});
  OSVOS_LAUNCH_CHECK();
  return 0;
}

// ws: the column distances g, then the distance-to-background map of prev_mask
extern "C" size_t osvos_adapt_ws_bytes(int N, int H, int W) {
  return 2 * osvos_mask_sqdist_ws_bytes(N, H, W);
}

extern "C" int osvos_adapt_targets(const float* logits, const unsigned char* prev_mask, float pos_logit, int erosion, int distance, float* label,
                                   void* counts, int N, int H, int W, void* ws, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(logits && prev_mask && label && counts && ws, "adapt_targets: null pointer");
  OSVOS_ARG_CHECK(sides_ok(N, H, W), "adapt_targets: N %d, H %d, W %d (N 1..65535, sides 1..%d)", N, H, W, OSVOS_SQDIST_MAX_SIDE);
  OSVOS_ARG_CHECK(erosion >= 0 && distance >= 0, "adapt_targets: erosion %d, distance %d (both >= 0)", erosion, distance);
  const size_t px = (size_t)N * H * W;
  int* g = reinterpret_cast<int*>(ws);
  int* d_bg = g + px;
  OSVOS_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * 3 * (size_t)N, stream));
  // 1. distance to the background of prev_mask
  launch_columns<false>(prev_mask, 1, nullptr, 0, g, N, H, W, stream);
  OSVOS_LAUNCH_CHECK();
  hipLaunchKernelGGL(sqdist_row_kernel<false>, dim3((unsigned)H, (unsigned)N), dim3(kRowThreads), sizeof(int) * (size_t)W, stream, g, d_bg, H, W,
                     LabelEpilogue{});
  OSVOS_LAUNCH_CHECK();
  // 2. distance to the eroded mask (its pixels are decided in the column pass), compared and labelled in the row pass
  launch_columns<true>(prev_mask, 0, d_bg, (long long)erosion * erosion, g, N, H, W, stream);
  OSVOS_LAUNCH_CHECK();
  LabelEpilogue ep;
  ep.logits = logits; ep.pos_logit = pos_logit; ep.distance2 = (long long)distance * distance; ep.label = label;
  ep.counts = reinterpret_cast<unsigned long long*>(counts);
  hipLaunchKernelGGL(sqdist_row_kernel<true>, dim3((unsigned)H, (unsigned)N), dim3(kRowThreads), sizeof(int) * (size_t)W, stream, g, nullptr, H, W, ep);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
