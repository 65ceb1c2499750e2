// Superpixel snapping: an integer grid-SLIC on the decoded frame and logit pooling over a labelling (the rule: include/osvos_hip.h).
//
//   assign: a pixel takes the minimiser of (D, k), D = S^2 dc + m^2 ds, over the clusters of the 3 x 3 cells around its home cell;
//   update: a centre component is floor((2 sum + count) / (2 count)) over the cluster's pixels.  All integers; the test is bit for bit.
//
// assign_kernel<INIT>  one workgroup of 256 lanes per tile of 64 x 16 pixels.  It stages the five centre components of every cluster whose
//   cell touches the tile plus one ring (the "ring": at most 35 x 11 clusters, at cell 2) in LDS next to six zeroed accumulators per ring
//   cluster.  Wave w takes rows w, w + 4, ..: a lane is a column, so a wave stores 64 consecutive labels.  Per pixel the nine candidates
//   are read from LDS in ascending k and compared with a strict <; the pixel then adds (x, y, b, g, r, 1) to its cluster's accumulators with
//   LDS integer atomics (a cluster's pixels lie in the 3 x 3 cells around it, so every label a tile produces is in its ring).  The flush is
//   one global atomic per non-zero accumulator.  INIT skips the candidates: the label is the home cell (labels_0).
// update_kernel        one lane per cluster: divides, keeps the centre of an empty cluster, writes count, re-zeroes the six sums.  A
//   separate launch: no workgroup waits for another.
// pool_accumulate      the same tile.  The tile's smallest valid label is taken with an LDS atomic min; labels less than POOL_SLOTS above it
//   (every label of a SLIC tile unless the grid is very wide) are summed in LDS -- a 64-bit sum and a count per slot -- and flushed with one
//   64-bit and one 32-bit global atomic per non-empty slot; any other valid label goes to global memory directly.  Right for any labelling.
// pool_apply           one gather and one 64-bit floor division per pixel.
//
// Integer sums: the arrival order of the atomics cannot change a result.  Vector stores only; the only floating point is the
// quantisation of a logit and the conversion back.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int TW = 64, TH = 16;                                             // pixels per tile
constexpr int RING_MAX = ((TW - 1) / 2 + 4) * ((TH - 1) / 2 + 4);           // clusters in a tile's ring at the smallest cell (35 x 11)
constexpr int POOL_SLOTS = 2048;                                            // labels a pooling tile sums in LDS

struct Grid {
  int H, W, GH, GW, S, m2;                                                   // m2 = compactness^2
};

// grid (ceil(W / TW), ceil(H / TH), N).  centres, acc: [N][K][6]
template <bool INIT>
__global__ __launch_bounds__(THREADS) void assign_kernel(const unsigned char* __restrict__ bgr, const int* __restrict__ centres,
                                                         int* __restrict__ labels, unsigned* __restrict__ acc, Grid g) {
  __shared__ int sC[INIT ? 1 : RING_MAX * 5];
  __shared__ unsigned sA[RING_MAX * 6];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int x1 = min(x0 + TW, g.W), y1 = min(y0 + TH, g.H);                  // (exclusive)
  const int cx0 = max(x0 / g.S - 1, 0), cx1 = min((x1 - 1) / g.S + 1, g.GW - 1);
  const int cy0 = max(y0 / g.S - 1, 0), cy1 = min((y1 - 1) / g.S + 1, g.GH - 1);
  const int rw = cx1 - cx0 + 1, rh = cy1 - cy0 + 1, ring = rw * rh;          // ring <= RING_MAX: x0 / S .. (x1 - 1) / S are at most (TW - 1) / S + 2 cells
  const size_t kbase = (size_t)n * g.GH * g.GW;

  for (int i = tid; i < ring; i += THREADS) {
    const int iy = i / rw, ix = i - iy * rw;
    if (!INIT) {
      const int* c = centres + (kbase + (size_t)(cy0 + iy) * g.GW + (cx0 + ix)) * 6;
#pragma unroll
      for (int j = 0; j < 5; ++j) sC[i * 5 + j] = c[j];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) sA[i * 6 + j] = 0u;
  }
  __syncthreads();

  const int x = x0 + (tid & (TW - 1));
  if (x < x1) {
    const int gx = x / g.S;
    const int S2 = g.S * g.S;
    for (int y = y0 + (tid >> 6); y < y1; y += THREADS / TW) {
      const int gy = y / g.S;
      const unsigned char* p = bgr + (((size_t)n * g.H + y) * g.W + x) * 3;
      const int b = p[0], gr = p[1], r = p[2];
      int slot = (gy - cy0) * rw + (gx - cx0);                               // ring slot of the home cell
      if (!INIT) {
        int best = 0x7fffffff;
#pragma unroll
        for (int oy = -1; oy <= 1; ++oy) {
#pragma unroll
          for (int ox = -1; ox <= 1; ++ox) {
            const int cy = gy + oy, cx = gx + ox;
            if (cy < 0 || cy >= g.GH || cx < 0 || cx >= g.GW) continue;
            const int s = (cy - cy0) * rw + (cx - cx0);
            const int* c = sC + s * 5;
            const int dx = x - c[0], dy = y - c[1], db = b - c[2], dg = gr - c[3], dr = r - c[4];
            const int d = S2 * (db * db + dg * dg + dr * dr) + g.m2 * (dx * dx + dy * dy);      // < 2^31 (header)
            if (d < best) {                                                  // ascending k, strict <: the smaller k keeps a tie
              best = d;
              slot = s;
            }
          }
        }
      }
      const int sy = slot / rw, sx = slot - sy * rw;
      labels[((size_t)n * g.H + y) * g.W + x] = (cy0 + sy) * g.GW + (cx0 + sx);
      unsigned* a = sA + slot * 6;
      atomicAdd(a + 0, (unsigned)x);
      atomicAdd(a + 1, (unsigned)y);
      atomicAdd(a + 2, (unsigned)b);
      atomicAdd(a + 3, (unsigned)gr);
      atomicAdd(a + 4, (unsigned)r);
      atomicAdd(a + 5, 1u);
    }
  }
  __syncthreads();

  for (int i = tid; i < ring * 6; i += THREADS) {
    const unsigned v = sA[i];
    if (v == 0u) continue;
    const int s = i / 6, j = i - s * 6;
    const int iy = s / rw, ix = s - iy * rw;
    atomicAdd(acc + (kbase + (size_t)(cy0 + iy) * g.GW + (cx0 + ix)) * 6 + j, v);
  }
}

// one lane per cluster of the batch: centres (the working copy in the workspace) and out (the caller's, may be NULL) [N K][6]
__global__ __launch_bounds__(THREADS) void update_kernel(unsigned* __restrict__ acc, int* __restrict__ centres, int* __restrict__ out, size_t clusters) {
  const size_t k = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (k >= clusters) return;
  unsigned* a = acc + k * 6;
  int* c = centres + k * 6;
  const unsigned count = a[5];
  int v[6];
#pragma unroll
  for (int j = 0; j < 5; ++j)
    v[j] = count ? (int)((2ull * a[j] + count) / (2ull * count)) : c[j];    // (an x sum reaches 2^32 - 1: 64 bits)
  v[5] = (int)count;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    c[j] = v[j];
    if (out) out[k * 6 + j] = v[j];
    a[j] = 0u;
  }
}

// rint(clamp(x, -16384, 16384) * 65536), half to even; a NaN fails the first comparison and takes the lower clamp
__device__ __forceinline__ int quantise(float x) {
  const float c = !(x > -16384.0f) ? -16384.0f : (x > 16384.0f ? 16384.0f : x);
  return (int)rintf(c * 65536.0f);
}

// grid (ceil(W / TW), ceil(H / TH), N).  sums [N][K] int64, counts [N][K] int32
__global__ __launch_bounds__(THREADS) void pool_accumulate(const float* __restrict__ logits, const int* __restrict__ labels,
                                                           unsigned long long* __restrict__ sums, unsigned* __restrict__ counts, int H, int W, int K) {
  __shared__ unsigned long long sSum[POOL_SLOTS];
  __shared__ unsigned sCount[POOL_SLOTS];
  __shared__ int sMin;
  const int tid = threadIdx.x, n = blockIdx.z;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int y1 = min(y0 + TH, H);
  const int x = x0 + (tid & (TW - 1));
  const size_t kbase = (size_t)n * K;
  for (int i = tid; i < POOL_SLOTS; i += THREADS) {
    sSum[i] = 0ull;
    sCount[i] = 0u;
  }
  if (tid == 0) sMin = 0x7fffffff;
  __syncthreads();

  constexpr int ROWS = TH / (THREADS / TW);
  int lab[ROWS], q[ROWS];
  int low = 0x7fffffff;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int y = y0 + (tid >> 6) + r * (THREADS / TW);
    lab[r] = -1;
    q[r] = 0;
    if (x < W && y < y1) {
      const size_t i = ((size_t)n * H + y) * W + x;
      const int l = labels[i];
      if (l >= 0 && l < K) {
        lab[r] = l;
        q[r] = quantise(logits[i]);
        low = min(low, l);
      }
    }
  }
  if (low != 0x7fffffff) atomicMin(&sMin, low);
  __syncthreads();
  const int base = sMin;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    if (lab[r] < 0) continue;
    const unsigned long long v = (unsigned long long)(long long)q[r];        // two's complement: the wrapped unsigned sum is the signed sum
    const int rel = lab[r] - base;
    if (rel < POOL_SLOTS) {
      atomicAdd(&sSum[rel], v);
      atomicAdd(&sCount[rel], 1u);
    } else {
      atomicAdd(sums + kbase + lab[r], v);
      atomicAdd(counts + kbase + lab[r], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < POOL_SLOTS; i += THREADS) {
    const unsigned c = sCount[i];
    if (c == 0u) continue;                                                   // (base + i < K: a slot is filled by a valid label only)
    atomicAdd(sums + kbase + base + i, sSum[i]);
    atomicAdd(counts + kbase + base + i, c);
  }
}

// floor(a / b) for b > 0 (C truncates towards zero)
__device__ __forceinline__ long long floor_div(long long a, long long b) {
  long long q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

// one lane per pixel; logits and out as 32-bit words so that a passed-through logit keeps its bits
__global__ __launch_bounds__(THREADS) void pool_apply(const unsigned* __restrict__ logits, const int* __restrict__ labels,
                                                      const unsigned long long* __restrict__ sums, const unsigned* __restrict__ counts,
                                                      unsigned* __restrict__ out, size_t pixels_per_image, int K) {
  const size_t p = (size_t)blockIdx.x * THREADS + threadIdx.x;
  const int n = blockIdx.y;
  if (p >= pixels_per_image) return;
  const size_t i = (size_t)n * pixels_per_image + p;
  const int l = labels[i];
  unsigned bits = logits[i];
  if (l >= 0 && l < K) {
    const long long s = (long long)sums[(size_t)n * K + l];
    const long long c = (long long)counts[(size_t)n * K + l];              // >= 1: this pixel was counted
    const float v = (float)(int)floor_div(2 * s + c, 2 * c) * (1.0f / 65536.0f);
    bits = __float_as_uint(v);
  }
  out[i] = bits;
}

bool side_ok(int v) { return v >= 1 && v <= OSVOS_SUPERPIXELS_MAX_SIDE; }
bool frames_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && side_ok(H) && side_ok(W) && (size_t)N * H * W <= ((size_t)1 << 38); }
bool cell_ok(int cell) { return cell >= 2 && cell <= OSVOS_SUPERPIXELS_MAX_CELL; }
bool pool_k_ok(int N, int K) { return N >= 1 && N <= 65535 && K >= 1 && K <= OSVOS_SUPERPIXELS_MAX_K; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

// the six sums and the working centres of every cluster
extern "C" size_t osvos_superpixels_ws_bytes(int N, int H, int W, int cell) {
  if (!frames_ok(N, H, W) || !cell_ok(cell)) return 0;
  return (size_t)N * ceil_div(H, cell) * ceil_div(W, cell) * 6 * (sizeof(unsigned) + sizeof(int));
}

extern "C" int osvos_superpixels_slic(const unsigned char* frames, int* labels, int* centres, void* ws, int N, int H, int W, int cell, int compactness,
                                      int iters, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(frames && labels && ws, "superpixels_slic: null pointer (frames, labels and ws are required)");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "superpixels_slic: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(side_ok(H) && side_ok(W), "superpixels_slic: bad size H %d W %d (1..%d per side)", H, W, OSVOS_SUPERPIXELS_MAX_SIDE);
  OSVOS_ARG_CHECK(cell_ok(cell), "superpixels_slic: cell %d (2..%d)", cell, OSVOS_SUPERPIXELS_MAX_CELL);
  OSVOS_ARG_CHECK(compactness >= 0 && compactness <= OSVOS_SUPERPIXELS_MAX_COMPACTNESS, "superpixels_slic: compactness %d (0..%d)", compactness,
                  OSVOS_SUPERPIXELS_MAX_COMPACTNESS);
  OSVOS_ARG_CHECK(iters >= 0 && iters <= OSVOS_SUPERPIXELS_MAX_ITERS, "superpixels_slic: iters %d (0..%d)", iters, OSVOS_SUPERPIXELS_MAX_ITERS);
  OSVOS_ARG_CHECK((size_t)N * H * W <= ((size_t)1 << 38), "superpixels_slic: %d frames of %d x %d are more pixels than one call takes (2^38)", N, H, W);
  OSVOS_ARG_CHECK((uintptr_t)labels % 4 == 0 && (uintptr_t)centres % 4 == 0 && (uintptr_t)ws % 4 == 0,
                  "superpixels_slic: labels, centres and ws must be 4-byte aligned");
  const size_t pixels = (size_t)N * H * W, clusters = (size_t)N * ceil_div(H, cell) * ceil_div(W, cell);
  const size_t ws_bytes = clusters * 6 * 8;
  OSVOS_ARG_CHECK(!overlap(labels, pixels * 4, frames, pixels * 3) && !overlap(ws, ws_bytes, frames, pixels * 3) && !overlap(ws, ws_bytes, labels, pixels * 4),
                  "superpixels_slic: aliasing: frames, labels and ws must be three buffers");
  OSVOS_ARG_CHECK(!centres || (!overlap(centres, clusters * 24, frames, pixels * 3) && !overlap(centres, clusters * 24, labels, pixels * 4) &&
                               !overlap(centres, clusters * 24, ws, ws_bytes)),
                  "superpixels_slic: aliasing: centres must not overlap frames, labels or ws");

  Grid g;
  g.H = H; g.W = W; g.S = cell; g.m2 = compactness * compactness;
  g.GH = ceil_div(H, cell); g.GW = ceil_div(W, cell);
  unsigned* acc = (unsigned*)ws;
  int* work = (int*)(acc + clusters * 6);
  const dim3 tiles((unsigned)ceil_div(W, TW), (unsigned)ceil_div(H, TH), (unsigned)N), block(THREADS);
  const dim3 per_cluster((unsigned)((clusters + THREADS - 1) / THREADS));
  OSVOS_HIP_CHECK(hipMemsetAsync(acc, 0, clusters * 6 * sizeof(unsigned), stream));
  hipLaunchKernelGGL(assign_kernel<true>, tiles, block, 0, stream, frames, (const int*)work, labels, acc, g);
  OSVOS_LAUNCH_CHECK();
  hipLaunchKernelGGL(update_kernel, per_cluster, block, 0, stream, acc, work, iters == 0 ? centres : (int*)nullptr, clusters);
  OSVOS_LAUNCH_CHECK();
  for (int t = 1; t <= iters; ++t) {
    hipLaunchKernelGGL(assign_kernel<false>, tiles, block, 0, stream, frames, (const int*)work, labels, acc, g);
    OSVOS_LAUNCH_CHECK();
    hipLaunchKernelGGL(update_kernel, per_cluster, block, 0, stream, acc, work, t == iters ? centres : (int*)nullptr, clusters);
    OSVOS_LAUNCH_CHECK();
  }
  return 0;
}

// a 64-bit sum and a count per label
extern "C" size_t osvos_superpixels_pool_ws_bytes(int N, int K) {
  if (!pool_k_ok(N, K)) return 0;
  return (size_t)N * K * (sizeof(unsigned long long) + sizeof(unsigned));
}

extern "C" int osvos_superpixels_pool(const float* logits, const int* labels, float* out, void* ws, int N, int H, int W, int K, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(logits && labels && out && ws, "superpixels_pool: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "superpixels_pool: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(side_ok(H) && side_ok(W), "superpixels_pool: bad size H %d W %d (1..%d per side)", H, W, OSVOS_SUPERPIXELS_MAX_SIDE);
  OSVOS_ARG_CHECK(K >= 1 && K <= OSVOS_SUPERPIXELS_MAX_K, "superpixels_pool: K %d labels (1..%d)", K, OSVOS_SUPERPIXELS_MAX_K);
  OSVOS_ARG_CHECK((size_t)N * H * W <= ((size_t)1 << 38), "superpixels_pool: %d frames of %d x %d are more pixels than one call takes (2^38)", N, H, W);
  OSVOS_ARG_CHECK((uintptr_t)logits % 4 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)ws % 8 == 0,
                  "superpixels_pool: logits, labels and out must be 4-byte aligned, ws 8-byte aligned");
  const size_t pixels = (size_t)N * H * W, slots = (size_t)N * K;
  OSVOS_ARG_CHECK(!overlap(out, pixels * 4, logits, pixels * 4) && !overlap(out, pixels * 4, labels, pixels * 4),
                  "superpixels_pool: aliasing: out must not overlap logits or labels (the apply pass reads both)");
  OSVOS_ARG_CHECK(!overlap(ws, slots * 12, logits, pixels * 4) && !overlap(ws, slots * 12, labels, pixels * 4) && !overlap(ws, slots * 12, out, pixels * 4),
                  "superpixels_pool: aliasing: ws must not overlap logits, labels or out");

  unsigned long long* sums = (unsigned long long*)ws;
  unsigned* counts = (unsigned*)(sums + slots);
  OSVOS_HIP_CHECK(hipMemsetAsync(ws, 0, slots * 12, stream));
  const dim3 tiles((unsigned)ceil_div(W, TW), (unsigned)ceil_div(H, TH), (unsigned)N), block(THREADS);
  hipLaunchKernelGGL(pool_accumulate, tiles, block, 0, stream, logits, labels, sums, counts, H, W, K);
  OSVOS_LAUNCH_CHECK();
  const size_t per_image = (size_t)H * W;
  hipLaunchKernelGGL(pool_apply, dim3((unsigned)((per_image + THREADS - 1) / THREADS), (unsigned)N), block, 0, stream, (const unsigned*)logits, labels,
                     (const unsigned long long*)sums, (const unsigned*)counts, (unsigned*)out, per_image, K);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
