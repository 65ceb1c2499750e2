// Multi-object results (DAVIS 2017): K per-object networks -> one label map per frame, and J / F per object from two label maps.
//
//   osvos_merge_objects     label = 0 when m > thr is false, else 1 + the lowest k with logits[k] == m, where m = max_k logits[k] is fmax's
//                           maximum (a NaN logit never wins; a pixel whose K logits are all NaN is background).  On logits, never on a sigmoid:
//                           the sigmoid is monotone, so the winner and the threshold test are the same, and ties stay exact.
//   osvos_labels_jf_counts  for every frame n and object id k = 1..K the six counts of osvos_mask_jf_counts (boundary.hip) with P = (pred == k),
//                           G = (gt == k); label 0 and labels above K belong to no object.
//
// merge_objects_kernel: lane i of a wave takes pixels 4 i .. 4 i + 3 of the flat [N H W] plane, so one load instruction of a wave is 1 KB of
// consecutive floats (eight whole 128-byte lines) per object plane, and one store instruction is 256 consecutive label bytes; every logit is
// read once, the running maximum and its index live in registers.  (The plane stride N H W must be a multiple of 4 for the 16-byte loads of
// planes 1.. to be aligned -- true of every DAVIS size; other sizes take the one-pixel-per-lane form of the same loop.)
// labels_pack_kernel: the two byte maps are read once, a wave takes 64 consecutive pixels of a row (four such words in flight); the 2 K ballots
// of a word are handed to lanes 0 .. K-1 (lane k keeps P_k and G_k), which then own object k: its two popcounts for J, and its two 8-byte
// stores into the bitmaps.  The bitmaps are laid out as jf_match_kernel reads them -- "frame" n K + k holds the P map of object k + 1 of
// frame n, then its G map -- so the match runs unchanged on N K frames (boundary.h), and its counts land in row n K + k of [N][K][6].
#include "common.h"
#include "boundary.h"

namespace {

typedef unsigned long long u64;

template <bool VEC>
__global__ __launch_bounds__(256) void merge_objects_kernel(const float* __restrict__ logits, unsigned char* __restrict__ labels, long total, int K,
                                                            float thr) {
  constexpr int PX = VEC ? 4 : 1;
  const long groups = total / PX, step = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += step) {
    float m[PX];
    unsigned l[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) { m[j] = -INFINITY; l[j] = 0u; }
    const float* __restrict__ x = logits + i * PX;
#pragma unroll 4
    for (int k = 0; k < K; ++k, x += total) {
      float v[PX];
      if constexpr (VEC) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(x);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      } else {
        v[0] = x[0];
      }
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (v[j] > m[j]) { m[j] = v[j]; l[j] = (unsigned)(k + 1); }                       // strict: the lowest index keeps a tie; NaN never wins
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) l[j] = m[j] > thr ? l[j] : 0u;
    if constexpr (VEC)
      *reinterpret_cast<unsigned*>(labels + i * 4) = l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24);
    else
      labels[i] = (unsigned char)l[0];
  }
}

// grid (workgroups, N); bits: per frame and object the P bitmap then the G bitmap, H * wpr words each
__global__ __launch_bounds__(256) void labels_pack_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt, int H, int W,
                                                          int wpr, int K, u64* __restrict__ bits, u64* __restrict__ counts) {
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long words = (long)H * wpr;
  const unsigned char* __restrict__ p = pred + (size_t)n * H * W;
  const unsigned char* __restrict__ g = gt + (size_t)n * H * W;
  u64* __restrict__ mine = bits + ((size_t)n * K + lane) * 2 * words;                      // (lanes < K only) P map of object lane + 1, G map behind it
  const long nw = (long)gridDim.x * 4;
  unsigned inter = 0, uni = 0;                                                            // of object lane + 1
  for (long base = (long)blockIdx.x * 4 + wave; base < words; base += 4 * nw) {           // four words in flight per wave
    unsigned pv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long idx = base + u * nw;
      const long y = idx / wpr;
      const long col = (idx - y * wpr) * 64 + lane;
      const bool ok = idx < words && col < W;
      pv[u] = ok ? p[y * W + col] : 0u;                                                   // label 0 is nobody's: bits past W are zero
      gv[u] = ok ? g[y * W + col] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long idx = base + u * nw;
      if (idx >= words) break;                                                             // (wave-uniform)
      u64 pw = 0ull, gw = 0ull;
      if (__ballot((pv[u] | gv[u]) != 0u) != 0ull) {                                      // (a word of background needs no ballots)
        for (int k = 0; k < K; ++k) {
          const u64 bp = __ballot(pv[u] == (unsigned)(k + 1)), bg = __ballot(gv[u] == (unsigned)(k + 1));
          if (lane == k) { pw = bp; gw = bg; }
        }
      }
      if (lane < K) {
        inter += __popcll(pw & gw);
        uni += __popcll(pw | gw);
        mine[idx] = pw;
        mine[words + idx] = gw;
      }
    }
  }
  __shared__ unsigned red[4][OSVOS_MAX_OBJECTS][2];
  if (lane < K) { red[wave][lane][0] = inter; red[wave][lane][1] = uni; }
  __syncthreads();
  if ((int)threadIdx.x < 2 * K) {
    const int k = threadIdx.x >> 1, c = threadIdx.x & 1;
    const unsigned s = red[0][k][c] + red[1][k][c] + red[2][k][c] + red[3][k][c];
    if (s) atomicAdd(&counts[6 * ((size_t)n * K + k) + c], (u64)s);
  }
}

}  // namespace

extern "C" int osvos_merge_objects(const float* logits, unsigned char* labels, int N, int K, int H, int W, float logit_threshold, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(logits && labels, "merge_objects: null pointer");
  OSVOS_ARG_CHECK((uintptr_t)logits % 4 == 0, "merge_objects: logits must be 4-byte aligned");
  OSVOS_ARG_CHECK(N >= 1 && H >= 1 && W >= 1, "merge_objects: bad size N %d H %d W %d", N, H, W);
  OSVOS_ARG_CHECK(K >= 1 && K <= OSVOS_MAX_OBJECTS, "merge_objects: K %d objects (1..%d)", K, OSVOS_MAX_OBJECTS);
  const long total = (long)N * H * W;
  const bool vec = total % 4 == 0 && (uintptr_t)logits % 16 == 0 && (uintptr_t)labels % 4 == 0;
  const long groups = vec ? total / 4 : total;
  long g = (groups + 255) / 256;
  g = g > 2048 ? 2048 : g;
  if (vec)
    hipLaunchKernelGGL(merge_objects_kernel<true>, dim3((unsigned)g), dim3(256), 0, stream, logits, labels, total, K, logit_threshold);
  else
    hipLaunchKernelGGL(merge_objects_kernel<false>, dim3((unsigned)g), dim3(256), 0, stream, logits, labels, total, K, logit_threshold);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t osvos_labels_jf_ws_bytes(int N, int K, int H, int W) {
  if (N < 1 || K < 1 || K > OSVOS_MAX_OBJECTS || H < 1 || W < 1) return 0;
  return (size_t)2 * N * K * H * ((W + 63) / 64) * sizeof(u64);
}

extern "C" int osvos_labels_jf_counts(const unsigned char* pred, const unsigned char* gt, void* ws, void* counts, int N, int K, int H, int W, int radius,
                                      int accumulate, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(pred && gt && ws && counts, "labels_jf_counts: null pointer");
  OSVOS_ARG_CHECK(((uintptr_t)ws | (uintptr_t)counts) % 8 == 0, "labels_jf_counts: ws and counts must be 8-byte aligned");
  OSVOS_ARG_CHECK(N >= 1 && H >= 1 && W >= 1, "labels_jf_counts: bad size N %d H %d W %d", N, H, W);
  OSVOS_ARG_CHECK(K >= 1 && K <= OSVOS_MAX_OBJECTS, "labels_jf_counts: K %d objects (1..%d)", K, OSVOS_MAX_OBJECTS);
  OSVOS_ARG_CHECK((long)N * K <= 65535, "labels_jf_counts: N * K = %ld frame-objects per call (at most 65535)", (long)N * K);
  OSVOS_ARG_CHECK(radius >= 1 && radius <= OSVOS_BOUNDARY_MAX_RADIUS, "labels_jf_counts: radius %d (1..%d pixels)", radius, OSVOS_BOUNDARY_MAX_RADIUS);
  const int wpr = (W + 63) / 64;
  const long words = (long)H * wpr;
  u64* c = reinterpret_cast<u64*>(counts);
  u64* bits = reinterpret_cast<u64*>(ws);
  if (!accumulate) OSVOS_HIP_CHECK(hipMemsetAsync(c, 0, sizeof(u64) * 6 * N * K, stream));
  long g = (words + 15) / 16;                                                             // >= 4 words per wave
  g = g > 1024 ? 1024 : g;
  hipLaunchKernelGGL(labels_pack_kernel, dim3((unsigned)g, (unsigned)N), dim3(256), 0, stream, pred, gt, H, W, wpr, K, bits, c);
  OSVOS_LAUNCH_CHECK();
  return osvos_jf_match("labels_jf_counts", bits, c, N * K, H, W, radius, stream);
}
