// DAVIS contour accuracy F next to the region measure J, from integer counts made on the device (the reference, train_online.py:181-189,
// writes PNGs and leaves both measures to the external DAVIS toolkit; osvos_mask_iou_counts in loss.hip is the J half).
//
//   P = logit > thr, G = gt > 0.5                                  (the two tests of mask_iou_kernel)
//   B(M)(y, x) = M differs from its right, lower or lower-right neighbour (last row: right only, last column: lower only, corner: never)
//   a pixel of B(P) is matched when B(G) has a pixel with dy*dy + dx*dx <= r*r (zeros outside the image), and the other way round
//   counts per frame: {|P & G|, |P | G|, |B(P)|, |B(G)|, matched of B(P), matched of B(G)};  the host forms J and F from them
//
// Two launches.  jf_pack_kernel reads the two float tensors ONCE: a wave takes 64 consecutive pixels of a row, __ballot turns the two tests
// into one 64-bit word each (bit i = pixel 64 k + i, bits past W are zero), popcounts give the J counts.  Only these bitmaps (1/32 of a float
// image each) live in HBM between the launches.  jf_match_kernel works on tiles of kTileRows x kTileWords words: it forms the BOUNDARY words of
// both maps for the tile plus a halo of r rows and one word on each side straight into LDS (word logic on four mask words; rows and words
// outside the image are zeros), then the non-empty boundary words of the tile are dealt to the waves in turn and a wave takes one word at a time -- lane i is pixel i of the word -- and walks
// dy = 0, +-1, .. +-r: the disk's half-width w(dy) = floor(sqrt(r*r - dy*dy)) turns the disk into the bit range [x - w, x + w] of row y + dy of
// the other map's boundary, at most three LDS words.  O(r) per boundary pixel, nothing per pixel that is not on a boundary, and the walk ends as
// soon as every pixel of the word has its match (a good mask matches at dy = 0).  Counts are wave-uniform popcounts, summed per workgroup,
// one 64-bit atomic add per workgroup and count: integer sums, so the result does not depend on the order.
#include "common.h"
#include "boundary.h"

namespace {

typedef unsigned long long u64;
constexpr int kMaxRadius = OSVOS_BOUNDARY_MAX_RADIUS;      // w(dy) <= 64: [x - w, x + w] stays inside the tile's one-word halo
constexpr int kTileRows = 8, kTileWords = 16;                   // small tiles: the walk of the busiest tile bounds the launch at one frame
constexpr int kMatchWaves = 8;
constexpr int kWinWords = kTileWords + 2;                   // LDS row stride of a boundary window (one halo word on each side)
static_assert(kMaxRadius <= 64, "the column halo is one word");

// grid (workgroups, N); bits: per frame the P bitmap then the G bitmap, H * wpr words each
__global__ __launch_bounds__(256) void jf_pack_kernel(const float* __restrict__ logits, const float* __restrict__ gt, int H, int W, int wpr, float thr,
                                                      u64* __restrict__ bits, u64* __restrict__ counts) {
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long words = (long)H * wpr;
  const float* __restrict__ x = logits + (size_t)n * H * W;
  const float* __restrict__ g = gt + (size_t)n * H * W;
  u64* __restrict__ pb = bits + (size_t)(2 * n) * words;
  u64* __restrict__ gb = pb + words;
  const long nw = (long)gridDim.x * 4;
  unsigned inter = 0, uni = 0;
  for (long base = (long)blockIdx.x * 4 + wave; base < words; base += 4 * nw) {      // four words in flight per wave
    float xv[4], gv[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long idx = base + u * nw;
      const long y = idx / wpr;
      const long col = (idx - y * wpr) * 64 + lane;
      ok[u] = idx < words && col < W;
      xv[u] = ok[u] ? x[y * W + col] : 0.f;
      gv[u] = ok[u] ? g[y * W + col] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long idx = base + u * nw;
      if (idx >= words) break;                                                         // (wave-uniform)
      const u64 p = __ballot(ok[u] && xv[u] > thr), q = __ballot(ok[u] && gv[u] > 0.5f);
      inter += __popcll(p & q);
      uni += __popcll(p | q);
      if (lane == 0) { pb[idx] = p; gb[idx] = q; }
    }
  }
  __shared__ unsigned red[4][2];
  if (lane == 0) { red[wave][0] = inter; red[wave][1] = uni; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned c = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (c) atomicAdd(&counts[6 * n + threadIdx.x], (u64)c);
  }
}

// word k of row y of B(M); zero outside the image
__device__ __forceinline__ u64 boundary_word(const u64* __restrict__ m, int y, int k, int H, int W, int wpr) {
  if (y < 0 || y >= H || k < 0 || k >= wpr) return 0ull;
  const u64* row = m + (size_t)y * wpr;
  const u64 c = row[k], cn = k + 1 < wpr ? row[k + 1] : 0ull;
  const u64 e = (c >> 1) | (cn << 63);                                                  // right neighbour
  const long lim = (long)(W - 1) - 64L * k;                                             // bits of this word with x < W - 1
  const u64 inner = lim >= 64 ? ~0ull : (lim <= 0 ? 0ull : (1ull << lim) - 1ull);
  if (y == H - 1) return (c ^ e) & inner;
  const u64 s = row[wpr + k], sn = k + 1 < wpr ? row[wpr + k + 1] : 0ull;
  const u64 se = (s >> 1) | (sn << 63);                                                 // lower-right neighbour
  return (((c ^ e) | (c ^ se)) & inner) | (c ^ s);                                      // (bits past W are zero in c and s)
}

// grid (row tiles * col_tiles, N); dynamic LDS: 2 maps x (kTileRows + 2 r) rows x kWinWords words
__global__ __launch_bounds__(64 * kMatchWaves) void jf_match_kernel(const u64* __restrict__ bits, int H, int W, int wpr, int r, int col_tiles,
                                                       u64* __restrict__ counts) {
  extern __shared__ u64 win[];
  __shared__ int wtab[kMaxRadius + 1];
  __shared__ unsigned red[kMatchWaves][4];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = (int)(blockIdx.x / col_tiles) * kTileRows, k0 = (int)(blockIdx.x % col_tiles) * kTileWords;
  const int rows = H - y0 < kTileRows ? H - y0 : kTileRows, tw = wpr - k0 < kTileWords ? wpr - k0 : kTileWords;
  const int wr = rows + 2 * r, ww = tw + 2;                                             // the part of the window this tile reads
  const int map_stride = (kTileRows + 2 * r) * kWinWords;
  const long words = (long)H * wpr;
  const u64* __restrict__ pb = bits + (size_t)(2 * n) * words;

  for (int i = threadIdx.x; i < 2 * wr * ww; i += blockDim.x) {
    const int map = i / (wr * ww), rem = i - map * (wr * ww), wy = rem / ww, wk = rem - wy * ww;
    win[map * map_stride + wy * kWinWords + wk] = boundary_word(pb + (size_t)map * words, y0 - r + wy, k0 - 1 + wk, H, W, wpr);
  }
  if ((int)threadIdx.x <= r) {
    const int d = threadIdx.x, t = r * r - d * d;
    int w = (int)sqrtf((float)t);
    while (w * w > t) --w;
    while ((w + 1) * (w + 1) <= t) ++w;
    wtab[d] = w;
  }
  __syncthreads();

  unsigned cnt[4] = {0, 0, 0, 0};                                                       // n_fb, n_gb, fb_match, gb_match (wave-uniform)
  const int per_map = rows * tw, total = 2 * per_map;
  int seen = 0;                                                                         // non-empty words so far: dealt to the waves in turn
  for (int chunk = 0; chunk < total; chunk += 64) {                                      // (every wave scans every word; only the walks are shared out)
    const int t = chunk + lane;
    u64 mine = 0ull;
    if (t < total) {
      const int map = t / per_map, rem = t - map * per_map, ty = rem / tw;
      mine = win[map * map_stride + (ty + r) * kWinWords + (rem - ty * tw) + 1];
    }
    u64 todo = __ballot(mine != 0ull);
    while (todo) {                                                                      // one non-empty boundary word per turn
      const int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      if ((seen++) % kMatchWaves != wave) continue;
      const u64 word = __shfl(mine, j, 64);
      const int tj = chunk + j, map = tj / per_map, rem = tj - map * per_map, ty = rem / tw, tk = rem - ty * tw;
      const u64* other = win + (1 - map) * map_stride + (ty + r) * kWinWords;
      const bool active = (word >> lane) & 1ull;
      const int xw = (tk + 1) * 64 + lane;                                               // bit position in the window row
      bool matched = false;
      for (int d = 0; d <= r; ++d) {
        const int w = wtab[d], xl = xw - w, xh = xw + w, a = xl >> 6, b = xh >> 6, sh = xl & 63;
        const u64 hm = ~0ull >> (63 - (xh & 63));
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          if (side == 1 && d == 0) break;
          const u64* row = other + (side ? -d : d) * kWinWords;
          const u64 va = row[a], vb = row[b];
          const u64 hit = a == b ? ((va & hm) >> sh) : ((va >> sh) | (vb & hm) | (b - a == 2 ? row[a + 1] : 0ull));
          matched |= hit != 0ull;
        }
        if (__ballot(active && !matched) == 0ull) break;
      }
      cnt[map] += __popcll(word);
      cnt[2 + map] += __popcll(__ballot(active && matched));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[wave][c] = cnt[c];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned c = 0;
#pragma unroll
    for (int v = 0; v < kMatchWaves; ++v) c += red[v][threadIdx.x];
    if (c) atomicAdd(&counts[6 * n + 2 + threadIdx.x], (u64)c);
  }
}

}  // namespace

// the match launch on `frames` bitmap pairs (boundary.h); the callers have checked frames <= 65535 and the radius
int osvos_jf_match(const char* who, const unsigned long long* bits, unsigned long long* counts, int frames, int H, int W, int radius, hipStream_t stream) {
  const int wpr = (W + 63) / 64;
  const int col_tiles = ceil_div(wpr, kTileWords);
  const long tiles = (long)ceil_div(H, kTileRows) * col_tiles;
  OSVOS_ARG_CHECK(tiles <= 0x7fffffffL, "%s: %d x %d is too large", who, H, W);
  const size_t lds = sizeof(u64) * 2 * (kTileRows + 2 * radius) * kWinWords;             // 7 KB at r = 8, 39 KB at r = 64
  hipLaunchKernelGGL(jf_match_kernel, dim3((unsigned)tiles, (unsigned)frames), dim3(64 * kMatchWaves), lds, stream, bits, H, W, wpr, radius, col_tiles,
                     counts);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t osvos_boundary_ws_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  return (size_t)2 * N * H * ((W + 63) / 64) * sizeof(u64);
}

extern "C" int osvos_mask_jf_counts(const float* logits, const float* gt, void* ws, void* counts, int N, int H, int W, float logit_threshold,
                                    int radius, int accumulate, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(logits && gt && ws && counts, "mask_jf_counts: null pointer");
  OSVOS_ARG_CHECK(((uintptr_t)ws | (uintptr_t)counts) % 8 == 0, "mask_jf_counts: ws and counts must be 8-byte aligned");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "mask_jf_counts: bad size N %d H %d W %d", N, H, W);
  OSVOS_ARG_CHECK(radius >= 1 && radius <= kMaxRadius, "mask_jf_counts: radius %d (1..%d pixels)", radius, kMaxRadius);
  const int wpr = (W + 63) / 64;
  const long words = (long)H * wpr;
  u64* c = reinterpret_cast<u64*>(counts);
  u64* bits = reinterpret_cast<u64*>(ws);
  if (!accumulate) OSVOS_HIP_CHECK(hipMemsetAsync(c, 0, sizeof(u64) * 6 * N, stream));
  long g = (words + 15) / 16;                                                           // >= 4 words per wave
  g = g > 1024 ? 1024 : g;
  hipLaunchKernelGGL(jf_pack_kernel, dim3((unsigned)g, (unsigned)N), dim3(256), 0, stream, logits, gt, H, W, wpr, logit_threshold, bits, c);
  OSVOS_LAUNCH_CHECK();
  return osvos_jf_match("mask_jf_counts", bits, c, N, H, W, radius, stream);
}
