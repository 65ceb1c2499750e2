// Interactive scribbles (Scribble-OSVOS, the baseline of the DAVIS interactive track): strokes become a label map, an error region becomes
// a stroke (include/osvos_hip.h, "interactive scribbles", states both rules).
//
//   osvos_scribble_raster   segs int32 [M][6] = (x0, y0, x1, y1, value, frame) -> uint8 [N][H][W]: 255 where no segment of the frame covers
//                           the pixel, else the value of the covering row with the highest index.
//   osvos_mask_thin         bytes [N][H][W] (non-zero = set) -> the Guo-Hall skeleton, bytes in {0, 1}, and info [N][2] = (iterations run,
//                           1 if the last one deleted nothing).
//
// Raster: one workgroup per 64 x 16 pixel tile and frame, four pixels per thread.  The workgroup walks segs from the HIGHEST index down in
// chunks of 256 rows, one row per lane: a row survives the cull when it belongs to the frame and its box, grown by r, meets the tile.  Each
// wave's ballot and the popcount of the ballot below a lane give the survivor its place, so the LDS list holds the survivors in descending
// index order; a pixel walks the list from its start and stops at its first hit, which is the covering row of the highest index.  The list
// holds kListCap rows: when the next chunk might not fit it is tested and emptied first (a "pass"), so no row is ever dropped, and a pass
// after which every pixel of the tile is decided ends the walk.  No atomics, the same bytes every run.  The coverage test is the header's,
// in signed 64-bit integers.
//
// Thinning works on a 1-bit plane, 64 pixels per word (bit i of word k of a row = column 64 k + i), built with the wave ballot.  The rule is
// bitwise logic on whole words: east and west neighbours are one-bit shifts with the carry of the adjacent word, "C == 1" and
// "2 <= min(N1, N2) <= 3" are sums of four one-bit terms taken pairwise (gh_word, the one place the rule is written).
//   Path 1, resident: the plane of a frame fits in LDS (at most kResidentWords words); ONE workgroup of 1024 threads per frame keeps it
//     there.  A sub-step: every thread computes its up to 8 words from the plane into registers, barrier, stores them, barrier.  The OR of
//     "a word changed" over the workgroup ends the loop.  No launch per iteration, no workgroup waits for another.
//   Path 2, global: two planes ping-pong in the workspace.  One launch per iteration: a workgroup takes a band of kBandRows rows over the
//     whole width with two halo rows on either side in LDS, runs sub-step 0 on the band and one halo row, then sub-step 1 on the band -- the
//     bytes of two separate passes.  A workgroup that deleted a pixel of its own rows stores 1 into changed[frame][iteration] (every writer
//     stores the same value: no atomic); the launch of iteration i returns at once for a frame whose changed[i - 1] is 0.  An iteration
//     that deletes nothing writes its input, so from then on both planes of the frame are equal and stay so.  The host enqueues max_iters
//     launches and reads nothing back.
// Bits past column W - 1 are never set: the pack leaves them 0 and the rule only clears bits.
#include "common.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

__device__ __forceinline__ int lanes_below(u64 ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

// ---------------------------------------------------------------- raster ----------------------------------------------------------------

constexpr int kTileW = 64, kTileH = 16, kChunk = 256, kListCap = OSVOS_SCRIBBLE_LIST_CAP;
static_assert(kListCap >= kChunk, "a chunk must fit the empty list");

struct Seg {
  int x0, y0, x1, y1, value;
};

// the coverage rule of include/osvos_hip.h; coordinates are below 2^14, so (w x d)^2 < 2^58 and r^2 L < 2^42
__device__ __forceinline__ bool seg_covers(const Seg s, int px, int py, i64 r2) {
  const i64 dx = s.x1 - s.x0, dy = s.y1 - s.y0, wx = px - s.x0, wy = py - s.y0;
  const i64 L = dx * dx + dy * dy, t = wx * dx + wy * dy;
  if (L == 0 || t <= 0) return wx * wx + wy * wy <= r2;
  if (t >= L) {
    const i64 ex = px - s.x1, ey = py - s.y1;
    return ex * ex + ey * ey <= r2;
  }
  const i64 c = wx * dy - wy * dx;
  return c * c <= r2 * L;
}

// grid (ceil(W / 64), ceil(H / 16), N), block 256
__global__ __launch_bounds__(256) void scribble_raster_kernel(const int* __restrict__ segs, int M, unsigned char* __restrict__ out, int H, int W,
                                                              int radius) {
  __shared__ Seg sList[kListCap];
  __shared__ int sWave[4];
  const int t = threadIdx.x, lane = t % 64, wave = t / 64, n = blockIdx.z;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int px = tx0 + lane;
  const i64 r2 = (i64)radius * radius;
  int value[4] = {255, 255, 255, 255};
  bool done[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) done[j] = px >= W || ty0 + wave + 4 * j >= H;      // pixels outside the frame have nothing to decide
  int count = 0;
  for (int hi = M; hi > 0; hi -= kChunk) {
    const int row = hi - 1 - t;                                                   // descending: lane order is list order
    bool keep = false;
    Seg s = {0, 0, 0, 0, 0};
    if (row >= 0) {
      const int* __restrict__ p = segs + (size_t)row * 6;
      s.x0 = p[0]; s.y0 = p[1]; s.x1 = p[2]; s.y1 = p[3]; s.value = p[4];
      keep = p[5] == n && max(s.x0, s.x1) + radius >= tx0 && min(s.x0, s.x1) - radius < tx0 + kTileW && max(s.y0, s.y1) + radius >= ty0 &&
             min(s.y0, s.y1) - radius < ty0 + kTileH;
    }
    const u64 ballot = __ballot(keep);
    if (lane == 0) sWave[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = sWave[w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (keep) sList[count + before + lanes_below(ballot, lane)] = s;
    count += all;
    __syncthreads();
    if (count + kChunk <= kListCap && hi > kChunk) continue;                      // (uniform) room for the next chunk: gather on
    for (int i = 0; i < count; ++i) {
      const Seg c = sList[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!done[j] && seg_covers(c, px, ty0 + wave + 4 * j, r2)) {
          value[j] = c.value;
          done[j] = true;
        }
      }
    }
    count = 0;
    if (__syncthreads_and(done[0] && done[1] && done[2] && done[3])) break;       // (also the barrier between this pass's reads and the next writes)
  }
  if (px < W) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = ty0 + wave + 4 * j;
      if (y < H) out[((size_t)n * H + y) * W + px] = (unsigned char)value[j];
    }
  }
}

// --------------------------------------------------------------- thinning ---------------------------------------------------------------

constexpr int kResidentThreads = 1024, kResidentPerThread = 8, kResidentWords = OSVOS_THIN_RESIDENT_WORDS;
constexpr int kBandRows = 8, kBandHalo = 2, kMaxIters = OSVOS_THIN_MAX_ITERS;
static_assert(kResidentWords <= kResidentThreads * kResidentPerThread && kResidentWords * 8 <= 65536 - 256, "the resident plane must fit LDS");

struct Row3 {
  u64 w, c, e;      // per bit: the pixel's west neighbour, the pixel, its east neighbour
};

// prev / cur / next: words k - 1, k, k + 1 of one row (0 outside the frame); bit i of a word is column 64 k + i
__device__ __forceinline__ Row3 row3(u64 prev, u64 cur, u64 next) {
  Row3 r;
  r.c = cur;
  r.w = (cur << 1) | (prev >> 63);
  r.e = (cur >> 1) | (next << 63);
  return r;
}

__device__ __forceinline__ u64 two_or_more(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// one Guo-Hall sub-step on the 64 pixels of a word: n, c, s = the rows above, of and below the word -> the word afterwards
__device__ __forceinline__ u64 gh_word(const Row3 n, const Row3 c, const Row3 s, int sub) {
  const u64 P2 = n.c, P3 = n.e, P4 = c.e, P5 = s.e, P6 = s.c, P7 = s.w, P8 = c.w, P9 = n.w;
  const u64 a1 = ~P2 & (P3 | P4), a2 = ~P4 & (P5 | P6), a3 = ~P6 & (P7 | P8), a4 = ~P8 & (P9 | P2);
  const u64 c_is_1 = ((a1 ^ a2) ^ (a3 ^ a4)) & ~(a1 & a2) & ~(a3 & a4);
  const u64 b1 = P9 | P2, b2 = P3 | P4, b3 = P5 | P6, b4 = P7 | P8;
  const u64 d1 = P2 | P3, d2 = P4 | P5, d3 = P6 | P7, d4 = P8 | P9;
  // 2 <= min(N1, N2) <= 3: both sums are at least 2 and they are not both 4
  const u64 nm_ok = two_or_more(b1, b2, b3, b4) & two_or_more(d1, d2, d3, d4) & ~(b1 & b2 & b3 & b4 & d1 & d2 & d3 & d4);
  const u64 side = sub == 0 ? (P2 | P3 | ~P5) & P4 : (P6 | P7 | ~P9) & P8;
  return c.c & ~(c_is_1 & nm_ok & ~side);
}

// the word (y, k) of a plane of H rows of WPR words after sub-step `sub`; rows and words outside the plane read as 0.  The rule only
// clears bits, so an empty word -- most words of most masks -- stays empty without a look at its neighbours.
template <typename Plane>
__device__ __forceinline__ u64 gh_at(const Plane& p, int y, int k, int H, int WPR, int sub) {
  if (p(y, k) == 0ull) return 0ull;
  Row3 r[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int yy = y + d - 1;
    const bool in = yy >= 0 && yy < H;
    const u64 prev = in && k > 0 ? p(yy, k - 1) : 0ull, cur = in ? p(yy, k) : 0ull, next = in && k + 1 < WPR ? p(yy, k + 1) : 0ull;
    r[d] = row3(prev, cur, next);
  }
  return gh_word(r[0], r[1], r[2], sub);
}

struct LdsPlane {
  const u64* w;
  int WPR;
  __device__ __forceinline__ u64 operator()(int y, int k) const { return w[y * WPR + k]; }
};

// Path 1.  grid N, block 1024; H WPR <= kResidentWords
__global__ __launch_bounds__(kResidentThreads) void thin_resident_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ out,
                                                                         int* __restrict__ info, int H, int W, int WPR, int max_iters) {
  __shared__ u64 sPlane[kResidentWords];
  const int t = threadIdx.x, lane = t % 64, wave = t / 64, n = blockIdx.x, words = H * WPR;
  const unsigned char* __restrict__ m = mask + (size_t)n * H * W;
  // a wave takes rows wave, wave + 16, ..: kLoadWords words of a row per step, their loads in flight together (wave-uniform: all 64 lanes
  // reach every ballot)
  constexpr int kLoadWords = 16;
  for (int y = wave; y < H; y += kResidentThreads / 64) {
    const unsigned char* __restrict__ row = m + (size_t)y * W;
    for (int k0 = 0; k0 < WPR; k0 += kLoadWords) {
      unsigned char b[kLoadWords];
#pragma unroll
      for (int u = 0; u < kLoadWords; ++u) {
        const int x = (k0 + u) * 64 + lane;
        b[u] = x < W ? row[x] : (unsigned char)0;
      }
#pragma unroll
      for (int u = 0; u < kLoadWords; ++u) {
        const u64 word = __ballot(b[u] != 0);
        if (lane == 0 && k0 + u < WPR) sPlane[y * WPR + k0 + u] = word;
      }
    }
  }
  __syncthreads();
  const LdsPlane plane = {sPlane, WPR};
  int ys[kResidentPerThread], ks[kResidentPerThread];                              // this thread's words: one division each, once
#pragma unroll
  for (int j = 0; j < kResidentPerThread; ++j) {
    const int item = min(t + kResidentThreads * j, words - 1);
    ys[j] = item / WPR;
    ks[j] = item - ys[j] * WPR;
  }
  int iters = 0, still = 0;
  while (iters < max_iters) {
    bool changed = false;
    for (int sub = 0; sub < 2; ++sub) {
      u64 next[kResidentPerThread];
#pragma unroll
      for (int j = 0; j < kResidentPerThread; ++j) {
        const int item = t + kResidentThreads * j;
        if (item < words) {
          next[j] = gh_at(plane, ys[j], ks[j], H, WPR, sub);
          changed |= next[j] != sPlane[item];
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kResidentPerThread; ++j) {
        const int item = t + kResidentThreads * j;
        if (item < words) sPlane[item] = next[j];
      }
      __syncthreads();
    }
    ++iters;
    if (!__syncthreads_or(changed)) {
      still = 1;
      break;
    }
  }
  unsigned char* __restrict__ o = out + (size_t)n * H * W;
  for (int y = wave; y < H; y += kResidentThreads / 64) {                          // a wave per row, a lane per bit of a word
    for (int k = 0; k < WPR; ++k) {
      const int x = k * 64 + lane;
      if (x < W) o[(size_t)y * W + x] = (unsigned char)((sPlane[y * WPR + k] >> lane) & 1ull);
    }
  }
  if (t == 0) {
    info[2 * n] = iters;
    info[2 * n + 1] = still;
  }
}

// Path 2.  grid (ceil(H WPR / 4), N), block 256: a wave per word
__global__ __launch_bounds__(256) void thin_pack_kernel(const unsigned char* __restrict__ mask, u64* __restrict__ plane, int H, int W, int WPR) {
  const int lane = threadIdx.x % 64, item = blockIdx.x * 4 + threadIdx.x / 64, n = blockIdx.y;
  if (item >= H * WPR) return;                                                     // (wave-uniform)
  const int y = item / WPR, x = (item - y * WPR) * 64 + lane;
  const u64 word = __ballot(x < W && mask[((size_t)n * H + y) * W + x] != 0);
  if (lane == 0) plane[(size_t)n * H * WPR + item] = word;
}

struct BandPlane {
  const u64* w;      // rows y_first .. of the frame, WPR words each
  int WPR, y_first;
  __device__ __forceinline__ u64 operator()(int y, int k) const { return w[(y - y_first) * WPR + k]; }
};

// One iteration.  grid (ceil(H / kBandRows), N), block 256, dynamic LDS (2 kBandRows + 3 kBandHalo) WPR words:
//   sIn  rows y0 - 2 .. y0 + kBandRows + 1 of the source plane (rows outside the frame as 0), sMid rows y0 - 1 .. y0 + kBandRows after sub-step 0
__global__ __launch_bounds__(256) void thin_band_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int* __restrict__ changed, int H, int WPR,
                                                        int iter) {
  extern __shared__ u64 sBand[];
  const int n = blockIdx.y, t = threadIdx.x, y0 = blockIdx.x * kBandRows;
  int* __restrict__ ch = changed + (size_t)n * kMaxIters;
  if (iter > 0 && ch[iter - 1] == 0) return;                                       // (uniform) the frame has stopped: both planes hold its result
  const u64* __restrict__ s = src + (size_t)n * H * WPR;
  u64* __restrict__ d = dst + (size_t)n * H * WPR;
  u64* sIn = sBand;
  u64* sMid = sBand + (kBandRows + 2 * kBandHalo) * WPR;
  for (int i = t; i < (kBandRows + 2 * kBandHalo) * WPR; i += 256) {
    const int y = y0 - kBandHalo + i / WPR;
    sIn[i] = y >= 0 && y < H ? s[(size_t)y * WPR + i % WPR] : 0ull;
  }
  __syncthreads();
  bool deleted = false;
  const BandPlane in = {sIn, WPR, y0 - kBandHalo};
  for (int i = t; i < (kBandRows + 2) * WPR; i += 256) {
    const int y = y0 - 1 + i / WPR, k = i % WPR;
    u64 v = 0ull;
    if (y >= 0 && y < H) {
      v = gh_at(in, y, k, H, WPR, 0);
      deleted |= y >= y0 && y < y0 + kBandRows && v != in(y, k);                   // a halo row's deletions are its own band's to report
    }
    sMid[i] = v;
  }
  __syncthreads();
  const BandPlane mid = {sMid, WPR, y0 - 1};
  for (int i = t; i < kBandRows * WPR; i += 256) {
    const int y = y0 + i / WPR, k = i % WPR;
    if (y < H) {
      const u64 v = gh_at(mid, y, k, H, WPR, 1);
      deleted |= v != mid(y, k);
      d[(size_t)y * WPR + k] = v;
    }
  }
  if (__syncthreads_or(deleted) && t == 0) ch[iter] = 1;
}

// grid (ceil(W / 256), H, N), block 256; the block (0, 0, n) also writes the frame's info
__global__ __launch_bounds__(256) void thin_unpack_kernel(const u64* __restrict__ plane, const int* __restrict__ changed, unsigned char* __restrict__ out,
                                                          int* __restrict__ info, int H, int W, int WPR, int max_iters) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x < W) out[((size_t)n * H + y) * W + x] = (unsigned char)((plane[((size_t)n * H + y) * WPR + x / 64] >> (x % 64)) & 1ull);
  if (blockIdx.x == 0 && y == 0 && threadIdx.x == 0) {
    const int* __restrict__ ch = changed + (size_t)n * kMaxIters;
    int deleting = 0;                                                              // changed is 1, .., 1, 0, .., 0
    while (deleting < max_iters && ch[deleting] != 0) ++deleting;
    const int iters = min(deleting + 1, max_iters);
    info[2 * n] = iters;
    info[2 * n + 1] = ch[iters - 1] == 0 ? 1 : 0;
  }
}

bool thin_sizes_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384; }
size_t thin_plane_words(int N, int H, int W) { return (size_t)N * H * ((W + 63) / 64); }

}  // namespace

// segs: device int32 [M][6] (may be null when M is 0); out: device uint8 [N][H][W]
extern "C" int osvos_scribble_raster(const int* segs, int M, unsigned char* out, int N, int H, int W, int radius, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(out && (segs || M == 0), "scribble_raster: null pointer");
  OSVOS_ARG_CHECK(M >= 0 && M <= OSVOS_SCRIBBLE_MAX_SEGMENTS, "scribble_raster: %d segments (0..%d)", M, OSVOS_SCRIBBLE_MAX_SEGMENTS);
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "scribble_raster: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "scribble_raster: bad size H %d W %d (1..16384 per side)", H, W);
  OSVOS_ARG_CHECK(radius >= 0 && radius <= OSVOS_SCRIBBLE_MAX_RADIUS, "scribble_raster: radius %d (0..%d)", radius, OSVOS_SCRIBBLE_MAX_RADIUS);
  OSVOS_ARG_CHECK((uintptr_t)segs % 4 == 0, "scribble_raster: segs must be 4-byte aligned");
  const dim3 grid((unsigned)ceil_div(W, kTileW), (unsigned)ceil_div(H, kTileH), (unsigned)N);
  hipLaunchKernelGGL(scribble_raster_kernel, grid, dim3(256), 0, stream, segs, M, out, H, W, radius);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t osvos_mask_thin_ws_bytes(int N, int H, int W) {
  if (!thin_sizes_ok(N, H, W)) return 0;
  return 2 * thin_plane_words(N, H, W) * sizeof(u64) + (size_t)N * kMaxIters * sizeof(int);
}

// mask, out: device bytes [N][H][W] (out may be mask); info: device int32 [N][2]; ws: device, osvos_mask_thin_ws_bytes(N, H, W) bytes, 8-byte aligned
extern "C" int osvos_mask_thin(const unsigned char* mask, unsigned char* out, int* info, int N, int H, int W, int max_iters, int path, void* ws,
                               void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(mask && out && info && ws, "mask_thin: null pointer");
  OSVOS_ARG_CHECK(thin_sizes_ok(N, H, W), "mask_thin: N %d frames (1..65535) of H %d W %d (1..16384 per side)", N, H, W);
  OSVOS_ARG_CHECK(max_iters >= 1 && max_iters <= kMaxIters, "mask_thin: max_iters %d (1..%d)", max_iters, kMaxIters);
  OSVOS_ARG_CHECK(path >= 0 && path <= 2, "mask_thin: path %d (0 automatic, 1 resident, 2 global)", path);
  OSVOS_ARG_CHECK((uintptr_t)info % 4 == 0 && (uintptr_t)ws % 8 == 0, "mask_thin: info must be 4-byte and ws 8-byte aligned");
  const int WPR = (W + 63) / 64;
  const bool fits = (size_t)H * WPR <= (size_t)kResidentWords;
  OSVOS_ARG_CHECK(path != 1 || fits, "mask_thin: path 1 keeps the plane in LDS: %d x %d is %zu words, more than %d", H, W, (size_t)H * WPR,
                  kResidentWords);
  if (path == 1 || (path == 0 && fits)) {
    hipLaunchKernelGGL(thin_resident_kernel, dim3((unsigned)N), dim3(kResidentThreads), 0, stream, mask, out, info, H, W, WPR, max_iters);
    OSVOS_LAUNCH_CHECK();
    return 0;
  }
  const size_t words = thin_plane_words(N, H, W);
  u64* planes[2] = {(u64*)ws, (u64*)ws + words};
  int* changed = (int*)((u64*)ws + 2 * words);
  OSVOS_HIP_CHECK(hipMemsetAsync(changed, 0, (size_t)N * kMaxIters * sizeof(int), stream));
  hipLaunchKernelGGL(thin_pack_kernel, dim3((unsigned)ceil_div(H * WPR, 4), (unsigned)N), dim3(256), 0, stream, mask, planes[0], H, W, WPR);
  OSVOS_LAUNCH_CHECK();
  const size_t lds = (size_t)(2 * kBandRows + 3 * kBandHalo) * WPR * sizeof(u64);
  for (int it = 0; it < max_iters; ++it) {
    hipLaunchKernelGGL(thin_band_kernel, dim3((unsigned)ceil_div(H, kBandRows), (unsigned)N), dim3(256), lds, stream, planes[it & 1], planes[(it + 1) & 1],
                       changed, H, WPR, it);
    OSVOS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(thin_unpack_kernel, dim3((unsigned)ceil_div(W, 256), (unsigned)H, (unsigned)N), dim3(256), 0, stream, planes[max_iters & 1], changed, out,
                     info, H, W, WPR, max_iters);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
