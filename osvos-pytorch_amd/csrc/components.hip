// Connected components of the thresholded mask, and the selection (area / largest / seed tracking) every practical OSVOS pipeline runs between
// the logits and the result writers.  Integers with one right answer: nothing here depends on the order in which workgroups run.
//
//   P = logit > thr (jf_pack_kernel's test: a NaN is background); a component is a maximal 4- or 8-connected subset of P inside ONE frame
//   labels = 0 off P, else 1 + the lowest flat index y W + x of the component;  area = the pixel count at that root pixel, 0 elsewhere
//   stats[n] = {components, |P|, largest area, label of the largest (lowest label on a tie, 0 when there is none)}
//
// Union-find over pixels with union-by-minimum-index: a parent is never larger than its child, so the root of a set IS its canonical label.
// `labels` itself is the parent array (1 + parent index).  osvos_mask_components is five launches on the caller's stream:
//   cc_tile_kernel     a workgroup takes a 64 x 32 tile; a wave loads 64 consecutive floats of a row per request, __ballot makes the row's
//                      mask word, horizontal runs are resolved from the word (a pixel starts as its run's first pixel), the runs of
//                      neighbouring rows are united in LDS, and the tile writes tile-rooted labels and the tile-local pixel count at each
//                      tile root (zeros elsewhere): nothing is assumed zero on entry.
//   cc_border_kernel   one thread per pixel next to a tile edge unites it with its neighbours across the edge (atomicMin).
//   cc_flatten_kernel  every foreground pixel walks to its root and takes it as its label; a former tile root hands its count to the root.
//   cc_stats_kernel    integer sums per frame, and ONE 64-bit atomicMax of (area << 32) | ~label: the largest area, lowest label on a tie.
//   cc_stats_final     unpacks that word into stats[2], stats[3].
// No workgroup ever waits for another: no flags, no spins, no grid-wide barrier.  The only loops that touch words other workgroups write are
// find (a parent chain strictly descends) and unite (the larger of its two indices strictly descends), so both end.  Such words are read with
// agent-scope atomic loads and changed only by atomicMin; a stale read is an older ancestor of the same set, which costs steps, never the
// result: a lost race shows in atomicMin's return value and the link is made again from there.  What needs the final state of a phase is
// the next launch.
//
// osvos_components_select: the seed map is packed into one bit per pixel (seed_pack_kernel), every foreground pixel looks for a seed bit in
// the disk dy*dy + dx*dx <= r*r -- per dy the bit range [x - w(dy), x + w(dy)] of row y + dy, jf_match_kernel's disk -- and raises its
// component's flag word (seed_mark_kernel; pixels of a component that is already flagged stop at once), select_apply_kernel writes kept and
// the filtered logits.  chain != 0 runs the three per frame, frame n seeded by kept[n - 1]: sequential by nature.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int kTW = 64, kTH = 32;                       // tile: one mask word wide, eight rows per wave
constexpr int kMaxRadius = OSVOS_BOUNDARY_MAX_RADIUS;

// ---- LDS union-find of a tile (indices r * 64 + c; -1 = background) ----
__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(const int* L, int a) {
  for (;;) {
    const int p = lds_ld(L + a);
    if (p == a) return a;
    a = p;                                                                               // p < a
  }
}
__device__ __forceinline__ void lds_unite(int* L, int a, int b) {
  for (;;) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }                                       // a > b: the larger root goes under the smaller
    const int old = atomicMin(L + a, b);
    if (old == a) return;                                                                // a was a root when it was linked
    a = old;                                                                             // a had a parent already: unite that one with b (old < a)
  }
}

// ---- global union-find of a frame (values v = 1 + index; lab[v - 1] <= v) ----
__device__ __forceinline__ int g_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* lab, int v) {
  for (;;) {
    const int p = g_ld(lab + (v - 1));
    if (p == v) return v;
    v = p;                                                                               // p < v
  }
}
__device__ __forceinline__ void g_unite(int* lab, int a, int b) {
  for (;;) {
    a = g_find(lab, a);
    b = g_find(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + (a - 1), b);
    if (old == a) return;
    a = old;
  }
}

// grid (tiles_x * tiles_y, N)
__global__ __launch_bounds__(256) void cc_tile_kernel(const float* __restrict__ logits, int* __restrict__ labels, int* __restrict__ area,
                                                      u64* __restrict__ stats, u64* __restrict__ packed, int H, int W, int tiles_x, float thr,
                                                      int conn) {
  __shared__ int L[kTH * kTW];
  __shared__ int cnt[kTH * kTW];
  __shared__ u64 rowmask[kTH];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = (int)(blockIdx.x / tiles_x) * kTH, x0 = (int)(blockIdx.x % tiles_x) * kTW;
  const size_t plane = (size_t)H * W;
  const float* __restrict__ x = logits + n * plane;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    packed[n] = 0ull;
    if (stats) { stats[4 * n] = 0ull; stats[4 * n + 1] = 0ull; stats[4 * n + 2] = 0ull; stats[4 * n + 3] = 0ull; }
  }
  const int xx = x0 + lane;
  float v[kTH / 4];
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int y = y0 + wave + 4 * j;
    v[j] = (y < H && xx < W) ? x[(size_t)y * W + xx] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int r = wave + 4 * j, y = y0 + r;
    const bool fg = y < H && xx < W && v[j] > thr;
    const u64 m = __ballot(fg);
    const u64 below = ~m & ((1ull << lane) - 1ull);                                      // background pixels left of this one
    const int start = below ? 64 - __clzll((long long)below) : 0;                        // first pixel of this pixel's run
    L[r * kTW + lane] = fg ? r * kTW + start : -1;
    cnt[r * kTW + lane] = 0;
    if (lane == 0) rowmask[r] = m;
  }
  __syncthreads();
  // the runs of row r and row r - 1: the leftmost column of every overlap makes the link (the columns right of it are the same two runs)
#pragma unroll 1
  for (int j = 0; j < kTH / 4; ++j) {
    const int r = wave + 4 * j;
    if (r == 0) continue;
    const u64 m = rowmask[r], u = rowmask[r - 1];
    if (!((m >> lane) & 1ull)) continue;
    const bool up = (u >> lane) & 1ull;
    const bool l = lane > 0 && ((m >> (lane - 1)) & 1ull), ul = lane > 0 && ((u >> (lane - 1)) & 1ull);
    const bool rt = lane < 63 && ((m >> (lane + 1)) & 1ull), ur = lane < 63 && ((u >> (lane + 1)) & 1ull);
    const int p = r * kTW + lane;
    if (up) {
      if (!(l && ul)) lds_unite(L, p, p - kTW);
    } else if (conn == 8) {
      if (ul && !l) lds_unite(L, p, p - kTW - 1);                                        // (with l set, l's upper neighbour is ul: l links)
      if (ur && !rt) lds_unite(L, p, p - kTW + 1);
    }
  }
  __syncthreads();
  int root[kTH / 4];
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int r = wave + 4 * j;
    const u64 m = rowmask[r];
    const bool fg = (m >> lane) & 1ull;
    const u64 below = ~m & ((1ull << lane) - 1ull);
    const int start = below ? 64 - __clzll((long long)below) : 0;
    int rt = -1;
    if (fg && start == lane) {                                                           // one walk and one count per run
      rt = lds_find(L, r * kTW + lane);
      const u64 t = ~(m >> lane);
      atomicAdd(cnt + rt, t ? __ffsll((long long)t) - 1 : 64);
    }
    rt = __shfl(rt, start, 64);
    root[j] = fg ? rt : -1;
  }
  __syncthreads();
  int* __restrict__ lab = labels + n * plane;
  int* __restrict__ ar = area + n * plane;
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int r = wave + 4 * j, y = y0 + r;
    if (y >= H || xx >= W) continue;
    const size_t g = (size_t)y * W + xx;
    const int rt = root[j];
    lab[g] = rt < 0 ? 0 : 1 + (y0 + rt / kTW) * W + x0 + rt % kTW;
    ar[g] = rt == r * kTW + lane ? cnt[rt] : 0;
  }
}

// grid (ceil(items / 256), N); items: hedges * W pixels of the rows below a horizontal tile edge, then vedges * H pixels right of a vertical one
__global__ __launch_bounds__(256) void cc_border_kernel(int* __restrict__ labels, int H, int W, int hedges, int vedges, int conn) {
  int* __restrict__ lab = labels + (size_t)blockIdx.y * H * W;
  const long item = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nh = (long)hedges * W;
  if (item >= nh + (long)vedges * H) return;
  if (item < nh) {
    const int y = (int)(item / W + 1) * kTH, x = (int)(item % W);
    const int* row = lab + (size_t)y * W;
    const int* rup = row - W;
    const int p = g_ld(row + x);
    if (p == 0) return;
    const bool up = g_ld(rup + x) != 0;
    const bool l = x > 0 && g_ld(row + x - 1) != 0, ul = x > 0 && g_ld(rup + x - 1) != 0;
    const int me = y * W + x + 1;
    if (up) {
      if (!(l && ul)) g_unite(lab, me, me - W);                                          // cc_tile_kernel's rule: the leftmost column of an overlap links
    } else if (conn == 8) {
      const bool rt = x + 1 < W && g_ld(row + x + 1) != 0, ur = x + 1 < W && g_ld(rup + x + 1) != 0;
      if (ul && !l) g_unite(lab, me, me - W - 1);
      if (ur && !rt) g_unite(lab, me, me - W + 1);
    }
  } else {
    const long it = item - nh;
    const int x = (int)(it / H + 1) * kTW, y = (int)(it % H);
    const int me = y * W + x + 1;
    if (g_ld(lab + (me - 1)) == 0) return;
    if (g_ld(lab + (me - 2)) != 0) {
      g_unite(lab, me, me - 1);                                                          // (the two diagonal neighbours, when set, touch the left one)
    } else if (conn == 8) {
      if (y > 0 && g_ld(lab + (me - 2 - W)) != 0) g_unite(lab, me, me - 1 - W);
      if (y + 1 < H && g_ld(lab + (me - 2 + W)) != 0) g_unite(lab, me, me - 1 + W);
    }
  }
}

// every pixel takes its root; a tile root that is no root any more hands its tile's count over (only roots ever receive)
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ labels, int* __restrict__ area, long plane, long total) {
  const long step = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const long n = i / plane;
    int* __restrict__ lab = labels + n * plane;
    const int me = (int)(i - n * plane) + 1;
    const int p = g_ld(lab + (me - 1));
    if (p == 0 || p == me) continue;                                                     // background, or a root
    const int r = g_find(lab, p);
    if (r != p) atomicMin(lab + (me - 1), r);
    const int c = area[i];
    if (c) {
      atomicAdd(area + n * plane + (r - 1), c);
      area[i] = 0;
    }
  }
}

// grid (workgroups, N)
__global__ __launch_bounds__(256) void cc_stats_kernel(const int* __restrict__ labels, const int* __restrict__ area, long plane, u64* __restrict__ stats,
                                                       u64* __restrict__ packed) {
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* __restrict__ lab = labels + n * plane;
  const int* __restrict__ ar = area + n * plane;
  unsigned comps = 0, fg = 0;
  u64 best = 0ull;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (long)gridDim.x * blockDim.x) {
    const int l = lab[i];
    fg += l != 0;
    if (l == (int)i + 1) {
      ++comps;
      const u64 k = ((u64)(unsigned)ar[i] << 32) | (u64)(~(unsigned)l);
      best = k > best ? k : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    comps += __shfl_xor(comps, o, 64);
    fg += __shfl_xor(fg, o, 64);
    const u64 other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  __shared__ unsigned red[4][2];
  __shared__ u64 redb[4];
  if (lane == 0) { red[wave][0] = comps; red[wave][1] = fg; redb[wave] = best; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned c = red[0][0] + red[1][0] + red[2][0] + red[3][0], f = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    u64 b = redb[0];
    for (int w = 1; w < 4; ++w) b = redb[w] > b ? redb[w] : b;
    if (c) atomicAdd(&stats[4 * n], (u64)c);
    if (f) atomicAdd(&stats[4 * n + 1], (u64)f);
    if (b) atomicMax(&packed[n], b);
  }
}

__global__ void cc_stats_final(u64* __restrict__ stats, const u64* __restrict__ packed, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const u64 b = packed[n];
  stats[4 * n + 2] = b >> 32;
  stats[4 * n + 3] = b ? (u64)(~(unsigned)b) : 0ull;
}

// ---- selection ----
// grid (workgroups, frames); bits: H * wpr words per frame, bit i of word k of row y is seed(y, 64 k + i) != 0, bits past W are zero
__global__ __launch_bounds__(256) void seed_pack_kernel(const unsigned char* __restrict__ seed, int H, int W, int wpr, u64* __restrict__ bits,
                                                        unsigned* __restrict__ any) {
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long words = (long)H * wpr;
  const unsigned char* __restrict__ s = seed + (size_t)n * H * W;
  u64* __restrict__ out = bits + (size_t)n * words;
  bool some = false;
  for (long idx = (long)blockIdx.x * 4 + wave; idx < words; idx += (long)gridDim.x * 4) {
    const long y = idx / wpr;
    const long col = (idx - y * wpr) * 64 + lane;
    const u64 w = __ballot(col < W && s[y * W + col] != 0);
    if (lane == 0) out[idx] = w;
    some |= w != 0ull;
  }
  if (some && lane == 0) atomicOr(&any[2 * n], 1u);
}

// grid (ceil(H W / 256), frames)
__global__ __launch_bounds__(256) void seed_mark_kernel(const int* __restrict__ labels, const u64* __restrict__ bits, int H, int W, int wpr, int r,
                                                        int* __restrict__ flags) {
  __shared__ int wtab[kMaxRadius + 1];
  if ((int)threadIdx.x <= r) {
    const int d = threadIdx.x, t = r * r - d * d;
    int w = (int)sqrtf((float)t);
    while (w * w > t) --w;
    while ((w + 1) * (w + 1) <= t) ++w;
    wtab[d] = w;
  }
  __syncthreads();
  const size_t plane = (size_t)H * W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)plane) return;
  const int l = labels[blockIdx.y * plane + i];
  if (l == 0) return;
  int* flag = flags + blockIdx.y * plane + (l - 1);
  if (g_ld(flag) != 0) return;                                                           // (a stale 0 costs the walk, nothing else)
  const u64* __restrict__ b = bits + (size_t)blockIdx.y * H * wpr;
  const int y = (int)(i / W), x = (int)(i % W);
  for (int d = 0; d <= r; ++d) {
    const int w = wtab[d];
    const int xl = x - w < 0 ? 0 : x - w, xh = x + w > W - 1 ? W - 1 : x + w;
    const int ka = xl >> 6, kb = xh >> 6;
    for (int side = 0; side < (d ? 2 : 1); ++side) {
      const int yy = side ? y - d : y + d;
      if (yy < 0 || yy >= H) continue;
      const u64* row = b + (size_t)yy * wpr;
      u64 hit = 0ull;
      for (int k = ka; k <= kb; ++k) {
        u64 m = ~0ull;
        if (k == ka) m &= ~0ull << (xl & 63);
        if (k == kb) m &= ~0ull >> (63 - (xh & 63));
        hit |= row[k] & m;
      }
      if (hit) {
        atomicOr(flag, 1);
        return;
      }
    }
  }
}

// grid-stride over frames * plane pixels; frame pointers are those of the first frame of this launch
__global__ __launch_bounds__(256) void select_apply_kernel(const float* logits, const int* __restrict__ labels, const int* __restrict__ area,
                                                           const u64* __restrict__ stats, const int* __restrict__ flags,
                                                           const unsigned* __restrict__ any, int use_seed, int min_area, int keep_largest, float fill,
                                                           float* out_logits, unsigned char* __restrict__ kept, long plane, long total) {
  const long step = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const long n = i / plane;
    const int l = labels[i];
    bool keep = false;
    if (l != 0) {
      const long root = n * plane + (l - 1);
      keep = area[root] >= min_area && (!keep_largest || (u64)l == stats[4 * n + 3]) && (!use_seed || any[2 * n] == 0u || flags[root] != 0);
    }
    if (kept) kept[i] = keep ? 1 : 0;
    if (out_logits) {
      const float v = logits[i];                                                          // (out_logits may be logits: one read, then one write, same pixel)
      out_logits[i] = (l != 0 && !keep) ? fill : v;
    }
  }
}

struct WsLayout {
  u64* packed;       // [N]     cc_stats_kernel's maximum
  unsigned* any;     // [2 N]   word 2 n: the seed map of frame n has a pixel
  int* flags;        // [N H W] the seed flag of a component at its root pixel; osvos_mask_components' area when the caller passes none
  u64* bits;         // [N][H][wpr] the seed maps, one bit per pixel
};

size_t flags_bytes(int N, int H, int W) { return align_up(sizeof(int) * (size_t)N * H * W, 8); }

WsLayout ws_layout(void* ws, int N, int H, int W) {
  char* p = reinterpret_cast<char*>(ws);
  WsLayout l;
  l.packed = reinterpret_cast<u64*>(p);
  l.any = reinterpret_cast<unsigned*>(p + sizeof(u64) * N);
  l.flags = reinterpret_cast<int*>(p + 2 * sizeof(u64) * N);
  l.bits = reinterpret_cast<u64*>(p + 2 * sizeof(u64) * N + flags_bytes(N, H, W));
  return l;
}

bool size_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long)H * W < 0x7fffffffL; }

unsigned stride_grid(long total) {
  long g = (total + 255) / 256;
  return (unsigned)(g > 4096 ? 4096 : g);
}

}  // namespace

extern "C" size_t osvos_components_ws_bytes(int N, int H, int W) {
  if (!size_ok(N, H, W)) return 0;
  return 2 * sizeof(u64) * N + flags_bytes(N, H, W) + sizeof(u64) * (size_t)N * H * ((W + 63) / 64);
}

extern "C" int osvos_mask_components(const float* logits, int* labels, int* area, void* stats_, void* ws, int N, int H, int W, float logit_threshold,
                                     int connectivity, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(logits && labels && ws, "mask_components: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "mask_components: bad size N %d H %d W %d", N, H, W);
  OSVOS_ARG_CHECK((long)H * W < 0x7fffffffL, "mask_components: %d x %d is too large (H * W must stay below 2^31 - 1)", H, W);
  OSVOS_ARG_CHECK(connectivity == 4 || connectivity == 8, "mask_components: connectivity %d (4 or 8)", connectivity);
  OSVOS_ARG_CHECK(((uintptr_t)logits | (uintptr_t)labels | (uintptr_t)area) % 4 == 0, "mask_components: logits, labels and area must be 4-byte aligned");
  OSVOS_ARG_CHECK(((uintptr_t)ws | (uintptr_t)stats_) % 8 == 0, "mask_components: stats and ws must be 8-byte aligned");
  const WsLayout l = ws_layout(ws, N, H, W);
  u64* stats = reinterpret_cast<u64*>(stats_);
  if (!area) area = l.flags;
  const long plane = (long)H * W, total = plane * N;
  const int tiles_x = ceil_div(W, kTW), tiles_y = ceil_div(H, kTH);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)N), dim3(256), 0, stream, logits, labels, area, stats, l.packed, H, W,
                     tiles_x, logit_threshold, connectivity);
  OSVOS_LAUNCH_CHECK();
  const long items = (long)(tiles_y - 1) * W + (long)(tiles_x - 1) * H;
  if (items > 0) {
    hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)N), dim3(256), 0, stream, labels, H, W, tiles_y - 1, tiles_x - 1,
                       connectivity);
    OSVOS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(stride_grid(total)), dim3(256), 0, stream, labels, area, plane, total);
    OSVOS_LAUNCH_CHECK();
  }
  if (stats) {
    long g = (plane + 1023) / 1024;
    g = g > 256 ? 256 : g;
    hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)g, (unsigned)N), dim3(256), 0, stream, labels, area, plane, stats, l.packed);
    OSVOS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_stats_final, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, stream, stats, l.packed, N);
    OSVOS_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int osvos_components_select(const float* logits, const int* labels, const int* area, const void* stats_, const unsigned char* seed, int chain,
                                       int seed_radius, int min_area, int keep_largest, float fill, float* out_logits, unsigned char* kept, void* ws,
                                       int N, int H, int W, float logit_threshold, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(logits && labels && area && ws, "components_select: null pointer");
  OSVOS_ARG_CHECK(stats_ || !keep_largest, "components_select: keep_largest needs stats");
  OSVOS_ARG_CHECK(out_logits || kept, "components_select: both outputs are null");
  OSVOS_ARG_CHECK(!chain || kept, "components_select: chain needs kept (frame n is seeded by kept[n - 1])");
  OSVOS_ARG_CHECK(!chain || seed, "components_select: chain needs the seed of frame 0");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "components_select: bad size N %d H %d W %d", N, H, W);
  OSVOS_ARG_CHECK((long)H * W < 0x7fffffffL, "components_select: %d x %d is too large (H * W must stay below 2^31 - 1)", H, W);
  OSVOS_ARG_CHECK(seed_radius >= 0 && seed_radius <= kMaxRadius, "components_select: seed radius %d (0..%d pixels)", seed_radius, kMaxRadius);
  OSVOS_ARG_CHECK(fill == fill && fill <= logit_threshold, "components_select: fill %g must be a number at or below the logit threshold %g", (double)fill,
                  (double)logit_threshold);
  OSVOS_ARG_CHECK(((uintptr_t)logits | (uintptr_t)labels | (uintptr_t)area | (uintptr_t)out_logits) % 4 == 0,
                  "components_select: logits, labels, area and out_logits must be 4-byte aligned");
  OSVOS_ARG_CHECK(((uintptr_t)ws | (uintptr_t)stats_) % 8 == 0, "components_select: stats and ws must be 8-byte aligned");
  const WsLayout l = ws_layout(ws, N, H, W);
  const u64* stats = reinterpret_cast<const u64*>(stats_);
  const long plane = (long)H * W;
  const int wpr = (W + 63) / 64;
  const long words = (long)H * wpr;
  if (seed)                                                                              // the `any` words and the flags, which lie behind them
    OSVOS_HIP_CHECK(hipMemsetAsync(l.any, 0, sizeof(u64) * N + sizeof(int) * (size_t)N * plane, stream));
  long pg = (words + 3) / 4;
  pg = pg > 1024 ? 1024 : pg;
  const int batches = chain ? N : 1, per = chain ? 1 : N;                                // chain: frame by frame, in order
  for (int b = 0; b < batches; ++b) {
    const size_t off = (size_t)b * plane;
    if (seed) {
      const unsigned char* s = chain && b > 0 ? kept + off - plane : seed;
      hipLaunchKernelGGL(seed_pack_kernel, dim3((unsigned)pg, (unsigned)per), dim3(256), 0, stream, s, H, W, wpr, l.bits + (size_t)b * words, l.any + 2 * b);
      OSVOS_LAUNCH_CHECK();
      hipLaunchKernelGGL(seed_mark_kernel, dim3((unsigned)((plane + 255) / 256), (unsigned)per), dim3(256), 0, stream, labels + off,
                         l.bits + (size_t)b * words, H, W, wpr, seed_radius, l.flags + off);
      OSVOS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(select_apply_kernel, dim3(stride_grid(plane * per)), dim3(256), 0, stream, logits + off, labels + off, area + off,
                       stats ? stats + 4 * b : stats, l.flags + off, l.any + 2 * b, seed ? 1 : 0, min_area, keep_largest, fill,
                       out_logits ? out_logits + off : out_logits, kept ? kept + off : kept, plane, plane * per);
    OSVOS_LAUNCH_CHECK();
  }
  return 0;
}
