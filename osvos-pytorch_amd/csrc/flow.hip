// Block-matching motion field between two decoded frames, its median filter and the integer warp (the rule: include/osvos_hip.h).
//
//   cost(d) = sum over the cell's B x B block of |Ycur(clamp(p)) - Yprev(clamp(p + d))| + penalty (|dx| + |dy|),  |dx|, |dy| <= R;
//   the cell's vector minimises (cost, dx^2 + dy^2, dy, dx).  All integers; the test is bit for bit.
//
// luma_kernel      both BGR frames -> two byte planes Y = (29 B + 150 G + 77 R + 128) >> 8 in the workspace, once per call.
// match_kernel     one workgroup of 256 lanes per tile of TCY x TCX cells (4 x 4 unless that would not fit LDS_BUDGET).  It stages as BYTES
//   sC  the current-frame luma the tile's blocks cover: rows gy0 .. gy0 + CH, columns gx0 .. , CH = (TCY - 1) S + B
//   sP  the previous-frame luma R pixels further out on every side (plus the words the sliding reads touch on the right)
//   both through clamped coordinates: clamp(p) and clamp(p + d) are functions of the absolute coordinate alone, so edge replication happens
//   once, at staging, and the candidate loop has no bounds test.
//   A work item is (cell, dy, group of four consecutive dx); lane t takes items t, t + 256, ...  The four dx of a group start where the
//   block's displaced left edge is 4-byte ALIGNED in sP (groups are laid out per cell from the aligned address at or below dx = -R, so a
//   group may hold up to three dx outside +-R: those are computed and not offered).  Per block row and per 4 pixels the lane then needs one
//   new aligned word of sP and one of sC: the current word is one funnel shift by the cell's own misalignment, and ONE v_qsad_pk_u16_u8
//   takes the 64-bit pair {hi, lo} of sP words and adds the four sliding sums of absolute byte differences (displacements 0, 1, 2, 3
//   bytes) into four packed 16-bit sums, unpacked into 32-bit registers every eight rows (a packed sum grows by at most 8160 a row).  2 LDS
//   reads and 2 vector instructions per 16 byte differences; the kernel is instantiated per words-per-row (1..8) so a row's reads are
//   issued together.  A block width that is no multiple of 4 masks the last word of both operands (|0 - 0| adds nothing) and sends it
//   through four v_sad_u8 on the displaced words {hi, lo} >> 8, 16, 24 (v_alignbit_b32) instead.
//   Each offered candidate becomes one 64-bit key  cost << 27 | (dx^2 + dy^2) << 14 | (dy + R) << 7 | (dx + R)  (cost < 2^23, the square
//   < 2^13): unsigned order of the keys IS the rule's lexicographic order, so the cell's answer is an integer minimum -- a 64-bit LDS
//   atomic min per item, exact and independent of the order of arrival.  One lane per cell decodes and stores vector and cost.
// median_kernel    one pass: per component the median of the 3 x 3 grid neighbourhood with clamped indices (by rank, no sort network).
// warp_kernel      out(y, x) = src(y + dy, x + dx) of the pixel's cell, or fill outside the frame; 32-bit words are moved as words, so
//                  float bit patterns (NaN payloads, -0) pass untouched.
//
// Vector stores only; no floating point anywhere but the fill value of the float warp.
#include <string.h>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int LDS_BUDGET = 48 * 1024;                                       // staged luma + keys of one workgroup
constexpr int TILE_CELLS = 4;                                               // cells per tile side before the budget shrinks it

struct Geometry {                                                            // of one osvos_flow_block_match call
  int H, W, GH, GW, B, S, R, penalty;
  int off;                                                                   // floor((S - B) / 2): block corner relative to its cell's corner
  int tcx, tcy;                                                              // cells per tile
  int nw;                                                                    // 4-byte words per block row, the last one partial when B % 4
  int ng;                                                                    // dx groups per (cell, dy)
  int CH, PH, pitchC, pitchP;                                                // staged rows, and bytes per staged row (multiples of 4)
  unsigned tail;                                                             // byte mask of the last word of a block row
};

__host__ __device__ inline int floor_half(int v) { return v >= 0 ? v / 2 : -((1 - v) / 2); }
__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// {hi, lo} >> 8 s, low word: the four bytes that start s bytes into lo
__device__ __forceinline__ unsigned funnel(unsigned hi, unsigned lo, unsigned s) {
  return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8u * s));
}

__global__ __launch_bounds__(THREADS) void luma_kernel(const unsigned char* __restrict__ prev, const unsigned char* __restrict__ cur,
                                                       unsigned char* __restrict__ yprev, unsigned char* __restrict__ ycur, size_t count) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= count) return;
  const unsigned char* p = prev + 3 * i;
  const unsigned char* c = cur + 3 * i;
  yprev[i] = (unsigned char)((29u * p[0] + 150u * p[1] + 77u * p[2] + 128u) >> 8);
  ycur[i] = (unsigned char)((29u * c[0] + 150u * c[1] + 77u * c[2] + 128u) >> 8);
}

// one row of one work item: the NW words of a block row in sC against the four displacements of a group in sP.  Words that are whole go
// through v_qsad_pk_u16_u8 -- D.u16[s] = sum of |S0 bytes s .. s + 3 - S1 bytes 0 .. 3| + S2.u16[s], S0 the 64-bit pair {hi, lo}: the four
// sliding sums in one instruction, into `packed`; a partial last word (B % 4 != 0) is masked on both sides and goes through four v_sad_u8
// into `a`
template <int NW>
__device__ __forceinline__ void match_row(const unsigned* __restrict__ cw, const unsigned* __restrict__ pw, unsigned ca, unsigned tail,
                                          unsigned long long& packed, unsigned (&a)[4]) {
  unsigned c[NW + 1], p[NW + 1];
#pragma unroll
  for (int k = 0; k <= NW; ++k) {
    c[k] = cw[k];
    p[k] = pw[k];
  }
#pragma unroll
  for (int k = 0; k + 1 < NW; ++k)
    packed = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)p[k + 1] << 32) | p[k], funnel(c[k + 1], c[k], ca), packed);
  const unsigned cv = funnel(c[NW], c[NW - 1], ca);
  if (tail == 0xffffffffu) {                                                 // (uniform)
    packed = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)p[NW] << 32) | p[NW - 1], cv, packed);
  } else {
    const unsigned cm = cv & tail;
    a[0] = __builtin_amdgcn_sad_u8(cm, p[NW - 1] & tail, a[0]);
    a[1] = __builtin_amdgcn_sad_u8(cm, funnel(p[NW], p[NW - 1], 1) & tail, a[1]);
    a[2] = __builtin_amdgcn_sad_u8(cm, funnel(p[NW], p[NW - 1], 2) & tail, a[2]);
    a[3] = __builtin_amdgcn_sad_u8(cm, funnel(p[NW], p[NW - 1], 3) & tail, a[3]);
  }
}

// grid (ceil(GW / tcx), ceil(GH / tcy), N), block 256, dynamic LDS: keys | sC | sP.  NW = g.nw, the words per block row
template <int NW>
__global__ __launch_bounds__(THREADS) void match_kernel(const unsigned char* __restrict__ yprev, const unsigned char* __restrict__ ycur,
                                                        int* __restrict__ vec, int* __restrict__ cost, Geometry g) {
  extern __shared__ unsigned long long lds[];
  const int ncells = g.tcx * g.tcy;
  unsigned long long* keys = lds;
  unsigned char* sC = (unsigned char*)(lds + ncells);
  unsigned char* sP = sC + g.pitchC * g.CH;
  const int tid = threadIdx.x, n = blockIdx.z;
  const int ci0 = blockIdx.y * g.tcy, cj0 = blockIdx.x * g.tcx;             // first cell of the tile
  const int gy0 = ci0 * g.S + g.off, gx0 = cj0 * g.S + g.off;               // frame coordinate of sC's origin; sP's is R further up and left
  const size_t plane = (size_t)n * g.H * g.W;

  for (int c = tid; c < ncells; c += THREADS) keys[c] = ~0ull;
  for (int i = tid; i < g.pitchC * g.CH; i += THREADS) {
    const int ly = i / g.pitchC, lx = i - ly * g.pitchC;
    sC[i] = ycur[plane + (size_t)clampi(gy0 + ly, 0, g.H - 1) * g.W + clampi(gx0 + lx, 0, g.W - 1)];
  }
  for (int i = tid; i < g.pitchP * g.PH; i += THREADS) {
    const int ly = i / g.pitchP, lx = i - ly * g.pitchP;
    sP[i] = yprev[plane + (size_t)clampi(gy0 - g.R + ly, 0, g.H - 1) * g.W + clampi(gx0 - g.R + lx, 0, g.W - 1)];
  }
  __syncthreads();

  const int ndy = 2 * g.R + 1;
  const int per_cell = ndy * g.ng, nitems = ncells * per_cell;
  for (int item = tid; item < nitems; item += THREADS) {
    const int c = item / per_cell, rest = item - c * per_cell;
    const int iy = rest / g.ng, grp = rest - iy * g.ng;
    const int li = c / g.tcx, lj = c - li * g.tcx;
    if (ci0 + li >= g.GH || cj0 + lj >= g.GW) continue;                      // a cell of a partial tile
    const int dy = iy - g.R;
    const int bx = lj * g.S;                                                 // the block's left edge in sC; in sP it is bx + R
    const int px = (bx & ~3) + 4 * grp;                                      // aligned sP column of this group's first candidate
    const int dx0 = px - (bx + g.R);
    const unsigned ca = (unsigned)(bx & 3);
    const unsigned char* crow = sC + (li * g.S) * g.pitchC + (bx & ~3);
    const unsigned char* prow = sP + (li * g.S + g.R + dy) * g.pitchP + px;
    unsigned sad[4] = {0, 0, 0, 0};
    // a packed sum grows by at most 4 NW 255 <= 8160 a row: eight rows stay below 2^16, then it is unpacked
    for (int r0 = 0; r0 < g.B; r0 += 8) {
      unsigned long long packed = 0;
      const int rows = min(8, g.B - r0);
      for (int r = 0; r < rows; ++r, crow += g.pitchC, prow += g.pitchP)
        match_row<NW>((const unsigned*)crow, (const unsigned*)prow, ca, g.tail, packed, sad);
#pragma unroll
      for (int s = 0; s < 4; ++s) sad[s] += (unsigned)(packed >> (16 * s)) & 0xffffu;
    }
    const int ady = dy < 0 ? -dy : dy;
    unsigned long long best = ~0ull;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int dx = dx0 + s, adx = dx < 0 ? -dx : dx;
      if (adx > g.R) continue;
      const unsigned long long key = ((unsigned long long)(sad[s] + (unsigned)(g.penalty * (adx + ady))) << 27) |
                                     ((unsigned long long)(dx * dx + dy * dy) << 14) | ((unsigned long long)(dy + g.R) << 7) |
                                     (unsigned long long)(dx + g.R);
      best = key < best ? key : best;
    }
    if (best != ~0ull) atomicMin(&keys[c], best);
  }
  __syncthreads();

  for (int c = tid; c < ncells; c += THREADS) {
    const int li = c / g.tcx, lj = c - li * g.tcx;
    const int ci = ci0 + li, cj = cj0 + lj;
    if (ci >= g.GH || cj >= g.GW) continue;
    const unsigned long long key = keys[c];
    const size_t cell = ((size_t)n * g.GH + ci) * g.GW + cj;
    vec[2 * cell] = (int)(key & 127u) - g.R;
    vec[2 * cell + 1] = (int)((key >> 7) & 127u) - g.R;
    if (cost) cost[cell] = (int)(key >> 27);
  }
}

typedef void (*MatchKernel)(const unsigned char*, const unsigned char*, int*, int*, Geometry);
const MatchKernel MATCH_KERNELS[OSVOS_FLOW_MAX_BLOCK / 4] = {match_kernel<1>, match_kernel<2>, match_kernel<3>, match_kernel<4>,
                                                             match_kernel<5>, match_kernel<6>, match_kernel<7>, match_kernel<8>};

// one thread per vector component: src, dst [N][GH][GW][2]
__global__ __launch_bounds__(THREADS) void median_kernel(const int* __restrict__ src, int* __restrict__ dst, int N, int GH, int GW) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= (size_t)N * GH * GW * 2) return;
  const int comp = (int)(i & 1);
  const size_t cell = i >> 1;
  const int cj = (int)(cell % GW), ci = (int)((cell / GW) % GH);
  const size_t image = cell / GW / GH * GH * GW;
  int v[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      v[3 * a + b] = src[2 * (image + (size_t)clampi(ci + a - 1, 0, GH - 1) * GW + clampi(cj + b - 1, 0, GW - 1)) + comp];
  // the median is the value with at most 4 values below it and at least 5 at or below it
  int med = v[0];
#pragma unroll
  for (int a = 0; a < 9; ++a) {
    int below = 0, upto = 0;
#pragma unroll
    for (int b = 0; b < 9; ++b) {
      below += v[b] < v[a];
      upto += v[b] <= v[a];
    }
    if (below <= 4 && upto >= 5) med = v[a];
  }
  dst[i] = med;
}

// one thread per output pixel; T is unsigned char or unsigned (a float's bits)
template <typename T>
__global__ __launch_bounds__(THREADS) void warp_kernel(const T* __restrict__ src, const int* __restrict__ vec, T* __restrict__ out, int H, int W,
                                                       int GH, int GW, int S, T fill) {
  const int x = blockIdx.x * THREADS + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x >= W) return;
  const int ci = min(y / S, GH - 1), cj = min(x / S, GW - 1);
  const int* d = vec + 2 * (((size_t)n * GH + ci) * GW + cj);
  const long long sx = (long long)x + d[0], sy = (long long)y + d[1];
  const size_t image = (size_t)n * H * W;
  T v = fill;
  if (sx >= 0 && sx < W && sy >= 0 && sy < H) v = src[image + (size_t)sy * W + (size_t)sx];
  out[image + (size_t)y * W + x] = v;
}

bool size_ok(int v) { return v >= 1 && v <= OSVOS_FLOW_MAX_SIDE; }
bool frames_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && size_ok(H) && size_ok(W); }
bool params_ok(int block, int step, int search, int median) {
  return block >= 1 && block <= OSVOS_FLOW_MAX_BLOCK && step >= 1 && step <= OSVOS_FLOW_MAX_STEP && search >= 0 && search <= OSVOS_FLOW_MAX_SEARCH &&
         median >= 0 && median <= OSVOS_FLOW_MAX_MEDIAN;
}
size_t luma_bytes(int N, int H, int W) { return align_up(2 * (size_t)N * H * W, 16); }

size_t lds_bytes(const Geometry& g) { return (size_t)g.tcx * g.tcy * 8 + (size_t)g.pitchC * g.CH + (size_t)g.pitchP * g.PH; }

// the staged extents of a tile of tcx x tcy cells.  sC: a row holds the blocks' span rounded up to words, plus the word the funnel shift
// of the last block word reads.  sP: the first group of the last cell starts at or below column (tcx - 1) S, the last group ng - 1 words
// further, and a block row reads nw + 1 words from there
void set_tile(Geometry& g, int tcx, int tcy) {
  g.tcx = tcx; g.tcy = tcy;
  g.CH = (tcy - 1) * g.S + g.B;
  g.PH = g.CH + 2 * g.R;
  g.pitchC = (int)align_up((size_t)(tcx - 1) * g.S, 4) + 4 * g.nw + 4;
  g.pitchP = (int)align_up((size_t)(tcx - 1) * g.S, 4) + 4 * g.ng + 4 * g.nw;
}

}  // namespace

extern "C" size_t osvos_flow_ws_bytes(int N, int H, int W, int block, int step, int search, int median) {
  if (!frames_ok(N, H, W) || !params_ok(block, step, search, median)) return 0;
  const size_t grid = median > 0 ? (size_t)N * ceil_div(H, step) * ceil_div(W, step) * 2 * sizeof(int) : 0;
  return luma_bytes(N, H, W) + grid;
}

extern "C" int osvos_flow_block_match(const unsigned char* prev_bgr, const unsigned char* cur_bgr, int* vec, int* cost, void* ws, int N, int H, int W,
                                      int block, int step, int search, int penalty, int median, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(prev_bgr && cur_bgr && vec && ws, "flow_block_match: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "flow_block_match: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W), "flow_block_match: bad size H %d W %d (1..%d per side)", H, W, OSVOS_FLOW_MAX_SIDE);
  OSVOS_ARG_CHECK(block >= 1 && block <= OSVOS_FLOW_MAX_BLOCK, "flow_block_match: block %d (1..%d)", block, OSVOS_FLOW_MAX_BLOCK);
  OSVOS_ARG_CHECK(step >= 1 && step <= OSVOS_FLOW_MAX_STEP, "flow_block_match: step %d (1..%d)", step, OSVOS_FLOW_MAX_STEP);
  OSVOS_ARG_CHECK(search >= 0 && search <= OSVOS_FLOW_MAX_SEARCH, "flow_block_match: search %d (0..%d)", search, OSVOS_FLOW_MAX_SEARCH);
  OSVOS_ARG_CHECK(penalty >= 0 && penalty <= OSVOS_FLOW_MAX_PENALTY, "flow_block_match: penalty %d (0..%d)", penalty, OSVOS_FLOW_MAX_PENALTY);
  OSVOS_ARG_CHECK(median >= 0 && median <= OSVOS_FLOW_MAX_MEDIAN, "flow_block_match: median %d passes (0..%d)", median, OSVOS_FLOW_MAX_MEDIAN);
  OSVOS_ARG_CHECK((uintptr_t)vec % 4 == 0 && (uintptr_t)cost % 4 == 0 && (uintptr_t)ws % 4 == 0, "flow_block_match: vec, cost and ws must be 4-byte aligned");
  OSVOS_ARG_CHECK((size_t)N * H * W <= ((size_t)1 << 38), "flow_block_match: %d frames of %d x %d are more pixels than one call takes (2^38)", N, H, W);
  OSVOS_ARG_CHECK((void*)vec != ws && (void*)cost != ws && (void*)vec != (void*)cost, "flow_block_match: vec, cost and ws must be three buffers");

  Geometry g;
  g.H = H; g.W = W; g.B = block; g.S = step; g.R = search; g.penalty = penalty;
  g.GH = ceil_div(H, step); g.GW = ceil_div(W, step);
  g.off = floor_half(step - block);
  g.nw = ceil_div(block, 4);
  g.ng = (2 * search + 7) / 4;
  g.tail = block % 4 ? (1u << (8 * (block % 4))) - 1u : 0xffffffffu;
  int tcx = TILE_CELLS, tcy = TILE_CELLS;
  set_tile(g, tcx, tcy);
  while (lds_bytes(g) > (size_t)LDS_BUDGET && tcx * tcy > 1) {
    if (tcy >= tcx) tcy = (tcy + 1) / 2; else tcx = (tcx + 1) / 2;
    set_tile(g, tcx, tcy);
  }
  OSVOS_ARG_CHECK(lds_bytes(g) <= (size_t)LDS_BUDGET, "flow_block_match: one cell needs %zu bytes of LDS (at most %d)", lds_bytes(g), LDS_BUDGET);

  const size_t count = (size_t)N * H * W;
  unsigned char* yprev = (unsigned char*)ws;
  unsigned char* ycur = yprev + count;
  int* spare = (int*)((unsigned char*)ws + luma_bytes(N, H, W));           // the second vector grid of the median passes
  hipLaunchKernelGGL(luma_kernel, dim3((unsigned)((count + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, prev_bgr, cur_bgr, yprev, ycur, count);
  OSVOS_LAUNCH_CHECK();
  int* dst = median % 2 == 0 ? vec : spare;                                 // the grids alternate so that the last pass writes vec
  const dim3 grid((unsigned)ceil_div(g.GW, g.tcx), (unsigned)ceil_div(g.GH, g.tcy), (unsigned)N);
  hipLaunchKernelGGL(MATCH_KERNELS[g.nw - 1], grid, dim3(THREADS), lds_bytes(g), stream, yprev, ycur, dst, cost, g);
  OSVOS_LAUNCH_CHECK();
  const size_t comps = (size_t)N * g.GH * g.GW * 2;
  for (int t = 0; t < median; ++t) {
    int* next = dst == vec ? spare : vec;
    hipLaunchKernelGGL(median_kernel, dim3((unsigned)((comps + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, dst, next, N, g.GH, g.GW);
    OSVOS_LAUNCH_CHECK();
    dst = next;
  }
  return 0;
}

extern "C" int osvos_flow_warp(const void* src, int dtype, const int* vec, void* out, int N, int H, int W, int step, float fill, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(src && vec && out, "flow_warp: null pointer");
  OSVOS_ARG_CHECK(dtype == 0 || dtype == 1, "flow_warp: dtype %d (0 = uint8, 1 = float32)", dtype);
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "flow_warp: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W), "flow_warp: bad size H %d W %d (1..%d per side)", H, W, OSVOS_FLOW_MAX_SIDE);
  OSVOS_ARG_CHECK(step >= 1 && step <= OSVOS_FLOW_MAX_STEP, "flow_warp: step %d (1..%d)", step, OSVOS_FLOW_MAX_STEP);
  OSVOS_ARG_CHECK(out != src && out != (const void*)vec, "flow_warp: out must not be src or vec (the warp is a gather)");
  OSVOS_ARG_CHECK((uintptr_t)vec % 4 == 0, "flow_warp: vec must be 4-byte aligned");
  const int GH = ceil_div(H, step), GW = ceil_div(W, step);
  const dim3 grid((unsigned)ceil_div(W, THREADS), (unsigned)H, (unsigned)N), block(THREADS);
  if (dtype == 0) {
    OSVOS_ARG_CHECK(fill >= 0.f && fill <= 255.f && fill == (float)(int)fill, "flow_warp: fill %g is no byte value (an integer in 0..255)", fill);
    hipLaunchKernelGGL(warp_kernel<unsigned char>, grid, block, 0, stream, (const unsigned char*)src, vec, (unsigned char*)out, H, W, GH, GW, step,
                       (unsigned char)(int)fill);
  } else {
    OSVOS_ARG_CHECK((uintptr_t)src % 4 == 0 && (uintptr_t)out % 4 == 0, "flow_warp: float32 src and out must be 4-byte aligned");
    unsigned bits;
    memcpy(&bits, &fill, sizeof(bits));
    hipLaunchKernelGGL(warp_kernel<unsigned>, grid, block, 0, stream, (const unsigned*)src, vec, (unsigned*)out, H, W, GH, GW, step, bits);
  }
  OSVOS_LAUNCH_CHECK();
  return 0;
}
