// Appearance matching, the two searches next to osvos_match_nearest (csrc/match.hip, which this file leaves alone; the rules: include/osvos_hip.h).
//
//   top-K:  t_ab = (float) dot(Q_a, R_b) * rinv_r[b] as in nearest; per query row and class the k = min(K, rows of the class) largest t,
//           v_1 >= .. >= v_k (a multiset: equal rows are separate members, no index is kept); s = v_1, s = s + v_i in that order; m = s / k
//           correctly rounded; sim = m * rinv_q[a]; an empty class gives -2.  K = 1 is nearest's sim bit for bit.
//   local:  queries and references on one h x w grid; the candidates of query cell (i, j) are the reference cells within `radius` rows and
//           columns of it, inside the grid, of the class; the largest t and the smallest reference row that attains it; (-2, -1) when empty.
//
// topk_kernel<L>    nearest_kernel's tiling: 256 lanes = 4 waves, grid (ceil(Pq / 128), slices, N), 128 query rows staged once in LDS for all
//   C, the slice of R walked in tiles of 128 rows by chunks of 64 channels through a double-buffered LDS image that is prefetched into
//   registers under the MFMAs, v_mfma_i32_32x32x32_i8 with the QUERY on the lane.  In place of the two (value, index) pairs a lane keeps, per
//   class, a descending list of the L best values in registers (L = 4, 8 or 16, the smallest that holds K; an empty slot is -inf).  A
//   candidate enters through a max / min chain (it sinks to its place, the smallest value falls off the end: equal values stay separate
//   members); the chain is guarded by a wave vote on "some lane's candidate beats its last slot", which is rarely true once the lists have
//   filled.  The two lane halves are merged at the end of the slice and the first K slots of both lists go to ws.
// topk_finish_kernel  one lane per (frame, class, query): merges the slices' lists through the same chain, counts the filled slots among
//   the first K, then the sum, the quotient and the product of the rule.
// local_kernel      128 lanes, a workgroup owns 4 x 8 query cells and four lanes share a cell: lane `part` holds the 16-byte pieces part,
//   part + 4, .. of the query row in registers (at most 16 pieces) and walks the window in ascending reference row with the 4-byte
//   integer dot instruction on the matching pieces of the reference row, read through the cache (a row is read by the cells around it; at
//   854x480 the whole of R is 3.3 MB); two quad shuffles add the four partial integer sums.  Strict > in ascending row order: the smaller
//   row keeps a tie.  Cells past the grid and rows of neither class are skipped, which is what zero rows under the void label would give.
//   No LDS, no barrier.  (The MFMA form would discard (2 radius + 1)^2 of (4 + 2 radius)(8 + 2 radius) x 32 products per tile.)
//
// No atomics, no float reductions across lanes other than min and max; vector stores only.
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256;
constexpr int BM = 128;                       // query rows per workgroup (32 per wave)
constexpr int BN = 128;                       // reference rows per tile (four MFMA tiles)
constexpr int KC = 64;                        // channels per staged chunk of R (two MFMA steps)
constexpr int RROW = KC + 16;                 // bytes per staged R row
constexpr int QPAD = 16;                      // bytes added to a staged Q row
constexpr int MAX_C = 1024, MAX_SLICES = 16, MAX_K = 16, MAX_RADIUS = 15;
constexpr long MAX_P = 1L << 20;
constexpr size_t TOPK_LDS_MAX = (size_t)BM * (MAX_C + QPAD) + 2 * BN * RROW;         // 153600 of the 163840 bytes of a CU
constexpr int LT_H = 4, LT_W = 8, LPARTS = 4, LTHREADS = LT_H * LT_W * LPARTS;       // local_kernel's tile
#define NEG_INF (-__builtin_inff())

// correctly rounded fp32 quotient through double (53 >= 2 * 24 + 2 bits)
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// a descending list takes one more member: c sinks to its place, the smallest falls off.  -inf changes nothing
template <int L>
__device__ __forceinline__ void insert(float (&list)[L], float c) {
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const float hi = fmaxf(list[i], c);
    c = fminf(list[i], c);
    list[i] = hi;
  }
}

// grid (ceil(Pq / BM), slices, N); dynamic LDS: BM (C + QPAD) + 2 BN RROW bytes.  part [N][slices][2][K][Pq]
template <int L>
__global__ __launch_bounds__(THREADS) void topk_kernel(const signed char* __restrict__ Q, const signed char* __restrict__ R,
                                                       const float* __restrict__ rinv_r, const unsigned char* __restrict__ label_r,
                                                       float* __restrict__ part, int NR, int Pq, int Pr, int C, int K, int tiles_per_slice) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ float sRinv[2][BN];
  __shared__ unsigned char sLab[2][BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int n = blockIdx.z, slice = blockIdx.y, slices = gridDim.y;
  const int a0 = blockIdx.x * BM;
  const int qrow = C + QPAD;
  unsigned char* sQ = lds;
  unsigned char* sR = lds + (size_t)BM * qrow;
  const size_t rn = NR == 1 ? 0 : (size_t)n;
  const signed char* Rn = R + rn * Pr * C;
  const float* rinv_n = rinv_r + rn * Pr;
  const unsigned char* lab_n = label_r + rn * Pr;

  // the workgroup's query rows, once
  const int qpieces = C >> 4;                                                 // 16-byte pieces per row
  for (int i = tid; i < BM * qpieces; i += THREADS) {
    const int r = i / qpieces, pc = i - r * qpieces;
    i32x4 v = {0, 0, 0, 0};
    if (a0 + r < Pq) v = *reinterpret_cast<const i32x4*>(Q + ((size_t)n * Pq + a0 + r) * C + pc * 16);
    *reinterpret_cast<i32x4*>(sQ + r * qrow + pc * 16) = v;
  }

  const int tiles_all = (Pr + BN - 1) / BN;
  const int tile0 = slice * tiles_per_slice;
  const int ntiles = min(tiles_per_slice, tiles_all - tile0);                 // >= 1: the host launches no empty slice
  const int kch = C / KC;
  const int T = ntiles * kch;

  // this lane's two 16-byte pieces of a chunk: rows tid >> 2 and 64 + (tid >> 2), piece tid & 3
  const int srow = tid >> 2, spc = tid & 3;
  i32x4 stage[2];
  float srinv = 0.0f;
  unsigned char slab = 255;
  auto fetch = [&](int t) {
    const int j = t / kch, kc = t - j * kch;
    const int b0 = (tile0 + j) * BN;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int b = b0 + srow + 64 * u;
      i32x4 v = {0, 0, 0, 0};
      if (b < Pr) v = *reinterpret_cast<const i32x4*>(Rn + (size_t)b * C + kc * KC + spc * 16);
      stage[u] = v;
    }
    if (kc == 0 && tid < BN) {
      const int b = b0 + tid;
      srinv = b < Pr ? rinv_n[b] : 0.0f;
      slab = b < Pr ? lab_n[b] : (unsigned char)255;
    }
  };
  auto commit = [&](int t) {
    const int j = t / kch, kc = t - j * kch;
    unsigned char* dst = sR + (size_t)(t & 1) * BN * RROW;
#pragma unroll
    for (int u = 0; u < 2; ++u) *reinterpret_cast<i32x4*>(dst + (srow + 64 * u) * RROW + spc * 16) = stage[u];
    if (kc == 0 && tid < BN) {
      sRinv[j & 1][tid] = srinv;
      sLab[j & 1][tid] = slab;
    }
  };

  fetch(0);
  commit(0);
  __syncthreads();

  i32x16 acc[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0;
  float fg[L], bg[L];
#pragma unroll
  for (int i = 0; i < L; ++i) fg[i] = bg[i] = NEG_INF;
  const unsigned char* myQ = sQ + (wave * 32 + col) * qrow + 16 * half;

  for (int t = 0; t < T; ++t) {
    const int j = t / kch, kc = t - j * kch;
    if (t + 1 < T) fetch(t + 1);
    const unsigned char* src = sR + (size_t)(t & 1) * BN * RROW + col * RROW + 16 * half;
#pragma unroll
    for (int ks = 0; ks < KC / 32; ++ks) {
      const i32x4 bq = *reinterpret_cast<const i32x4*>(myQ + kc * KC + ks * 32);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const i32x4 ar = *reinterpret_cast<const i32x4*>(src + mt * 32 * RROW + ks * 32);
        acc[mt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ar, bq, acc[mt], 0, 0, 0);
      }
    }
    if (kc == kch - 1) {                                                     // the tile is complete: route by label into the lists
      const float* rv = sRinv[j & 1];
      const unsigned char* lb = sLab[j & 1];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float tv = (float)acc[mt][r] * rv[row];
          const unsigned char l = lb[row];
          const float cf = l == 1 ? tv : NEG_INF, cb = l == 0 ? tv : NEG_INF;
          if (__any(cf > fg[L - 1])) insert(fg, cf);                         // (a wave vote: the branch is uniform)
          if (__any(cb > bg[L - 1])) insert(bg, cb);
          acc[mt][r] = 0;
        }
      }
    }
    if (t + 1 < T) commit(t + 1);
    __syncthreads();
  }

  // the other lane half saw the other reference rows of every tile
  float of[L], ob[L];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    of[i] = __shfl_xor(fg[i], 32, 64);
    ob[i] = __shfl_xor(bg[i], 32, 64);
  }
#pragma unroll
  for (int i = 0; i < L; ++i) {
    insert(fg, of[i]);
    insert(bg, ob[i]);
  }
  const int a = a0 + wave * 32 + col;
  if (half == 0 && a < Pq) {
    const size_t base = ((size_t)n * slices + slice) * 2 * K;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      if (i < K) {
        part[(base + i) * Pq + a] = fg[i];
        part[(base + K + i) * Pq + a] = bg[i];
      }
    }
  }
}

// grid (ceil(Pq / THREADS), 2, N)
__global__ __launch_bounds__(THREADS) void topk_finish_kernel(const float* __restrict__ part, const float* __restrict__ rinv_q, float* __restrict__ sim,
                                                              int Pq, int K, int slices) {
  const int a = blockIdx.x * THREADS + threadIdx.x, cls = blockIdx.y, n = blockIdx.z;
  if (a >= Pq) return;
  float list[MAX_K];
#pragma unroll
  for (int i = 0; i < MAX_K; ++i) list[i] = NEG_INF;
  for (int s = 0; s < slices; ++s) {
    const size_t base = (((size_t)n * slices + s) * 2 + cls) * K;
    for (int i = 0; i < K; ++i) {
      const float v = part[(base + i) * Pq + a];
      if (!(v > NEG_INF)) break;                                             // a slice's list is descending: the rest is empty
      insert(list, v);
    }
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < MAX_K; ++i) k += (i < K && list[i] > NEG_INF) ? 1 : 0;
  float s = list[0];
#pragma unroll
  for (int i = 1; i < MAX_K; ++i)
    if (i < k) s = s + list[i];
  sim[((size_t)n * 2 + cls) * Pq + a] = k == 0 ? -2.0f : div_rn(s, (float)k) * rinv_q[(size_t)n * Pq + a];
}

struct Best {
  float v;
  int i;
};
__device__ __forceinline__ void take(Best& b, float t, int idx) {            // strict >: walking in ascending row, the smaller row keeps a tie
  if (t > b.v) {
    b.v = t;
    b.i = idx;
  }
}

// grid (tiles of LT_H x LT_W cells, N)
__global__ __launch_bounds__(LTHREADS) void local_kernel(const signed char* __restrict__ Q, const float* __restrict__ rinv_q,
                                                         const signed char* __restrict__ R, const float* __restrict__ rinv_r,
                                                         const unsigned char* __restrict__ label_r, float* __restrict__ sim, int* __restrict__ idx,
                                                         int NR, int h, int w, int C, int radius) {
  const int tid = threadIdx.x, part = tid & (LPARTS - 1), cell = tid / LPARTS;
  const int tiles_x = (w + LT_W - 1) / LT_W;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i = ty * LT_H + cell / LT_W, j = tx * LT_W + cell % LT_W;
  if (i >= h || j >= w) return;                                               // (the four lanes of a cell leave together: the shuffles stay inside a quad)
  const int n = blockIdx.y, P = h * w, a = i * w + j;
  const size_t rn = NR == 1 ? 0 : (size_t)n;
  const signed char* Rn = R + rn * P * C;
  const float* rinv_n = rinv_r + rn * P;
  const unsigned char* lab_n = label_r + rn * P;
  const int per = C >> 6;                                                     // 16-byte pieces per lane
  i32x4 q[MAX_C / 64];
#pragma unroll
  for (int u = 0; u < MAX_C / 64; ++u) {
    q[u] = i32x4{0, 0, 0, 0};
    if (u < per) q[u] = *reinterpret_cast<const i32x4*>(Q + ((size_t)n * P + a) * C + (part + LPARTS * u) * 16);
  }
  Best fg = {NEG_INF, -1}, bg = {NEG_INF, -1};
  const int i0 = max(i - radius, 0), i1 = min(i + radius, h - 1), j0 = max(j - radius, 0), j1 = min(j + radius, w - 1);
  for (int ii = i0; ii <= i1; ++ii) {
    for (int jj = j0; jj <= j1; ++jj) {                                       // ascending reference row
      const int b = ii * w + jj;
      const unsigned char l = lab_n[b];
      if (l > 1) continue;                                                    // void: in neither class
      const signed char* row = Rn + (size_t)b * C + part * 16;
      int d = 0;
#pragma unroll
      for (int u = 0; u < MAX_C / 64; ++u) {
        if (u < per) {
          const i32x4 v = *reinterpret_cast<const i32x4*>(row + LPARTS * 16 * u);
#pragma unroll
          for (int e = 0; e < 4; ++e) d = __builtin_amdgcn_sdot4(q[u][e], v[e], d, false);
        }
      }
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      const float tv = (float)d * rinv_n[b];
      if (l == 1) take(fg, tv, b);
      else take(bg, tv, b);
    }
  }
  if (part == 0) {
    const float rq = rinv_q[(size_t)n * P + a];
    const size_t o = (size_t)n * 2 * P + a;
    sim[o] = fg.i < 0 ? -2.0f : fg.v * rq;
    sim[o + P] = bg.i < 0 ? -2.0f : bg.v * rq;
    if (idx) {
      idx[o] = fg.i;
      idx[o + P] = bg.i;
    }
  }
}

bool channels_ok(int C) { return C >= 64 && C <= MAX_C && C % 64 == 0; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

// how the reference rows are cut, as osvos_match_nearest cuts them: a function of the sizes alone
void slicing(int N, int Pq, int Pr, int* tiles_per_slice, int* slices) {
  const int tiles = ceil_div(Pr, BN);
  const long blocks = (long)N * ceil_div(Pq, BM);
  long want = (512 + blocks - 1) / blocks;
  if (want > MAX_SLICES) want = MAX_SLICES;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  *tiles_per_slice = ceil_div(tiles, (int)want);
  *slices = ceil_div(tiles, *tiles_per_slice);
}

template <int L>
int launch_topk(const signed char* Q, const signed char* R, const float* rinv_r, const unsigned char* label_r, float* ws, int N, int NR, int Pq, int Pr,
                int C, int K, int tps, int slices, hipStream_t stream) {
  if (int rc = osvos_set_dyn_lds_once<&topk_kernel<L>>(TOPK_LDS_MAX)) return rc;
  const size_t lds_bytes = (size_t)BM * (C + QPAD) + 2 * BN * RROW;
  hipLaunchKernelGGL(topk_kernel<L>, dim3((unsigned)ceil_div(Pq, BM), (unsigned)slices, (unsigned)N), dim3(THREADS), lds_bytes, stream, Q, R, rinv_r, label_r,
                     ws, NR, Pq, Pr, C, K, tps);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// the per-slice lists of both classes: K values per slice, class and query
extern "C" size_t osvos_match_topk_ws_bytes(int N, int Pq, int Pr, int C, int K) {
  if (N < 1 || N > 65535 || Pq < 1 || Pq > MAX_P || Pr < 1 || Pr > MAX_P || !channels_ok(C) || K < 1 || K > MAX_K) return 0;
  int tps, slices;
  slicing(N, Pq, Pr, &tps, &slices);
  return (size_t)N * slices * 2 * K * Pq * sizeof(float);
}

extern "C" int osvos_match_topk(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r,
                                float* sim, void* ws, int N, int NR, int Pq, int Pr, int C, int K, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(Q && rinv_q && R && rinv_r && label_r && sim && ws, "match_topk: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "match_topk: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(NR == N || NR == 1, "match_topk: NR %d reference frames (N = %d, or 1 to broadcast)", NR, N);
  OSVOS_ARG_CHECK(Pq >= 1 && Pq <= MAX_P, "match_topk: Pq %d query rows (1..2^20)", Pq);
  OSVOS_ARG_CHECK(Pr >= 1 && Pr <= MAX_P, "match_topk: Pr %d reference rows (1..2^20)", Pr);
  OSVOS_ARG_CHECK(channels_ok(C), "match_topk: C %d channels (a multiple of 64, 64..%d)", C, MAX_C);
  OSVOS_ARG_CHECK(K >= 1 && K <= MAX_K, "match_topk: K %d rows averaged (1..%d)", K, MAX_K);
  OSVOS_ARG_CHECK((uintptr_t)Q % 16 == 0 && (uintptr_t)R % 16 == 0, "match_topk: misaligned: Q and R must be 16-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)ws % 8 == 0, "match_topk: misaligned: ws must be 8-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)rinv_q % 4 == 0 && (uintptr_t)rinv_r % 4 == 0 && (uintptr_t)sim % 4 == 0,
                  "match_topk: misaligned: rinv_q, rinv_r and sim must be 4-byte aligned");
  int tps, slices;
  slicing(N, Pq, Pr, &tps, &slices);
  const size_t qb = (size_t)N * Pq * C, rqb = (size_t)N * Pq * 4, rb = (size_t)NR * Pr * C, rrb = (size_t)NR * Pr * 4, lb = (size_t)NR * Pr;
  const size_t ob = (size_t)N * 2 * Pq * 4, wb = (size_t)N * slices * 2 * K * Pq * sizeof(float);
  const void* ins[5] = {Q, rinv_q, R, rinv_r, label_r};
  const size_t in_bytes[5] = {qb, rqb, rb, rrb, lb};
  for (int i = 0; i < 5; ++i)
    OSVOS_ARG_CHECK(!overlap(sim, ob, ins[i], in_bytes[i]) && !overlap(ws, wb, ins[i], in_bytes[i]), "match_topk: aliasing: sim and ws must not overlap an input");
  OSVOS_ARG_CHECK(!overlap(sim, ob, ws, wb), "match_topk: aliasing: sim and ws must be two buffers");

  int rc;
  if (K <= 4) rc = launch_topk<4>(Q, R, rinv_r, label_r, (float*)ws, N, NR, Pq, Pr, C, K, tps, slices, stream);
  else if (K <= 8) rc = launch_topk<8>(Q, R, rinv_r, label_r, (float*)ws, N, NR, Pq, Pr, C, K, tps, slices, stream);
  else rc = launch_topk<16>(Q, R, rinv_r, label_r, (float*)ws, N, NR, Pq, Pr, C, K, tps, slices, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(topk_finish_kernel, dim3((unsigned)ceil_div(Pq, THREADS), 2u, (unsigned)N), dim3(THREADS), 0, stream, (const float*)ws, rinv_q, sim, Pq, K,
                     slices);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

extern "C" int osvos_match_local(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r,
                                 float* sim, int* idx, int N, int NR, int h, int w, int C, int radius, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(Q && rinv_q && R && rinv_r && label_r && sim, "match_local: null pointer (only idx may be NULL)");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "match_local: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(NR == N || NR == 1, "match_local: NR %d reference frames (N = %d, or 1 to broadcast)", NR, N);
  OSVOS_ARG_CHECK(h >= 1 && w >= 1 && (long)h * w <= MAX_P, "match_local: grid h %d w %d (both >= 1, h w <= 2^20)", h, w);
  OSVOS_ARG_CHECK(channels_ok(C), "match_local: C %d channels (a multiple of 64, 64..%d)", C, MAX_C);
  OSVOS_ARG_CHECK(radius >= 0 && radius <= MAX_RADIUS, "match_local: radius %d cells (0..%d)", radius, MAX_RADIUS);
  OSVOS_ARG_CHECK((uintptr_t)Q % 16 == 0 && (uintptr_t)R % 16 == 0, "match_local: misaligned: Q and R must be 16-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)rinv_q % 4 == 0 && (uintptr_t)rinv_r % 4 == 0 && (uintptr_t)sim % 4 == 0 && (uintptr_t)idx % 4 == 0,
                  "match_local: misaligned: rinv_q, rinv_r, sim and idx must be 4-byte aligned");
  const size_t P = (size_t)h * w;
  const size_t qb = (size_t)N * P * C, rqb = (size_t)N * P * 4, rb = (size_t)NR * P * C, rrb = (size_t)NR * P * 4, lb = (size_t)NR * P;
  const size_t ob = (size_t)N * 2 * P * 4;
  const void* ins[5] = {Q, rinv_q, R, rinv_r, label_r};
  const size_t in_bytes[5] = {qb, rqb, rb, rrb, lb};
  for (int i = 0; i < 5; ++i)
    OSVOS_ARG_CHECK(!overlap(sim, ob, ins[i], in_bytes[i]) && !overlap(idx, ob, ins[i], in_bytes[i]), "match_local: aliasing: sim and idx must not overlap an input");
  OSVOS_ARG_CHECK(!overlap(sim, ob, idx, ob), "match_local: aliasing: sim and idx must be two buffers");
  const unsigned tiles = (unsigned)ceil_div(h, LT_H) * (unsigned)ceil_div(w, LT_W);
  hipLaunchKernelGGL(local_kernel, dim3(tiles, (unsigned)N), dim3(LTHREADS), 0, stream, Q, rinv_q, R, rinv_r, label_r, sim, idx, NR, h, w, C, radius);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
