// Appearance matching, the softmax readout over the bank's rows next to osvos_match_nearest (csrc/match.hip and csrc/match_ext.hip, which this
// file leaves alone; the rule: include/osvos_hip.h).  STM / STCN / XMem read their memory this way: every row votes, and a class's evidence
// is the mass of its votes.
//
//   soft:  t_ab = (float) dot(Q_a, R_b) * rinv_r[b] as in nearest; cos_ab = t_ab * rinv_q[a]; e_ab = (cos_ab - 1) * k with k = beta log2(e),
//          formed once on the host; w_ab = 2^e_ab (the hardware exponential); S_c[a] = the fp32 sum of w_ab over the rows b of class c in an
//          order the sizes alone fix; lse_c[a] = 1 + ln(S_c[a]) / beta, formed in double; an empty class gives -2.  The cosine is at most 1,
//          so no weight exceeds 1: no running maximum, no rescaling, and the partial sums of slices merge by addition.  beta <= 40 keeps
//          e >= -116: no weight is denormal or zero, and S == 0 says "the class has no row".
//   best:  on request also nearest's sim, bit for bit: the largest t of the class times rinv_q, -2 for an empty class.
//
// soft_kernel<BEST>   nearest_kernel's tiling: 256 lanes = 4 waves, grid (ceil(Pq / 128), slices, N), 128 query rows staged once in LDS for all
//   C, the slice of R walked in tiles of 128 rows by chunks of 64 channels through a double-buffered LDS image that is prefetched into
//   registers under the MFMAs, v_mfma_i32_32x32x32_i8 with the QUERY on the lane.  A lane holds its query's rinv_q and four running values:
//   the sum and (BEST) the maximum of either class.  Per score: the convert, two multiplies, the subtract, the multiply by k, the
//   exponential, and the add into the sum of the row's class -- both classes take an add, the other one of +0, which changes no bit of a
//   positive sum; the label is read once per register (a broadcast read).  A row of neither class, a row past Pr among them, adds +0 to
//   both: it is masked by its label, never trusted to be small (a zero row has cosine 0 and weight exp(-beta)).  The two lane halves are
//   merged with one shuffle, low half plus high half, and the slice's partial sums (and maxima) go to ws.
// soft_finish_kernel  one lane per (frame, class, query): adds the slices' sums in ascending order, forms lse in double; with best, the
//   maximum over the slices times rinv_q.
//
// Two launches.  No atomics, no workgroup waits on another, no float reduction across lanes other than the one add of the two halves; vector
// stores only.  Every word of ws that is read was written by the same call.
#include "common.h"

#include <cmath>

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
constexpr int MAX_C = 1024, MAX_SLICES = 16;
constexpr long MAX_P = 1L << 20;
constexpr int PLANES = 4;                     // per slice in ws: S_fg, S_bg, best_fg, best_bg, each [Pq] (the last two only with best)
constexpr size_t SOFT_LDS_MAX = (size_t)BM * (MAX_C + QPAD) + 2 * BN * RROW;         // 153600 of the 163840 bytes of a CU
#define NEG_INF (-__builtin_inff())

// grid (ceil(Pq / BM), slices, N); dynamic LDS: BM (C + QPAD) + 2 BN RROW bytes.  part [N][slices][PLANES][Pq]
template <bool BEST>
__global__ __launch_bounds__(THREADS) void soft_kernel(const signed char* __restrict__ Q, const float* __restrict__ rinv_q,
                                                       const signed char* __restrict__ R, const float* __restrict__ rinv_r,
                                                       const unsigned char* __restrict__ label_r, float* __restrict__ part, int NR, int Pq, int Pr,
                                                       int C, float k, int tiles_per_slice) {
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
  const int a = a0 + wave * 32 + col;                                         // this lane's query
  const float rq = a < Pq ? rinv_q[(size_t)n * Pq + a] : 0.0f;

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
  float sum_fg = 0.0f, sum_bg = 0.0f, best_fg = NEG_INF, best_bg = NEG_INF;
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
    if (kc == kch - 1) {                                                     // the tile is complete: every row votes for its class
      const float* rv = sRinv[j & 1];
      const unsigned char* lb = sLab[j & 1];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float tv = (float)acc[mt][r] * rv[row];
          const unsigned char l = lb[row];
          const float cs = tv * rq;
          const float e = (cs - 1.0f) * k;                                   // (two operations: the file contracts nothing)
          const float w = __builtin_amdgcn_exp2f(e);
          sum_fg = sum_fg + (l == 1 ? w : 0.0f);                             // (+0 changes no bit of a sum that is +0 or positive)
          sum_bg = sum_bg + (l == 0 ? w : 0.0f);
          if (BEST) {
            if (l == 1 && tv > best_fg) best_fg = tv;
            if (l == 0 && tv > best_bg) best_bg = tv;
          }
          acc[mt][r] = 0;
        }
      }
    }
    if (t + 1 < T) commit(t + 1);
    __syncthreads();
  }

  // the other lane half saw the other reference rows of every tile: low half plus high half
  const float s_fg = sum_fg + __shfl_xor(sum_fg, 32, 64), s_bg = sum_bg + __shfl_xor(sum_bg, 32, 64);
  const size_t base = ((size_t)n * slices + slice) * PLANES * Pq;
  if (half == 0 && a < Pq) {
    part[base + a] = s_fg;
    part[base + Pq + a] = s_bg;
  }
  if (BEST) {
    const float bf = fmaxf(best_fg, __shfl_xor(best_fg, 32, 64)), bb = fmaxf(best_bg, __shfl_xor(best_bg, 32, 64));
    if (half == 0 && a < Pq) {
      part[base + 2 * (size_t)Pq + a] = bf;
      part[base + 3 * (size_t)Pq + a] = bb;
    }
  }
}

// grid (ceil(Pq / THREADS), 2, N)
__global__ __launch_bounds__(THREADS) void soft_finish_kernel(const float* __restrict__ part, const float* __restrict__ rinv_q, float* __restrict__ lse,
                                                              float* __restrict__ best, int Pq, int slices, float beta) {
  const int a = blockIdx.x * THREADS + threadIdx.x, cls = blockIdx.y, n = blockIdx.z;
  if (a >= Pq) return;
  const float* p = part + ((size_t)n * slices * PLANES + cls) * Pq + a;
  const size_t step = (size_t)PLANES * Pq;
  float s = p[0];
  for (int i = 1; i < slices; ++i) s = s + p[i * step];                      // ascending slices
  const size_t o = ((size_t)n * 2 + cls) * Pq + a;
  lse[o] = s > 0.0f ? (float)(1.0 + log((double)s) / (double)beta) : -2.0f;
  if (best) {
    float m = NEG_INF;
    for (int i = 0; i < slices; ++i) {
      const float v = p[2 * (size_t)Pq + i * step];
      if (v > m) m = v;
    }
    best[o] = m > NEG_INF ? m * rinv_q[(size_t)n * Pq + a] : -2.0f;
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

template <bool BEST>
int launch_soft(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r, float* ws, int N,
                int NR, int Pq, int Pr, int C, float k, int tps, int slices, hipStream_t stream) {
  if (int rc = osvos_set_dyn_lds_once<&soft_kernel<BEST>>(SOFT_LDS_MAX)) return rc;
  const size_t lds_bytes = (size_t)BM * (C + QPAD) + 2 * BN * RROW;
  hipLaunchKernelGGL(soft_kernel<BEST>, dim3((unsigned)ceil_div(Pq, BM), (unsigned)slices, (unsigned)N), dim3(THREADS), lds_bytes, stream, Q, rinv_q, R,
                     rinv_r, label_r, ws, NR, Pq, Pr, C, k, tps);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// the per-slice partial sums and maxima of both classes: four floats per slice and query
extern "C" size_t osvos_match_soft_ws_bytes(int N, int Pq, int Pr, int C) {
  if (N < 1 || N > 65535 || Pq < 1 || Pq > MAX_P || Pr < 1 || Pr > MAX_P || !channels_ok(C)) return 0;
  int tps, slices;
  slicing(N, Pq, Pr, &tps, &slices);
  return (size_t)N * slices * PLANES * Pq * sizeof(float);
}

extern "C" int osvos_match_soft(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r,
                                float* lse, float* best, void* ws, int N, int NR, int Pq, int Pr, int C, float beta, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(Q && rinv_q && R && rinv_r && label_r && lse && ws, "match_soft: null pointer (only best may be NULL)");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "match_soft: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(NR == N || NR == 1, "match_soft: NR %d reference frames (N = %d, or 1 to broadcast)", NR, N);
  OSVOS_ARG_CHECK(Pq >= 1 && Pq <= MAX_P, "match_soft: Pq %d query rows (1..2^20)", Pq);
  OSVOS_ARG_CHECK(Pr >= 1 && Pr <= MAX_P, "match_soft: Pr %d reference rows (1..2^20)", Pr);
  OSVOS_ARG_CHECK(channels_ok(C), "match_soft: C %d channels (a multiple of 64, 64..%d)", C, MAX_C);
  OSVOS_ARG_CHECK(beta >= OSVOS_MATCH_MIN_BETA && beta <= OSVOS_MATCH_MAX_BETA, "match_soft: beta %g is not a finite temperature in %g..%g", (double)beta,
                  (double)OSVOS_MATCH_MIN_BETA, (double)OSVOS_MATCH_MAX_BETA);      // (a NaN fails both comparisons)
  OSVOS_ARG_CHECK((uintptr_t)Q % 16 == 0 && (uintptr_t)R % 16 == 0, "match_soft: misaligned: Q and R must be 16-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)ws % 8 == 0, "match_soft: misaligned: ws must be 8-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)rinv_q % 4 == 0 && (uintptr_t)rinv_r % 4 == 0 && (uintptr_t)lse % 4 == 0 && (uintptr_t)best % 4 == 0,
                  "match_soft: misaligned: rinv_q, rinv_r, lse and best must be 4-byte aligned");
  int tps, slices;
  slicing(N, Pq, Pr, &tps, &slices);
  const size_t qb = (size_t)N * Pq * C, rqb = (size_t)N * Pq * 4, rb = (size_t)NR * Pr * C, rrb = (size_t)NR * Pr * 4, lb = (size_t)NR * Pr;
  const size_t ob = (size_t)N * 2 * Pq * 4, wb = (size_t)N * slices * PLANES * Pq * sizeof(float);
  const void* outs[3] = {lse, best, ws};
  const size_t out_bytes[3] = {ob, ob, wb};
  const void* ins[5] = {Q, rinv_q, R, rinv_r, label_r};
  const size_t in_bytes[5] = {qb, rqb, rb, rrb, lb};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 5; ++i)
      OSVOS_ARG_CHECK(!overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]), "match_soft: aliasing: lse, best and ws must not overlap an input");
    for (int p = 0; p < o; ++p)
      OSVOS_ARG_CHECK(!overlap(outs[o], out_bytes[o], outs[p], out_bytes[p]), "match_soft: aliasing: lse, best and ws must be three buffers");
  }

  const float k = (float)((double)beta * 1.4426950408889634);                // beta log2(e), once
  const int rc = best ? launch_soft<true>(Q, rinv_q, R, rinv_r, label_r, (float*)ws, N, NR, Pq, Pr, C, k, tps, slices, stream)
                      : launch_soft<false>(Q, rinv_q, R, rinv_r, label_r, (float*)ws, N, NR, Pq, Pr, C, k, tps, slices, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(soft_finish_kernel, dim3((unsigned)ceil_div(Pq, THREADS), 2u, (unsigned)N), dim3(THREADS), 0, stream, (const float*)ws, rinv_q, lse, best,
                     Pq, slices, beta);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
