// Appearance matching: per-pixel int8 quantisation of a trunk feature, cell labels of a mask on the feature grid, and the labelled
// nearest-neighbour search between two quantised feature sets on the integer matrix pipe (the rule: include/osvos_hip.h).
//
//   quantise: m = max_c |f_c|; s = 127 / m; q_c = clamp(rint(f_c * s), -127, 127); n = sum q_c^2; rinv = 1 / sqrt(n)   (zeros when m is 0 or
//             not finite).  Every float operation is one IEEE fp32 operation; the two divisions and the square root are formed in double and
//             rounded once more, which is the correctly rounded fp32 result (53 >= 2 * 24 + 2 bits) whatever the fp32 code generation does.
//   nearest:  t_ab = (float) dot(Q_a, R_b) * rinv_r[b]; per query row and class (label 1 / label 0) the largest t and the smallest b that
//             attains it; sim = best * rinv_q[a]; an empty class gives (-2, -1).  Integer dots are exact: the test is bit for bit.
//
// quantize_kernel   one wave per pixel, four pixels per workgroup.  Lane l holds channels l, l + 64, .. (C / 64 <= 16 of them): coalesced loads,
//   two wave reductions (the maximum and "any element not finite"; then the integer sum of squares), coalesced byte stores.
// cell_labels_kernel  one lane per cell: counts the object pixels of the cell's (ragged at the border) footprint.
// nearest_kernel    256 lanes = 4 waves per workgroup, grid (ceil(Pq / 128), slices, N).  A workgroup owns 128 query rows, staged ONCE in LDS
//   for all C (rows of C + 16 bytes); wave w owns rows 32 w .. 32 w + 31.  It walks its slice of R in tiles of 128 reference rows, each
//   in chunks of 64 channels through a double-buffered LDS image (rows of 80 bytes) that is prefetched into registers under the MFMAs of the
//   previous chunk: one barrier per chunk.  v_mfma_i32_32x32x32_i8 with A = the reference tile, B = the wave's queries: the result has the
//   QUERY on the lane (col = lane & 31) and 16 reference rows in the registers ((reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so the running
//   (value, index) maxima of a query are two pairs of registers per lane and need no cross-lane traffic until the end.  A lane's A and B
//   fragments are the same 16 bytes (32 k + 16 (lane >> 5) ..) of a reference row and of a query row: whatever order the pipe gives the
//   32 k values of a step inside the instruction, it is the same for both operands, and an integer sum does not depend on it.  Four
//   accumulator tiles (64 registers) per wave; the epilogue of a tile reads rinv_r and the label of a row from LDS (broadcast reads),
//   walks the rows in ascending b with a strict > (the smaller b keeps a tie), and the score matrix is never written.  The two lane halves
//   are merged with one shuffle and the slice's partial (value, index) pairs go to ws.  Rows past Pq load zeros and store nothing;
//   rows past Pr load zeros and carry the void label.
// finish_kernel     one lane per (frame, class, query): walks the slices in ascending order (strict >), multiplies by rinv_q, stores.
//
// No atomics, no float reductions across lanes other than max; vector stores only.
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
constexpr int MAX_C = 1024, MAX_SLICES = 16;
constexpr long MAX_P = 1L << 20;
constexpr size_t NEAREST_LDS_MAX = (size_t)BM * (MAX_C + QPAD) + 2 * BN * RROW;      // 153600 of the 163840 bytes of a CU

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// correctly rounded fp32 quotient and square root through double (header comment)
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }

// grid ceil(P / 4); feat [P][C] fp32 (FORMAT 0) or bf16 (FORMAT 1)
template <int FORMAT>
__global__ __launch_bounds__(THREADS) void quantize_kernel(const void* __restrict__ feat, signed char* __restrict__ q, float* __restrict__ rinv,
                                                           long P, int C) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (p >= P) return;                                                        // (a whole wave: no reduction is left short)
  const int per = C >> 6;
  float f[MAX_C / 64];
  float m = 0.0f;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < MAX_C / 64; ++j) {
    f[j] = 0.0f;
    if (j < per) {
      const size_t i = (size_t)p * C + j * 64 + lane;
      f[j] = FORMAT == 1 ? bf16_to_f32(reinterpret_cast<const bf16_t*>(feat)[i]) : reinterpret_cast<const float*>(feat)[i];
      const float a = fabsf(f[j]);
      bad = bad || !(a < __builtin_inff());                                  // inf or NaN
      m = a > m ? a : m;                                                     // (a NaN never enters m; `bad` carries it)
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float other = __shfl_xor(m, o, 64);
    m = other > m ? other : m;
  }
  const bool zero = __any(bad) || m == 0.0f;
  const float s = zero ? 0.0f : div_rn(127.0f, m);
  int n = 0;
#pragma unroll
  for (int j = 0; j < MAX_C / 64; ++j) {
    if (j < per) {
      float v = rintf(f[j] * s);                                             // one multiply, half to even
      if (v != v) v = 0.0f;                                                  // 0 * inf (m below 127 / FLT_MAX): the zero stays zero
      v = v < -127.0f ? -127.0f : (v > 127.0f ? 127.0f : v);
      const int qi = (int)v;
      n += qi * qi;
      q[(size_t)p * C + j * 64 + lane] = (signed char)qi;
    }
  }
  n = wave_sum_i(n);
  if (lane == 0) rinv[p] = n ? div_rn(1.0f, sqrt_rn((float)n)) : 0.0f;       // n < 2^24: (float) n is exact
}

// one lane per cell of [N][h][w]
__global__ __launch_bounds__(THREADS) void cell_labels_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ label, int H, int W,
                                                              int h, int w, int S) {
  const int c = blockIdx.x * THREADS + threadIdx.x, n = blockIdx.y;
  if (c >= h * w) return;
  const int i = c / w, j = c - i * w;
  const int y0 = S * i, y1 = min(y0 + S, H), x0 = S * j, x1 = min(x0 + S, W);
  int k = 0;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = mask + ((size_t)n * H + y) * W;
    for (int x = x0; x < x1; ++x) k += row[x] != 0;
  }
  const int a = (y1 - y0) * (x1 - x0);
  label[(size_t)n * h * w + c] = 4 * k >= 3 * a ? 1 : (4 * k <= a ? 0 : 255);
}

struct Best {
  float v;
  int i;
};
__device__ __forceinline__ void take(Best& b, float t, int idx) {
  if (t > b.v) {
    b.v = t;
    b.i = idx;
  }
}

// grid (ceil(Pq / BM), slices, N); dynamic LDS: BM (C + QPAD) + 2 BN RROW bytes.  part [N][slices][2][Pq] (value, index)
__global__ __launch_bounds__(THREADS) void nearest_kernel(const signed char* __restrict__ Q, const signed char* __restrict__ R,
                                                          const float* __restrict__ rinv_r, const unsigned char* __restrict__ label_r,
                                                          int2* __restrict__ part, int NR, int Pq, int Pr, int C, int tiles_per_slice) {
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
  Best fg = {-__builtin_inff(), -1}, bg = {-__builtin_inff(), -1};
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
    if (kc == kch - 1) {                                                     // the tile is complete: route by label, ascending b
      const int b0 = (tile0 + j) * BN;
      const float* rv = sRinv[j & 1];
      const unsigned char* lb = sLab[j & 1];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float tv = (float)acc[mt][r] * rv[row];
          const unsigned char l = lb[row];
          if (l == 1) take(fg, tv, b0 + row);
          else if (l == 0) take(bg, tv, b0 + row);
          acc[mt][r] = 0;
        }
      }
    }
    if (t + 1 < T) commit(t + 1);
    __syncthreads();
  }

  // the other lane half saw the other reference rows of every tile
  auto merge = [&](Best& b) {
    const float ov = __shfl_xor(b.v, 32, 64);
    const int oi = __shfl_xor(b.i, 32, 64);
    if (ov > b.v || (ov == b.v && oi >= 0 && (b.i < 0 || oi < b.i))) {
      b.v = ov;
      b.i = oi;
    }
  };
  merge(fg);
  merge(bg);
  const int a = a0 + wave * 32 + col;
  if (half == 0 && a < Pq) {
    const size_t base = ((size_t)n * slices + slice) * 2 * Pq;
    part[base + a] = make_int2(__float_as_int(fg.v), fg.i);
    part[base + Pq + a] = make_int2(__float_as_int(bg.v), bg.i);
  }
}

// grid (ceil(Pq / THREADS), 2, N)
__global__ __launch_bounds__(THREADS) void finish_kernel(const int2* __restrict__ part, const float* __restrict__ rinv_q, float* __restrict__ sim,
                                                         int* __restrict__ idx, int Pq, int slices) {
  const int a = blockIdx.x * THREADS + threadIdx.x, cls = blockIdx.y, n = blockIdx.z;
  if (a >= Pq) return;
  float best = -__builtin_inff();
  int bi = -1;
  for (int s = 0; s < slices; ++s) {
    const int2 p = part[(((size_t)n * slices + s) * 2 + cls) * Pq + a];
    const float v = __int_as_float(p.x);
    if (p.y >= 0 && v > best) {                                              // ascending slices, strict >: the smaller index keeps a tie
      best = v;
      bi = p.y;
    }
  }
  const size_t o = ((size_t)n * 2 + cls) * Pq + a;
  sim[o] = bi < 0 ? -2.0f : best * rinv_q[(size_t)n * Pq + a];
  if (idx) idx[o] = bi;
}

bool channels_ok(int C) { return C >= 64 && C <= MAX_C && C % 64 == 0; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

// how the reference rows are cut: tiles of BN per slice, slices (a function of the sizes alone: ws is sized without a device)
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

}  // namespace

extern "C" int osvos_match_quantize(const void* feat, int format, signed char* q, float* rinv, long P, int C, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(feat && q && rinv, "match_quantize: null pointer (feat, q and rinv are required)");
  OSVOS_ARG_CHECK(format == 0 || format == 1, "match_quantize: format %d (0 fp32, 1 bf16)", format);
  OSVOS_ARG_CHECK(P >= 1 && P <= (1L << 30), "match_quantize: P %ld pixels (1..2^30)", P);
  OSVOS_ARG_CHECK(channels_ok(C), "match_quantize: C %d channels (a multiple of 64, 64..%d)", C, MAX_C);
  OSVOS_ARG_CHECK((uintptr_t)feat % (format ? 2 : 4) == 0 && (uintptr_t)q % 16 == 0 && (uintptr_t)rinv % 4 == 0,
                  "match_quantize: misaligned: feat by its element, q by 16 bytes, rinv by 4");
  const size_t fbytes = (size_t)P * C * (format ? 2 : 4), qbytes = (size_t)P * C, rbytes = (size_t)P * 4;
  OSVOS_ARG_CHECK(!overlap(q, qbytes, feat, fbytes) && !overlap(rinv, rbytes, feat, fbytes) && !overlap(q, qbytes, rinv, rbytes),
                  "match_quantize: aliasing: feat, q and rinv must be three buffers");
  const dim3 grid((unsigned)((P + THREADS / 64 - 1) / (THREADS / 64))), block(THREADS);
  if (format == 1) hipLaunchKernelGGL(quantize_kernel<1>, grid, block, 0, stream, feat, q, rinv, P, C);
  else hipLaunchKernelGGL(quantize_kernel<0>, grid, block, 0, stream, feat, q, rinv, P, C);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

extern "C" int osvos_match_cell_labels(const unsigned char* mask, unsigned char* label, int N, int H, int W, int h, int w, int stride, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(mask && label, "match_cell_labels: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "match_cell_labels: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "match_cell_labels: bad size H %d W %d (1..16384 per side)", H, W);
  OSVOS_ARG_CHECK(stride >= 1 && stride <= 64 && (stride & (stride - 1)) == 0, "match_cell_labels: stride %d (a power of two, 1..64)", stride);
  OSVOS_ARG_CHECK(h == ceil_div(H, stride) && w == ceil_div(W, stride), "match_cell_labels: grid h %d w %d is not ceil(H / stride) x ceil(W / stride) = %d x %d",
                  h, w, ceil_div(H, stride), ceil_div(W, stride));
  OSVOS_ARG_CHECK(!overlap(label, (size_t)N * h * w, mask, (size_t)N * H * W), "match_cell_labels: aliasing: label must not overlap mask");
  hipLaunchKernelGGL(cell_labels_kernel, dim3((unsigned)ceil_div(h * w, THREADS), (unsigned)N), dim3(THREADS), 0, stream, mask, label, H, W, h, w, stride);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

// the per-slice partial (value, index) pairs of both classes
extern "C" size_t osvos_match_ws_bytes(int N, int Pq, int Pr, int C) {
  if (N < 1 || N > 65535 || Pq < 1 || Pq > MAX_P || Pr < 1 || Pr > MAX_P || !channels_ok(C)) return 0;
  int tps, slices;
  slicing(N, Pq, Pr, &tps, &slices);
  return (size_t)N * slices * 2 * Pq * sizeof(int2);
}

extern "C" int osvos_match_nearest(const signed char* Q, const float* rinv_q, const signed char* R, const float* rinv_r, const unsigned char* label_r,
                                   float* sim, int* idx, void* ws, int N, int NR, int Pq, int Pr, int C, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(Q && rinv_q && R && rinv_r && label_r && sim && ws, "match_nearest: null pointer (only idx may be NULL)");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "match_nearest: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(NR == N || NR == 1, "match_nearest: NR %d reference frames (N = %d, or 1 to broadcast)", NR, N);
  OSVOS_ARG_CHECK(Pq >= 1 && Pq <= MAX_P, "match_nearest: Pq %d query rows (1..2^20)", Pq);
  OSVOS_ARG_CHECK(Pr >= 1 && Pr <= MAX_P, "match_nearest: Pr %d reference rows (1..2^20)", Pr);
  OSVOS_ARG_CHECK(channels_ok(C), "match_nearest: C %d channels (a multiple of 64, 64..%d)", C, MAX_C);
  OSVOS_ARG_CHECK((uintptr_t)Q % 16 == 0 && (uintptr_t)R % 16 == 0, "match_nearest: misaligned: Q and R must be 16-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)ws % 8 == 0, "match_nearest: misaligned: ws must be 8-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)rinv_q % 4 == 0 && (uintptr_t)rinv_r % 4 == 0 && (uintptr_t)sim % 4 == 0 && (uintptr_t)idx % 4 == 0,
                  "match_nearest: misaligned: rinv_q, rinv_r, sim and idx must be 4-byte aligned");
  int tps, slices;
  slicing(N, Pq, Pr, &tps, &slices);
  const size_t qb = (size_t)N * Pq * C, rqb = (size_t)N * Pq * 4, rb = (size_t)NR * Pr * C, rrb = (size_t)NR * Pr * 4, lb = (size_t)NR * Pr;
  const size_t ob = (size_t)N * 2 * Pq * 4, wb = (size_t)N * slices * 2 * Pq * sizeof(int2);
  const void* outs[3] = {sim, idx, ws};
  const size_t out_bytes[3] = {ob, ob, wb};
  const void* ins[5] = {Q, rinv_q, R, rinv_r, label_r};
  const size_t in_bytes[5] = {qb, rqb, rb, rrb, lb};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 5; ++i)
      OSVOS_ARG_CHECK(!overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]), "match_nearest: aliasing: sim, idx and ws must not overlap an input");
    for (int p = 0; p < o; ++p)
      OSVOS_ARG_CHECK(!overlap(outs[o], out_bytes[o], outs[p], out_bytes[p]), "match_nearest: aliasing: sim, idx and ws must be three buffers");
  }

  if (int rc = osvos_set_dyn_lds_once<&nearest_kernel>(NEAREST_LDS_MAX)) return rc;
  const size_t lds_bytes = (size_t)BM * (C + QPAD) + 2 * BN * RROW;
  hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)ceil_div(Pq, BM), (unsigned)slices, (unsigned)N), dim3(THREADS), lds_bytes, stream, Q, R, rinv_r, label_r,
                     (int2*)ws, NR, Pq, Pr, C, tps);
  OSVOS_LAUNCH_CHECK();
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)ceil_div(Pq, THREADS), 2u, (unsigned)N), dim3(THREADS), 0, stream, (const int2*)ws, rinv_q, sim, idx, Pq,
                     slices);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
