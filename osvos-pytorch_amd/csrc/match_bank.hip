// Appearance matching, the memory bank that grows over the sequence: osvos_match_bank_update (the rule: include/osvos_hip.h).  The searches of
// csrc/match.hip and csrc/match_ext.hip are left alone: a bank of `cap` rows whose unused rows carry the void label is searched by them as it is.
//
//   select:    row a of the frame is selected iff label_q[a] is 0 or 1, rinv_q[a] > 0, own < tau and fl32(own - other) >= margin, own / other the
//              frame's own search result against this bank for the label's class / the other class.  Single fp32 comparisons: a NaN selects nothing.
//   subsample: n selected rows, m = min(n, max_new, ring); rank r (ascending row) is kept iff floor((r + 1) m / n) > floor(r m / n), as kept row
//              j = floor(r m / n), in 64-bit integers.
//   write:     kept row j goes to slot protected + (cursor + j) mod ring: C bytes, rinv, label.  state = {cursor, filled, calls, added_last}.
//
// Three launches on the caller's stream, 256 lanes = 4 waves, one row per lane, a workgroup owns 256 consecutive rows:
// flag_kernel     grid (ceil(P / 256), N): the flag of every row (a byte in ws) and the workgroup's count, from one __ballot per wave and the
//   four population counts added through LDS.
// scan_kernel     grid (N): ONE workgroup per bank.  Lane t adds its contiguous share of the counts, the 256 sums are scanned (shuffles inside
//   a wave, LDS across the four), and every count is replaced by the number of selected rows before its workgroup.  Lane 0 then reads state,
//   forms n, m and the cursor the scatter uses into ws, and writes the new state.  Nothing else reads or writes state, so the scatter of
//   this call and the scan of the next cannot race on it.
// scatter_kernel  grid (ceil(P / 256), N): a row's rank = its workgroup's offset + the counts of the waves before its own + the population
//   count of the ballot below its lane.  The kept rows of a wave are then copied one after the other by the whole wave, lane l moving
//   16-byte piece l of the row (C / 16 <= 64 pieces: one vector load and one vector store per lane and row); the row's own lane writes
//   rinv and the label.  m <= ring, so no slot is written twice in a call.
//
// No atomics and no workgroup that waits on another one of its launch: the order between the three steps is the stream's.  Vector stores only.
// Deterministic: identical calls give identical bytes.
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_C = 1024;
constexpr long MAX_P = 1L << 20;
constexpr int HDR = 4;                          // ints per bank at the head of ws: {n, m, cursor before the call, 0}

inline int blocks_of(int P) { return ceil_div(P, THREADS); }
// ws: hdr int [N][HDR], offs int [N][blocks], flags uint8 [N][P]
inline size_t ws_ints(int N, int P) { return (size_t)N * (HDR + blocks_of(P)); }

__device__ __forceinline__ int lanes_below(unsigned long long ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(THREADS) void flag_kernel(const float* __restrict__ rinv_q, const unsigned char* __restrict__ label_q,
                                                       const float* __restrict__ sim, unsigned char* __restrict__ flags, int* __restrict__ counts,
                                                       int P, float tau, float margin) {
  __shared__ int sCount[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.y, a = blockIdx.x * THREADS + tid;
  bool sel = false;
  if (a < P) {
    const unsigned char l = label_q[(size_t)n * P + a];
    if (l <= 1) {
      const float* s = sim + (size_t)n * 2 * P;
      const float fg = s[a], bg = s[P + a];
      const float own = l == 1 ? fg : bg, other = l == 1 ? bg : fg;
      const float gap = own - other;
      sel = rinv_q[(size_t)n * P + a] > 0.0f && own < tau && gap >= margin;
    }
    flags[(size_t)n * P + a] = sel ? 1 : 0;
  }
  const unsigned long long ballot = __ballot(sel);
  if (lane == 0) sCount[wave] = __popcll(ballot);
  __syncthreads();
  if (tid == 0) counts[(size_t)n * gridDim.x + blockIdx.x] = sCount[0] + sCount[1] + sCount[2] + sCount[3];
}

__global__ __launch_bounds__(THREADS) void scan_kernel(int* __restrict__ hdr, int* __restrict__ offs, int* __restrict__ state, int blocks, int cap,
                                                       int protected_rows, int max_new) {
  __shared__ int sWave[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  int* my = offs + (size_t)n * blocks;
  const int share = (blocks + THREADS - 1) / THREADS;
  const int b0 = min(tid * share, blocks), b1 = min(b0 + share, blocks);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += my[b];
  int incl = sum;                                                            // inclusive scan inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) sWave[wave] = incl;
  __syncthreads();
  int before = incl - sum;
  for (int w = 0; w < wave; ++w) before += sWave[w];
  for (int b = b0; b < b1; ++b) {                                            // counts -> selected rows before the workgroup
    const int c = my[b];
    my[b] = before;
    before += c;
  }
  if (tid == 0) {
    const int total = sWave[0] + sWave[1] + sWave[2] + sWave[3];
    int* st = state + (size_t)n * 4;
    const int ring = cap - protected_rows;
    int m = min(total, min(max_new, ring));
    int cursor = st[0], filled = st[1];
    if (ring > 0) {                                                          // (a state this function wrote is in range already)
      cursor %= ring;
      if (cursor < 0) cursor += ring;
    } else {
      cursor = 0;
    }
    int* h = hdr + (size_t)n * HDR;
    h[0] = total;
    h[1] = m;
    h[2] = cursor;
    h[3] = 0;
    if (m > 0) {
      st[0] = (cursor + m) % ring;
      st[1] = min(filled + m, ring);
    }
    st[2] = st[2] + 1;
    st[3] = m;
  }
}

__global__ __launch_bounds__(THREADS) void scatter_kernel(const signed char* __restrict__ q, const float* __restrict__ rinv_q,
                                                          const unsigned char* __restrict__ label_q, const unsigned char* __restrict__ flags,
                                                          const int* __restrict__ hdr, const int* __restrict__ offs, signed char* __restrict__ R,
                                                          float* __restrict__ rinv_r, unsigned char* __restrict__ label_r, int P, int C, int cap,
                                                          int protected_rows) {
  __shared__ int sCount[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.y, a = blockIdx.x * THREADS + tid;
  const int* h = hdr + (size_t)n * HDR;
  const int total = h[0], m = h[1], cursor = h[2];
  if (m <= 0 || total <= 0) return;                                          // (the whole workgroup: nothing is written)
  const int ring = cap - protected_rows;
  const bool sel = a < P && flags[(size_t)n * P + a] != 0;
  const unsigned long long ballot = __ballot(sel);
  if (lane == 0) sCount[wave] = __popcll(ballot);
  __syncthreads();
  int r = offs[(size_t)n * gridDim.x + blockIdx.x] + lanes_below(ballot, lane);
  for (int w = 0; w < wave; ++w) r += sCount[w];
  bool kept = false;
  int slot = 0;
  if (sel) {
    const long long j = (long long)r * m / total;
    kept = ((long long)(r + 1) * m / total) > j;
    slot = protected_rows + (int)((cursor + j) % ring);
  }
  kept = kept && slot >= protected_rows && slot < cap;                       // (always true under the rule: never a store outside the ring)
  signed char* Rn = R + (size_t)n * cap * C;
  const signed char* qn = q + (size_t)n * P * C;
  if (kept) {
    rinv_r[(size_t)n * cap + slot] = rinv_q[(size_t)n * P + a];
    label_r[(size_t)n * cap + slot] = label_q[(size_t)n * P + a];
  }
  const int pieces = C >> 4;                                                 // <= 64
  unsigned long long todo = __ballot(kept);
  while (todo) {                                                             // wave-uniform
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int row = __shfl(a, src, 64), dst = __shfl(slot, src, 64);
    if (lane < pieces)
      *reinterpret_cast<i32x4*>(Rn + (size_t)dst * C + lane * 16) = *reinterpret_cast<const i32x4*>(qn + (size_t)row * C + lane * 16);
  }
}

bool channels_ok(int C) { return C >= 64 && C <= MAX_C && C % 64 == 0; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
bool is_finite(float v) { return v == v && v - v == 0.0f; }

}  // namespace

// {n, m, cursor, 0} and one int per workgroup of 256 rows, then one flag byte per row
extern "C" size_t osvos_match_bank_ws_bytes(int N, int P) {
  if (N < 1 || N > 65535 || P < 1 || P > MAX_P) return 0;
  return align_up(ws_ints(N, P) * sizeof(int) + (size_t)N * P, 16);
}

extern "C" int osvos_match_bank_update(const signed char* q, const float* rinv_q, const unsigned char* label_q, const float* sim, signed char* R,
                                       float* rinv_r, unsigned char* label_r, int* state, void* ws, int N, int P, int C, int cap, int protected_rows,
                                       int max_new, float tau, float margin, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(q && rinv_q && label_q && sim && R && rinv_r && label_r && state && ws, "match_bank_update: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "match_bank_update: N %d banks (1..65535)", N);
  OSVOS_ARG_CHECK(P >= 1 && P <= MAX_P, "match_bank_update: P %d frame rows (1..2^20)", P);
  OSVOS_ARG_CHECK(channels_ok(C), "match_bank_update: C %d channels (a multiple of 64, 64..%d)", C, MAX_C);
  OSVOS_ARG_CHECK(cap >= 1 && cap <= MAX_P, "match_bank_update: cap %d bank rows (1..2^20)", cap);
  OSVOS_ARG_CHECK(protected_rows >= 0 && protected_rows <= cap, "match_bank_update: protected_rows %d (0..cap = %d)", protected_rows, cap);
  OSVOS_ARG_CHECK(max_new >= 0, "match_bank_update: max_new %d rows per call (>= 0)", max_new);
  OSVOS_ARG_CHECK(is_finite(tau), "match_bank_update: tau %g (finite)", (double)tau);
  OSVOS_ARG_CHECK(is_finite(margin), "match_bank_update: margin %g (finite)", (double)margin);
  OSVOS_ARG_CHECK((uintptr_t)q % 16 == 0 && (uintptr_t)R % 16 == 0, "match_bank_update: misaligned: q and R must be 16-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)ws % 8 == 0, "match_bank_update: misaligned: ws must be 8-byte aligned");
  OSVOS_ARG_CHECK((uintptr_t)rinv_q % 4 == 0 && (uintptr_t)sim % 4 == 0 && (uintptr_t)rinv_r % 4 == 0 && (uintptr_t)state % 4 == 0,
                  "match_bank_update: misaligned: rinv_q, sim, rinv_r and state must be 4-byte aligned");
  const void* buf[9] = {q, rinv_q, label_q, sim, R, rinv_r, label_r, state, ws};
  const size_t bytes[9] = {(size_t)N * P * C, (size_t)N * P * 4, (size_t)N * P, (size_t)N * 2 * P * 4, (size_t)N * cap * C, (size_t)N * cap * 4, (size_t)N * cap,
                           (size_t)N * 4 * sizeof(int), osvos_match_bank_ws_bytes(N, P)};
  for (int o = 4; o < 9; ++o)
    for (int i = 0; i < o; ++i)
      OSVOS_ARG_CHECK(!overlap(buf[o], bytes[o], buf[i], bytes[i]), "match_bank_update: aliasing: the bank, state and ws must not overlap the frame or each other");

  const int blocks = blocks_of(P);
  int* hdr = (int*)ws;
  int* offs = hdr + (size_t)N * HDR;
  unsigned char* flags = (unsigned char*)(hdr + ws_ints(N, P));
  const dim3 grid((unsigned)blocks, (unsigned)N);
  hipLaunchKernelGGL(flag_kernel, grid, dim3(THREADS), 0, stream, rinv_q, label_q, sim, flags, offs, P, tau, margin);
  OSVOS_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)N), dim3(THREADS), 0, stream, hdr, offs, state, blocks, cap, protected_rows, max_new);
  OSVOS_LAUNCH_CHECK();
  hipLaunchKernelGGL(scatter_kernel, grid, dim3(THREADS), 0, stream, q, rinv_q, label_q, (const unsigned char*)flags, (const int*)hdr, (const int*)offs, R, rinv_r,
                     label_r, P, C, cap, protected_rows);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
