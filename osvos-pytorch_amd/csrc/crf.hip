// Mask refinement: mean field of a local two-label dense CRF, logits in, logits out (the rule: include/osvos_hip.h).
//
//   z_i' = u_i + sum_{j in W(i)} k(i, j) s_j,   s_j = 2 sigmoid(z_j) - 1,   k = w_a exp(-(a_s ds + a_c dc)) + w_s exp(-g_s ds)
//
// One launch per iteration (every pixel reads a neighbourhood of the previous state, so an iteration is a grid-wide step).  A workgroup is
// 64 lanes along x times 4 waves and owns a 64 x 16 pixel tile: a thread owns the four pixels (x, y + 4 j) of its column, so the per-offset
// scalars (the two spatial factors, the LDS offset) are fetched once for four neighbours.  It stages the tile plus a halo of
// reach = radius * dilation on every side in LDS, two words per pixel:
//   sS  s = 2 sigmoid(z) - 1 of the source state (not z: one sigmoid per STAGED pixel -- 4.2 per output pixel at reach 15 -- instead of one
//       per neighbour read, 120 per output pixel at radius 5), 0 outside the image: such a neighbour adds k * 0 = 0, so the window loop
//       has no bounds test
//   sC  the frame as b | g << 8 | r << 16
// (64 + 2 reach) x (16 + 2 reach) x 8 bytes: 34.6 KB at reach 15, 36.9 KB at the limit 16 -- four workgroups per CU.  A wave reads 64
// consecutive words of one LDS row per instruction: no bank conflicts at any row pitch.
//
// Per neighbour: two ds_read_b32, three v_cvt_f32_ubyteN (unpack and convert in one instruction), three subtractions, a multiply and two
// fmas for dc (EXACT in fp32: an integer <= 195075 < 2^24), one multiply and one v_exp_f32 for the colour factor E = exp2(c2 dc) with
// c2 = -a_c log2(e), one fma for k = A E + S (A = w_a exp(-a_s ds), S = w_s exp(-g_s ds): float64 on the host, rounded once, handed over in
// the kernel arguments indexed by |dy|, |dx|) and one fma into the sum.  The alternative colour factor -- the product of three lookups of
// exp(-a_c d^2) in a 256-entry LDS table: three byte extractions, three absolute differences, three data-dependent LDS reads (64 scattered
// addresses over the banks) and two multiplies instead of the conversions, the fmas and the exp -- was built, measured 13-20 % slower and
// removed (profiles/crf_timing.txt).
//
// Error of one step against the float64 rule, in units of 2^-24 (tests/crf_cases.py derives the test bound from this): the argument
// t = c2 dc carries the rounding of c2 and of the product, a relative error of 2 x 2^-24 with x = a_c dc on E -- absolutely at most
// 2 x e^-x <= 0.74 units of A; v_exp_f32 is 1 ulp; the two fmas round once each; s carries the exp, two additions and the division.
//
// Fixed order (dy, then dx, ascending; one accumulator per pixel), no atomics: identical calls give identical bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 16, ROWS = 4;                          // tile, and the rows of it a thread owns
constexpr int MAX_LW = TILE_W + 2 * OSVOS_CRF_MAX_REACH, MAX_LH = TILE_H + 2 * OSVOS_CRF_MAX_REACH;
constexpr int NTAB = OSVOS_CRF_MAX_RADIUS + 1;

struct CrfArgs {
  const float* unary;            // [N][H][W]
  const float* src;              // [N][H][W] the state this iteration reads
  const unsigned char* bgr;      // [N][H][W][3]
  float* dst;                    // [N][H][W] the state it writes
  int H, W, radius, dilation;
  float c2;                      // -a_c log2(e)
  float A[NTAB][NTAB];           // w_a exp(-a_s ds) at (|dy|, |dx|)
  float S[NTAB][NTAB];           // w_s exp(-g_s ds)
};

// 2 sigmoid(z) - 1 = sign(z) (1 - e) / (1 + e), e = exp(-|z|) <= 1: no cancellation near 0, +-1 once e underflows
__device__ __forceinline__ float crf_s(float z) {
  const float e = expf(-fabsf(z));
  return copysignf((1.f - e) / (1.f + e), z);
}

// grid (ceil(W / 64), ceil(H / 16), N), block (64, 4)
__global__ __launch_bounds__(256) void crf_step_kernel(CrfArgs a) {
  __shared__ float sS[MAX_LH * MAX_LW];
  __shared__ unsigned sC[MAX_LH * MAX_LW];
  const int tx = threadIdx.x, ty = threadIdx.y, n = blockIdx.z;
  const int R = a.radius, D = a.dilation, reach = R * D;
  const int LW = TILE_W + 2 * reach, LH = TILE_H + 2 * reach;
  const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
  const size_t image = (size_t)n * a.H * a.W;

  for (int ly = ty; ly < LH; ly += 4) {
    const int gy = y0 - reach + ly;
    for (int lx = tx; lx < LW; lx += 64) {
      const int gx = x0 - reach + lx;
      float s = 0.f;
      unsigned c = 0u;
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
        const size_t p = image + (size_t)gy * a.W + gx;
        s = crf_s(a.src[p]);
        const unsigned char* __restrict__ q = a.bgr + p * 3;
        c = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
      }
      sS[ly * LW + lx] = s;
      sC[ly * LW + lx] = c;
    }
  }
  __syncthreads();

  const int centre = (ty + reach) * LW + tx + reach;                        // of pixel 0; pixel j is ROWS LDS rows further down
  float cb[ROWS], cg[ROWS], cr[ROWS], acc[ROWS];
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    const unsigned c = sC[centre + j * 4 * LW];
    cb[j] = (float)(c & 0xffu); cg[j] = (float)((c >> 8) & 0xffu); cr[j] = (float)((c >> 16) & 0xffu);
    acc[j] = 0.f;
  }
  for (int dy = -R; dy <= R; ++dy) {
    const int row = centre + dy * D * LW, ady = dy < 0 ? -dy : dy;
    for (int dx = -R; dx <= R; ++dx) {
      if (dy == 0 && dx == 0) continue;                                      // (uniform)
      const int adx = dx < 0 ? -dx : dx;
      const float A = a.A[ady][adx], S = a.S[ady][adx];
      const int at = row + dx * D;
#pragma unroll
      for (int j = 0; j < ROWS; ++j) {
        const float s = sS[at + j * 4 * LW];
        const unsigned c = sC[at + j * 4 * LW];
        const float db = (float)(c & 0xffu) - cb[j], dg = (float)((c >> 8) & 0xffu) - cg[j], dr = (float)((c >> 16) & 0xffu) - cr[j];
        const float dc = __builtin_fmaf(dr, dr, __builtin_fmaf(dg, dg, db * db));
        const float E = __builtin_amdgcn_exp2f(a.c2 * dc);
        acc[j] = __builtin_fmaf(__builtin_fmaf(A, E, S), s, acc[j]);
      }
    }
  }
  const int gx = x0 + tx;
  if (gx >= a.W) return;
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    const int gy = y0 + ty + 4 * j;
    if (gy >= a.H) continue;
    const size_t p = image + (size_t)gy * a.W + gx;
    const float u = a.unary[p];
    a.dst[p] = acc[j] == 0.f ? u : u + acc[j];                               // no messages: u itself, -0 included
  }
}

bool size_ok(int v) { return v >= 1 && v <= 16384; }
bool coeff_ok(float v) { return isfinite(v) && v >= 0.f; }

}  // namespace

extern "C" size_t osvos_crf_ws_bytes(int N, int H, int W, int iters) {
  if (N < 1 || N > 65535 || !size_ok(H) || !size_ok(W) || iters < 2 || iters > OSVOS_CRF_MAX_ITERS) return 0;
  return (size_t)N * H * W * sizeof(float);
}

extern "C" int osvos_crf_refine(const float* unary, const float* init, const unsigned char* bgr, float* out, void* ws, int N, int H, int W,
                                int iters, int radius, int dilation, float w_a, float w_s, float a_s, float a_c, float g_s, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(unary && bgr && out, "crf_refine: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "crf_refine: N %d images (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W), "crf_refine: bad size H %d W %d (1..16384 per side)", H, W);
  OSVOS_ARG_CHECK(iters >= 0 && iters <= OSVOS_CRF_MAX_ITERS, "crf_refine: iters %d (0..%d)", iters, OSVOS_CRF_MAX_ITERS);
  OSVOS_ARG_CHECK(radius >= 0 && radius <= OSVOS_CRF_MAX_RADIUS, "crf_refine: radius %d (0..%d)", radius, OSVOS_CRF_MAX_RADIUS);
  OSVOS_ARG_CHECK(dilation >= 1, "crf_refine: dilation %d (>= 1)", dilation);
  OSVOS_ARG_CHECK((long)radius * dilation <= OSVOS_CRF_MAX_REACH, "crf_refine: radius %d x dilation %d reaches %ld pixels (at most %d)", radius,
                  dilation, (long)radius * dilation, OSVOS_CRF_MAX_REACH);
  OSVOS_ARG_CHECK(coeff_ok(w_a) && coeff_ok(w_s) && coeff_ok(a_s) && coeff_ok(a_c) && coeff_ok(g_s),
                  "crf_refine: coefficients w_a %g w_s %g a_s %g a_c %g g_s %g must be finite and >= 0", w_a, w_s, a_s, a_c, g_s);
  OSVOS_ARG_CHECK(ws || iters < 2, "crf_refine: ws is a null pointer with iters %d (needed from 2 iterations on)", iters);
  OSVOS_ARG_CHECK((uintptr_t)unary % 4 == 0 && (uintptr_t)init % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)ws % 4 == 0,
                  "crf_refine: unary, init, out and ws must be 4-byte aligned");
  OSVOS_ARG_CHECK(out != unary && out != init, "crf_refine: out must not be unary or init (an iteration reads a neighbourhood of its source)");
  OSVOS_ARG_CHECK(!(iters >= 2 && ((const void*)ws == (const void*)unary || (const void*)ws == (const void*)init || ws == (void*)out)),
                  "crf_refine: ws must not be unary, init or out");
  const float* state = init ? init : unary;
  if (iters == 0) {
    OSVOS_HIP_CHECK(hipMemcpyAsync(out, state, (size_t)N * H * W * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
  }
  CrfArgs a;
  a.unary = unary; a.bgr = bgr; a.H = H; a.W = W; a.radius = radius; a.dilation = dilation;
  a.c2 = (float)(-(double)a_c * 1.4426950408889634074);
  for (int dy = 0; dy < NTAB; ++dy)
    for (int dx = 0; dx < NTAB; ++dx) {
      const double ds = (double)(dy * dilation) * (dy * dilation) + (double)(dx * dilation) * (dx * dilation);
      const bool used = dy <= radius && dx <= radius;
      a.A[dy][dx] = used ? (float)((double)w_a * exp(-(double)a_s * ds)) : 0.f;
      a.S[dy][dx] = used ? (float)((double)w_s * exp(-(double)g_s * ds)) : 0.f;
    }
  const dim3 grid((unsigned)ceil_div(W, TILE_W), (unsigned)ceil_div(H, TILE_H), (unsigned)N), block(64, 4);
  for (int t = 0; t < iters; ++t) {
    a.src = state;
    a.dst = (iters - 1 - t) % 2 == 0 ? out : (float*)ws;                     // the last iteration writes out
    hipLaunchKernelGGL(crf_step_kernel, grid, block, 0, stream, a);
    OSVOS_LAUNCH_CHECK();
    state = a.dst;
  }
  return 0;
}
