// The integer-tap bilinear sampling rule of include/osvos_hip.h (tta_tap: the one place it is written) and the thread -> pixel layout of the
// map kernels built on it (tta.hip, roi.hip): a workgroup is 64 lanes along x times 4 rows, a thread owns four pixels of its row.
#pragma once
#include "common.h"

struct Tap {
  int i0, i1;
  float f;      // weight of i1; the weight of i0 is 1 - f
};

static __device__ __forceinline__ Tap tta_tap(int i, int n_dst, int n_src) {
  const int t = (2 * i + 1) * n_src - n_dst;
  const unsigned num = t > 0 ? (unsigned)t : 0u, den = 2u * (unsigned)n_dst;
  const unsigned q = num / den;
  Tap tap;
  tap.i0 = min((int)q, n_src - 1);
  tap.i1 = min(tap.i0 + 1, n_src - 1);
  tap.f = (float)(num - q * den) / (float)den;
  return tap;
}

static __device__ __forceinline__ float tta_lerp(float a, float b, float f) {
#pragma clang fp contract(off)
  return f == 0.f ? a : (1.f - f) * a + f * b;
}

// column of pixel j of this thread
template <bool VEC>
static __device__ __forceinline__ int tta_column(int j) {
  return VEC ? (int)(blockIdx.x * 64 + threadIdx.x) * 4 + j : (int)(blockIdx.x * 256 + j * 64 + threadIdx.x);
}

template <bool VEC>
static __device__ __forceinline__ void tta_store4(float* __restrict__ row, int W, const float* v) {
  if constexpr (VEC) {
    const int x = tta_column<true>(0);
    if (x < W) {
      f32x4 q;
      q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3];
      *reinterpret_cast<f32x4*>(row + x) = q;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = tta_column<false>(j);
      if (x < W) row[x] = v[j];
    }
  }
}
