// Test-time augmentation around the network (multi-scale and mirrored views, fused on the device).
//
//   osvos_tta_view   decoded uint8 BGR frames [N][H][W][3] -> one network input [N][3][Hv][Wv] fp32: the bilinear resample of every channel
//                    minus mean3[c], optionally mirrored (destination column x holds what the plain view holds at column Wv - 1 - x).
//   osvos_tta_fuse   V logit maps [N][Hv[v]][Wv[v]] of different sizes -> out [N][H][W] = sum_v weight[v] * sample_v(y, x): each view resampled
//                    onto the H x W grid, read through column Wv - 1 - c when it came from a mirrored input.  Logits, never sigmoids.
//
// Sampling rule (tta_tap in tta_tap.h, the one place it is written): separable bilinear with half-pixel centres -- F.interpolate(mode='bilinear',
// align_corners=False)'s geometry -- with the taps in INTEGERS: for destination i of n_dst over n_src,
//   num = max((2 i + 1) n_src - n_dst, 0), den = 2 n_dst, i0 = min(num / den, n_src - 1), i1 = min(i0 + 1, n_src - 1), f = (num % den) / den
// (sizes <= 16384 keep num inside int32; num % den and den are exact in fp32, so f carries one rounding and is 0 exactly when the tap falls on
// a source sample).  A tap of weight zero is SELECTED away, never multiplied by zero (tta_lerp): a view of the grid's own size passes through
// bit for bit whatever it holds, inf and NaN included, and the same-size unmirrored view of osvos_tta_view is osvos_augment_frame's identity
// output ((float)byte - mean, the same two operations).  The x pass comes first, then the y pass; no fused multiply-adds.
//
// Both kernels are maps with no LDS, atomics or workspace.  A workgroup is 64 lanes along x times 4 rows, one wave per row; a thread owns
// four pixels of its row, so a row's y taps (per view, in the fuse kernel) are computed once per thread, not per pixel, and a whole-pixel
// row (f = 0 in y: every same-height view) never loads its second source row (a wave-uniform branch).  VEC: the four pixels are consecutive
// and leave as one 16-byte store -- a wave's store instruction is 1 KB of one row -- which needs the row length to be a multiple of 4 and a
// 16-byte aligned output; otherwise the thread's pixels are 64 apart and every store instruction of a wave is 256 consecutive bytes.  The
// sources are gathered with 1- and 4-byte loads (neighbouring lanes read neighbouring or equal addresses), so views need 4-byte alignment
// only.  The fuse kernel takes its table of views BY VALUE in the kernel arguments: no device upload, nothing to free.
#include "common.h"
#include "tta_tap.h"      // Tap, tta_tap, tta_lerp, tta_column, tta_store4 (shared with roi.hip)

namespace {

struct ViewArgs {
  const unsigned char* bgr;      // [N][H][W][3]
  float* out;                    // [N][3][Hv][Wv]
  float mean[3];
  int H, W, Hv, Wv, flip;
};

// grid (ceil(Wv / 256), ceil(Hv / 4), N), block (64, 4)
template <bool VEC>
__global__ __launch_bounds__(256) void tta_view_kernel(ViewArgs a) {
#pragma clang fp contract(off)
  const int y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (y >= a.Hv) return;
  const Tap ty = tta_tap(y, a.Hv, a.H);
  const unsigned char* __restrict__ r0 = a.bgr + ((size_t)n * a.H + ty.i0) * a.W * 3;
  const unsigned char* __restrict__ r1 = a.bgr + ((size_t)n * a.H + ty.i1) * a.W * 3;
  float v[3][4] = {};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = tta_column<VEC>(j);
    if (x >= a.Wv) continue;
    const Tap tx = tta_tap(a.flip ? a.Wv - 1 - x : x, a.Wv, a.W);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][j] = tta_lerp((float)r0[tx.i0 * 3 + c], (float)r0[tx.i1 * 3 + c], tx.f);
    if (ty.f != 0.f) {                                                                     // (wave-uniform)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][j] = tta_lerp(v[c][j], tta_lerp((float)r1[tx.i0 * 3 + c], (float)r1[tx.i1 * 3 + c], tx.f), ty.f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][j] = v[c][j] - a.mean[c];
  }
  const size_t plane = (size_t)a.Hv * a.Wv;
  float* __restrict__ o = a.out + (size_t)n * 3 * plane + (size_t)y * a.Wv;
#pragma unroll
  for (int c = 0; c < 3; ++c) tta_store4<VEC>(o + c * plane, a.Wv, v[c]);
}

struct FuseArgs {
  const float* view[OSVOS_TTA_MAX_VIEWS];      // [N][hv][wv]
  int hv[OSVOS_TTA_MAX_VIEWS], wv[OSVOS_TTA_MAX_VIEWS], flip[OSVOS_TTA_MAX_VIEWS];
  float weight[OSVOS_TTA_MAX_VIEWS];
  float* out;                                  // [N][H][W]
  int V, H, W;
};

// grid (ceil(W / 256), ceil(H / 4), N), block (64, 4)
template <bool VEC>
__global__ __launch_bounds__(256) void tta_fuse_kernel(FuseArgs a) {
#pragma clang fp contract(off)
  const int y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (y >= a.H) return;
  float acc[4] = {};
  for (int v = 0; v < a.V; ++v) {
    const int hv = a.hv[v], wv = a.wv[v], flip = a.flip[v];
    const float w = a.weight[v];
    const Tap ty = tta_tap(y, a.H, hv);                                                    // once per view and row, for the thread's four pixels
    const float* __restrict__ r0 = a.view[v] + ((size_t)n * hv + ty.i0) * wv;
    const float* __restrict__ r1 = a.view[v] + ((size_t)n * hv + ty.i1) * wv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = tta_column<VEC>(j);
      if (x >= a.W) continue;
      const Tap tx = tta_tap(x, a.W, wv);
      const int c0 = flip ? wv - 1 - tx.i0 : tx.i0, c1 = flip ? wv - 1 - tx.i1 : tx.i1;
      float s = tta_lerp(r0[c0], r0[c1], tx.f);
      if (ty.f != 0.f) s = tta_lerp(s, tta_lerp(r1[c0], r1[c1], tx.f), ty.f);              // (wave-uniform)
      acc[j] = v == 0 ? w * s : acc[j] + w * s;                                            // the first view starts the sum: no 0 + x
    }
  }
  tta_store4<VEC>(a.out + ((size_t)n * a.H + y) * a.W, a.W, acc);
}

bool size_ok(int v) { return v >= 1 && v <= 16384; }

}  // namespace

// bgr: device uint8 [N][H][W][3]; mean3: HOST pointer to 3 floats; out: device fp32 [N][3][Hv][Wv]
extern "C" int osvos_tta_view(const unsigned char* bgr, const float* mean3, float* out, int N, int H, int W, int Hv, int Wv, int flip, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(bgr && mean3 && out, "tta_view: null pointer");
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "tta_view: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W) && size_ok(Hv) && size_ok(Wv), "tta_view: bad size H %d W %d -> Hv %d Wv %d (1..16384 per side)", H, W, Hv,
                  Wv);
  OSVOS_ARG_CHECK((uintptr_t)out % 4 == 0, "tta_view: out must be 4-byte aligned");
  ViewArgs a;
  a.bgr = bgr; a.out = out; a.H = H; a.W = W; a.Hv = Hv; a.Wv = Wv; a.flip = flip ? 1 : 0;
  for (int c = 0; c < 3; ++c) a.mean[c] = mean3[c];
  const dim3 grid((unsigned)((Wv + 255) / 256), (unsigned)((Hv + 3) / 4), (unsigned)N), block(64, 4);
  if (Wv % 4 == 0 && (uintptr_t)out % 16 == 0)
    hipLaunchKernelGGL(tta_view_kernel<true>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(tta_view_kernel<false>, grid, block, 0, stream, a);
  OSVOS_LAUNCH_CHECK();
  return 0;
}

// views, Hv, Wv, flip, weight: HOST arrays of length V (views holds device pointers; weight may be NULL: 1 / V each); out: device fp32 [N][H][W]
extern "C" int osvos_tta_fuse(const float* const* views, const int* Hv, const int* Wv, const int* flip, const float* weight, int V, float* out, int N,
                              int H, int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OSVOS_ARG_CHECK(views && Hv && Wv && flip && out, "tta_fuse: null pointer");
  OSVOS_ARG_CHECK(V >= 1 && V <= OSVOS_TTA_MAX_VIEWS, "tta_fuse: V %d views (1..%d)", V, OSVOS_TTA_MAX_VIEWS);
  OSVOS_ARG_CHECK(N >= 1 && N <= 65535, "tta_fuse: N %d frames (1..65535)", N);
  OSVOS_ARG_CHECK(size_ok(H) && size_ok(W), "tta_fuse: bad size H %d W %d (1..16384 per side)", H, W);
  OSVOS_ARG_CHECK((uintptr_t)out % 4 == 0, "tta_fuse: out must be 4-byte aligned");
  FuseArgs a;
  a.out = out; a.V = V; a.H = H; a.W = W;
  for (int v = 0; v < OSVOS_TTA_MAX_VIEWS; ++v) {
    const int s = v < V ? v : 0;                                                           // (unused slots repeat view 0: never read)
    if (v < V) {
      OSVOS_ARG_CHECK(views[v] != nullptr, "tta_fuse: view %d is a null pointer", v);
      OSVOS_ARG_CHECK((uintptr_t)views[v] % 4 == 0, "tta_fuse: view %d must be 4-byte aligned", v);
      OSVOS_ARG_CHECK(size_ok(Hv[v]) && size_ok(Wv[v]), "tta_fuse: view %d has bad size Hv %d Wv %d (1..16384 per side)", v, Hv[v], Wv[v]);
    }
    a.view[v] = views[s]; a.hv[v] = Hv[s]; a.wv[v] = Wv[s]; a.flip[v] = flip[s] ? 1 : 0;
    a.weight[v] = weight ? weight[s] : 1.0f / (float)V;
  }
  const dim3 grid((unsigned)((W + 255) / 256), (unsigned)((H + 3) / 4), (unsigned)N), block(64, 4);
  if (W % 4 == 0 && (uintptr_t)out % 16 == 0)
    hipLaunchKernelGGL(tta_fuse_kernel<true>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(tta_fuse_kernel<false>, grid, block, 0, stream, a);
  OSVOS_LAUNCH_CHECK();
  return 0;
}
