// Internal helpers shared by the HIP translation units of libosvos_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/osvos_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short bf16_t;   // raw bfloat16 bits
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));

void osvos_set_error(const char* fmt, ...);
int osvos_x3_pieces();             // op-level setting of osvos_set_x3_pieces on this thread (errors.cpp): read by the extern "C" op entries of api.cpp only

#define OSVOS_ARG_CHECK(cond, ...)                   \
  do {                                               \
    if (!(cond)) {                                   \
      osvos_set_error(__VA_ARGS__);                  \
      return -1;                                     \
    }                                                \
  } while (0)

#define OSVOS_HIP_CHECK(expr)                                                        \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) {                                                          \
      osvos_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      return (int)e_;                                                                \
    }                                                                                \
  } while (0)

#define OSVOS_LAUNCH_CHECK() OSVOS_HIP_CHECK(hipGetLastError())

// per-device one-time state (kernel attributes): a process may drive more than one GPU
#define OSVOS_MAX_DEVICES 64
static inline int osvos_current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= OSVOS_MAX_DEVICES) d = 0;
  return d;
}
// compute units of the current device (cached per device)
static inline int osvos_cu_count() {
  static int cus[OSVOS_MAX_DEVICES] = {};
  int& c = cus[osvos_current_device()];
  if (c == 0) {
    int v = 0;
    c = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, osvos_current_device()) == hipSuccess && v > 0) ? v : 256;
  }
  return c;
}
// a kernel's dynamic-LDS limit, raised once per device (hipFuncSetAttribute is per device).  Two host threads that launch for the first time
// may both set it (the same value); neither launches before it is set
template <auto Kernel>
static inline int osvos_set_dyn_lds_once(size_t bytes) {
  static std::atomic<bool> done[OSVOS_MAX_DEVICES];
  std::atomic<bool>& d = done[osvos_current_device()];
  if (!d.load(std::memory_order_acquire)) {
    OSVOS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    d.store(true, std::memory_order_release);
  }
  return 0;
}
// integer environment knob, read once per process (tuning / test switches must not cost a getenv per launch)
#define OSVOS_ENV_INT(var, name, dflt) static const int var = [] { const char* e_ = getenv(name); return e_ ? atoi(e_) : (dflt); }()

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// bf16 <-> f32 (round to nearest even), device + host
__host__ __device__ inline float bf16_to_f32(bf16_t v) {
  union { uint32_t u; float f; } c;
  c.u = (uint32_t)v << 16;
  return c.f;
}
__host__ __device__ inline bf16_t f32_to_bf16(float f) {
  union { uint32_t u; float f; } c;
  c.f = f;
  if ((c.u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((c.u >> 16) | 0x40);  // NaN
  uint32_t r = c.u + 0x7fffu + ((c.u >> 16) & 1u);
  return (bf16_t)(r >> 16);
}

// wave (64 lanes) sum reductions
__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// channels per 16-byte group / padded channel counts for a dtype
static inline int osvos_group(int dtype) { return dtype == OSVOS_BF16 ? 8 : 4; }
static inline int osvos_cin_pad(int cin, int dtype) { int g2 = 2 * osvos_group(dtype); return (cin + g2 - 1) / g2 * g2; }
static inline int osvos_cout_pad(int cout) { return (cout + 31) / 32 * 32; }
static inline size_t osvos_elem(int dtype) { return dtype == OSVOS_BF16 ? 2 : 4; }   // activation element size
static inline bool osvos_dtype_built(int dtype) { return dtype == OSVOS_F32 || dtype == OSVOS_F32_BF16MFMA || dtype == OSVOS_F32_X3; }

// The "dtype word" of the network calls and of the plan / pack queries (osvos_hip.h): the dtype in the low byte, OSVOS_FLAG_* above it.  Decoded
// here and nowhere else (composed in one place too: autograd.py, Precision).
struct DtypeWord {
  int dtype = OSVOS_F32;
  bool generic = false;      // OSVOS_FLAG_GENERIC_DECONV
  bool infer = false;        // OSVOS_FLAG_INFERENCE
  bool defer_join = false;   // OSVOS_FLAG_DEFER_JOIN
  bool w2 = false;           // OSVOS_FLAG_BF16_W2: two-piece forward packs (dtype OSVOS_F32_BF16MFMA only)
  bool half_fwd = false;     // OSVOS_FLAG_X3_HALF_PIECES: FP16 pairs in this call / osvos_net_pack: forward packs in that format
  bool half_bwd = false;     // OSVOS_FLAG_X3_HALF_PIECES_BWD (osvos_net_pack only): data-gradient packs in that format
  // Pieces per operand of the f32x3 kernels of the call (ConvCall::pieces, WgradCall::pieces): 3 bf16 (six products), 2 bf16 ('fp32x2',
  // OSVOS_FLAG_X3_TWO_PIECES: three products) or 22 = two FP16 under block exponents ('fp32h2', OSVOS_FLAG_X3_HALF_PIECES; h2split.h -- the packs
  // the call reads must be in that format).  3 for every other dtype
  int pieces = 3;
};
// Fills *d from `word` and makes the checks every entry makes: the dtype is built, OSVOS_FLAG_BF16_W2 only with OSVOS_F32_BF16MFMA.  false (and the
// error set, `what` = the entry's name, `not_built_note` appended to the first message) otherwise
static inline bool osvos_dtype_word(int word, const char* what, DtypeWord* d, const char* not_built_note = "") {
  d->dtype = word & 0xff;
  d->generic = (word & OSVOS_FLAG_GENERIC_DECONV) != 0;
  d->infer = (word & OSVOS_FLAG_INFERENCE) != 0;
  d->defer_join = (word & OSVOS_FLAG_DEFER_JOIN) != 0;
  d->w2 = (word & OSVOS_FLAG_BF16_W2) != 0;
  d->half_fwd = (word & OSVOS_FLAG_X3_HALF_PIECES) != 0;
  d->half_bwd = (word & OSVOS_FLAG_X3_HALF_PIECES_BWD) != 0;
  const bool x3 = d->dtype == OSVOS_F32_X3;
  d->pieces = x3 && d->half_fwd ? 22 : (x3 && (word & OSVOS_FLAG_X3_TWO_PIECES) ? 2 : 3);
  if (!osvos_dtype_built(d->dtype)) {
    osvos_set_error("%s: dtype %d not built%s", what, d->dtype, not_built_note);
    return false;
  }
  if (d->w2 && d->dtype != OSVOS_F32_BF16MFMA) {
    osvos_set_error("%s: OSVOS_FLAG_BF16_W2 needs dtype OSVOS_F32_BF16MFMA (got dtype %d)", what, d->dtype);
    return false;
  }
  return true;
}

// Slots of the 52-entry parameter / gradient arrays of osvos_net_pack / osvos_net_backward: state_dict order of networks/vgg_osvos.py.  Named here
// and nowhere else on the C side (_lib.py names the same groups for the Python side)
namespace slot {
constexpr int upscale(int i) { return i; }                 // upscale[i].weight [16][16][k][k], i = 0..3 (the fused head's deconvolutions)
constexpr int upscale_(int i) { return 4 + i; }            // upscale_[i].weight [1][1][k][k] (the side heads')
constexpr int conv_w(int l) { return 8 + 2 * l; }          // 3x3 convolution l: 0..12 the trunk (stages.*), 13..16 side_prep[0..3]
constexpr int conv_b(int l) { return conv_w(l) + 1; }
constexpr int score_dsn_w(int i) { return 42 + 2 * i; }    // score_dsn[i], i = 0..3
constexpr int score_dsn_b(int i) { return score_dsn_w(i) + 1; }
constexpr int fuse_w = 50, fuse_b = 51;
static_assert(fuse_b + 1 == OSVOS_NPARAMS && conv_w(17) == score_dsn_w(0), "the slots tile the parameter array");
}  // namespace slot
// `which` of osvos_net_ws_query: 13 trunk activations, the pooled inputs of stages 1-4, the four side_prep outputs, the NHWC input
namespace ws_which {
constexpr int act = 0, pooled = 13, prep = 17, input = 21, count = 22;
}
