// Per-thread error string + version (libosvos_hip.so).
#include "common.h"
#include <stdlib.h>

static thread_local char g_err[512] = "";

void osvos_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* osvos_last_error(void) { return g_err; }
extern "C" int osvos_version(void) { return OSVOS_ABI_VERSION; }

// pieces per operand of the f32x3 kernels for the OP-LEVEL entries called on this host thread (api.cpp copies it into the ConvCall / WgradCall / pack it
// builds): 3 (default: three bf16 pieces, six products, fp32-grade), 2 (two bf16 pieces, three products: precision 'fp32x2') or 22 (two FP16 pieces with
// block exponents, three products: precision 'fp32h2', h2split.h).  The network calls never read it: they take the pieces from their dtype flags (net.cpp)
static thread_local int g_x3_pieces = 3;
int osvos_x3_pieces() { return g_x3_pieces; }
extern "C" int osvos_set_x3_pieces(int pieces) {
  OSVOS_ARG_CHECK(pieces == 2 || pieces == 3 || pieces == 22, "set_x3_pieces: %d (2, 3 or 22)", pieces);
  g_x3_pieces = pieces;
  return 0;
}
