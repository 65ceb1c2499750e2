// Host-only check of the weight-gradient launchers' decisions under the address / undefined-behaviour sanitizers: osvos_wgrad_plan (the family
// choice of api.cpp and every family's choose()), the two older plan queries and osvos_wgrad_ws_bytes over the calls tests/test_wgrad_plan_cpu.py
// pins (17 layers x 4 frames x 6 arithmetics) and over the calls no launcher takes.  Needs no GPU and launches nothing; built and run by
// tools/native/wgrad_plan_check.sh.
#include <stdio.h>
#include <string.h>

#include "../../include/osvos_hip.h"

static int g_bad = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("line %d: %s  (last error: %s)\n", __LINE__, #cond, osvos_last_error()); \
      ++g_bad;                                                          \
    }                                                                   \
  } while (0)

int main() {
  static const int stage_n[5] = {2, 2, 3, 3, 3}, stage_c[5] = {64, 128, 256, 512, 512};
  struct Layer { int stage, cin, cin_s, cout; } layers[17];
  int l = 0, cin = 3;
  for (int si = 0; si < 5; ++si)
    for (int j = 0; j < stage_n[si]; ++j) {
      layers[l++] = {si, cin, cin == 3 ? 8 : cin, stage_c[si]};
      cin = stage_c[si];
    }
  for (int i = 0; i < 4; ++i) layers[13 + i] = {i + 1, stage_c[i + 1], stage_c[i + 1], 16};
  static const int frames[4][3] = {{1, 480, 854}, {12, 480, 854}, {4, 1080, 1920}, {2, 37, 53}};
  struct Mode { int dtype, store; } modes[6] = {{OSVOS_F32, 0}, {OSVOS_F32_X3, 0}, {OSVOS_F32_X3 | OSVOS_FLAG_X3_TWO_PIECES, 0},
                                               {OSVOS_F32_X3 | OSVOS_FLAG_X3_HALF_PIECES, 0}, {OSVOS_F32_BF16MFMA, 1}, {OSVOS_F32_BF16MFMA, 0}};
  int out[OSVOS_WGRAD_PLAN_INTS], wide[12], c3[5], cases = 0;
  for (const Mode& m : modes)
    for (const auto& f : frames) {
      int hs[5] = {f[1]}, ws[5] = {f[2]};
      for (int k = 1; k < 5; ++k) { hs[k] = (hs[k - 1] + 1) / 2; ws[k] = (ws[k - 1] + 1) / 2; }
      for (int li = 0; li < 17; ++li) {
        const Layer& y = layers[li];
        const int H = hs[y.stage], W = ws[y.stage];
        const int flags = (m.store && li != 0 ? OSVOS_WGRAD_PLAN_X_BF16 : 0) | (m.store ? OSVOS_WGRAD_PLAN_DY_BF16 : 0);
        EXPECT(osvos_wgrad_plan(f[0], H, W, y.cin, y.cin_s, y.cout, y.cout, m.dtype, flags, out) == 0);
        EXPECT(out[8] >= 1 && (long)(out[8] - 1) * out[7] < out[6] && (long)out[8] * out[7] >= out[6] && out[11] == out[8] * out[9] * out[10]);
        EXPECT(osvos_wgrad_ws_bytes(f[0], H, W, y.cin_s, y.cout, m.dtype & 0xff) >= ((size_t)out[14] + (size_t)out[15]) * 4);
        EXPECT(osvos_wgrad_plan(f[0], H, W, y.cin, y.cin_s, y.cout, y.cout, m.dtype, flags | OSVOS_WGRAD_PLAN_NO_BIAS, out) == 0);
        const bool is_wide = out[0] == OSVOS_WGRAD_FAMILY_F32X3 || out[0] == OSVOS_WGRAD_FAMILY_BF16;
        EXPECT((osvos_wgrad_wide_plan(f[0], H, W, y.cin_s, y.cout, m.dtype & 0xff, m.store, wide) == 0) == is_wide);
        if (is_wide) EXPECT(memcmp(wide, out + 2, 11 * sizeof(int)) == 0);
        if (li == 0) EXPECT(osvos_wgrad_c3_plan(f[0], H, W, m.store, c3) == 0 && memcmp(c3, out + 4, 5 * sizeof(int)) == 0);
        ++cases;
      }
    }
  // calls no launcher takes: each is an argument error, none a crash
  EXPECT(osvos_wgrad_plan(1, 16, 16, 64, 64, 64, 64, OSVOS_F32_X3, 0, nullptr) < 0);
  EXPECT(osvos_wgrad_plan(0, 16, 16, 64, 64, 64, 64, OSVOS_F32_X3, 0, out) < 0);
  EXPECT(osvos_wgrad_plan(1, 16, 16, 64, 64, 64, 64, OSVOS_BF16, 0, out) < 0);
  EXPECT(osvos_wgrad_plan(1, 16, 16, 64, 64, 64, 64, OSVOS_F32_X3, OSVOS_WGRAD_PLAN_X_BF16, out) < 0);
  EXPECT(osvos_wgrad_plan(1, 16, 16, 64, 64, 64, 64, OSVOS_F32_BF16MFMA, OSVOS_WGRAD_PLAN_DY_BF16, out) < 0);
  EXPECT(osvos_wgrad_plan(1, 16, 16, 32, 32, 16, 16, OSVOS_F32_BF16MFMA, OSVOS_WGRAD_PLAN_DY_BF16, out) < 0);
  EXPECT(osvos_wgrad_plan(1, 16, 16, 24, 24, 64, 64, OSVOS_F32_BF16MFMA, OSVOS_WGRAD_PLAN_X_BF16 | OSVOS_WGRAD_PLAN_DY_BF16, out) < 0);
  EXPECT(osvos_wgrad_plan(1, 16, 16, 3, 8, 62, 62, OSVOS_F32, 0, out) < 0);                  // Cout % 4
  EXPECT(osvos_wgrad_plan(1, 16, 16, 64, 62, 64, 64, OSVOS_F32, 0, out) < 0);                // Cin > Cin_s
  EXPECT(osvos_wgrad_plan(1, 40000, 40000, 64, 64, 64, 64, OSVOS_F32_X3, 0, out) < 0);       // 31-bit byte offsets
  EXPECT(osvos_wgrad_plan(1, 1, 1, 3, 8, 64, 64, OSVOS_F32, 0, out) == 0 && out[8] == 1);    // one pixel, one split
  EXPECT(osvos_wgrad_wide_plan(2, 8, 8, 64, 64, OSVOS_F32_X3, 0, nullptr) < 0);
  EXPECT(osvos_wgrad_wide_plan(2, 8, 8, 64, 64, OSVOS_F32, 0, wide) < 0);
  EXPECT(osvos_wgrad_c3_plan(0, 8, 8, 0, c3) < 0);
  EXPECT(osvos_wgrad_ws_bytes(1, 1, 1, 1, 1, OSVOS_F32) > 0);
  printf("wgrad_plan_check: %d pinned cases, %d failed expectations\n", cases, g_bad);
  return g_bad ? 1 : 0;
}
