// The match half of the DAVIS boundary measure (boundary.hip), shared with the per-object evaluator (objects.hip): ONE jf_match_kernel and
// ONE boundary_word serve both, a caller only has to lay its bitmaps out the way the kernel reads them.
#pragma once
#include "common.h"

// bits: per "frame" f < frames the P bitmap then the G bitmap, H * ceil(W / 64) words each -- bit i of word k of row y is pixel (y, 64 k + i),
// bits past W are zero.  Adds {|B(P)|, |B(G)|, matched of B(P), matched of B(G)} of frame f to counts[6 f + 2 .. 6 f + 5]; counts[6 f + 0 .. 1]
// (the region counts) belong to the caller's pack kernel.  frames <= 65535 (grid.y), 1 <= radius <= OSVOS_BOUNDARY_MAX_RADIUS: checked by the caller.
// who: the entry point's name, for the error text.  Internal to the library: not exported.
__attribute__((visibility("hidden"))) int osvos_jf_match(const char* who, const unsigned long long* bits, unsigned long long* counts, int frames, int H, int W,
                                                         int radius, hipStream_t stream);
