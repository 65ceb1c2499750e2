#!/usr/bin/env python3
"""Every size and offset the network calls answer for a dtype word, for comparing two builds byte for byte (host only: nothing touches a GPU).

    python tools/net_layouts.py [--repo OTHER_CHECKOUT] > layouts.txt

Prints osvos_net_wbuf_bytes for the dtype words of all eight precisions (tests/test_bf16w2_cpu.py, DTYPE_WORDS), each with and without
OSVOS_FLAG_GENERIC_DECONV, and osvos_net_ws_bytes, osvos_net_ws_bytes_infer and the 22 osvos_net_ws_query records of dtypes 0, 2, 3 at four
frames.  Run it without the layout knobs (OSVOS_BF16_STORE, OSVOS_MASK_BITS, OSVOS_POOL_CODE, OSVOS_X3_STREAMK) in the environment."""
import argparse
import ctypes as C
import os
import sys

WORDS = (0x0, 0x2, 0x3, 0x803, 0x1003, 0x2003, 0x3003, 0x4002)
FRAMES = ((1, 480, 854), (12, 480, 854), (2, 48, 64), (1, 33, 47))

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=None, help="the checkout whose library answers (default: this one)")
repo = os.path.abspath(ap.parse_args().repo or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, repo)
os.environ["OSVOS_AUTOBUILD"] = "0"
from osvos_pytorch_amd import _lib  # noqa: E402

lib = _lib.lib()
for word in WORDS:
    for generic in (0, 0x100):
        print("wbuf 0x%04x %d" % (word | generic, lib.osvos_net_wbuf_bytes(word | generic)))
for dt in (0, 2, 3):
    for n, h, w in FRAMES:
        print("ws dtype %d %dx%dx%d %d infer %d" % (dt, n, h, w, lib.osvos_net_ws_bytes(n, h, w, dt), lib.osvos_net_ws_bytes_infer(n, h, w, dt)))
        for which in range(22):
            off, el, ch, hh, ww = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
            rc = lib.osvos_net_ws_query(n, h, w, dt, which, C.byref(off), C.byref(el), C.byref(ch), C.byref(hh), C.byref(ww))
            print("  query %2d rc %d offset %d elems %d channels %d h %d w %d format %d"
                  % (which, rc, off.value, el.value, ch.value, hh.value, ww.value, lib.osvos_net_ws_format(dt, which)))
