"""CPU: the byte layouts of the packed-parameter buffer and of the workspace are pinned.

The Python side, osvos_net_ws_query and captured graphs address both buffers by offset, so a host-side change that moves one
offset by one byte is an ABI break.  tests/golden/net_layouts.json holds every size and all 22 osvos_net_ws_query records for the
four dtype words the network runs with, at four frame sizes, as the library computed them before net.cpp's tensor handles
replaced the aliasing `*_b` offsets.  Host functions only: nothing touches a GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "net_layouts.json")
# the knobs ws_layout reads (once per process): the table is that of the defaults
KNOBS = ("OSVOS_BF16_STORE", "OSVOS_MASK_BITS", "OSVOS_POOL_CODE", "OSVOS_X3_STREAMK")

DTYPES = {"F32": 0, "BF16MFMA": 2, "BF16MFMA+W2": 2 | 0x4000, "F32_X3": 3}
FRAMES = [(1, 480, 854), (12, 480, 854), (4, 1080, 1920), (2, 37, 53)]


def layout_table(lib):
    """{"dtype": {"wbuf": bytes, "N x H x W": {"ws": bytes, "ws_infer": bytes, "query": [[offset, elems, channels, h, w] x 22]}}}"""
    lib.osvos_net_wbuf_bytes.restype = lib.osvos_net_ws_bytes.restype = lib.osvos_net_ws_bytes_infer.restype = C.c_size_t
    table = {}
    for name, dt in DTYPES.items():
        t = table[name] = {"wbuf": lib.osvos_net_wbuf_bytes(dt)}
        for n, h, w in FRAMES:
            q = []
            for which in range(22):
                off, el = C.c_size_t(), C.c_size_t()
                ch, hh, ww = C.c_int(), C.c_int(), C.c_int()
                assert lib.osvos_net_ws_query(n, h, w, dt, which, C.byref(off), C.byref(el), C.byref(ch), C.byref(hh), C.byref(ww)) == 0
                q.append([off.value, el.value, ch.value, hh.value, ww.value])
            t["%dx%dx%d" % (n, h, w)] = {"ws": lib.osvos_net_ws_bytes(n, h, w, dt), "ws_infer": lib.osvos_net_ws_bytes_infer(n, h, w, dt), "query": q}
    return table


def test_layouts_equal_the_recorded_ones():
    # a fresh process without the layout knobs: the library caches them at first use
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    code = ("import json, sys; sys.path[:0] = [%r, %r]; from osvos_pytorch_amd import _lib; import test_net_layout_cpu as t; "
            "print('LAYOUT ' + json.dumps(t.layout_table(_lib.lib())))" % (REPO, os.path.join(REPO, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LAYOUT ")][-1][7:])
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    for dt in want:
        assert got[dt]["wbuf"] == want[dt]["wbuf"], dt
        for frame in want[dt]:
            assert got[dt][frame] == want[dt][frame], (dt, frame)
    assert len(want) == 4 and all(len(want[dt]) == 5 and all(len(v["query"]) == 22 for k, v in want[dt].items() if k != "wbuf") for dt in want)
