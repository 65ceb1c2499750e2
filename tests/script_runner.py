"""One runner for the GPU tests that run train_online.py as a program: a subprocess on the seeded synthetic sequence 'blackswan', results and
models under the test's own directory."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def train_online(tmp, *args, height=48, width=64, epochs=5, frames=0, timeout=600):
    """``train_online.py --synthetic`` with ``args`` at the given frame size and epochs -> the finished process (its return code is 0: that
    is asserted here), with ``masks``: the bytes of Results/blackswan/%05d.png for the first ``frames`` frames (each must exist)."""
    tmp = str(tmp)
    os.makedirs(tmp, exist_ok=True)
    env = dict(os.environ, OSVOS_SAVE_ROOT=tmp, OSVOS_MODELS_DIR=tmp, PYTHONPATH=REPO, SEQ_NAME="blackswan")
    r = subprocess.run([sys.executable, "train_online.py", "--synthetic", "--epochs", str(epochs), "--height", str(height), "--width", str(width)]
                       + list(args), cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r.masks = []
    for f in range(frames):
        png = os.path.join(tmp, "Results", "blackswan", "%05d.png" % f)
        assert os.path.exists(png), png
        with open(png, "rb") as fh:
            r.masks.append(fh.read())
    return r
