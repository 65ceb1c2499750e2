"""GPU: train_online.py with the stages of the test phase stacked -- each recipe of osvos_pytorch_amd.sequence once, as a program, on the
smallest synthetic run the script tests use (48 x 64, 5 epochs).  The order of the stages is asserted on the CPU, tests/test_sequence_cpu.py;
here the real stages run together and each one's summary line is printed."""
import pytest

import script_runner

pytestmark = pytest.mark.gpu


def test_train_online_single_object_with_the_stages_stacked(tmp_path):
    out = script_runner.train_online(tmp_path, "--device-augment", "--synthetic-frames", "3", "--match-gain", "2", "--adapt-steps", "2", "--adapt-mix", "2",
                                     "--adapt-erosion", "2", "--adapt-distance", "12", "--flow-search", "8", "--flow-block", "8", "--crf-iters", "1",
                                     "--snap-cell", "6", "--track-components", "2", frames=3).stdout
    assert "J&F on blackswan:" in out and "Components kept on blackswan:" in out, out[-2000:]
    assert "Online adaptation on blackswan: 2 frames seen" in out, out[-2000:]


def test_train_online_multi_object_with_the_stages_stacked(tmp_path):
    out = script_runner.train_online(tmp_path, "--multi-object", "--match-gain", "2", "--match-previous", "--crf-iters", "1", "--snap-cell", "6",
                                     "--snap-iters", "2", "--track-components", "2", frames=1).stdout
    assert "J&F on blackswan (2 objects):" in out and "Components kept on blackswan object 2:" in out, out[-2000:]
