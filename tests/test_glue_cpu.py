"""CPU: the host plumbing every stage wrapper shares (osvos_pytorch_amd._glue).  Its shape rules, number checks, workspace rule and
option-list parser read shape, dtype and device only, so they are exercised here on CPU tensors; the device-guarded call itself is covered on
the GPU (tests/test_gpu_glue.py and every stage's GPU test)."""
import numpy as np
import pytest
import torch

from osvos_pytorch_amd import _glue as g
from osvos_pytorch_amd import flow, superpixels


def test_planes_accept_the_three_layouts_and_refuse_the_rest():
    for shape, nhw in (((2, 1, 5, 7), (2, 5, 7)), ((2, 5, 7), (2, 5, 7)), ((5, 7), (1, 5, 7))):
        t, n, h, w = g.planes(torch.zeros(shape), "x", (torch.float32,), 16)
        assert (n, h, w) == nhw and tuple(t.shape) == shape and t.is_contiguous()
    t = g.planes(torch.zeros(7, 2, 5).permute(1, 2, 0), "x", (torch.float32,))[0]
    assert t.is_contiguous() and tuple(t.shape) == (2, 5, 7)
    with pytest.raises(ValueError, match="x must be"):
        g.planes(torch.zeros(2, 2, 5, 7), "x", (torch.float32,))                       # two channels
    with pytest.raises(ValueError, match="x must be"):
        g.planes(torch.zeros(2, 5, 7, dtype=torch.float64), "x", (torch.float32, torch.uint8))
    with pytest.raises(ValueError, match="sides 1..6"):
        g.planes(torch.zeros(2, 5, 7), "x", (torch.float32,), 6)
    with pytest.raises(ValueError, match="N >= 1"):
        g.planes(torch.zeros(0, 5, 7), "x", (torch.float32,), 16)
    with pytest.raises(ValueError, match="x must be"):
        g.planes(torch.zeros(5, 7), "x", (torch.float32,), dims=(3, 4))                 # a caller that takes no single plane
    assert g.planes(torch.zeros(2, 5, 7, dtype=torch.float64), "x")[1:] == (2, 5, 7)       # dtypes None: any
    assert g.planes(torch.zeros(0, 5, 70000), "x")[1:] == (0, 5, 70000)                    # no limit given, none applied


def test_frames_take_a_single_frame_only_where_the_caller_does():
    one, four = torch.zeros(5, 7, 3, dtype=torch.uint8), torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    assert tuple(g.frames(one, "f", 16).shape) == (1, 5, 7, 3) and tuple(g.frames(four, "f", 16).shape) == (2, 5, 7, 3)
    assert g.frames(four.permute(0, 2, 1, 3), "f").is_contiguous()
    with pytest.raises(ValueError, match=r"f must be a uint8 \[N,H,W,3\] tensor"):
        g.frames(one, "f", single=False)
    with pytest.raises(ValueError, match=r"f must be a uint8 \[H,W,3\] tensor"):
        g.frames(four, "f", batch=False)
    for bad in (torch.zeros(2, 5, 7, 3), torch.zeros(2, 5, 7, 4, dtype=torch.uint8), torch.zeros(7, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="f must be"):
            g.frames(bad, "f", 16)
    with pytest.raises(ValueError, match="sides 1..6"):
        g.frames(four, "f", 6)
    assert tuple(g.frames(four, "f").shape) == (2, 5, 7, 3)                                # no limit given, none applied


def test_out_buffer_checks_dtype_shape_contiguity_device_and_aliasing():
    dev = torch.device("cpu")
    out = torch.zeros(2, 1, 5, 7)
    assert g.out_buffer(out, torch.float32, (2, 1, 5, 7), dev, "the device") is out
    new = g.out_buffer(None, torch.int32, (2, 4), dev, "the device")
    assert new.dtype == torch.int32 and tuple(new.shape) == (2, 4)
    for bad in (out.double(), torch.zeros(2, 5, 7), torch.zeros(2, 1, 7, 5).transpose(2, 3), out.to("meta")):
        with pytest.raises(ValueError, match="out must be a contiguous float32"):
            g.out_buffer(bad, torch.float32, (2, 1, 5, 7), dev, "the device")
    with pytest.raises(ValueError, match="out must not be the logits"):
        g.out_buffer(out, torch.float32, (2, 1, 5, 7), dev, "the device", alias=(("init", None), ("the logits", out.view(2, 5, 7))))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.out_buffer(out, torch.float32, (2, 1, 5, 7), dev, "the device", module="roi")


def test_need_cuda_refuses_cpu_tensors_and_non_tensors():
    for bad in (torch.zeros(3), None, np.zeros(3), 1.0):
        with pytest.raises(RuntimeError, match=r"osvos_pytorch_amd\.flow needs CUDA \(ROCm\) tensors \(src\); there is no CPU fallback"):
            g.need_cuda(bad, "src", "flow")


def test_check_int_and_check_number():
    for ok in (3, np.int64(3), np.uint8(3)):
        g.check_int("k", ok, 1, 3, "stage")
    g.check_int("k", 10 ** 12, 1, None, "stage")
    for bad in (True, 2.0, np.float32(2), "2", None):
        with pytest.raises(ValueError, match="stage: k must be an integer"):
            g.check_int("k", bad, 0, 3, "stage")
    for bad in (-1, 4):
        with pytest.raises(ValueError, match=r"stage: k -?\d \(0\.\.3\)"):
            g.check_int("k", bad, 0, 3, "stage")
    with pytest.raises(ValueError, match=r"stage: k 0 \(>= 1\)"):
        g.check_int("k", 0, 1, None, "stage")
    with pytest.raises(ValueError, match="must be an integer"):
        g.check_int("k", np.int64(3), 1, 3, "stage", numpy=False)
    for ok in (0, 0.5, 1.0, np.float32(0.25), np.int32(1)):
        g.check_number("p", ok, 0, 1, "stage")
    for bad in (True, "0.5", None, float("nan"), float("inf"), -0.1, 1.5):
        with pytest.raises(ValueError, match="stage: p .* finite number in 0..1"):
            g.check_number("p", bad, 0, 1, "stage")
    g.check_number("z", 1e30, 1, None, "stage")
    with pytest.raises(ValueError, match="stage: z .*>= 1"):
        g.check_number("z", 0.5, 1, None, "stage")
    with pytest.raises(ValueError):
        g.check_number("z", np.float32(2), 1, None, "stage", numpy=False)


def test_grid_shape_is_one_function():
    assert g.grid_shape(13, 18, 4) == (4, 5) and g.grid_shape(12, 16, 4) == (3, 4) and g.grid_shape(1, 1, 64) == (1, 1)
    assert flow.grid_shape is g.grid_shape and superpixels.grid_shape is g.grid_shape


def test_workspace_compares_bytes_and_reuses_what_fits():
    cpu = torch.device("cpu")
    ws = torch.zeros(4, dtype=torch.int32)
    assert g.workspace(16, cpu, ws) is ws                                                   # 4 int32 are 16 bytes
    assert g.workspace(np.uint64(9), cpu, ws) is ws
    grown = g.workspace(17, cpu, ws)
    assert grown is not ws and grown.dtype == torch.uint8 and grown.numel() == 17
    assert g.workspace(16, torch.device("meta"), ws).device.type == "meta"                   # on another device: a new one
    fresh = g.workspace(17, cpu, dtype=torch.int64)
    assert fresh.dtype == torch.int64 and fresh.numel() == 3 and fresh.device == cpu
    assert g.workspace(8, cpu, "not a tensor").numel() == 8
    off = torch.zeros(32, dtype=torch.uint8)[4:]
    assert g.workspace(8, cpu, off) is off and g.workspace(8, cpu, off, align=8) is not off      # (the allocation starts on a multiple of 8)
    with pytest.raises(ValueError, match="stage: no workspace size for 3 frames"):
        g.workspace(0, cpu, ws, "3 frames", "stage")


def test_parse_numbers():
    assert g.parse_numbers("4, 1", (float, float), "--w") == (4.0, 1.0)
    got = g.parse_numbers("25,8", (int, int), "--m")
    assert got == (25, 8) and all(type(v) is int for v in got)
    assert g.parse_numbers("240x427", (int, int), "--c", sep="x") == (240, 427) and g.parse_numbers("240X427", (int, int), "--c", sep="x") == (240, 427)
    assert g.parse_numbers("0.2,20", (float, int), "--t") == (0.2, 20) and g.parse_numbers("0.5", (float,), "--d") == (0.5,)
    for bad in ("4", "4,x", "4,1,2", "", None, "4,1.5"):
        with pytest.raises(ValueError, match="--m takes 2 comma-separated numbers, got"):
            g.parse_numbers(bad, (float, int), "--m")
    with pytest.raises(ValueError, match=r"--c takes HxW, got '240,427'"):
        g.parse_numbers("240,427", (int, int), "--c", sep="x", expect="HxW")
    with pytest.raises(ValueError, match="--w takes finite numbers, got 'nan,1'"):
        g.parse_numbers("nan,1", (float, float), "--w", finite=True)
    with pytest.raises(ValueError, match="--w takes finite numbers"):
        g.parse_numbers("1,inf", (float, float), "--w", finite=True)
    assert np.isnan(g.parse_numbers("nan,1", (float, float), "--w")[0])                      # finite numbers only where they are asked for
