"""Shared helpers of the ctypes op shims (torch is only the owner of device memory and streams)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .._lib import Paddle3DAmdError, check, lib

__all__ = ["lib", "check", "Paddle3DAmdError", "ptr", "stream_ptr", "require_gpu", "gpu_tensor", "gpu_rows", "nchw_pitch",
           "host_f32", "host_i32", "workspace"]


def ptr(t):
    """Device (or host) pointer of a tensor / ndarray as c_void_p; None stays NULL."""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, np.ndarray):
        return C.c_void_p(t.ctypes.data)
    return C.c_void_p(t.data_ptr())


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(t: torch.Tensor, op: str, dtype=torch.float32) -> torch.Tensor:
    """The reference ops throw PD_THROW("Unsupported device type ...") off-GPU; there is no CPU path here."""
    gpu_tensor(op, None, t, dtype=None, contiguous=False)
    if t.dtype != dtype:
        raise RuntimeError(f"{op}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def gpu_tensor(op, what, t, dtype=torch.float32, dev=None, shape=None, contiguous=True):
    """The shims' argument check: a CUDA tensor of `dtype` (None: any), on `dev` and of exactly `shape` where given,
    checked in that order; returns it contiguous unless contiguous=False."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"Unsupported device type for {op} operator.")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{op}: {what} must be {dtype}, got {t.dtype}")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{op}: {what} is on {t.device}, expected {dev}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{op}: {what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous() if contiguous else t


def gpu_rows(op, what, t, width, dtype=torch.float32):
    """gpu_tensor for a [rows, width] matrix (width None: any)."""
    gpu_tensor(op, what, t, dtype, contiguous=False)
    if t.dim() != 2 or (width is not None and int(t.shape[1]) != width):
        raise RuntimeError(f"{op}: {what} must be [rows, {width if width is not None else 'C'}], got {tuple(t.shape)}")
    return t.contiguous()


def nchw_pitch(t):
    """A [B, C, H, W] view whose rows are contiguous and whose channel planes are H * pitch apart: (tensor, batch
    stride, pitch), copied to a contiguous tensor when the view is anything else."""
    b, c, h, w = t.shape
    sb, sc, sh, sw = t.stride()
    if not (sw == 1 and sh >= w and sc == h * sh and sb >= c * sc):
        t = t.contiguous()
        sb, sh = c * h * w, w
    return t, int(sb), int(sh)


def host_f32(values, n=None):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} floats, got {a.size}")
    return a


def host_i32(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1))


def workspace(nbytes: int, device) -> torch.Tensor:
    # torch's caching allocator hands back 512-byte aligned blocks; the library wants 256
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
