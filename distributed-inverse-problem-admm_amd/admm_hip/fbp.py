"""Filtered back projection on the GPU.

The reference's legacy loader reserves ``agg_fbp_recon`` for an "optional FBP
reconstruction" and leaves it None (block_2_test.py:11,77,135-140,164).  Here

    fbp(A, b) = A.T @ ramp_filter(b, A.geom, filter, scale=c),   c = dtheta * tau / h^2

with ``A.T`` the exact Joseph adjoint (admm_project_adj, unchanged) and ``ramp_filter`` one
HIP launch (admm_fbp_filter, csrc/fbp.hip): q[t][j] = c * tau * sum_k b[t][k] h[j - k], a direct
float64 convolution along the detector axis with the spatial taps of the band-limited ramp.

Scale.  Per angle the adjoint's two interpolation weights at a pixel sum to h^2 / tau (path
length h/|alpha| times the hat function's mass |alpha| h / tau), so A^T q ~ (h^2 / tau)
sum_t q_t(s(x)), while FBP is the integral dtheta * sum_t q_t(s(x)): c = dtheta * tau / h^2
(tau = detector spacing 2 * det_width_factor / N, h = pixel size 2 / N, dtheta =
(angle_max - angle_min) / n_angles).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .geometry import RayTransform, current_stream_handle, default_device

FILTERS = ("ram-lak", "shepp-logan", "hann")
_CODES = {"ram-lak": _lib.ADMM_FBP_RAMLAK, "shepp-logan": _lib.ADMM_FBP_SHEPP_LOGAN, "hann": _lib.ADMM_FBP_HANN}


def _check_filter(name) -> str:
    if name not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {name!r}")
    return name


def _ramlak(n: int, tau: float) -> np.ndarray:
    k = np.arange(n, dtype=np.float64)
    h = np.zeros(n, dtype=np.float64)
    odd = (np.arange(n) & 1) == 1
    h[odd] = -1.0 / (((math.pi * math.pi) * (k[odd] * k[odd])) * (tau * tau))
    h[0] = 1.0 / (4.0 * (tau * tau))
    return h


def filter_taps(name: str, n_det: int, det_spacing: float) -> np.ndarray:
    """h[0 .. n_det-1] (float64; h[-k] = h[k]) of the ramp filter ``name`` at detector spacing
    tau = ``det_spacing`` -- the closed forms csrc/fbp.hip evaluates:
    ram-lak h[0] = 1/(4 tau^2), h[k] = -1/(pi^2 k^2 tau^2) for odd k, 0 for even k;
    shepp-logan h[k] = -2/(pi^2 tau^2 (4 k^2 - 1));
    hann h[k] = rl[k]/2 + (rl[k-1] + rl[k+1])/4 with rl the ram-lak taps."""
    _check_filter(name)
    n_det = int(n_det)
    tau = float(det_spacing)
    if n_det < 1:
        raise ValueError("n_det must be >= 1")
    if not tau > 0:
        raise ValueError("det_spacing must be > 0")
    if name == "shepp-logan":
        k = np.arange(n_det, dtype=np.float64)
        return -2.0 / (((math.pi * math.pi) * (tau * tau)) * (4.0 * (k * k) - 1.0))
    rl = _ramlak(n_det + 1, tau)
    if name == "ram-lak":
        return rl[:n_det].copy()
    left = np.concatenate([rl[1:2], rl[:n_det - 1]])  # rl[k-1], rl[-1] = rl[1]
    return 0.5 * rl[:n_det] + 0.25 * (left + rl[1:n_det + 1])


def det_spacing(geom) -> float:
    """tau: uniform_partition(-w/2, w/2, n_det) cell size, w = 2 * det_width_factor."""
    return 2.0 * float(geom.det_width_factor) / geom.n_det


def fbp_scale(geom) -> float:
    """c = dtheta * tau / h^2 (module docstring): A.T @ (c-scaled filtered sinogram) is the FBP image."""
    dtheta = (float(geom.angle_max) - float(geom.angle_min)) / geom.n_angles
    hpix = 2.0 / geom.N
    return dtheta * det_spacing(geom) / (hpix * hpix)


def ramp_filter(sino, geom, filter: str = "ram-lak", scale: float = 1.0, dtype: str | None = None,
                device: int | None = None):
    """scale * tau * (sino * h) along the detector axis, on the GPU (admm_fbp_filter).

    ``sino``: a (k, m) or (m,) sinogram, m = n_angles * n_det of the parallel-beam ``geom``, as a
    numpy array or a torch tensor; returns the same kind and shape, like ``RayTransform.apply``.
    ``dtype`` "float32" / "float64": the sample type the filter reads and writes (None: float64
    for float64 input, else float32); the sums are float64 either way."""
    import torch
    _check_filter(filter)
    if not hasattr(geom, "det_width_factor"):
        raise ValueError("ramp_filter needs a parallel-beam geometry (a matrix has no detector axis)")
    if not 1 <= geom.n_det <= _lib.FBP_MAX_DET:
        raise ValueError(f"n_det must be in [1, {_lib.FBP_MAX_DET}], got {geom.n_det}")
    is_np = not isinstance(sino, torch.Tensor)
    st = torch.as_tensor(np.asarray(sino) if is_np else sino)
    if dtype is None:
        dtype = "float64" if st.dtype == torch.float64 else "float32"
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be float32 or float64")
    tdt = torch.float64 if dtype == "float64" else torch.float32
    if device is None:
        device = st.device.index if st.is_cuda else default_device()
    dev = torch.device("cuda", device)
    squeeze = st.dim() == 1
    if squeeze:
        st = st.unsqueeze(0)
    if st.dim() != 2 or st.shape[-1] != geom.m:
        raise ValueError(f"sinogram has shape {tuple(st.shape)}, expected (k, {geom.m}) or ({geom.m},)")
    st = st.to(device=dev, dtype=tdt).contiguous()
    k = st.shape[0]
    out = torch.empty_like(st)
    lib = _lib.load()
    code = _lib.ADMM_DTYPE_F64 if dtype == "float64" else _lib.ADMM_DTYPE_F32
    cap = max(1, ((1 << 31) - 1) // geom.m)  # images per launch: nimg * m < 2^31
    with torch.cuda.device(dev):
        s = current_stream_handle(dev)
        for c0 in range(0, k, cap):
            c1 = min(k, c0 + cap)
            _lib.check(lib.admm_fbp_filter(C.c_void_p(st[c0:c1].data_ptr()), C.c_void_p(out[c0:c1].data_ptr()), code,
                                           geom.n_angles, geom.n_det, c1 - c0, det_spacing(geom), float(scale),
                                           _CODES[filter], C.c_void_p(s)), "admm_fbp_filter")
    if squeeze:
        out = out[0]
    if is_np:
        return out.double().cpu().numpy() if np.asarray(sino).dtype == np.float64 else out.cpu().numpy()
    return out


def fbp(A, sino, filter: str = "ram-lak"):
    """Filtered back projection of ``sino`` with the geometric ray transform ``A``:
    ``A.T @ ramp_filter(sino, A.geom, filter, scale=fbp_scale(A.geom))`` in A's sample dtype on
    A's device.  ``sino``: (k, m), (m,) or one (n_angles, n_det) sinogram, numpy or torch;
    returns (k, n) / (n,) images of the same kind."""
    if not isinstance(A, RayTransform):
        raise ValueError("fbp needs a geometric RayTransform: an explicit-matrix operator has no detector axis")
    if A._adjoint:
        raise ValueError("fbp needs the forward operator A, not its adjoint view A.T")
    _check_filter(filter)
    g = A.geom
    shp = tuple(sino.shape) if hasattr(sino, "shape") else np.asarray(sino).shape
    if len(shp) == 2 and shp == (g.n_angles, g.n_det) and shp[1] != g.m:
        sino = sino.reshape(-1) if hasattr(sino, "reshape") else np.asarray(sino).reshape(-1)
    q = ramp_filter(sino, g, filter, scale=fbp_scale(g), dtype=A.dtype, device=A.device)
    return A.T @ q
