"""PSNR and SSIM of reconstructions against a reference image, on the GPU (SURVEY.md 8f row f6;
DESIGN.md 6.7).

The reference scores strategies by PSNR (test_final_integration.py:41-50):

    mse = mean((x_hat - x_true)^2);  psnr = 20 log10(L) - 10 log10(mse)   (inf when mse == 0)

with L = ``data_range`` = x_true.max() - x_true.min(), then the mean over nodes.  SSIM is Wang et
al. 2004 as skimage's ``structural_similarity(gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=L)`` computes it: the mean of the SSIM map over the valid
window centres 5 <= i, j <= N - 6, c1 = (0.01 L)^2, c2 = (0.03 L)^2.

One launch pair (admm_image_metrics, csrc/metrics.hip) returns the squared error and the SSIM sum
of every image of a float64 ``(V, n)`` device batch; the divisions by the pixel counts and the
logarithms are elementwise torch expressions on the device, so nothing here synchronises with the
host once a ``Scorer`` exists.  ``run_admm(metrics=...)`` scores every iteration's images with it.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .geometry import current_stream_handle, default_device

METRICS = ("psnr", "ssim")
RADIUS = 5  # 11 x 11 window


def check_metrics(metrics):
    """None, or the requested subset of METRICS as a tuple (a single name is accepted)."""
    if metrics is None:
        return None
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(metrics)
    if not metrics or any(m not in METRICS for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics must be None or a subset of {METRICS}, got {metrics!r}")
    return metrics


def check_side(N) -> int:
    N = int(N)
    if N < _lib.METRICS_MIN_N:
        raise ValueError(f"image metrics need N >= {_lib.METRICS_MIN_N} (one 11 x 11 SSIM window), got N = {N}")
    if N > _lib.METRICS_MAX_N:
        raise ValueError(f"image metrics need N <= {_lib.METRICS_MAX_N}, got N = {N}")
    return N


def check_data_range(data_range):
    """None or a float > 0 (ValueError otherwise): argument check, no device work."""
    if data_range is None:
        return None
    L = float(data_range)
    if not (L > 0 and math.isfinite(L)):
        raise ValueError(f"data_range must be > 0 and finite, got {data_range!r}")
    return L


def _side(numel: int) -> int:
    N = math.isqrt(int(numel))
    if N * N != numel:
        raise ValueError(f"an image of {numel} pixels is not square")
    return N


def _shape_of(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape


def _ref_side(ref) -> int:
    shp = _shape_of(ref)
    if len(shp) == 2 and shp[0] == shp[1]:
        return check_side(shp[0])
    if len(shp) == 1:
        return check_side(_side(shp[0]))
    raise ValueError(f"ref must be one (N, N) or (n,) image, got shape {shp}")


def _check_mask_shape(mask, N: int) -> None:
    shp = _shape_of(mask)
    if shp not in ((N, N), (N * N,)):
        raise ValueError(f"mask has shape {shp}, expected ({N}, {N}) or ({N * N},)")


def _batch_shape(x, N: int):
    """(V, squeeze) of an image batch shaped (N, N), (n,), (V, n) or (V, N, N)."""
    shp = _shape_of(x)
    n = N * N
    if shp in ((N, N), (n,)):
        return 1, True
    if len(shp) == 2 and shp[1] == n or len(shp) == 3 and shp[1:] == (N, N):
        if shp[0] < 1:
            raise ValueError("x holds no image")
        return shp[0], False
    raise ValueError(f"x has shape {shp}; expected ({N}, {N}), ({n},), (V, {n}) or (V, {N}, {N}) to match ref")


class Scorer:
    """Scores float64 device image batches against one reference: the state ``image_metrics`` and
    ``run_admm`` share -- the reference and mask on the device, L, c1, c2, the two pixel counts
    (computed once from the mask with torch) and the kernel's scratch.  Argument errors are raised
    before any device work."""

    def __init__(self, ref, data_range=None, mask=None, device: int | None = None, max_images: int = 1):
        import torch
        N = _ref_side(ref)
        L = check_data_range(data_range)
        self.N, self.n = N, N * N
        v = N - 2 * RADIUS
        self.count, self.count_valid = float(self.n), float(v * v)
        mt = None
        if mask is not None:  # counted where the mask lives, before anything is uploaded
            _check_mask_shape(mask, N)
            mt = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
            mt = mt.reshape(N, N) != 0
            self.count = float(mt.sum().item())
            self.count_valid = float(mt[RADIUS:N - RADIUS, RADIUS:N - RADIUS].sum().item())
            if self.count_valid < 1:
                raise ValueError("mask has no pixel in the valid SSIM region 5 <= i, j <= N - 6")
        rt = ref if isinstance(ref, torch.Tensor) else torch.as_tensor(np.asarray(ref))
        if device is None:
            device = rt.device.index if rt.is_cuda else default_device()
        self.dev = torch.device("cuda", device)
        self.ref = rt.reshape(-1).to(device=self.dev, dtype=torch.float64).contiguous()
        if L is None:
            L = float((self.ref.max() - self.ref.min()).item())
            if not (L > 0 and math.isfinite(L)):
                raise ValueError(f"ref.max() - ref.min() = {L}: a constant reference needs an explicit data_range > 0")
        self.data_range = L
        self.c1, self.c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        self.mask = None if mt is None else mt.to(device=self.dev, dtype=torch.uint8).contiguous()
        self._counts = torch.tensor([self.count, self.count_valid], dtype=torch.float64, device=self.dev)
        self.lib = _lib.load()
        self._work = None
        self._cap = 0
        self._reserve(max_images)

    def _reserve(self, nimg: int) -> None:
        if nimg <= self._cap:
            return
        self._work = _lib.work_buffer("admm_image_metrics_work", self.N, int(nimg), device=self.dev)
        self._cap = nimg

    def sums(self, x):
        """(V, 2) float64 device tensor [squared error, SSIM sum] of the float64 device batch ``x``
        ((V, n), unit pixel stride, any row stride >= n: no copy), on the current stream."""
        import torch
        V = x.shape[0]
        if x.dtype != torch.float64 or x.device != self.dev or x.dim() != 2 or x.shape[1] != self.n:
            raise ValueError("Scorer.sums needs a float64 (V, n) batch on the scorer's device")
        if x.stride(1) != 1 or (V > 1 and x.stride(0) < self.n):
            x = x.contiguous()
        self._reserve(V)
        out = torch.empty((V, 2), dtype=torch.float64, device=self.dev)
        p = _lib.ptr
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.admm_image_metrics(p(x), int(x.stride(0)) if V > 1 else self.n, p(self.ref), p(self.mask),
                                                   self.N, V, self.c1, self.c2, p(self._work), p(out),
                                                   C.c_void_p(current_stream_handle(self.dev))), "admm_image_metrics")
        return out

    def finish(self, sums):
        """{"mse", "psnr", "ssim"} (length-V float64 device tensors) from ``sums``: elementwise, so a
        row's values do not depend on the rows around it.  psnr is +inf where the squared error is 0
        (-10 log10 0), as in the reference's helper."""
        import torch
        q = sums / self._counts  # tensor / tensor: IEEE divisions (a Python scalar would multiply by 1 / count)
        mse = q[:, 0]
        psnr = 20.0 * math.log10(self.data_range) - 10.0 * torch.log10(mse)
        return {"mse": mse, "psnr": psnr, "ssim": q[:, 1]}

    def score(self, x):
        return self.finish(self.sums(x))

    def columns(self, x, names):
        """(V, len(names)) device tensor of the metrics ``names`` of the batch ``x``."""
        import torch
        m = self.score(x)
        return torch.stack([m[k] for k in names], dim=1)


def image_metrics(x, ref, data_range=None, mask=None):
    """{"mse", "psnr", "ssim"} of the image(s) ``x`` against ``ref``: float64 device tensors of
    length V.  ``x``: numpy or torch, (N, N), (n,), (V, n) or (V, N, N); ``ref``: one (N, N) or (n,)
    image.  Inputs are converted to float64 on the device (ref's device, else x's, else the
    default one); a float64 device batch -- also a row-strided view of a wider tensor -- is read in
    place.  ``data_range`` L defaults to ref.max() - ref.min() and must be > 0; ``mask`` ((N, N) or
    (n,), nonzero = counted) restricts the squared error to its pixels and SSIM to its valid window
    centres.  ValueError: data_range <= 0, N < 11, shapes that do not match, a mask without a pixel
    in the valid region."""
    import torch
    N = _ref_side(ref)
    check_data_range(data_range)
    V, _ = _batch_shape(x, N)
    if mask is not None:
        _check_mask_shape(mask, N)
    device = None
    for t in (ref, x):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            device = t.device.index
            break
    sc = Scorer(ref, data_range, mask, device=device, max_images=V)
    xt = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    xt = xt.to(device=sc.dev, dtype=torch.float64)
    if xt.dim() == 3 and V > 1 and not (xt.stride(2) == 1 and xt.stride(1) == N):
        xt = xt.contiguous()
    if xt.dim() == 3 and V > 1:
        xt = xt.as_strided((V, N * N), (xt.stride(0), 1))
    else:
        xt = xt.reshape(V, N * N)
    return sc.score(xt)


def psnr(x, ref, data_range=None, mask=None):
    """``image_metrics(...)["psnr"]``: the reference's psnr (test_final_integration.py:41-45) per image."""
    return image_metrics(x, ref, data_range, mask)["psnr"]


def ssim(x, ref, data_range=None, mask=None):
    """``image_metrics(...)["ssim"]``: mean SSIM (Wang et al. 2004, Gaussian 11 x 11, sigma 1.5) per image."""
    return image_metrics(x, ref, data_range, mask)["ssim"]
