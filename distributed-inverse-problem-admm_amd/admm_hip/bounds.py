"""Bound constraints lo <= x <= hi on the images (scope row f8).

Host side of ``admm_bound_project`` / ``admm_bound_project_relaxed`` (csrc/bounds.hip): the argument checks, which need no device
(``check_bounds``, ``check_bound_weight``), and ``BoundProjector``, which owns the kernel's scratch
and the device copies of the maps and enqueues one projection

    t = x + f,   w' = clip(t, l, h),   f' = t - w',   l = max(lo, lo_map),  h = min(hi, hi_map)

of a batch of images with its three sums per image: |x - w'|^2 (the constraint's primal residual),
|w' - w|^2 (its dual residual, up to rho) and |x - clip(x)|^2 (how far x itself lies outside the box).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .plan import derived_z_requested

BOUND_STATS = 3  # |x - w'|^2, |w' - w|^2, |x - clip(x)|^2
BOUND_KEYS = ("bound_primal", "bound_dual", "bound_violation", "bound_pri_per_node", "bound_violation_per_node")


@dataclass(frozen=True)
class Bounds:
    """A checked box: scalars ``lo`` <= ``hi`` (-inf / +inf: that side is off) and per-pixel maps
    ((n,) float64 host arrays or None); the box of pixel p is [max(lo, lo_map[p]), min(hi, hi_map[p])]."""
    lo: float
    hi: float
    lo_map: np.ndarray | None
    hi_map: np.ndarray | None

    def arrays(self, n: int):
        """(l, h): the per-pixel bounds as (n,) float64 arrays."""
        l = np.full(n, self.lo) if self.lo_map is None else np.maximum(self.lo, self.lo_map)
        h = np.full(n, self.hi) if self.hi_map is None else np.minimum(self.hi, self.hi_map)
        return l, h


def _side(v, n: int, name: str, off: float):
    """One of ``bounds``' two entries -> (scalar, map or None)."""
    if v is None:
        return off, None
    if isinstance(v, torch.Tensor):
        v = v.detach().to("cpu").numpy()
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        if math.isnan(float(a)):
            raise ValueError(f"bounds: {name} is NaN")
        return float(a), None
    if a.size != n:
        raise ValueError(f"bounds: {name} has {a.size} entries, expected a scalar or one per pixel ({n})")
    a = np.ascontiguousarray(a.reshape(-1))
    if np.isnan(a).any():
        raise ValueError(f"bounds: {name} holds NaN")
    return off, a


def check_bounds(bounds, N: int) -> Bounds | None:
    """``bounds`` = None or (lo, hi), each None, a scalar, or an (N, N) / (n,) array or tensor shared
    by every node, as a ``Bounds`` (None stays None).  Raises ValueError on a wrong shape, a NaN, or
    lo > hi at any pixel.  Host work only."""
    if bounds is None or isinstance(bounds, Bounds):
        return bounds
    try:
        lo, hi = bounds
    except (TypeError, ValueError):
        raise ValueError("bounds must be None or a pair (lo, hi)") from None
    n = int(N) * int(N)
    lo_s, lo_map = _side(lo, n, "lo", -math.inf)
    hi_s, hi_map = _side(hi, n, "hi", math.inf)
    b = Bounds(lo_s, hi_s, lo_map, hi_map)
    if lo_s == math.inf or hi_s == -math.inf:
        raise ValueError("bounds: lo = +inf or hi = -inf leaves no finite value in the box")
    l, h = b.arrays(n)
    bad = np.flatnonzero(l > h)
    if bad.size:
        p = int(bad[0])
        raise ValueError(f"bounds: lo > hi at {bad.size} pixel(s), first at pixel {p}: lo = {l[p]}, hi = {h[p]}")
    if (l == math.inf).any() or (h == -math.inf).any():
        raise ValueError("bounds: lo = +inf or hi = -inf leaves no finite value in the box")
    return b


def check_bound_weight(bound_weight, bounds) -> float:
    """kappa of q_c,i = kappa * Wi_list[i] (default 1; finite and > 0; needs ``bounds``)."""
    if bound_weight is None:
        return 1.0
    if bounds is None:
        raise ValueError("bound_weight needs bounds=(lo, hi)")
    k = float(bound_weight)
    if not (k > 0 and math.isfinite(k)):
        raise ValueError(f"bound_weight must be finite and > 0, got {bound_weight!r}")
    return k


def check_bound_run(bounds, fusion: str, edge_state, env_edge_state: str = ""):
    """The combinations a bounded run does not support, as ValueError (host work only): the
    constraint slot is a stored z row updated by the midpoint kernels' x-update."""
    if bounds is None:
        return
    if fusion != "midpoint":
        raise ValueError("bounds need fusion='midpoint' (the constraint slot has one dual)")
    if derived_z_requested(edge_state, env_edge_state):
        raise ValueError("bounds need stored z (edge_state='stored'): the constraint variable w is a stored z row")


class BoundProjector:
    """The projection of up to ``max_images`` images of ``n`` pixels on ``device``: owns the kernel's
    scratch, the [max_images][3] sums and the device copies of the maps."""

    def __init__(self, bounds: Bounds, n: int, device, max_images: int):
        self.lib = _lib.load()
        self.bounds = bounds
        self.n = int(n)
        self.max_images = int(max_images)
        dev = torch.device("cuda", device) if isinstance(device, int) else device
        self.dev = dev
        self.work = _lib.work_buffer("admm_bound_project_work", self.n, self.max_images, device=dev)
        self.sums = torch.zeros((self.max_images, BOUND_STATS), dtype=torch.float64, device=dev)
        put = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
        self.lo_map, self.hi_map = put(bounds.lo_map), put(bounds.hi_map)
        l, h = bounds.arrays(self.n)
        self.l, self.h = torch.from_numpy(l).to(dev), torch.from_numpy(h).to(dev)

    def clip(self, x: torch.Tensor) -> torch.Tensor:
        """clip(x) elementwise with the kernel's comparisons (rows of n pixels)."""
        return torch.where(x < self.l, self.l, torch.where(x > self.h, self.h, x))

    def run(self, x: torch.Tensor, w: torch.Tensor, f: torch.Tensor, stream: int, alpha=None) -> torch.Tensor:
        """w, f <- the projection step around the images x (each (nimg, n) float64 with unit pixel
        stride; w and f share one row stride), in place, on ``stream``; returns the (nimg, 3) sums
        (a view of this object's buffer, rewritten by the next call).  ``alpha``: the over-relaxed
        step around alpha x + (1 - alpha) w (admm_bound_project_relaxed; relax.Relaxer)."""
        nimg = x.shape[0]
        if not (1 <= nimg <= self.max_images):
            raise ValueError(f"{nimg} images, the projector holds scratch for {self.max_images}")
        for t, name in ((x, "x"), (w, "w"), (f, "f")):
            if t.dtype != torch.float64 or t.device != self.dev or t.dim() != 2 or t.shape != (nimg, self.n):
                raise ValueError(f"{name} must be a ({nimg}, {self.n}) float64 tensor on {self.dev}")
            if t.stride(1) != 1 or (nimg > 1 and t.stride(0) < self.n):
                raise ValueError(f"{name}: rows must be contiguous and must not overlap")
        if nimg > 1 and w.stride(0) != f.stride(0):
            raise ValueError("w and f must share one row stride")
        p = _lib.ptr
        xs = x.stride(0) if nimg > 1 else self.n
        ws = w.stride(0) if nimg > 1 else self.n
        box = (p(x), xs, p(w), p(f), ws, p(self.lo_map), p(self.hi_map), float(self.bounds.lo), float(self.bounds.hi),
               self.n, nimg)
        out = (p(self.work), p(self.sums), C.c_void_p(stream))
        if alpha is None:
            _lib.check(self.lib.admm_bound_project(*box, *out), "admm_bound_project")
        else:
            _lib.check(self.lib.admm_bound_project_relaxed(*box, float(alpha), *out), "admm_bound_project_relaxed")
        return self.sums[:nimg]
