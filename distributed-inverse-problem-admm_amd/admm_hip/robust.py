"""The Huber data term by reweighted rays (scope row f12).

Least squares spreads an outlier ray -- a zinger, a flickering bin, metal -- over the whole image.
The Huber loss psi_delta(a) = a^2 / 2 for |a| <= delta, delta |a| - delta^2 / 2 beyond, bounds each
ray's pull by delta.  Majorise-minimise (half-quadratic, IRLS): after an x-update the residual
r = A x - b gives h_r = 1 where |r_r| <= delta, else delta / |r_r|, and the next x-update is the
weighted least-squares update with omega^eff = omega h (omega: the caller's ``ray_weights``, or 1).

``check_robust`` is the host check of ``run_admm(robust=...)``; ``HuberWeights`` owns the kernel's
scratch and enqueues ``admm_huber_weights`` (csrc/robust.hip; include/admm_tomo.h states the
arithmetic); ``huber_weights`` is the standalone function; ``run_admm`` goes through
groups.RankGroups.enable_robust / reweight.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import _lib
from .geometry import current_stream_handle

ROBUST_STATS = 2  # the weighted Huber value, the outlier count
ROBUST_KEYS = ("robust_loss_per_node", "robust_loss_total", "robust_outliers_per_node", "robust_outliers_total")
ROBUST_CFG_KEYS = ("delta", "every", "until")
ROBUST_MATRIX_MSG = ("robust is not supported for explicit-matrix operators: it reweights the rays through "
                     "ray_weights, which those operators do not take")


def _delta(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a real number > 0 (inf allowed), got {v!r}")
    f = float(v)
    if math.isnan(f) or not f > 0.0:
        raise ValueError(f"{what} must be > 0 (inf allowed) and not NaN, got {v!r}")
    return f


def _count(v, what: str, lo: int) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or int(v) < lo:
        raise ValueError(f"{what} must be an int >= {lo}, got {v!r}")
    return int(v)


def check_robust(robust) -> dict | None:
    """``robust`` = None (off), a real delta > 0 (inf allowed) or a dict with ``delta`` (required),
    ``every`` (1, an int >= 1: reweight every this many iterations) and ``until`` (None, or an int >= 0:
    after that many iterations the weights stay as they are).  Returns the complete configuration or
    None.  Raises ValueError for anything else: a bool, NaN, delta <= 0, unknown keys.  Host work only."""
    if robust is None:
        return None
    if not isinstance(robust, dict):
        return dict(delta=_delta(robust, "robust"), every=1, until=None)
    unknown = sorted(set(robust) - set(ROBUST_CFG_KEYS), key=str)
    if unknown:
        raise ValueError(f"robust has unknown keys {unknown}; known: {ROBUST_CFG_KEYS}")
    if "delta" not in robust:
        raise ValueError("robust needs 'delta', the Huber threshold")
    every = _count(robust.get("every", 1), "robust['every']", 1)
    until = robust.get("until")
    if until is not None:
        until = _count(until, "robust['until']", 0)
    return dict(delta=_delta(robust["delta"], "robust['delta']"), every=every, until=until)


def applies(cfg: dict, k: int) -> bool:
    """The weights formed after iteration ``k`` (0-based) are applied: (k + 1) % every == 0 and
    k + 1 <= until."""
    return (k + 1) % cfg["every"] == 0 and (cfg["until"] is None or k + 1 <= cfg["until"])


class HuberWeights:
    """The kernel on batches of ``nimg`` sinograms of ``m`` rays of ``dtype`` on ``device``: its
    scratch, the [nimg][m] weights it writes and its (nimg, 2) sums."""

    def __init__(self, m: int, nimg: int, dtype, device):
        self.lib = _lib.load()
        self.m, self.nimg = int(m), int(nimg)
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"the sample dtype must be float32 or float64, got {dtype}")
        self.dtype = dtype
        self.code = _lib.ADMM_DTYPE_F64 if dtype == torch.float64 else _lib.ADMM_DTYPE_F32
        self.work = _lib.work_buffer("admm_huber_weights_work", self.m, self.nimg, device=device)
        self.w_out = torch.empty((self.nimg, self.m), dtype=dtype, device=device)
        self.sums = torch.zeros((self.nimg, ROBUST_STATS), dtype=torch.float64, device=device)

    def _rows(self, t, what):
        if t.dtype != self.dtype or tuple(t.shape) != (self.nimg, self.m) or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {self.dtype} ({self.nimg}, {self.m}) device tensor, got "
                             f"{tuple(t.shape)} {t.dtype}")

    def run(self, ax, b, w, delta: float, stream: int) -> torch.Tensor:
        """``w_out`` <- the Huber weights of ax - b times ``w`` (None: 1) and ``sums`` <- the weighted
        Huber value and the outlier count per image, on ``stream``.  Returns ``sums``."""
        self._rows(ax, "ax")
        self._rows(b, "b")
        if w is not None:
            self._rows(w, "ray_weights")
        p = _lib.ptr
        _lib.check(self.lib.admm_huber_weights(p(ax), p(b), p(w), p(self.w_out), self.code, self.m, self.nimg,
                                               float(delta), p(self.work), p(self.sums), C.c_void_p(stream)),
                   "admm_huber_weights")
        return self.sums


def huber_weights(ax, b, delta, ray_weights=None):
    """(w_out, loss, outliers) of the residual ``ax`` - ``b``: device tensors (m,) or (k, m) of one
    sample dtype (float32 / float64); ``ray_weights``: None or the same shape and dtype (0 masks a
    ray).  w_out = ray_weights * h with h = 1 where |ax - b| <= delta and delta / |ax - b| beyond;
    loss (k,) float64 = sum_r ray_weights_r psi_delta((ax - b)_r); outliers (k,) float64 = the number
    of unmasked rays beyond delta.  On the current stream; nothing synchronises."""
    delta = _delta(delta, "delta")
    for name, t in (("ax", ax), ("b", b), ("ray_weights", ray_weights)):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise ValueError(f"{name} must be a device tensor")
    squeeze = ax.dim() == 1
    rows = lambda t: None if t is None else (t.unsqueeze(0) if t.dim() == 1 else t).contiguous()  # noqa: E731
    ax2, b2, w2 = rows(ax), rows(b), rows(ray_weights)
    if ax2.dim() != 2:
        raise ValueError(f"ax must be (m,) or (k, m), got {tuple(ax.shape)}")
    hw = HuberWeights(ax2.shape[1], ax2.shape[0], ax2.dtype, ax2.device)
    sums = hw.run(ax2, b2, w2, delta, current_stream_handle(ax2.device))
    w_out = hw.w_out[0] if squeeze else hw.w_out
    return w_out, sums[:, 0].clone(), sums[:, 1].clone()
