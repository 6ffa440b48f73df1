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

The self-scaling form (scope row f13) gives the threshold in units of the data's own
residual scale: robust={"scale": k} makes delta_i = k * 1.4826 * median|A x_i - b_i| per node and
iteration, an exact order statistic found on the device (``RayQuantile`` / ``ray_quantile``:
``admm_ray_quantile``, csrc/scale.hip) and read by the Huber kernel from device memory
(``admm_huber_weights_dev``): no host synchronisation.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import sys

import torch

from . import _lib
from .geometry import current_stream_handle

ROBUST_STATS = 2  # the weighted Huber value, the outlier count
ROBUST_KEYS = ("robust_loss_per_node", "robust_loss_total", "robust_outliers_per_node", "robust_outliers_total")
ROBUST_CFG_KEYS = ("delta", "every", "until")
ROBUST_SCALE_STATS = 3  # the scale form's block: the two sums and the threshold in force
ROBUST_SCALE_KEYS = ROBUST_KEYS + ("robust_delta_per_node",)
ROBUST_SCALE_CFG_KEYS = ("scale", "quantile", "delta_min", "consistency", "every", "until")
QUANTILE_STATS = 3  # admm_ray_quantile's out: delta, a_k, cnt
GAUSSIAN_CONSISTENCY = 1.4826  # 1 / Phi^-1(3/4): the median absolute deviation of N(0, sigma) times this is sigma
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


def _real(v, what: str, lo: float, hi: float, lo_open: bool, rule: str) -> float:
    """``v`` as a float in (lo, hi] or [lo, hi]; a bool, a non-real and NaN raise."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a real number {rule}, got {v!r}")
    f = float(v)
    if math.isnan(f) or f < lo or f > hi or (lo_open and f == lo):
        raise ValueError(f"{what} must be {rule} and not NaN, got {v!r}")
    return f


def check_robust(robust) -> dict | None:
    """``robust`` = None (off), a real delta > 0 (inf allowed) or a dict with either ``delta`` (the Huber
    threshold in sinogram units) or ``scale`` (the threshold in units of the residual scale), and ``every``
    (1, an int >= 1: reweight every this many iterations) and ``until`` (None, or an int >= 0: after that
    many iterations the weights -- and a scale form's estimate -- stay as they are).  With ``scale`` (a
    finite real > 0; no default: DESIGN.md 6.14) also ``quantile`` (0.5, in [0, 1]), ``delta_min`` (0.0, a
    real >= 0, inf allowed: the threshold's floor) and ``consistency`` (1.4826, a finite real > 0); the
    kernel's factor is scale * consistency (``scale_factor``, one float64 multiply on the host).  Returns
    the complete configuration -- delta, every, until for the delta form, exactly as before; scale,
    quantile, delta_min, consistency, every, until for the scale form -- or None; a complete configuration
    passes unchanged.  Raises ValueError for anything else: a
    bool, NaN, delta <= 0, both or neither of delta and scale, unknown keys.  Host work only."""
    if robust is None:
        return None
    if not isinstance(robust, dict):
        return dict(delta=_delta(robust, "robust"), every=1, until=None)
    scaled = "scale" in robust
    if scaled and "delta" in robust:
        raise ValueError("robust takes either 'delta' or 'scale', not both")
    known = ROBUST_SCALE_CFG_KEYS if scaled else ROBUST_CFG_KEYS
    unknown = sorted(set(robust) - set(known), key=str)
    if unknown:
        raise ValueError(f"robust has unknown keys {unknown}; known: {known}")
    if not scaled and "delta" not in robust:
        raise ValueError("robust needs 'delta', the Huber threshold, or 'scale', the threshold in units of the "
                         "residual scale")
    every = _count(robust.get("every", 1), "robust['every']", 1)
    until = robust.get("until")
    if until is not None:
        until = _count(until, "robust['until']", 0)
    if not scaled:
        return dict(delta=_delta(robust["delta"], "robust['delta']"), every=every, until=until)
    big = sys.float_info.max
    scale = _real(robust["scale"], "robust['scale']", 0.0, big, True, "finite and > 0")
    quantile = _real(robust.get("quantile", 0.5), "robust['quantile']", 0.0, 1.0, False, "in [0, 1]")
    delta_min = _real(robust.get("delta_min", 0.0), "robust['delta_min']", 0.0, math.inf, False, ">= 0 (inf allowed)")
    consistency = _real(robust.get("consistency", GAUSSIAN_CONSISTENCY), "robust['consistency']", 0.0, big, True,
                        "finite and > 0")
    cfg = dict(scale=scale, quantile=quantile, delta_min=delta_min, consistency=consistency, every=every, until=until)
    c = scale_factor(cfg)
    if not (c > 0.0 and math.isfinite(c)):
        raise ValueError(f"robust: scale * consistency = {c!r} must be finite and > 0")
    return cfg


def scale_factor(cfg: dict) -> float:
    """The quantile kernel's ``c`` of a scale form: scale * consistency, one float64 multiply on the host."""
    return cfg["scale"] * cfg["consistency"]


def estimates(cfg: dict, k: int) -> bool:
    """A scale form's threshold is estimated again from iteration ``k``'s images (0-based): always at
    k = 0, then while k + 1 <= until; afterwards it stays at its last value."""
    return k == 0 or cfg["until"] is None or k + 1 <= cfg["until"]


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

    def run(self, ax, b, w, delta, stream: int) -> torch.Tensor:
        """``w_out`` <- the Huber weights of ax - b times ``w`` (None: 1) and ``sums`` <- the weighted
        Huber value and the outlier count per image, on ``stream``.  ``delta``: a float, or a float64
        device tensor whose element v * stride(0) is image v's threshold ((nimg,), or a column of
        ``RayQuantile.out``), read on the device (admm_huber_weights_dev; the caller answers for
        thresholds > 0 and not NaN).  Returns ``sums``."""
        self._rows(ax, "ax")
        self._rows(b, "b")
        if w is not None:
            self._rows(w, "ray_weights")
        p = _lib.ptr
        if isinstance(delta, torch.Tensor):
            if (delta.dtype != torch.float64 or delta.dim() != 1 or delta.shape[0] != self.nimg
                    or delta.device != self.w_out.device or (self.nimg > 1 and delta.stride(0) < 1)):
                raise ValueError(f"delta must be a float64 ({self.nimg},) tensor on {self.w_out.device}, got "
                                 f"{tuple(delta.shape)} {delta.dtype} on {delta.device}")
            _lib.check(self.lib.admm_huber_weights_dev(p(ax), p(b), p(w), p(self.w_out), self.code, self.m,
                                                       self.nimg, p(delta), max(int(delta.stride(0)), 1),
                                                       p(self.work), p(self.sums), C.c_void_p(stream)),
                       "admm_huber_weights_dev")
            return self.sums
        _lib.check(self.lib.admm_huber_weights(p(ax), p(b), p(w), p(self.w_out), self.code, self.m, self.nimg,
                                               float(delta), p(self.work), p(self.sums), C.c_void_p(stream)),
                   "admm_huber_weights")
        return self.sums


class RayQuantile:
    """The quantile kernel on batches of ``nimg`` sinograms of ``m`` rays of ``dtype`` on ``device``: its
    (nimg, 3) float64 ``out`` -- the threshold, the order statistic a_k, the unmasked rays -- and its
    scratch (none today: admm_ray_quantile_work reports 0 bytes)."""

    def __init__(self, m: int, nimg: int, dtype, device):
        self.lib = _lib.load()
        self.m, self.nimg = int(m), int(nimg)
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"the sample dtype must be float32 or float64, got {dtype}")
        self.dtype = dtype
        self.code = _lib.ADMM_DTYPE_F64 if dtype == torch.float64 else _lib.ADMM_DTYPE_F32
        need = _lib.work_size("admm_ray_quantile_work", self.m, self.nimg)
        self.work = torch.empty(need, dtype=torch.uint8, device=device) if need else None
        self.out = torch.zeros((self.nimg, QUANTILE_STATS), dtype=torch.float64, device=device)
        self.out[:, 0] = math.inf  # before the first estimate: least squares

    @property
    def delta(self) -> torch.Tensor:
        """(nimg,) view of ``out``: the thresholds, stride 3."""
        return self.out[:, 0]

    _rows = HuberWeights._rows

    def run(self, ax, b, w, q: float, c: float, floor: float, stream: int) -> torch.Tensor:
        """``out`` <- per image (max(c * a_k, floor) or +inf, a_k, cnt) of the unmasked |ax - b| (``w``:
        None, or 0 masks a ray), a_k the floor(q (cnt - 1))-th smallest, on ``stream``.  Returns ``out``."""
        self._rows(ax, "ax")
        self._rows(b, "b")
        if w is not None:
            self._rows(w, "ray_weights")
        p = _lib.ptr
        _lib.check(self.lib.admm_ray_quantile(p(ax), p(b), p(w), self.code, self.m, self.nimg, float(q), float(c),
                                              float(floor), p(self.work), p(self.out), C.c_void_p(stream)),
                   "admm_ray_quantile")
        return self.out


def _as_rows(ax, b, ray_weights):
    """The standalone functions' arguments as contiguous (k, m) rows, and whether ``ax`` was (m,)."""
    for name, t in (("ax", ax), ("b", b), ("ray_weights", ray_weights)):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise ValueError(f"{name} must be a device tensor")
    squeeze = ax.dim() == 1
    rows = lambda t: None if t is None else (t.unsqueeze(0) if t.dim() == 1 else t).contiguous()  # noqa: E731
    ax2, b2, w2 = rows(ax), rows(b), rows(ray_weights)
    if ax2.dim() != 2:
        raise ValueError(f"ax must be (m,) or (k, m), got {tuple(ax.shape)}")
    return ax2, b2, w2, squeeze


def ray_quantile(ax, b, q=0.5, ray_weights=None, c=1.0, floor=0.0):
    """(delta, value, count), each (k,) float64 on the device, of the residual ``ax`` - ``b``: device
    tensors (m,) or (k, m) of one sample dtype; ``ray_weights``: None or the same shape and dtype, 0 masks a
    ray.  value = the floor(q (count - 1))-th smallest |ax - b| among the count unmasked rays, exactly
    (q = 0.5: the lower median; NaN sorts last); delta = max(c * value, floor), or +inf when that is not a
    finite number > 0 or no ray is unmasked.  On the current stream; nothing synchronises."""
    q = _real(q, "q", 0.0, 1.0, False, "in [0, 1]")
    c = _real(c, "c", 0.0, math.inf, True, "> 0")
    floor = _real(floor, "floor", 0.0, math.inf, False, ">= 0 (inf allowed)")
    ax2, b2, w2, _ = _as_rows(ax, b, ray_weights)
    rq = RayQuantile(ax2.shape[1], ax2.shape[0], ax2.dtype, ax2.device)
    out = rq.run(ax2, b2, w2, q, c, floor, current_stream_handle(ax2.device))
    return out[:, 0].clone(), out[:, 1].clone(), out[:, 2].clone()


def huber_weights(ax, b, delta, ray_weights=None):
    """(w_out, loss, outliers) of the residual ``ax`` - ``b``: device tensors (m,) or (k, m) of one
    sample dtype (float32 / float64); ``ray_weights``: None or the same shape and dtype (0 masks a
    ray).  w_out = ray_weights * h with h = 1 where |ax - b| <= delta and delta / |ax - b| beyond;
    loss (k,) float64 = sum_r ray_weights_r psi_delta((ax - b)_r); outliers (k,) float64 = the number
    of unmasked rays beyond delta.  ``delta``: a real > 0 (inf allowed), or a float64 device tensor (k,)
    of per-image thresholds read on the device (the caller answers for values > 0 and not NaN; a stride
    is honoured, so a column of ``ray_quantile``'s kernel output is read in place).  On the current stream;
    nothing synchronises."""
    if not isinstance(delta, torch.Tensor):
        delta = _delta(delta, "delta")
    ax2, b2, w2, squeeze = _as_rows(ax, b, ray_weights)
    hw = HuberWeights(ax2.shape[1], ax2.shape[0], ax2.dtype, ax2.device)
    sums = hw.run(ax2, b2, w2, delta, current_stream_handle(ax2.device))
    w_out = hw.w_out[0] if squeeze else hw.w_out
    return w_out, sums[:, 0].clone(), sums[:, 1].clone()
