"""Residual-balancing rho and the scale-free stop test (scope row f10).

Host side of ``admm_batch_set_rho`` (csrc/admm_tomo.hip, reached through NodeBatch.set_rho) and
``admm_node_norms`` (csrc/norms.hip): the argument checks and the two rules, which need no device
(``check_adapt_rho``, ``balance``, ``check_stop_tolerances``, ``check_tolerance_run``, ``thresholds``),
and ``NodeNorms``, which owns the kernel's scratch and enqueues the three norms of a NodeBatch.

Residual balancing (Boyd et al. 3.4.1): after iteration k, rho <- rho * factor where the primal
residual r exceeds ratio * s, rho / factor where the dual residual s exceeds ratio * r.  The scaled
duals stand for rho y, so a change rescales them by rho_old / rho_new (exact for factor 2).

The stop test (Boyd et al. 3.12) for the stacked constraint "x_i - z_e = 0 at both ends of every edge"
(and x_i - w_i = 0 with bounds), ninc_i the incidences of node i:

    eps_pri_k  = sqrt(n sum_i ninc_i) eps_abs + eps_rel max(sqrt(sum_i ninc_i X2_i), sqrt(sum_i Z2_i))
    eps_dual_k = sqrt(n V_total)      eps_abs + eps_rel rho_k sqrt(sum_i U2_i)

with X2_i, Z2_i, U2_i the three sums of admm_node_norms.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _lib
from .plan import derived_z_requested

NORM_STATS = 3  # X2, Z2, U2
NORM_KEYS = ("eps_pri_history", "eps_dual_history", "ax_norm", "bz_norm", "aty_norm")
ADAPT_KEYS = ("ratio", "factor", "every", "until", "rho_min", "rho_max")
RHO_SPAN = 1024.0  # default clamps: rho_0 / 1024 .. rho_0 * 1024


def _real(v, what: str) -> float:
    """``v`` as a float: a real number, no bool, no NaN (ValueError otherwise)."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a real number, got {v!r}")
    f = float(v)
    if math.isnan(f):
        raise ValueError(f"{what} must not be NaN")
    return f


def _count(v, what: str, lo: int) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or int(v) < lo:
        raise ValueError(f"{what} must be an int >= {lo}, got {v!r}")
    return int(v)


def check_adapt_rho(adapt_rho, rho) -> dict | None:
    """``adapt_rho`` = None / False (off), True (the defaults) or a dict with keys of ``ADAPT_KEYS``:
    ratio (10.0, > 1), factor (2.0, > 1), every (1, an int >= 1), until (None, or an int >= 0: no
    change after that many iterations), rho_min / rho_max (rho / 1024, rho * 1024; 0 < rho_min <= rho
    <= rho_max, finite).  Returns the complete configuration or None.  Raises ValueError for anything
    else: unknown keys, bools used as numbers, NaN, a rho that is not finite and > 0.  Host work only."""
    if adapt_rho is None or adapt_rho is False:
        return None
    if adapt_rho is True:
        adapt_rho = {}
    if not isinstance(adapt_rho, dict):
        raise ValueError(f"adapt_rho must be None, True or a dict with keys of {ADAPT_KEYS}, got {adapt_rho!r}")
    unknown = sorted(set(adapt_rho) - set(ADAPT_KEYS), key=str)
    if unknown:
        raise ValueError(f"adapt_rho has unknown keys {unknown}; known: {ADAPT_KEYS}")
    rho0 = _real(rho, "adapt_rho needs rho: rho")
    if not (math.isfinite(rho0) and rho0 > 0.0):
        raise ValueError(f"adapt_rho needs a finite rho > 0, got {rho!r}")
    ratio = _real(adapt_rho.get("ratio", 10.0), "adapt_rho['ratio']")
    factor = _real(adapt_rho.get("factor", 2.0), "adapt_rho['factor']")
    for name, v in (("ratio", ratio), ("factor", factor)):
        if not (math.isfinite(v) and v > 1.0):
            raise ValueError(f"adapt_rho[{name!r}] must be finite and > 1, got {v!r}")
    every = _count(adapt_rho.get("every", 1), "adapt_rho['every']", 1)
    until = adapt_rho.get("until")
    if until is not None:
        until = _count(until, "adapt_rho['until']", 0)
    rho_min = _real(adapt_rho.get("rho_min", rho0 / RHO_SPAN), "adapt_rho['rho_min']")
    rho_max = _real(adapt_rho.get("rho_max", rho0 * RHO_SPAN), "adapt_rho['rho_max']")
    if not (math.isfinite(rho_min) and math.isfinite(rho_max) and 0.0 < rho_min <= rho0 <= rho_max):
        raise ValueError(f"adapt_rho needs finite 0 < rho_min <= rho <= rho_max, got rho_min={rho_min!r}, "
                         f"rho={rho0!r}, rho_max={rho_max!r}")
    return dict(ratio=ratio, factor=factor, every=every, until=until, rho_min=rho_min, rho_max=rho_max)


def balance(rho: float, r: float, s: float, cfg: dict, k: int) -> float:
    """rho after iteration ``k`` (0-based) with primal residual r and dual residual s: the rule is
    applied when (k + 1) % every == 0 and k + 1 <= until; r > ratio * s -> min(rho * factor, rho_max),
    s > ratio * r -> max(rho / factor, rho_min), otherwise (and for a residual that is not finite) rho."""
    if (k + 1) % cfg["every"] != 0 or (cfg["until"] is not None and k + 1 > cfg["until"]):
        return rho
    if not (math.isfinite(r) and math.isfinite(s)):
        return rho
    if r > cfg["ratio"] * s:
        return min(rho * cfg["factor"], cfg["rho_max"])
    if s > cfg["ratio"] * r:
        return max(rho / cfg["factor"], cfg["rho_min"])
    return rho


def check_stop_tolerances(eps_abs, eps_rel):
    """(eps_abs, eps_rel) as floats, or None when both are None (the absolute test of eps_pri /
    eps_dual stays).  Otherwise each is a finite real >= 0 (a None beside a number is 0) and not both
    are 0; anything else raises ValueError.  Host work only."""
    if eps_abs is None and eps_rel is None:
        return None
    out = []
    for name, v in (("eps_abs", eps_abs), ("eps_rel", eps_rel)):
        f = 0.0 if v is None else _real(v, name)
        if not (math.isfinite(f) and f >= 0.0):
            raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
        out.append(f)
    if out[0] == 0.0 and out[1] == 0.0:
        raise ValueError("eps_abs and eps_rel must not both be 0: the stop test could never fire")
    return out[0], out[1]


def check_tolerance_run(tol, edge_state, env_edge_state: str = ""):
    """The combination the scale-free stop test does not support, as ValueError (host work only): its
    norm ||Bz|| reads the stored z rows, which a derived-z run does not have."""
    if tol is None:
        return
    if derived_z_requested(edge_state, env_edge_state):
        raise ValueError("eps_abs / eps_rel need stored z (edge_state='stored'): the stop thresholds read "
                         "||z|| from the stored edge rows")


def incidences(edges, V_total: int, bounded: bool) -> np.ndarray:
    """ninc_i of every graph node: its degree, + 1 for the constraint slot of a run with bounds."""
    ninc = np.full(V_total, 1.0 if bounded else 0.0)
    for a, b in edges:
        ninc[a] += 1.0
        ninc[b] += 1.0
    return ninc


def thresholds(eps_abs: float, eps_rel: float, n: int, ninc, norms, rho: float):
    """Boyd et al. (3.12) from the global (V_total, 3) table ``norms`` of X2, Z2, U2 and ninc (V_total,):
    returns (eps_pri_k, eps_dual_k, ||Ax||, ||Bz||, ||A^T y||), the last with the unscaled dual
    y = rho u: rho sqrt(sum_i U2_i)."""
    ninc = np.asarray(ninc, dtype=np.float64)
    norms = np.asarray(norms, dtype=np.float64)
    ax = math.sqrt(float(np.sum(ninc * norms[:, 0])))
    bz = math.sqrt(float(np.sum(norms[:, 1])))
    aty = rho * math.sqrt(float(np.sum(norms[:, 2])))
    eps_pri = math.sqrt(n * float(np.sum(ninc))) * eps_abs + eps_rel * max(ax, bz)
    eps_dual = math.sqrt(n * len(ninc)) * eps_abs + eps_rel * aty
    return eps_pri, eps_dual, ax, bz, aty


class NodeNorms:
    """The three norms of ``nimg`` images of ``n`` pixels on ``device``: the kernel's scratch and its
    (nimg, 3) output."""

    def __init__(self, n: int, nimg: int, device):
        self.lib = _lib.load()
        self.n = int(n)
        self.nimg = int(nimg)
        self.work = _lib.work_buffer("admm_node_norms_work", self.n, self.nimg, device=device)
        self.sums = torch.zeros((self.nimg, NORM_STATS), dtype=torch.float64, device=device)

    def run(self, x, y, y_b, z, inc_off, inc_edge, inc_sign, n_edges: int, stream: int) -> torch.Tensor:
        """``sums`` <- X2, Z2, U2 of the rows of ``x`` ((nimg, n) float64, unit inner stride) on
        ``stream``; y, z (and y_b or None) hold ``n_edges`` rows of n doubles."""
        if x.dim() != 2 or x.shape[0] != self.nimg or x.shape[1] != self.n or x.stride(1) != 1:
            raise ValueError(f"x must be ({self.nimg}, {self.n}) with unit inner stride, got {tuple(x.shape)}")
        for name, t in (("y", y), ("y_b", y_b), ("z", z)):
            if t is not None and n_edges > 0 and (not t.is_contiguous() or t.numel() < n_edges * self.n):
                raise ValueError(f"{name} must be contiguous and hold {n_edges} rows of {self.n} doubles")
        if inc_off.numel() < self.nimg + 1:
            raise ValueError(f"inc_off needs {self.nimg + 1} entries, got {inc_off.numel()}")
        p = _lib.ptr
        _lib.check(self.lib.admm_node_norms(p(x), int(x.stride(0)), p(y), p(y_b), p(z), self.n, self.nimg, p(inc_off),
                                            p(inc_edge), p(inc_sign), int(n_edges), p(self.work), p(self.sums),
                                            C.c_void_p(stream)), "admm_node_norms")
        return self.sums
