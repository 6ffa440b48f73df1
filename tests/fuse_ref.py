"""NumPy restatement of the fixed-point fusion arithmetic (include/admm_tomo.h, csrc/fuse.hip;
DESIGN.md 6.12).  Every line is one IEEE float64 operation or an exact int64 one.

    B = max |t|;  B == 0: s = 0, else B = m 2^e (frexp), L = bit_length(V_total - 1), s = 61 - e - L
    q = rint(ldexp(t, s)) as int64;  S = sum_i q_i;  fixed_sum = ldexp(float64(S), -s)
    xbar = fixed_sum(w x) / fixed_sum(w);  spread = sqrt(fixed_sum(w ((x - xbar) (x - xbar))) / fixed_sum(w))
    dev2_i = sum_p (x_i - xbar)^2  (math.fsum here: the device's fixed-order sum is held to 1e-13 of it)

A term that is NaN or infinite makes B = +inf and every output NaN.  ``parts`` splits the nodes into
groups that are summed one after the other, as batches and ranks are: the result must not depend on it.
"""
from __future__ import annotations

import math

import numpy as np


def shift(B: float, V_total: int) -> int:
    """s of the largest term B >= 0 (finite) and the node count."""
    if B == 0.0:
        return 0
    _, e = math.frexp(B)
    L = max(int(V_total) - 1, 0).bit_length()
    return 61 - e - L


def absmax(terms) -> float:
    """max |t|, +inf if any term is NaN or infinite."""
    t = np.asarray(terms, dtype=np.float64)
    return float(np.max(np.abs(t))) if np.all(np.isfinite(t)) else math.inf


def quantise(terms, s: int):
    return np.rint(np.ldexp(np.asarray(terms, dtype=np.float64), s)).astype(np.int64)


def fixed_sum(terms, V_total=None, parts=None):
    """(fixed_sum (n,), s, S int64 (n,)) of the (V, n) ``terms``; ``V_total`` (default V) may exceed V (one
    rank's share of a larger network); ``parts``: index groups summed one after the other (default: all at
    once).  A non-finite term: (all-NaN, None, None)."""
    t = np.asarray(terms, dtype=np.float64)
    V, n = t.shape
    V_total = V if V_total is None else int(V_total)
    parts = [slice(0, V)] if parts is None else parts
    B = max(absmax(t[p]) for p in parts)  # a max of maxes: exact in any order
    if not math.isfinite(B):
        return np.full(n, np.nan), None, None
    s = shift(B, V_total)
    S = np.zeros(n, dtype=np.int64)
    for p in parts:
        S += quantise(t[p], s).sum(axis=0, dtype=np.int64)
    with np.errstate(over="ignore"):  # (a sum beyond the double range is +-inf)
        return np.ldexp(S.astype(np.float64), -s), s, S


def fuse(x, w=None, V_total=None, parts=None, spread=False):
    """xbar (n,) of the (V, n) images (``w`` None: uniform), and with ``spread`` (xbar, spread)."""
    x = np.asarray(x, dtype=np.float64)
    V, n = x.shape
    V_total = V if V_total is None else int(V_total)
    if w is None:
        num, den = fixed_sum(x, V_total, parts)[0], np.full(n, float(V_total))
    else:
        w = np.asarray(w, dtype=np.float64)
        num, den = fixed_sum(w * x, V_total, parts)[0], fixed_sum(w, V_total, parts)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        xbar = num / den
        if not spread:
            return xbar
        d = x - xbar
        dd = d * d
        var = fixed_sum(dd if w is None else w * dd, V_total, parts)[0]
        return xbar, np.sqrt(var / den)


def dev2(x, xbar):
    """|x_i - xbar|^2 of every image: the squares as the device forms them, their sum by math.fsum."""
    x = np.asarray(x, dtype=np.float64)
    d = x - np.asarray(xbar, dtype=np.float64)
    return np.array([math.fsum(r * r) for r in d])
