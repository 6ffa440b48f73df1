"""References for the per-ray weights of the data term, 1/2 sum_r w_r (A x - b)_r^2, built on the
unchanged oracle (oracle.node_solver, oracle.admm) and on tests/state_ref.py.

Two forms of the same problem:

* ``WeightedAdjoint`` / ``oracle_update_weighted``: ``oracle.node_solver.node_update`` takes A, A^T,
  A^T b and b separately; handed ``AT' : s -> A^T (w * s)`` (duck-typed, as oracle.admm's
  ``_Serialized``) and ``Atb = A^T (w * b)`` it solves the weighted problem in the kernels' own
  operation order -- the weight applied once, where the sinogram is formed, and cast to the
  emulated sample dtype (the float32 yardstick's operator is state_ref.as_f32_matrix);
* ``row_scaled``: ``diag(sqrt w) A`` and ``sqrt w * b`` pose the same problem to the plain oracle;
  with w = s^2 and s from ``S_VALUES`` the square roots are exact.  The whole-run reference
  (``oracle.admm.decentralized_admm`` on per-node scaled matrices and sinograms) uses this form.

``ray_weights``: the test weights -- U[0, 2] with a tenth of the rays zeroed, one whole angle and
one whole detector column zeroed, different per node.  ``WEIGHT_CASES`` / ``WEIGHT_REUSE_CASES``:
the x-update cases of test_gpu_a_ray_weights.py, kept here so that test_ray_weights_cpu.py checks
their conditions (state_ref.conditions) on the oracle without a GPU.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

import state_ref as sr
from oracle import node_solver as ons

S_VALUES = (0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0)  # sqrt(w) of the whole-run weights: w = s^2 exactly


def ray_weights(a_per: int, n_det: int, nodes, seed: int, dtype: str):
    """{g: w_g (a_per * n_det,)} as float64 holding values of the sample dtype."""
    out = {}
    for g in nodes:
        rng = np.random.default_rng([seed, 55, g])
        w = rng.uniform(0.0, 2.0, size=(a_per, n_det))
        w[rng.random((a_per, n_det)) < 0.1] = 0.0
        w[int(rng.integers(a_per)), :] = 0.0
        w[:, int(rng.integers(n_det))] = 0.0
        w = w.reshape(-1)
        out[g] = w.astype(np.float32).astype(np.float64) if dtype == "float32" else w
    return out


def s_weights(a_per: int, n_det: int, nodes, seed: int):
    """{g: s_g}: per-ray factors drawn from S_VALUES, different per node; the weights are s^2."""
    return {g: np.random.default_rng([seed, 66, g]).choice(np.array(S_VALUES), size=a_per * n_det) for g in nodes}


class WeightedAdjoint:
    """s -> A^T (w * s): w and the product in ``dtype`` (one rounding), as the device applies it."""

    def __init__(self, AT, w, dtype=np.float64):
        self.AT, self.w, self.dtype = AT, np.asarray(w, dtype=dtype), dtype
        self.shape = AT.shape

    def __matmul__(self, s):
        return self.AT @ np.asarray(self.w * np.asarray(s, dtype=self.dtype), dtype=self.dtype)


def row_scaled(A, b, s):
    """(diag(s) A, s * b) with A's sparsity structure kept (rows of s = 0 become stored zeros)."""
    A2 = sp.csr_matrix(A, copy=True)
    A2.data = A2.data * np.repeat(np.asarray(s, dtype=A2.data.dtype), np.diff(A2.indptr))
    return A2, np.asarray(s, dtype=np.float64) * np.asarray(b, dtype=np.float64)


def oracle_update_weighted(host_state, plan, A, b, w, q_fn, params, fusion, dtype=np.float64, phantom=None):
    """state_ref.oracle_update for the weighted data term (``w``: {g: (m,)}, a missing node has
    w = 1): the same loop with AT' and A^T (w b); the MSE_SINO column is sum_r w_r s_r^2 of the
    final x, s = A x - b formed in ``dtype`` and the sum in float64."""
    st = host_state
    n = st["x_ext"].shape[1]
    N = int(round(math.sqrt(n)))
    V = plan.V
    AT = A.T.tocsr()
    out = {"x": np.zeros((V, n)), "d": np.zeros((V, 2, n)), "e": np.zeros((V, 2, n)), "stats": np.zeros((V, 6))}
    for k, g in enumerate(plan.local_nodes):
        qv = []
        for s in range(plan.inc_off[k], plan.inc_off[k + 1]):
            e = plan.inc_edge[s]
            if plan.inc_sign[s] > 0:
                yi = st["y"][e]
            else:
                yi = st["y_b"][e] if fusion == "weighted" else -st["y"][e]
            qv.append((np.asarray(q_fn(g, plan.inc_nbr[s]), dtype=np.float64), sr.z_of(st, plan, e) - yi))
        D, c = ons.assemble(qv, n)
        cast = lambda v: np.array(v, dtype=dtype)  # noqa: E731
        ns = ons.NodeState(cast(st["x_ext"][k]), cast(st["d"][k, 0]), cast(st["d"][k, 1]),
                           cast(st["e"][k, 0]), cast(st["e"][k, 1]))
        bg = np.asarray(b[g], dtype=np.float64).reshape(-1)
        wg = np.asarray(w[g], dtype=np.float64).reshape(-1) if g in w else np.ones_like(bg)
        ATw = WeightedAdjoint(AT, wg, dtype)
        # A^T (w b): the product rounded once in ``dtype``, then A^T as state_ref.oracle_update forms A^T b
        Atb = AT @ (ATw.w * cast(bg)).astype(np.float64)
        dg = ons.node_update(A, Atb, bg, D, c, qv, ns, N, params, dtype=dtype, AT=ATw)
        x = ns.x.astype(np.float64)
        out["x"][k] = x
        out["d"][k, 0], out["d"][k, 1] = ns.dx, ns.dy
        out["e"][k, 0], out["e"][k, 1] = ns.ex, ns.ey
        s = (cast(A @ ns.x) - cast(bg)).astype(np.float64)
        mse = float(np.dot(np.asarray(ATw.w, dtype=np.float64), s * s))
        img = float(np.sum((x - phantom) ** 2)) if phantom is not None else np.nan
        out["stats"][k] = (mse, dg.g_norm ** 2, dg.tv, dg.quad, img, dg.sb_res ** 2)
    return out


def oracle_update_row_scaled(host_state, plan, A, b, s, q_fn, params, fusion, phantom=None):
    """The same update posed as the plain problem of diag(s_g) A and s_g b_g (float64): one
    state_ref.oracle_update per node, each with its own matrix."""
    V = plan.V
    n = host_state["x_ext"].shape[1]
    out = {"x": np.zeros((V, n)), "d": np.zeros((V, 2, n)), "e": np.zeros((V, 2, n)), "stats": np.zeros((V, 6))}
    for k, g in enumerate(plan.local_nodes):
        A2, b2 = row_scaled(A, b[g], s[g])
        one = sr.oracle_update(host_state, plan, A2, {h: b2 for h in plan.local_nodes}, q_fn, params, fusion,
                               phantom=phantom)
        for f in out:
            out[f][k] = one[f][k]
    return out


# --------------------------------------------------------------------------------------
# the weighted x-update cases (state_ref.Case; dwf: the detector width factor -- at 64^2 a
# detector four times the image's width has no grouped forward plan, so k_fwd runs)
# --------------------------------------------------------------------------------------
def _c(N, V, graph, iters, kind, a_per, mirror, seed=1):
    return sr.Case(N, V, graph, iters[0], iters[1], kind, a_per, mirror, "midpoint", False, seed)


WEIGHT_CASES = [
    _c(33, 1, "none", (1, 1), "iso", 12, "1"),
    _c(33, 3, "ring", (1, 1), "aniso", 12, "1", seed=839),
    _c(33, 5, "star", (2, 3), "iso", 9, None),
    _c(33, 8, "ring", (2, 3), "iso", 12, "0"),
    _c(33, 11, "ring", (1, 1), "iso", 12, "1"),
    _c(64, 3, "path", (2, 3), "iso", 24, "0"),
    _c(64, 5, "ring", (1, 1), "iso", 9, None),
    _c(64, 8, "ring", (2, 3), "iso", 24, "1"),
    _c(64, 11, "ring", (2, 3), "iso", 12, "1"),
]
WEIGHT_REUSE_CASES = [
    _c(33, 3, "ring", (2, 3), "iso", 12, "1"),
    _c(64, 8, "ring", (2, 3), "iso", 24, "0"),
]
KFWD_CASE = _c(64, 3, "ring", (2, 3), "iso", 12, "0")  # with KFWD_DWF: no grouped plan
KFWD_DWF = 4.0


def case_problem(c, dtype: str, dwf: float = 1.0):
    """state_ref.case_problem plus the case's weights ``w``; ``dwf``: detector width factor."""
    from oracle.geometry import Geometry, joseph_matrix
    P = sr.case_problem(c, dtype)
    if dwf != 1.0:
        P["A"] = joseph_matrix(Geometry(c.N, c.a_per, dwf))
        P["b"], P["ph"] = sr.sinograms(P["A"], c.N, P["plan"].local_nodes, c.seed, dtype)
    P["w"] = ray_weights(c.a_per, c.N, P["plan"].local_nodes, c.seed, dtype)
    return P
