"""References for the Huber data term by reweighted rays (run_admm(robust=delta), csrc/robust.hip),
built on tests/weights_ref.py and tests/state_ref.py.

* ``huber_weights_ref``: admm_huber_weights' operation order in NumPy -- every line one IEEE operation
  of the device's, so ``w_out`` is bitwise the kernel's --, the sums by math.fsum;
* ``irls_run``: whole iterations from the zero state, composed of weights_ref.oracle_update_weighted
  (the x-update under the current weights), the reweighting of its residual, state_ref.consensus_ref
  and state_ref.continue_state;
* ``near_threshold``: the rays of such a run whose |residual| lies within margin * delta of delta --
  the rays whose side of the threshold a rounding may change;
* the cases: ``PARITY_RUNS`` (run_admm against ``irls_run``) and the zinger case (``zinger_problem``,
  ``zinger_runs``), kept here so that test_robust_cpu.py checks their conditions without a GPU.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import state_ref as sr
import weights_ref as wr
from oracle import node_solver as ons

DELTA = 0.3


# --------------------------------------------------------------------------------------
# the kernel
# --------------------------------------------------------------------------------------
def huber_weights_ref(ax, b, delta, w=None, dtype=np.float64):
    """(w_out, loss, outliers) of one image's rays: ``ax``, ``b``, ``w`` (or None) hold values of
    ``dtype``; w_out is an array of ``dtype``, loss = fsum(w psi) a float, outliers an int."""
    ax, b = np.asarray(ax, dtype=dtype).reshape(-1), np.asarray(b, dtype=dtype).reshape(-1)
    delta = float(delta)
    hd = 0.5 * (delta * delta)
    with np.errstate(all="ignore"):  # both branches of a where are formed: inf - inf, 0 / 0 on the unused side
        r = ax - b
        a = np.abs(r.astype(np.float64))
        inl = a <= delta
        h64 = np.where(inl, 1.0, delta / a)
        h = h64.astype(dtype)
        psi = np.where(inl, 0.5 * (a * a), delta * a - hd)
        beyond = a > delta
        if w is None:
            w_out, terms, counted = h, psi, beyond
        else:
            w = np.asarray(w, dtype=dtype).reshape(-1)
            masked = w == 0
            w_out = np.where(masked, np.zeros_like(h), w * h).astype(dtype)
            terms = np.where(masked, 0.0, w.astype(np.float64) * psi)
            counted = beyond & ~masked
    loss = float("nan") if np.any(np.isnan(terms)) else math.fsum(terms)
    return w_out, loss, int(np.count_nonzero(counted))


def huber_closed_form(r, delta, w=None):
    """sum_r w_r psi_delta(r_r) written as the textbook min-form, in float64 (not the kernel's order)."""
    a = np.abs(np.asarray(r, dtype=np.float64))
    q = np.minimum(a, delta)
    psi = q * (a - 0.5 * q)
    return math.fsum(psi if w is None else np.asarray(w, dtype=np.float64) * psi)


# --------------------------------------------------------------------------------------
# whole iterations
# --------------------------------------------------------------------------------------
def zero_state(plan, n: int):
    """The state run_admm starts from: everything zero, stored z."""
    E = max(len(plan.stored_edges), 1)
    return {"x_ext": np.zeros((plan.n_xext, n)), "d": np.zeros((plan.V, 2, n)), "e": np.zeros((plan.V, 2, n)),
            "y": np.zeros((E, n)), "y_b": None, "z": np.zeros((E, n)), "x_prev": None}


def applies(k: int, every: int, until) -> bool:
    return (k + 1) % every == 0 and (until is None or k + 1 <= until)


def irls_run(plan, A, b, q_fn, prm, iters: int, delta=None, every: int = 1, until=None, w=None, phantom=None,
             dtype=np.float64):
    """``iters`` ADMM iterations from the zero state on the single-rank ``plan`` (midpoint fusion, stored
    z) in float64 arithmetic (``dtype``: the sample type the residual and the weights are formed in).
    ``delta`` None: plain (weighted) least squares.  ``w``: {g: (m,)} caller weights, a missing node has 1.
    Returns a dict: x (V, n), primal, loss_total, loss / outliers (per iteration (V,) arrays),
    img_err (sqrt(sum_i |x_i - phantom|^2 / V) per iteration), residuals (per iteration (V, m), in
    float64) and base (V, m): the caller's weights."""
    n = A.shape[1]
    V = plan.V
    w = dict(w or {})
    st = zero_state(plan, n)
    weff = dict(w)
    edges = [(plan.edge_a_row[k], plan.edge_b_row[k]) for k in range(len(plan.stored_edges))]
    out = {"primal": [], "loss_total": [], "loss": [], "outliers": [], "img_err": [], "residuals": []}
    base = np.stack([np.asarray(w[g], dtype=np.float64) if g in w else np.ones(A.shape[0])
                     for g in plan.local_nodes])
    for k in range(iters):
        upd = wr.oracle_update_weighted(st, plan, A, b, weff, q_fn, prm, "midpoint", phantom=phantom)
        x = upd["x"]
        loss, cnt, res = np.zeros(V), np.zeros(V), []
        for r, g in enumerate(plan.local_nodes):
            ax = np.asarray(A @ np.asarray(x[r], dtype=dtype), dtype=dtype)
            bg = np.asarray(b[g], dtype=dtype).reshape(-1)
            res.append((ax - bg).astype(np.float64))
            if delta is not None:
                wo, loss[r], cnt[r] = huber_weights_ref(ax, bg, delta, w.get(g), dtype)
                if applies(k, every, until):
                    weff[g] = wo.astype(np.float64)
        x_ext = np.array(st["x_ext"])
        x_ext[:V] = x
        if edges:
            zn, yn, _, es = sr.consensus_ref(x_ext, st["y"], None, st["z"], None, edges, "midpoint")
            st = sr.continue_state(st, upd, y=yn, z=zn)
            out["primal"].append(math.sqrt(math.fsum(es[:, 0]) + math.fsum(es[:, 1])))
        else:
            st = sr.continue_state(st, upd)
            out["primal"].append(0.0)
        out["loss"].append(loss)
        out["loss_total"].append(float(np.sum(loss)))
        out["outliers"].append(cnt)
        out["residuals"].append(np.stack(res))
        if phantom is not None:
            out["img_err"].append(math.sqrt(float(np.sum((x - phantom[None, :]) ** 2)) / V))
    out["x"] = st["x_ext"][:V].copy()
    out["base"] = base
    return out


def near_threshold(run, delta: float, margin: float) -> int:
    """Unmasked rays of ``run`` (every iteration, every node) with ||r| - delta| <= margin * delta."""
    live = run["base"] != 0
    return int(sum(np.count_nonzero((np.abs(np.abs(r) - delta) <= margin * delta) & live) for r in run["residuals"]))


# --------------------------------------------------------------------------------------
# the parity cases: run_admm(robust=DELTA) against irls_run, 3 iterations of 2 x 3 from zero
# --------------------------------------------------------------------------------------
PARITY_ITERS = 3
_CASES = {
    "ring33": sr.Case(33, 3, "ring", 2, 3, "iso", 12, "1", "midpoint", False, 1),
    "ring33w": sr.Case(33, 3, "ring", 2, 3, "iso", 12, "1", "midpoint", False, 2),  # (seed 1 has a ray at the threshold)
    "star33": sr.Case(33, 5, "star", 2, 3, "iso", 9, None, "midpoint", False, 1),
    "ring64": sr.Case(64, 4, "ring", 2, 3, "iso", 24, "0", "midpoint", False, 1),
}
# (case, every, caller weights)
PARITY_RUNS = [("ring33", 1, False), ("ring33", 2, False), ("ring33w", 1, True), ("star33", 1, False),
               ("star33", 2, False), ("ring64", 1, False), ("ring64", 2, False)]
PARITY_MARGIN = 1e-5   # no ray of a parity run lies this close (relative to delta) to the threshold
COUNT_MARGIN = 1e-4    # float32 samples: rays this close may fall on the other side


def parity_id(p) -> str:
    return f"{p[0]}-every{p[1]}" + ("-weights" if p[2] else "")


@functools.lru_cache(maxsize=None)
def parity_problem(name: str, dtype: str, weights: bool):
    c = _CASES[name]
    P = wr.case_problem(c, dtype) if weights else sr.case_problem(c, dtype)
    P["case"] = c
    return P


@functools.lru_cache(maxsize=None)
def parity_reference(name: str, every: int, weights: bool, dtype: str):
    """``irls_run`` of a parity run on the sinograms (and weights) of sample type ``dtype``, in float64."""
    P = parity_problem(name, dtype, weights)
    return irls_run(P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], PARITY_ITERS, DELTA, every=every,
                    w=P.get("w"), phantom=P["ph"])


# --------------------------------------------------------------------------------------
# the zinger case: 33^2, a 4-node ring, 24 angles per node, 12 iterations of 4 x 5; 3 % of the rays
# off by +-3; the clean-data parameters rho = 1, lam = 0.01, mu = 0.1, state_ref.precisions
# --------------------------------------------------------------------------------------
Z_N, Z_V, Z_APER, Z_ITERS, Z_SEED = 33, 4, 24, 12, 1
Z_FRACTION, Z_AMPLITUDE = 0.03, 3.0
Z_RHO, Z_LAM, Z_MU, Z_TV, Z_CG = 1.0, 0.01, 0.1, 4, 5


@functools.lru_cache(maxsize=None)
def zinger_problem():
    """The case's plan, matrix, clean (noisy, outlier-free) and corrupted sinograms, phantom, precisions."""
    c = sr.Case(Z_N, Z_V, "ring", Z_TV, Z_CG, "iso", Z_APER, None, "midpoint", False, Z_SEED)
    P = sr.case_problem(c, "float64")
    P["prm"] = ons.NodeParams(rho=Z_RHO, lam=Z_LAM, mu=Z_MU, tv_iters=Z_TV, cg_iters=Z_CG, tv_kind="iso")
    rng = np.random.default_rng([Z_SEED, 333])
    bad = {}
    for g in P["plan"].local_nodes:
        b = np.array(P["b"][g], dtype=np.float64)
        hit = rng.random(b.shape) < Z_FRACTION
        b[hit] += np.where(rng.random(b.shape) < 0.5, -Z_AMPLITUDE, Z_AMPLITUDE)[hit]
        bad[g] = b
    P["b_zinger"] = bad
    P["case"] = c
    return P


@functools.lru_cache(maxsize=None)
def zinger_runs():
    """{"plain", "clean", "robust"}: irls_run on the corrupted data without and with the Huber loss, and
    on the clean data without."""
    P = zinger_problem()
    run = lambda b, delta: irls_run(P["plan"], P["A"], b, P["q_fn"], P["prm"], Z_ITERS, delta,  # noqa: E731
                                    phantom=P["ph"])
    return {"plain": run(P["b_zinger"], None), "clean": run(P["b"], None), "robust": run(P["b_zinger"], DELTA),
            "robust_clean": run(P["b"], DELTA)}
