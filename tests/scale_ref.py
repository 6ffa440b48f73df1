"""References for the self-scaling Huber threshold (run_admm(robust={"scale": k}), csrc/scale.hip),
built on tests/robust_ref.py, tests/state_ref.py and tests/weights_ref.py.

* ``ray_quantile_ref``: admm_ray_quantile's definition (include/admm_tomo.h) in NumPy -- np.sort of the
  unmasked |ax - b| in the sample type, one multiply and a floor for the rank, one multiply for the
  threshold -- so all three outputs are bitwise the kernel's;
* ``irls_scale_run``: robust_ref.irls_run with each node's threshold formed by ``ray_quantile_ref`` from
  the iteration's own residual, and the freeze rule: estimated at k = 0 and while k + 1 <= until, then kept;
* ``near_threshold`` / ``rank_gap``: the rays of such a run whose side of their node's threshold a rounding
  may change, and how far the selected order statistic lies from its neighbours (0: a tie at the rank);
* the cases: ``PARITY_RUNS`` and the zinger runs at scale = 4 and 1.345, kept here so that
  test_scale_cpu.py checks their conditions without a GPU.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import robust_ref as rr
import state_ref as sr
import weights_ref as wr

SCALE = 4.0
CONSISTENCY = 1.4826
TEXTBOOK = 1.345  # the 95 %-efficiency constant


# --------------------------------------------------------------------------------------
# the kernel
# --------------------------------------------------------------------------------------
def ray_quantile_ref(ax, b, q=0.5, c=1.0, floor=0.0, w=None, dtype=np.float64):
    """(delta, a_k, cnt) of one image's rays as floats: ``ax``, ``b``, ``w`` (or None) hold values of
    ``dtype``."""
    ax, b = np.asarray(ax, dtype=dtype).reshape(-1), np.asarray(b, dtype=dtype).reshape(-1)
    with np.errstate(all="ignore"):
        a = np.abs(ax - b)  # in dtype; |-0| = +0
    if w is not None:
        a = a[np.asarray(w, dtype=dtype).reshape(-1) != 0]
    cnt = int(a.size)
    if cnt == 0:
        return math.inf, 0.0, 0.0
    k = int(math.floor(float(q) * float(cnt - 1)))
    ak = float(np.sort(a)[k])  # NaN sorts last, +inf before it
    with np.errstate(all="ignore"):
        t = float(np.float64(c) * np.float64(ak))
    delta = max(t, float(floor)) if (math.isfinite(t) and t > 0.0) else math.inf
    return delta, ak, float(cnt)


# --------------------------------------------------------------------------------------
# whole iterations
# --------------------------------------------------------------------------------------
def estimates(k: int, until) -> bool:
    return k == 0 or until is None or k + 1 <= until


def irls_scale_run(plan, A, b, q_fn, prm, iters: int, scale: float, every: int = 1, until=None, w=None,
                   phantom=None, dtype=np.float64, quantile=0.5, delta_min=0.0, consistency=CONSISTENCY):
    """robust_ref.irls_run with delta_g = max(scale * consistency * a_k, delta_min) per node and
    iteration (``ray_quantile_ref`` of that iteration's residual under the caller's mask), frozen as
    ``estimates`` says.  Returns irls_run's dict and ``delta`` / ``value``: per iteration (V,) arrays of the
    threshold in force and of the order statistic last estimated."""
    n = A.shape[1]
    V = plan.V
    w = dict(w or {})
    c = float(scale) * float(consistency)
    st = rr.zero_state(plan, n)
    weff = dict(w)
    edges = [(plan.edge_a_row[k], plan.edge_b_row[k]) for k in range(len(plan.stored_edges))]
    out = {"primal": [], "loss_total": [], "loss": [], "outliers": [], "img_err": [], "residuals": [], "delta": [],
           "value": []}
    base = np.stack([np.asarray(w[g], dtype=np.float64) if g in w else np.ones(A.shape[0])
                     for g in plan.local_nodes])
    delta, value = np.full(V, math.inf), np.zeros(V)
    for k in range(iters):
        upd = wr.oracle_update_weighted(st, plan, A, b, weff, q_fn, prm, "midpoint", phantom=phantom)
        x = upd["x"]
        loss, cnt, res = np.zeros(V), np.zeros(V), []
        for r, g in enumerate(plan.local_nodes):
            ax = np.asarray(A @ np.asarray(x[r], dtype=dtype), dtype=dtype)
            bg = np.asarray(b[g], dtype=dtype).reshape(-1)
            res.append((ax - bg).astype(np.float64))
            if estimates(k, until):
                delta[r], value[r], _ = ray_quantile_ref(ax, bg, quantile, c, delta_min, w.get(g), dtype)
            wo, loss[r], cnt[r] = rr.huber_weights_ref(ax, bg, delta[r], w.get(g), dtype)
            if rr.applies(k, every, until):
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
        out["delta"].append(delta.copy())
        out["value"].append(value.copy())
        if phantom is not None:
            out["img_err"].append(math.sqrt(float(np.sum((x - phantom[None, :]) ** 2)) / V))
    out["x"] = st["x_ext"][:V].copy()
    out["base"] = base
    return out


def near_threshold(run, margin: float) -> int:
    """Unmasked rays of ``run`` (every iteration, every node) with ||r| - delta_g| <= margin * delta_g."""
    live = run["base"] != 0
    tot = 0
    for r, d in zip(run["residuals"], run["delta"]):
        fin = np.isfinite(d)[:, None] & live
        dd = np.where(np.isfinite(d), d, 1.0)[:, None]
        tot += int(np.count_nonzero((np.abs(np.abs(r) - dd) <= margin * dd) & fin))
    return tot


def rank_gap(run, quantile=0.5, until=None) -> float:
    """The smallest relative distance, over the iterations that estimate and the nodes, between the selected
    order statistic and its nearer neighbour in the sorted unmasked |r|: 0 means a tie at the rank."""
    live = run["base"] != 0
    gap = math.inf
    for k, r in enumerate(run["residuals"]):
        if not estimates(k, until):
            continue
        for v in range(r.shape[0]):
            a = np.sort(np.abs(r[v][live[v]]))
            j = int(math.floor(quantile * float(a.size - 1)))
            for i in (j - 1, j + 1):
                if 0 <= i < a.size:
                    gap = min(gap, abs(a[i] - a[j]) / a[j])
    return gap


# --------------------------------------------------------------------------------------
# the parity cases: run_admm(robust={"scale": 4}) against irls_scale_run, 3 iterations of 2 x 3 from zero
# on the shapes of robust_ref (33^2 V = 3 ring with the mirror, 33^2 V = 5 star with 9 angles, 64^2 V = 4
# ring without)
# --------------------------------------------------------------------------------------
PARITY_ITERS = rr.PARITY_ITERS
PARITY_MARGIN = rr.PARITY_MARGIN
COUNT_MARGIN = rr.COUNT_MARGIN
# (case, every, caller weights, until, scale).  From zero, three iterations leave residuals whose bulk is
# wide: at scale = 4 no ray lies beyond its threshold yet, so those runs check the estimate, the loss and
# the plumbing; the runs at the textbook 1.345 add thresholds that cut, so the reweighting under a moving
# per-node delta is compared too.
PARITY_RUNS = [("ring33", 1, False, None, SCALE), ("ring33", 2, False, None, SCALE),
               ("ring33w", 1, True, None, SCALE), ("star33", 1, False, None, SCALE),
               ("star33", 2, False, None, SCALE), ("ring64", 1, False, None, SCALE),
               ("ring64", 2, False, None, SCALE), ("ring33", 1, False, 2, SCALE),
               ("ring33", 1, False, None, TEXTBOOK), ("ring33w", 1, True, 2, TEXTBOOK),
               ("ring64", 2, False, None, TEXTBOOK)]


def parity_id(p) -> str:
    return (f"{p[0]}-every{p[1]}" + ("-weights" if p[2] else "") + (f"-until{p[3]}" if p[3] is not None else "")
            + f"-scale{p[4]:g}")


@functools.lru_cache(maxsize=None)
def parity_reference(name: str, every: int, weights: bool, until, scale: float, dtype: str):
    """``irls_scale_run`` of a parity run on the sinograms (and weights) of sample type ``dtype``, in
    float64."""
    P = rr.parity_problem(name, dtype, weights)
    return irls_scale_run(P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], PARITY_ITERS, scale, every=every,
                          until=until, w=P.get("w"), phantom=P["ph"])


# --------------------------------------------------------------------------------------
# the zinger case of robust_ref at a dimensionless threshold
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zinger_scale_runs():
    """{"scale4", "scale4_clean", "textbook", "c7", "c7_clean"}: irls_scale_run on robust_ref's zinger case
    at scale = 4 on the corrupted and the clean data, at scale = 1.345 on the corrupted data, and at
    c = 7.0 (scale = 7 / 1.4826) on both."""
    P = rr.zinger_problem()
    run = lambda b, s: irls_scale_run(P["plan"], P["A"], b, P["q_fn"], P["prm"], rr.Z_ITERS, s,  # noqa: E731
                                      phantom=P["ph"])
    return {"scale4": run(P["b_zinger"], SCALE), "scale4_clean": run(P["b"], SCALE),
            "textbook": run(P["b_zinger"], TEXTBOOK), "c7": run(P["b_zinger"], 7.0 / CONSISTENCY),
            "c7_clean": run(P["b"], 7.0 / CONSISTENCY)}
