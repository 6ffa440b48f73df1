"""References for residual-balancing rho and the scale-free stop test (run_admm(adapt_rho=...,
eps_abs=..., eps_rel=...), csrc/norms.hip, admm_batch_set_rho), built on the unchanged oracle and on
tests/relax_ref.py / tests/bounds_ref.py.

* ``node_norms_ref``: the three sums of admm_node_norms in NumPy, in the kernel's operation order per
  pixel (over a node's incidences ascending: s += yv, zz += z * z; then x * x, zz, s * s), each sum over
  the pixels by math.fsum;
* ``complete`` / ``balance_ref`` / ``thresholds_ref``: the rules of Boyd et al. 3.4.1 and (3.12), written
  here a second time (the code under test is admm_hip/penalty.py);
* ``adaptive_admm``: relax_ref.relaxed_admm's loop (alpha, bounds, weighted fusion) with the balancing
  rule, the dual rescale and the stop test.  With both features off it is that loop bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

import bounds_ref as br
import relax_ref as rr
from oracle import node_solver as ons
from oracle.admm import EXTRA_KEYS, HISTORY_KEYS, canonical_edges, eps_target

NORM_KEYS = ("eps_pri_history", "eps_dual_history", "ax_norm", "bz_norm", "aty_norm")


def node_norms_ref(x, y, y_b, z, inc_off, inc_edge, inc_sign):
    """(nimg, 3) X2, Z2, U2 of the rows of x: over image v's incidences q = inc_off[v] .. inc_off[v+1]-1
    ascending, yv = y[e] where inc_sign[q] > 0, else y_b[e] (or -y[e] without y_b); s += yv,
    zz += z[e] * z[e] from +0; X2 = fsum(x * x), Z2 = fsum(zz), U2 = fsum(s * s)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((x.shape[0], 3))
    for v in range(x.shape[0]):
        s, zz = np.zeros(x.shape[1]), np.zeros(x.shape[1])
        for q in range(int(inc_off[v]), int(inc_off[v + 1])):
            e = int(inc_edge[q])
            yv = y[e] if inc_sign[q] > 0 else (y_b[e] if y_b is not None else -y[e])
            s = s + yv
            zz = zz + z[e] * z[e]
        out[v] = (math.fsum(x[v] * x[v]), math.fsum(zz), math.fsum(s * s))
    return out


def complete(adapt, rho):
    """The full configuration of ``adapt`` (True or a dict) around rho_0 = rho."""
    cfg = dict(ratio=10.0, factor=2.0, every=1, until=None, rho_min=rho / 1024.0, rho_max=rho * 1024.0)
    if adapt is not True:
        cfg.update(adapt)
    return cfg


def balance_ref(rho, r, s, cfg, k):
    """(rho after iteration k, the two margins r / (ratio s) and s / (ratio r) when the rule was
    evaluated, else None)."""
    if (k + 1) % cfg["every"] != 0 or (cfg["until"] is not None and k + 1 > cfg["until"]):
        return rho, None
    if not (math.isfinite(r) and math.isfinite(s)):
        return rho, None
    margins = (r / (cfg["ratio"] * s), s / (cfg["ratio"] * r))
    if r > cfg["ratio"] * s:
        return min(rho * cfg["factor"], cfg["rho_max"]), margins
    if s > cfg["ratio"] * r:
        return max(rho / cfg["factor"], cfg["rho_min"]), margins
    return rho, margins


def thresholds_ref(eps_abs, eps_rel, n, ninc, norms, rho):
    """(eps_pri_k, eps_dual_k, ||Ax||, ||Bz||, ||A^T y||) of Boyd et al. (3.12)."""
    ax = math.sqrt(sum(float(c) * float(v) for c, v in zip(ninc, norms[:, 0])))
    bz = math.sqrt(math.fsum(norms[:, 1]))
    aty = rho * math.sqrt(math.fsum(norms[:, 2]))
    return (math.sqrt(n * float(sum(ninc))) * eps_abs + eps_rel * max(ax, bz),
            math.sqrt(n * len(ninc)) * eps_abs + eps_rel * aty, ax, bz, aty)


def adaptive_admm(ops, sinograms, G, Qij_diag_fn, N, adapt=None, eps_abs=None, eps_rel=None, alpha=1.0,
                  fusion="midpoint", Wi_list=None, bounds=None, bound_weight=1.0, lam_tv=0.01, rho=1.0, max_iters=10,
                  eps_pri=0.0, eps_dual=0.0, phantom_true=None, mu=None, tv_iters=10, cg_iters=5, tv_kind="iso",
                  dtype=np.float64, trace=None):
    """relax_ref.relaxed_admm with ``adapt`` (None, True or a dict: residual balancing) and eps_abs /
    eps_rel (None: the absolute test).  The history gains rho_history (adapt), NORM_KEYS (tolerances)
    and, with adapt, ``margins``: per evaluated decision (k, r / (ratio s), s / (ratio r)).  ``trace``: a
    list that receives (k, rho_old, rho_new, y before, y after) of every change, y as {edge: array}.
    Returns (x_list, w_list, history)."""
    weighted = fusion == "weighted"
    bounded = bounds is not None
    assert fusion in ("midpoint", "weighted") and not (weighted and bounded)
    cfg = None if adapt is None or adapt is False else complete(adapt, rho)
    tol = None if eps_abs is None and eps_rel is None else (float(eps_abs or 0.0), float(eps_rel or 0.0))
    alpha = float(alpha)
    om = 1.0 - alpha
    V, n = len(ops), N * N
    mu = 10.0 * lam_tv if mu is None else mu
    rho0 = rho
    prm = ons.NodeParams(rho=rho, lam=lam_tv, mu=mu, tv_iters=tv_iters, cg_iters=cg_iters, tv_kind=tv_kind)
    edges = canonical_edges(G)
    b = [np.asarray(s, dtype=np.float64).reshape(-1) for s in sinograms]
    ATs = [A.T.tocsr() for A in ops]
    Atb = [ATs[i] @ b[i] for i in range(V)]
    states = [ons.NodeState.zeros(n, dtype) for _ in range(V)]
    y = {e: np.zeros(n) for e in edges}
    z = {e: np.zeros(n) for e in edges}
    y2 = {e: np.zeros(n) for e in edges} if weighted else None
    if weighted or bounded:
        W = [np.asarray(w, dtype=np.float64).reshape(-1) for w in Wi_list]
    if bounded:
        l, h = br.box(bounds, n)
        qc = [bound_weight * W[i] for i in range(V)]
    w = [np.zeros(n) for _ in range(V)]
    f = [np.zeros(n) for _ in range(V)]
    nbrs = {i: list(G.neighbors(i)) for i in range(V)}
    hist = {k: [] for k in HISTORY_KEYS + EXTRA_KEYS + (br.BOUND_KEYS if bounded else ())}
    if cfg is not None:
        hist["rho_history"], hist["margins"] = [], []
    if tol is not None:
        hist.update({k: [] for k in NORM_KEYS})
        # node i's incidences: its edges in the run's edge order, then its constraint slot E + i
        off, inc_e, inc_s = [0], [], []
        for i in range(V):
            for ge, e in enumerate(edges):
                if i in e:
                    inc_e.append(ge)
                    inc_s.append(1 if i == e[0] else -1)
            if bounded:
                inc_e.append(len(edges) + i)
                inc_s.append(1)
            off.append(len(inc_e))
        ninc = [off[i + 1] - off[i] for i in range(V)]
    ph = None if phantom_true is None else np.asarray(phantom_true, dtype=np.float64).reshape(-1)
    x = [np.zeros(n) for _ in range(V)]
    for k in range(max_iters):
        obj_i, g_i, mse_i, sb_i = np.zeros(V), np.zeros(V), np.zeros(V), np.zeros(V)
        for i in range(V):
            qv = []
            for j in nbrs[i]:
                e = (min(i, j), max(i, j))
                yi = y[e] if i == e[0] else (y2[e] if weighted else -y[e])
                qv.append((np.asarray(Qij_diag_fn(i, j), dtype=np.float64), z[e] - yi))
            if bounded:
                qv.append((qc[i], w[i] - f[i]))
            D, c = ons.assemble(qv, n)
            d = ons.node_update(ops[i], Atb[i], b[i], D, c, qv, states[i], N, prm, dtype=dtype, AT=ATs[i])
            obj_i[i], sb_i[i], g_i[i], mse_i[i] = d.obj, d.sb_res, d.g_norm, d.mse_sino
        x = [st.x.astype(np.float64) for st in states]
        hist["g_norm_history"].append(g_i)
        hist["eps_used_history"].append(np.full(V, np.nan))
        hist["sb_res_history"].append(sb_i)
        hist["inner_updates_history"].append(np.ones(V, dtype=np.int64))
        hist["eps_target_history"].append(np.full(V, eps_target(k)))
        hist["mse_sino_per_node"].append(mse_i)
        hist["mse_sino_total"].append(float(np.sum(mse_i)))
        img = np.array([float((xi - ph) @ (xi - ph)) for xi in x]) if ph is not None else np.full(V, np.nan)
        hist["img_mse_per_node"].append(img)
        hist["img_mse_total"].append(float(np.sum(img)))
        r2 = s2 = 0.0
        pri, dua = np.zeros(V), np.zeros(V)
        for e in edges:
            a_, b_ = e
            hz = om * z[e]
            xha = alpha * x[a_] + hz
            xhb = alpha * x[b_] + hz
            aa = xha + y[e]
            if weighted:
                ab = xhb + y2[e]
                zn = (W[a_] * aa + W[b_] * ab) / (W[a_] + W[b_])
                y2[e] = (y2[e] + xhb) - zn
            else:
                ab = xhb - y[e]
                zn = (aa + ab) * 0.5
            y[e] = (y[e] + xha) - zn
            ra, rb, dz = x[a_] - zn, x[b_] - zn, zn - z[e]
            z[e] = zn
            ra2, rb2, dz2 = float(ra @ ra), float(rb @ rb), float(dz @ dz)
            r2 += ra2 + rb2
            pri[a_] += ra2
            pri[b_] += rb2
            s2 += rho * rho * dz2
            dua[a_] += rho * rho * dz2
            dua[b_] += rho * rho * dz2
        pn, dn = math.sqrt(r2), math.sqrt(s2)
        hist["primal"].append(pn)
        hist["dual"].append(dn)
        hist["obj_per_node"].append(obj_i)
        hist["obj_total"].append(float(np.sum(obj_i)))
        hist["pri_per_node"].append(np.sqrt(pri))
        hist["dual_per_node"].append(np.sqrt(dua))
        stop = pn < eps_pri and dn < eps_dual
        r_k, s_k = pn, dn
        if bounded:  # the relaxed projection, after the edge updates
            wn, fn, sums = rr.project_ref(np.stack(x), np.stack(w), np.stack(f), l, h, alpha)
            w, f = list(wn), list(fn)
            bp, bd = math.sqrt(float(np.sum(sums[:, 0]))), rho * math.sqrt(float(np.sum(sums[:, 1])))
            hist["bound_primal"].append(bp)
            hist["bound_dual"].append(bd)
            hist["bound_violation"].append(math.sqrt(float(np.sum(sums[:, 2]))))
            hist["bound_pri_per_node"].append(sums[:, 0].copy())
            hist["bound_violation_per_node"].append(sums[:, 2].copy())
            stop = stop and bp < eps_pri and bd < eps_dual
            r_k, s_k = math.sqrt(pn * pn + bp * bp), math.sqrt(dn * dn + bd * bd)
        if cfg is not None:
            hist["rho_history"].append(float(rho))
        if tol is not None:  # the scale-free test replaces the absolute one
            ys = np.stack([y[e] for e in edges] + (f if bounded else []))
            zs = np.stack([z[e] for e in edges] + (w if bounded else []))
            y2s = np.stack([y2[e] for e in edges]) if weighted else None
            norms = node_norms_ref(np.stack(x), ys, y2s, zs, off, inc_e, inc_s)
            vals = thresholds_ref(tol[0], tol[1], n, ninc, norms, rho)
            for key, val in zip(NORM_KEYS, vals):
                hist[key].append(val)
            stop = r_k < vals[0] and s_k < vals[1]
        if stop:
            break
        if cfg is not None and k + 1 < max_iters:
            new, margins = balance_ref(rho, r_k, s_k, cfg, k)
            if margins is not None:
                hist["margins"].append((k,) + margins)
            if new != rho:  # the scaled duals stand for rho y: rescale them, keep z, d, e
                c = rho / new
                before = {e: y[e].copy() for e in edges}
                for e in edges:
                    y[e] = y[e] * c
                    if weighted:
                        y2[e] = y2[e] * c
                f = [fi * c for fi in f]
                if trace is not None:
                    trace.append((k, rho, new, before, {e: y[e].copy() for e in edges}))
                rho = new
                prm = ons.NodeParams(rho=rho, lam=lam_tv, mu=mu, tv_iters=tv_iters, cg_iters=cg_iters, tv_kind=tv_kind)
    assert cfg is not None or rho == rho0
    return x, (w if bounded else None), hist
