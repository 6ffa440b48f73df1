"""References for unreliable links (run_admm(links=...), csrc/links.hip), built on tests/relax_ref.py and the
unchanged oracle.

At every iteration each edge is up or down.  An up edge performs relax_ref.edge_ref's update (alpha = 1: the
plain one); a down edge keeps y, z (and y_b) as they are and reports

    RA2 = sum (x_a - z)^2,  RB2 = sum (x_b - z)^2,  DZ2 = +0.0.

* ``edge_ref``: one gated update of every edge slot in NumPy, the sums by math.fsum;
* ``gated_admm``: relax_ref.relaxed_admm's loop (midpoint and weighted fusion, optional bounds, alpha) with a
  bool table (iterations, edges) in oracle.admm.canonical_edges order; an all-true table reproduces
  relaxed_admm bit for bit (test_links_cpu.py).  Every node runs its x-update every iteration and the
  constraint's projection is never gated.
"""
from __future__ import annotations

import math

import numpy as np

import bounds_ref as br
import relax_ref as rr
from oracle import node_solver as ons
from oracle.admm import EXTRA_KEYS, HISTORY_KEYS, canonical_edges, eps_target


def edge_ref(x_ext, y, z, edge_a, edge_b, up, alpha=1.0, y_b=None, W=None):
    """One gated update of every edge slot: relax_ref.edge_ref where ``up[e]``, the state kept and the sums
    above where not.  Returns y', z', y_b' (None for midpoint fusion) and the (E, 3) sums.  The inputs are not
    changed."""
    x_ext, y, z = (np.asarray(a, dtype=np.float64) for a in (x_ext, y, z))
    yn, zn, ybn, sums = rr.edge_ref(x_ext, y, z, edge_a, edge_b, alpha, y_b=y_b, W=W)
    for e in range(y.shape[0]):
        if up[e]:
            continue
        yn[e], zn[e] = y[e], z[e]
        if ybn is not None:
            ybn[e] = np.asarray(y_b, dtype=np.float64)[e]
        for c, d in enumerate((x_ext[edge_a[e]] - z[e], x_ext[edge_b[e]] - z[e])):
            sums[e, c] = math.fsum(d * d)
        sums[e, 2] = 0.0
    return yn, zn, ybn, sums


def gated_admm(ops, sinograms, G, Qij_diag_fn, N, table, alpha=1.0, fusion="midpoint", Wi_list=None, bounds=None,
               bound_weight=1.0, lam_tv=0.01, rho=1.0, max_iters=10, eps_pri=0.0, eps_dual=0.0, phantom_true=None,
               mu=None, tv_iters=10, cg_iters=5, tv_kind="iso", dtype=np.float64):
    """relax_ref.relaxed_admm with ``table[k, e]`` = edge e of canonical_edges(G) is up in iteration k.
    Returns (x_list, w_list, history); w_list is None without bounds."""
    weighted = fusion == "weighted"
    bounded = bounds is not None
    assert fusion in ("midpoint", "weighted") and not (weighted and bounded)
    alpha = float(alpha)
    om = 1.0 - alpha
    V, n = len(ops), N * N
    mu = 10.0 * lam_tv if mu is None else mu
    prm = ons.NodeParams(rho=rho, lam=lam_tv, mu=mu, tv_iters=tv_iters, cg_iters=cg_iters, tv_kind=tv_kind)
    edges = canonical_edges(G)
    table = np.asarray(table, dtype=bool)
    assert table.shape[0] >= max_iters and table.shape[1] == len(edges)
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
        for ge, e in enumerate(edges):
            a_, b_ = e
            if table[k, ge]:
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
            else:  # down: y, z (y2) stay; the disagreement with the last agreed z
                ra, rb = x[a_] - z[e], x[b_] - z[e]
                ra2, rb2, dz2 = float(ra @ ra), float(rb @ rb), 0.0
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
        if bounded:  # the (relaxed) projection, after the edge updates: node-local, never gated
            wn, fn, sums = rr.project_ref(np.stack(x), np.stack(w), np.stack(f), l, h, alpha)
            w, f = list(wn), list(fn)
            bp, bd = math.sqrt(float(np.sum(sums[:, 0]))), rho * math.sqrt(float(np.sum(sums[:, 1])))
            hist["bound_primal"].append(bp)
            hist["bound_dual"].append(bd)
            hist["bound_violation"].append(math.sqrt(float(np.sum(sums[:, 2]))))
            hist["bound_pri_per_node"].append(sums[:, 0].copy())
            hist["bound_violation_per_node"].append(sums[:, 2].copy())
            stop = stop and bp < eps_pri and bd < eps_dual
        if stop:
            break
    return x, (w if bounded else None), hist
