"""References for over-relaxation (run_admm(relaxation=alpha), csrc/relax.hip), built on the unchanged
oracle (oracle.node_solver, oracle.admm's loops restated) and on tests/bounds_ref.py.

Over-relaxation replaces x_i in the z- and y-updates by xh_i = alpha x_i + (1 - alpha) z_old
(Eckstein-Bertsekas; Boyd et al. 3.4.3).  With om = 1 - alpha formed once:

    hz = om * z,   xha = alpha * x_a + hz,   xhb = alpha * x_b + hz
    midpoint:  aa = xha + y,  ab = xhb - y,    z' = (aa + ab) * 0.5
    weighted:  aa = xha + y,  ab = xhb + y_b,  z' = (W_a aa + W_b ab) / (W_a + W_b),  y_b' = (y_b + xhb) - z'
    y' = (y + xha) - z'
    RA2 = sum (x_a - z')^2,  RB2 = sum (x_b - z')^2,  DZ2 = sum (z' - z)^2      (the true x)

and for a bound-constraint slot:  xh = alpha * x + om * w,  t = xh + f,  w' = clip(t),  f' = t - w'.

* ``edge_ref`` / ``project_ref``: the two updates in NumPy in exactly that operation order (every line
  one IEEE operation), their sums by math.fsum;
* ``relaxed_admm``: oracle.admm.decentralized_admm's midpoint and weighted loops (fixed counts) with
  optional bounds (bounds_ref.bounded_admm's loop) and ``alpha``; alpha = 1 reproduces them bit for bit;
* ``iters_to``: the first iteration count at which every given residual history is below a tolerance.
"""
from __future__ import annotations

import math

import numpy as np

import bounds_ref as br
from oracle import node_solver as ons
from oracle.admm import EXTRA_KEYS, HISTORY_KEYS, canonical_edges, eps_target


def relaxed(alpha, om, x, z):
    """alpha * x + om * z: two products and one sum, each rounded once."""
    return alpha * x + om * z


def edge_ref(x_ext, y, z, edge_a, edge_b, alpha, y_b=None, W=None):
    """One relaxed update of every edge slot e = (edge_a[e], edge_b[e]) (rows of x_ext) around
    y, z (E, n) (weighted: y_b (E, n) and W, one row per x_ext row).  Returns y', z', y_b' (None for
    midpoint fusion) and the (E, 3) sums RA2, RB2, DZ2, each by math.fsum.  The inputs are not changed."""
    x_ext, y, z = (np.asarray(a, dtype=np.float64) for a in (x_ext, y, z))
    alpha = float(alpha)
    om = 1.0 - alpha
    yn, zn = np.empty_like(y), np.empty_like(z)
    ybn = None if y_b is None else np.empty_like(np.asarray(y_b, dtype=np.float64))
    sums = np.zeros((y.shape[0], 3))
    for e in range(y.shape[0]):
        xa, xb = x_ext[edge_a[e]], x_ext[edge_b[e]]
        hz = om * z[e]
        xha = alpha * xa + hz
        xhb = alpha * xb + hz
        aa = xha + y[e]
        if y_b is None:
            ab = xhb - y[e]
            zn[e] = (aa + ab) * 0.5
        else:
            wa, wb = W[edge_a[e]], W[edge_b[e]]
            ab = xhb + y_b[e]
            zn[e] = (wa * aa + wb * ab) / (wa + wb)
            ybn[e] = (y_b[e] + xhb) - zn[e]
        yn[e] = (y[e] + xha) - zn[e]
        for c, d in enumerate((xa - zn[e], xb - zn[e], zn[e] - z[e])):
            sums[e, c] = math.fsum(d * d)
    return yn, zn, ybn, sums


def project_ref(x, w, f, l, h, alpha):
    """bounds_ref.project_ref around the relaxed images: returns w', f' and the (nimg, 3) sums
    |x - w'|^2, |w' - w|^2, |x - clip(x)|^2 (the true x), each by math.fsum."""
    x, w, f = (np.asarray(a, dtype=np.float64) for a in (x, w, f))
    alpha = float(alpha)
    om = 1.0 - alpha
    t = relaxed(alpha, om, x, w) + f
    wn = br.clip(t, l, h)
    fn = t - wn
    sums = np.zeros((x.shape[0], 3))
    for v in range(x.shape[0]):
        for c, d in enumerate((x[v] - wn[v], wn[v] - w[v], x[v] - br.clip(x[v], l, h))):
            sums[v, c] = math.fsum(d * d)
    return wn, fn, sums


def relaxed_admm(ops, sinograms, G, Qij_diag_fn, N, alpha=1.0, fusion="midpoint", Wi_list=None, bounds=None,
                 bound_weight=1.0, lam_tv=0.01, rho=1.0, max_iters=10, eps_pri=0.0, eps_dual=0.0, phantom_true=None,
                 mu=None, tv_iters=10, cg_iters=5, tv_kind="iso", dtype=np.float64):
    """oracle.admm.decentralized_admm (fixed counts, midpoint or weighted fusion) with the relaxed edge
    updates above; ``bounds`` (midpoint only) adds bounds_ref.bounded_admm's constraint, its projection
    relaxed too.  The statistics are formed as the oracle forms them (dot products).  Returns
    (x_list, w_list, history); w_list is None without bounds."""
    weighted = fusion == "weighted"
    bounded = bounds is not None
    assert fusion in ("midpoint", "weighted") and not (weighted and bounded)
    alpha = float(alpha)
    om = 1.0 - alpha
    V, n = len(ops), N * N
    mu = 10.0 * lam_tv if mu is None else mu
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
        if bounded:  # the relaxed projection, after the edge updates
            wn, fn, sums = project_ref(np.stack(x), np.stack(w), np.stack(f), l, h, alpha)
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


def iters_to(hist, tol, keys=("primal", "dual")):
    """Iterations until every history of ``keys`` is below ``tol`` at once (1-based), or None."""
    ok = np.all([np.asarray(hist[k]) < tol for k in keys], axis=0)
    return int(np.argmax(ok)) + 1 if ok.any() else None
