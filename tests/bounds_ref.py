"""References for the bound constraints lo <= x <= hi, built on the unchanged oracle
(oracle.node_solver, oracle.admm's midpoint branch restated) and on tests/state_ref.py.

The constraint enters node i's subproblem through the splitting x_i = w_i, w_i in [l, h]: one more
term (rho / 2) ||x - (w_i - f_i)||^2_{q_c,i} appended to the node's ``qv`` list (after its edges, so
D and c add it last), and after the edge updates the projection

    t = x_i + f_i,   w_i' = clip(t),   f_i' = t - w_i',   clip(t) = l where t < l, h where t > h, else t.

* ``clip`` / ``project_ref``: the projection in NumPy in the kernel's operation order (each of w', f'
  a single IEEE operation), its three sums by math.fsum;
* ``bounded_admm``: oracle.admm.decentralized_admm's midpoint loop with the constraint;
* ``host_state`` / ``random_state`` / ``oracle_update_bounded``: one x-update from a random warm
  state with random w, f and q_c (state_ref's machinery, the y and z arrays E + V rows long);
* ``BOUND_CASES`` / ``BOUND_REUSE_CASES``: the x-update cases of test_gpu_bounds.py.
"""
from __future__ import annotations

import math

import numpy as np

import state_ref as sr
from oracle import node_solver as ons
from oracle.admm import EXTRA_KEYS, HISTORY_KEYS, canonical_edges, eps_target

BOUND_KEYS = ("bound_primal", "bound_dual", "bound_violation", "bound_pri_per_node", "bound_violation_per_node")


def blocks_phantom(N: int):
    """(n,) phantom with values in {0, 1}: a rectangle and a small square on a zero background."""
    ph = np.zeros((N, N))
    ph[N // 4: (3 * N) // 4, N // 3: (5 * N) // 6] = 1.0
    ph[N // 8: N // 4, N // 8: N // 3] = 1.0
    return ph.reshape(-1)


def box(bounds, n: int):
    """(l, h) per-pixel float64 arrays of ``bounds`` = (lo, hi), each None, a scalar or an array."""
    lo, hi = bounds
    l = np.full(n, -np.inf) if lo is None else np.broadcast_to(np.asarray(lo, dtype=np.float64).reshape(-1), (n,))
    h = np.full(n, np.inf) if hi is None else np.broadcast_to(np.asarray(hi, dtype=np.float64).reshape(-1), (n,))
    return np.array(l), np.array(h)


def clip(t, l, h):
    """Comparisons, not minimum / maximum: t = -0 with l = 0 stays -0, a NaN passes through."""
    return np.where(t < l, l, np.where(t > h, h, t))


def project_ref(x, w, f, l, h):
    """One projection of the images x (nimg, n) around (w, f): returns w', f' and the (nimg, 3) sums
    |x - w'|^2, |w' - w|^2, |x - clip(x)|^2, each by math.fsum."""
    x, w, f = (np.asarray(a, dtype=np.float64) for a in (x, w, f))
    t = x + f
    wn = clip(t, l, h)
    fn = t - wn
    sums = np.zeros((x.shape[0], 3))
    for v in range(x.shape[0]):
        for c, d in enumerate((x[v] - wn[v], wn[v] - w[v], x[v] - clip(x[v], l, h))):
            sums[v, c] = math.fsum(d * d)
    return wn, fn, sums


def column_weights(A):
    """W = max(column sums of A o A, 1e-12): admm_hip.data.make_precisions' W_i for a matrix."""
    return np.maximum(np.asarray(A.multiply(A).sum(axis=0)).reshape(-1), 1e-12)


def bounded_admm(ops, sinograms, G, Qij_diag_fn, Wi_list, N, bounds, bound_weight=1.0, lam_tv=0.01, rho=1.0,
                 max_iters=10, eps_pri=0.0, eps_dual=0.0, phantom_true=None, mu=None, tv_iters=10, cg_iters=5,
                 tv_kind="iso", dtype=np.float64, x_init=None):
    """oracle.admm.decentralized_admm, midpoint fusion and fixed counts, with lo <= x <= hi.
    ``bounds`` None runs the unconstrained loop (no extra term, no extra key).  ``x_init``: one image
    per node; the run then starts from z_e = (x_a + x_b) / 2, w = clip(x), f = 0, zero duals.
    Returns (x_list, w_list, f_list, history)."""
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
    bounded = bounds is not None
    if bounded:
        l, h = box(bounds, n)
        qc = [bound_weight * np.asarray(Wi_list[i], dtype=np.float64).reshape(-1) for i in range(V)]
    w = [np.zeros(n) for _ in range(V)]
    f = [np.zeros(n) for _ in range(V)]
    if x_init is not None:
        for i in range(V):
            states[i].x[:] = np.asarray(x_init[i], dtype=np.float64).reshape(-1)
        for (a_, b_) in edges:
            z[(a_, b_)] = (states[a_].x.astype(np.float64) + states[b_].x.astype(np.float64)) * 0.5
        if bounded:
            w = [clip(states[i].x.astype(np.float64), l, h) for i in range(V)]
    nbrs = {i: list(G.neighbors(i)) for i in range(V)}
    hist = {k: [] for k in HISTORY_KEYS + EXTRA_KEYS + (BOUND_KEYS if bounded else ())}
    ph = None if phantom_true is None else np.asarray(phantom_true, dtype=np.float64).reshape(-1)
    x = [st.x.astype(np.float64) for st in states]
    for k in range(max_iters):
        obj_i, g_i, mse_i, sb_i = np.zeros(V), np.zeros(V), np.zeros(V), np.zeros(V)
        for i in range(V):
            qv = []
            for j in nbrs[i]:
                e = (min(i, j), max(i, j))
                yi = y[e] if i == e[0] else -y[e]
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
            aa = x[a_] + y[e]
            ab = x[b_] - y[e]
            zn = (aa + ab) * 0.5
            y[e] = y[e] + x[a_] - zn
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
        if bounded:  # the projection, after the edge updates
            wn, fn, sums = project_ref(np.stack(x), np.stack(w), np.stack(f), l, h)
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
    return x, w, f, hist


# --------------------------------------------------------------------------------------
# one x-update from a random warm state with a constraint slot per node
# --------------------------------------------------------------------------------------
def host_state(plan, n: int, seed: int, x_ext=None):
    """state_ref.host_state (stored z, midpoint) with V more rows of y and z after the E real ones:
    random f and w (w not inside any box: the x-update only reads it)."""
    st = sr.host_state(plan, n, seed, "midpoint", False, x_ext=x_ext)
    E, V = len(plan.stored_edges), plan.V
    rng = np.random.default_rng([seed, 13])
    st["y"] = np.concatenate([st["y"][:E], 0.5 * rng.standard_normal((V, n))])
    st["z"] = np.concatenate([st["z"][:E], rng.standard_normal((V, n))])
    return st


def random_state(nb, seed: int, keep_x: bool = False):
    """Fill the bound NodeBatch ``nb`` (built with bounds) in place with ``host_state``; ``keep_x``:
    every field but x_ext.  Returns the host float64 copies."""
    import torch
    torch.cuda.synchronize()
    x = nb.x_ext.detach().cpu().numpy() if keep_x else None
    st = host_state(nb.plan, nb.geom.n, seed, x_ext=x)
    for k in ("x_ext", "d", "e", "y", "z"):
        if keep_x and k == "x_ext":
            continue
        t = getattr(nb, k)
        assert tuple(t.shape) == st[k].shape, (k, tuple(t.shape), st[k].shape)
        t.copy_(torch.from_numpy(st[k]))
    torch.cuda.synchronize()
    return st


def rerandomised(plan, n: int, case):
    """The second draw of a start-reuse case: every field but x_ext."""
    st = host_state(plan, n, case.seed + 1000)
    del st["x_ext"]
    return st


def oracle_update_bounded(host_state, plan, A, b, q_fn, qc, params, dtype=np.float64, phantom=None):
    """state_ref.oracle_update with (qc[g], w_k - f_k) appended to local node k's qv list
    (w_k = z[E + k], f_k = y[E + k]); the QUAD statistic therefore includes the constraint's term."""
    st = host_state
    n = st["x_ext"].shape[1]
    N = int(round(math.sqrt(n)))
    V, E = plan.V, len(plan.stored_edges)
    AT = A.T.tocsr()
    out = {"x": np.zeros((V, n)), "d": np.zeros((V, 2, n)), "e": np.zeros((V, 2, n)), "stats": np.zeros((V, 6))}
    for k, g in enumerate(plan.local_nodes):
        qv = []
        for s in range(plan.inc_off[k], plan.inc_off[k + 1]):
            e = plan.inc_edge[s]
            yi = st["y"][e] if plan.inc_sign[s] > 0 else -st["y"][e]
            qv.append((np.asarray(q_fn(g, plan.inc_nbr[s]), dtype=np.float64), st["z"][e] - yi))
        qv.append((np.asarray(qc[g], dtype=np.float64), st["z"][E + k] - st["y"][E + k]))
        D, c = ons.assemble(qv, n)
        cast = lambda v: np.array(v, dtype=dtype)  # noqa: E731
        ns = ons.NodeState(cast(st["x_ext"][k]), cast(st["d"][k, 0]), cast(st["d"][k, 1]),
                           cast(st["e"][k, 0]), cast(st["e"][k, 1]))
        bg = np.asarray(b[g], dtype=np.float64).reshape(-1)
        dg = ons.node_update(A, AT @ bg, bg, D, c, qv, ns, N, params, dtype=dtype, AT=AT)
        x = ns.x.astype(np.float64)
        out["x"][k] = x
        out["d"][k, 0], out["d"][k, 1] = ns.dx, ns.dy
        out["e"][k, 0], out["e"][k, 1] = ns.ex, ns.ey
        img = float(np.sum((x - phantom) ** 2)) if phantom is not None else np.nan
        out["stats"][k] = (dg.mse_sino, dg.g_norm ** 2, dg.tv, dg.quad, img, dg.sb_res ** 2)
    return out


def _c(N, V, graph, a_per, mirror, seed=1):
    return sr.Case(N, V, graph, 2, 3, "iso", a_per, mirror, "midpoint", False, seed)


# N in {33, 64}, V in {1, 3, 8, 11}, ring / star / none, mirror on / off (None: an odd angle count)
BOUND_CASES = [
    _c(33, 1, "none", 12, "1"),
    _c(33, 3, "ring", 12, "0"),
    _c(33, 8, "star", 9, None),
    _c(33, 11, "ring", 12, "1", seed=2),  # (seed 1 misses state_ref's GMIN: test_bounds_cpu.py checks them)
    _c(64, 1, "none", 24, "0"),
    _c(64, 3, "star", 24, "1"),
    _c(64, 8, "ring", 24, "1"),
    _c(64, 11, "ring", 12, "0"),
]
BOUND_REUSE_CASES = [
    _c(33, 3, "ring", 12, "1"),
    _c(64, 8, "ring", 24, "0"),
]
UPDATE_BOUNDS = (0.0, 1.0)  # the batches' box: the x-update never reads it
