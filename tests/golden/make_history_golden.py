"""Writes tests/golden/history_parent.json: the histories that commit 9521003's host path (run_admm's
_take_metrics / _take_bounds / _take_norms / _take_fuse / _record / _flush_pipelined and
penalty.thresholds) forms from seeded synthetic statistics tables.  That commit is the last one with
those functions, so this script runs only in a checkout of it:

    git worktree add /tmp/parent 9521003
    PYTHONPATH=/tmp/parent/distributed-inverse-problem-admm_amd python tests/golden/make_history_golden.py

tests/test_history_cpu.py builds the same tables (``cases`` / ``tables`` below, which import nothing of
the package) and holds the recorder of today's run_admm to these values, bit for bit: the file keeps, per
case and history key, the values with every float as its ``float.hex()`` -- of an array-valued key their
digest (tests/history_hex.py).

Shape: V_total = 5, a 5-cycle plus the chord (0, 2) (E = 6), 3 iterations.  Cases: the 16 on / off
combinations of metrics ("psnr", "ssim"), bounds, norms and fuse, each with and without a phantom.  The
cases with norms run with a rho that changes between the iterations (as with adapt_rho) and with eps_used
/ inner-update columns as the tolerance mode fills them; the others with one rho and NaN / 1, so that
their pipelined flush -- recorded too -- must give the same histories (where the parent's flush did give
the same entries as the live histories, the file says "pipelined": "live" instead of repeating them).
"""
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np

PARENT = "9521003"
V_TOTAL, ITERS, N_PIXELS = 5, 3, 48 * 48
EDGES = [(0, 1), (0, 4), (0, 2), (1, 2), (2, 3), (3, 4)]  # canonical (min, max), 5-cycle + chord
# (no rho a power of two: a product with one is exact in any grouping and would hide a regrouped expression)
LAM_TV, RHO, RHOS_ADAPTED, TOL = 0.02, 1.7, (1.7, 3.1, 0.9), (1e-3, 1e-4)
METRICS = ("psnr", "ssim")
NODE_STATS, EDGE_STATS, BOUND_STATS, NORM_STATS, FUSE_SCALARS = 6, 3, 3, 3, 1


def cases():
    """[(name, metrics on, bounds on, norms on, fuse on, phantom given)], 32 of them."""
    return [(f"metrics{m}_bounds{b}_norms{n}_fuse{f}_phantom{p}", bool(m), bool(b), bool(n), bool(f), bool(p))
            for m, b, n, f, p in itertools.product((0, 1), repeat=5)]


def width(m, b, n, f):
    """Columns of the node table (groups.RankGroups.node_stat_width at 9521003)."""
    k = len(METRICS) if m else 0
    return NODE_STATS + k + (BOUND_STATS if b else 0) + (NORM_STATS if n else 0) + (1 + FUSE_SCALARS + k if f else 0)


def tables(index, m, b, n, f):
    """The case's per-iteration inputs [(ns, es, rho_k, eps_used, n_upd)]: squares of N(0, 1) draws; the
    fusion's scalars stand in the row of global node 0 only, as on the device."""
    rng = np.random.default_rng(1000 + index)
    w = width(m, b, n, f)
    out = []
    for k in range(ITERS):
        ns = rng.standard_normal((V_TOTAL, w)) ** 2
        es = rng.standard_normal((len(EDGES), EDGE_STATS)) ** 2
        if f:
            ns[1:, w - (FUSE_SCALARS + (len(METRICS) if m else 0)):] = 0.0
        eps_used = rng.standard_normal(V_TOTAL) ** 2 if n else np.full(V_TOTAL, np.nan)
        n_upd = np.floor(1.0 + 3.0 * rng.random(V_TOTAL)) if n else np.ones(V_TOTAL)
        out.append((ns, es, RHOS_ADAPTED[k] if n else RHO, eps_used, n_upd))
    return out


def main():
    import torch
    from admm_hip import admm
    from admm_hip.bounds import BOUND_KEYS
    from admm_hip.fuse import FUSE_KEYS
    from admm_hip.penalty import NORM_KEYS, incidences, thresholds
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from history_hex import digest_history, dump, encode

    def new_hist(m, b, n, f):  # run_admm's history dict (admm.py:269-279; no adapt_rho: the loop owns that key)
        hist = {k: [] for k in admm.HISTORY_KEYS + admm.EXTRA_KEYS}
        for name in METRICS if m else ():
            hist[f"{name}_per_node"], hist[f"{name}_mean"] = [], []
        if b:
            hist.update({k: [] for k in BOUND_KEYS})
        if n:
            hist.update({k: [] for k in NORM_KEYS})
        if f:
            hist.update({k: [] for k in FUSE_KEYS + tuple(f"fused_{x}" for x in (METRICS if m else ()))})
        return hist

    out = {"parent": PARENT, "cases": {}}
    for index, (name, m, b, n, f, p) in enumerate(cases()):
        metrics = METRICS if m else None
        ninc = incidences(EDGES, V_TOTAL, b) if n else None
        rows = tables(index, m, b, n, f)
        hist, returned = new_hist(m, b, n, f), []
        for k, (ns, es, rho_k, eps_used, n_upd) in enumerate(rows):  # the live loop, admm.py:337-354
            ns = np.concatenate([ns, np.stack([eps_used, n_upd], axis=1)], axis=1)
            ns, bres = admm._take_bounds(hist, b, admm._take_metrics(hist, metrics, ns), rho_k)
            ns, norms = admm._take_norms(n, ns)
            ns = admm._take_fuse(hist, f, metrics, ns, p)
            pn, dn = admm._record(hist, ns, es, EDGES, V_TOTAL, rho_k, LAM_TV, admm.eps_target(k), p)
            eps = None
            if n:
                ep, ed, ax, bz, aty = thresholds(TOL[0], TOL[1], N_PIXELS, ninc, norms, rho_k)
                for key, val in zip(NORM_KEYS, (ep, ed, ax, bz, aty)):
                    hist[key].append(val)
                eps = (ep, ed)
            returned.append([pn, dn, bres, eps])
        case = {"live": digest_history(hist), "returned": encode(returned)}
        if not n:
            hist = new_hist(m, b, n, f)
            flat = torch.from_numpy(np.stack([np.concatenate([ns.ravel(), es.ravel()]) for ns, es, *_ in rows]))
            rg = SimpleNamespace(node_stat_width=width(m, b, n, f),
                                 batches=[SimpleNamespace(edge_stats=torch.zeros((1, EDGE_STATS)))])
            admm._flush_pipelined(hist, flat, 0, ITERS, rg, V_TOTAL, EDGES, RHO, LAM_TV, p, False, metrics, b, f)
            case["pipelined"] = digest_history(hist)
            if case["pipelined"] == case["live"]:  # (every NaN encodes alike): stored once
                case["pipelined"] = "live"
        out["cases"][name] = case
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "history_parent.json")
    dump(out, path)
    print(f"{path}: {len(out['cases'])} cases")


if __name__ == "__main__":
    main()
