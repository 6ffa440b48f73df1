"""Cost of the Huber reweighting in the loop.

Default (``--ab``): C3 (512^2, 16-node ring, float32 samples; bench.py's constants) through run_admm
in the pipelined mode, 20 iterations, alternating all-ones ``ray_weights`` (the weighted launches, no
reweighting), ``robust=inf`` (the reweighting, weights that stay 1) and ``robust=delta`` (weights that
move), five runs each after a warm-up of all three: ms per iteration of every run and the ranges.

``--one ones|inf|delta``: one such run and nothing else, for a kernel-stats profile
(rocprofv3 --kernel-trace --stats -- python scripts/time_robust.py --one delta;
scripts/top_kernels.py lists k_huber_weights' average duration)."""
import json
import math
import sys

import networkx as nx
import numpy as np

sys.path[:0] = ["distributed-inverse-problem-admm_amd", "."]

DELTA = 0.3
FORMS = ("ones", "inf", "delta")


def setup():
    import bench
    from admm_hip.data import make_precisions, make_sinograms, shepp_logan
    from admm_hip.solver import make_operators
    cfg = bench.CONFIGS["C3"]
    N, V = cfg["N"], cfg["nodes"]
    ops = make_operators(N, V, angles_total=max(180, 3 * N), dtype=cfg["dtype"], device=0)
    ph = shepp_logan(N)
    sinos = make_sinograms(ops, ph, 0.005, seed=1000)
    Wi, Q = make_precisions(ops)
    ones = np.ones(ops[0].geom.m)

    def run(form, iters=20):
        from admm_hip.admm import run_admm
        t = {}
        kw = dict(ray_weights=ones) if form == "ones" else dict(robust=math.inf if form == "inf" else DELTA)
        run_admm(ops, sinos, nx.cycle_graph(V), Wi, Q, N, lam_tv=bench.LAM, rho=bench.RHO, max_iters=iters,
                 eps_pri=0.0, eps_dual=0.0, verbose=False, phantom_true=ph, tv_iters=bench.TV_ITERS,
                 cg_iters=bench.CG_ITERS, tv_kind=cfg["tv"], write_params=False, return_tensors=True, timing=t, **kw)
        return 1e3 * t["loop_s"] / t["iters"]
    return run


def ab(runs=5):
    run = setup()
    for f in FORMS:  # warm-up: library load, allocator, clocks
        run(f)
    ms = {f: [] for f in FORMS}
    for _ in range(runs):
        for f in FORMS:
            ms[f].append(run(f))
    rec = dict(config="C3", iters=20, delta=DELTA)
    for f in FORMS:
        rec[f + "_ms_per_iter"] = [round(v, 4) for v in ms[f]]
        rec[f + "_range_ms"] = [round(min(ms[f]), 4), round(max(ms[f]), 4)]
    med = {f: float(np.median(ms[f])) for f in FORMS}
    rec["inf_minus_ones_ms"] = round(med["inf"] - med["ones"], 4)
    rec["delta_minus_ones_ms"] = round(med["delta"] - med["ones"], 4)
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    if "--one" in sys.argv:
        which = sys.argv[sys.argv.index("--one") + 1]
        print(json.dumps({which: round(setup()(which), 4)}))
    else:
        ab()  # (prints its record as one JSON line)
