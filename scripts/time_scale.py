"""Cost of the self-scaling Huber threshold in the loop.

Default (``--ab``): C3 (512^2, 16-node ring, float32 samples; bench.py's constants) through run_admm
in the pipelined mode, 20 iterations, alternating ``robust=0.3`` (the hand-given threshold) and
``robust={"scale": 4.0}`` (the threshold from each node's median |residual|: one admm_ray_quantile launch
more per iteration, the Huber kernel reading it from the device), five runs each after a warm-up of
both: ms per iteration of every run, the ranges and the medians' difference.

``--one delta|scale``: one such run and nothing else, for a kernel-stats profile
(rocprofv3 --kernel-trace --stats -- python scripts/time_scale.py --one scale;
k_ray_quantile's average duration is the figure of section 6.14)."""
import json
import sys

import networkx as nx
import numpy as np

sys.path[:0] = ["distributed-inverse-problem-admm_amd", "."]

DELTA = 0.3
SCALE = 4.0
FORMS = ("delta", "scale")


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

    def run(form, iters=20, hist=None):
        from admm_hip.admm import run_admm
        t = {}
        robust = DELTA if form == "delta" else {"scale": SCALE}
        _, h = run_admm(ops, sinos, nx.cycle_graph(V), Wi, Q, N, lam_tv=bench.LAM, rho=bench.RHO, max_iters=iters,
                        eps_pri=0.0, eps_dual=0.0, verbose=False, phantom_true=ph, tv_iters=bench.TV_ITERS,
                        cg_iters=bench.CG_ITERS, tv_kind=cfg["tv"], write_params=False, return_tensors=True,
                        timing=t, robust=robust)
        if hist is not None:
            hist.update(h)
        return 1e3 * t["loop_s"] / t["iters"]
    return run


def ab(runs=5):
    run = setup()
    h = {}
    for f in FORMS:  # warm-up: library load, allocator, clocks
        run(f, hist=h if f == "scale" else None)
    ms = {f: [] for f in FORMS}
    for _ in range(runs):
        for f in FORMS:
            ms[f].append(run(f))
    rec = dict(config="C3", iters=20, delta=DELTA, scale=SCALE)
    for f in FORMS:
        rec[f + "_ms_per_iter"] = [round(v, 4) for v in ms[f]]
        rec[f + "_range_ms"] = [round(min(ms[f]), 4), round(max(ms[f]), 4)]
        rec[f + "_median_ms"] = round(float(np.median(ms[f])), 4)
    rec["scale_minus_delta_ms"] = round(rec["scale_median_ms"] - rec["delta_median_ms"], 4)
    d = np.stack(h["robust_delta_per_node"])  # what the rule chose on this data
    rec["delta_chosen_first_last"] = [[round(float(d[i].min()), 5), round(float(d[i].max()), 5)] for i in (0, -1)]
    rec["outliers_last"] = h["robust_outliers_total"][-1]
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    if "--one" in sys.argv:
        which = sys.argv[sys.argv.index("--one") + 1]
        print(json.dumps({which: round(setup()(which), 4)}))
    else:
        ab()  # (prints its record as one JSON line)
