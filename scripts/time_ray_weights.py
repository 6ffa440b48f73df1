"""Cost of the per-ray weights in the x-update.

Default (``--ab``): C3 (512^2, 16-node ring, float32 samples; bench.py's constants) through
run_admm in the pipelined mode, alternating ``ray_weights=None`` and all-ones weights (the same
arithmetic results, the weighted launches), five runs each after a warm-up of both: ms per
iteration of every run, the mean overhead and the unweighted runs' own spread.

``--one plain|weighted``: one such run and nothing else, for a kernel-stats profile of either
form (rocprofv3 --kernel-trace --stats -- python scripts/time_ray_weights.py --one weighted;
scripts/top_kernels.py lists k_fwd_combine_mirror's average duration)."""
import json
import sys

import networkx as nx
import numpy as np

sys.path[:0] = ["distributed-inverse-problem-admm_amd", "."]


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

    def run(weighted, iters=20):
        from admm_hip.admm import run_admm
        t = {}
        run_admm(ops, sinos, nx.cycle_graph(V), Wi, Q, N, lam_tv=bench.LAM, rho=bench.RHO, max_iters=iters,
                 eps_pri=0.0, eps_dual=0.0, verbose=False, phantom_true=ph, tv_iters=bench.TV_ITERS,
                 cg_iters=bench.CG_ITERS, tv_kind=cfg["tv"], write_params=False, return_tensors=True, timing=t,
                 ray_weights=ones if weighted else None)
        return 1e3 * t["loop_s"] / t["iters"]
    return run


def ab(runs=5):
    run = setup()
    run(False)  # warm-up: library load, allocator, clocks
    run(True)
    off, on = [], []
    for _ in range(runs):
        off.append(run(False))
        on.append(run(True))
    rec = dict(config="C3", iters=20, plain_ms_per_iter=[round(v, 4) for v in off],
               unit_weights_ms_per_iter=[round(v, 4) for v in on],
               overhead_ms=round(float(np.mean(on) - np.mean(off)), 4),
               overhead_pct=round(100.0 * float(np.mean(on) / np.mean(off) - 1.0), 2),
               plain_spread_ms=round(float(max(off) - min(off)), 4))
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    if "--one" in sys.argv:
        which = sys.argv[sys.argv.index("--one") + 1]
        print(json.dumps({which: round(setup()(which == "weighted"), 4)}))
    else:
        ab()  # (prints its record as one JSON line)
