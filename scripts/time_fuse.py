"""Cost of the network-fused image and the consensus error.

Default (``--ab``): C3 (512^2, 16-node ring, float32 samples; bench.py's constants) through
run_admm in the pipelined mode, alternating ``fuse=None`` and ``fuse="precision"``, five runs each
after a warm-up of both: ms per iteration of every run, the mean overhead and the fuse=None runs'
own spread.  The fused run streams x three times and W twice per iteration (admm_fuse_absmax,
admm_fuse_accumulate, admm_fuse_finish, admm_fuse_deviation twice) and widens the node table by three
columns.

``--one off|on``: one such run and nothing else, for a kernel-stats profile of either form
(rocprofv3 --kernel-trace --stats -- python scripts/time_fuse.py --one on; scripts/top_kernels.py
lists the k_fuse_* kernels next to k_bound_project's figure of section 6.9)."""
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

    def run(fused, iters=20):
        from admm_hip.admm import run_admm
        t = {}
        run_admm(ops, sinos, nx.cycle_graph(V), Wi, Q, N, lam_tv=bench.LAM, rho=bench.RHO, max_iters=iters,
                 eps_pri=0.0, eps_dual=0.0, verbose=False, phantom_true=ph, tv_iters=bench.TV_ITERS,
                 cg_iters=bench.CG_ITERS, tv_kind=cfg["tv"], write_params=False, return_tensors=True, timing=t,
                 fuse="precision" if fused else None)
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
    rec = dict(config="C3", iters=20, off_ms_per_iter=[round(v, 4) for v in off],
               fuse_ms_per_iter=[round(v, 4) for v in on],
               overhead_ms=round(float(np.mean(on) - np.mean(off)), 4),
               overhead_pct=round(100.0 * float(np.mean(on) / np.mean(off) - 1.0), 2),
               off_spread_ms=round(float(max(off) - min(off)), 4))
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    if "--one" in sys.argv:
        which = sys.argv[sys.argv.index("--one") + 1]
        print(json.dumps({which: round(setup()(which == "on"), 4)}))
    else:
        ab()  # (prints its record as one JSON line)
