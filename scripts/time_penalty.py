"""Cost of residual balancing and of the scale-free stop test.

C3 (512^2, 16-node ring, float32 samples; bench.py's constants) through run_admm:

* the norms launch pair (k_node_norms + k_row_sums<3>) of the rank's one batch: device events around
  ``--reps`` back-to-back calls, us per call and the achieved B/s for the 8 (1 + 2 deg) = 40 B per
  pixel-node the kernel requests on the ring;
* one ``RankGroups.set_rho`` call (host clock around the synchronous call, rho doubled and halved in
  turn so that the state ends where it began), set against one ADMM iteration of the same run;
* ms per iteration of alternating runs without the keywords (pipelined), with eps_abs / eps_rel
  (per-iteration read-back + the norms) and with adapt_rho too, after a warm-up of each.

``--one norms``: one run with the tolerances on and nothing else, for a kernel-stats profile
(rocprofv3 --kernel-trace --stats -- python scripts/time_penalty.py --one norms; scripts/top_kernels.py
lists k_node_norms)."""
import json
import sys
import time

import networkx as nx
import numpy as np

sys.path[:0] = ["distributed-inverse-problem-admm_amd", "."]

TOLS = dict(eps_abs=1e-12, eps_rel=1e-12)  # on, and never met: every run does all its iterations


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

    def run(iters=20, inspect=None, **kw):
        from admm_hip.admm import run_admm
        t = {}
        run_admm(ops, sinos, nx.cycle_graph(V), Wi, Q, N, lam_tv=bench.LAM, rho=bench.RHO, max_iters=iters,
                 eps_pri=0.0, eps_dual=0.0, verbose=False, phantom_true=ph, tv_iters=bench.TV_ITERS,
                 cg_iters=bench.CG_ITERS, tv_kind=cfg["tv"], write_params=False, return_tensors=True, timing=t,
                 inspect=inspect, **kw)
        return 1e3 * t["loop_s"] / t["iters"]
    return run, N * N, V, bench.RHO


def probe(rg, reps, rho, out):
    """Inside a finished run with the tolerances on: the norms pair and set_rho on its device state."""
    import torch
    torch.cuda.synchronize()
    for _ in range(5):
        rg.node_norms()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        rg.node_norms()
    ev1.record()
    torch.cuda.synchronize()
    out["norms_us"] = 1e3 * ev0.elapsed_time(ev1) / reps
    calls = []
    for new in (2.0 * rho, rho, 2.0 * rho, rho, 0.5 * rho, rho):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rg.set_rho(new)
        torch.cuda.synchronize()
        calls.append(1e3 * (time.perf_counter() - t0))
    out["set_rho_ms"] = calls


def main(reps=200, runs=3):
    run, n, V, rho = setup()
    out = {}
    with_tols = run(inspect=lambda rg: probe(rg, reps, rho, out), **TOLS)
    off, tol, both = [], [], []
    run()
    run(adapt_rho=True, **TOLS)
    for _ in range(runs):
        off.append(run())
        tol.append(run(**TOLS))
        both.append(run(adapt_rho=True, **TOLS))
    nbytes = 40.0 * n * V
    rec = dict(config="C3", iters=20, reps=reps, norms_pair_us=round(out["norms_us"], 2),
               norms_bytes=int(nbytes), norms_GBps=round(nbytes / (out["norms_us"] * 1e-6) / 1e9, 1),
               set_rho_ms=[round(v, 3) for v in out["set_rho_ms"]], iter_ms_same_run=round(with_tols, 4),
               off_ms_per_iter=[round(v, 4) for v in off], tolerances_ms_per_iter=[round(v, 4) for v in tol],
               adaptive_ms_per_iter=[round(v, 4) for v in both],
               tolerances_overhead_ms=round(float(np.mean(tol) - np.mean(off)), 4),
               adaptive_overhead_ms=round(float(np.mean(both) - np.mean(off)), 4),
               off_spread_ms=round(float(max(off) - min(off)), 4))
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    if "--one" in sys.argv:
        print(json.dumps({"norms": round(setup()[0](**TOLS), 4)}))
    else:
        reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 200
        main(reps)
