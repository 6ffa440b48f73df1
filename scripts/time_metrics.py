"""Cost of the image metrics.

Default: event-timed averages of one admm_image_metrics call (both launches) at 512^2 x 16 and
2048^2 x 8, one process, warm-up first, repeated launches between two events, with the achieved
bytes/s against the compulsory bytes 8 n (nimg + 1) (every image and the reference read once).

``--ab``: C3 (512^2, 16-node ring, float32 samples; bench.py's constants) through run_admm in the
pipelined mode, alternating metrics off / on, five runs each: ms per iteration of every run, the
mean overhead and the off-runs' own spread."""
import json
import os
import sys

import networkx as nx
import numpy as np
import torch

sys.path[:0] = ["distributed-inverse-problem-admm_amd", "."]
from admm_hip.metrics import Scorer  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def kernel_times():
    out = []
    for N, nimg, reps in ((512, 16, 50), (2048, 8, 20)):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)
        ref = torch.rand((N * N,), generator=gen, device="cuda", dtype=torch.float64)
        x = ref + 0.05 * torch.randn((nimg, N * N), generator=gen, device="cuda", dtype=torch.float64)
        sc = Scorer(ref, 1.0, None, device=0, max_images=nimg)
        ms = timed(lambda: sc.sums(x), reps)
        compulsory = 8 * N * N * (nimg + 1)
        rec = dict(N=N, nimg=nimg, reps=reps, metrics_ms=round(ms, 4), compulsory_bytes=compulsory,
                   achieved_gb_per_s=round(compulsory / ms / 1e6, 1))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del x, ref, sc
        torch.cuda.empty_cache()
    return out


def ab(iters=20, runs=5):
    import bench
    from admm_hip.admm import run_admm
    from admm_hip.data import make_precisions, make_sinograms, shepp_logan
    from admm_hip.solver import make_operators
    cfg = bench.CONFIGS["C3"]
    N, V = cfg["N"], cfg["nodes"]
    ops = make_operators(N, V, angles_total=max(180, 3 * N), dtype=cfg["dtype"], device=0)
    ph = shepp_logan(N)
    sinos = make_sinograms(ops, ph, 0.005, seed=1000)
    Wi, Q = make_precisions(ops)
    G = nx.cycle_graph(V)

    def run(metrics):
        t = {}
        run_admm(ops, sinos, G, Wi, Q, N, lam_tv=bench.LAM, rho=bench.RHO, max_iters=iters, eps_pri=0.0, eps_dual=0.0,
                 verbose=False, phantom_true=ph, tv_iters=bench.TV_ITERS, cg_iters=bench.CG_ITERS, tv_kind=cfg["tv"],
                 write_params=False, return_tensors=True, timing=t, metrics=metrics)
        return 1e3 * t["loop_s"] / t["iters"]

    run(None)  # warm-up: library load, allocator, clocks
    run(("psnr", "ssim"))
    off, on = [], []
    for _ in range(runs):
        off.append(run(None))
        on.append(run(("psnr", "ssim")))
    rec = dict(config="C3", iters=iters, off_ms_per_iter=[round(v, 4) for v in off],
               on_ms_per_iter=[round(v, 4) for v in on], overhead_ms=round(float(np.mean(on) - np.mean(off)), 4),
               off_spread_ms=round(float(max(off) - min(off)), 4))
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    res = dict(ab=ab()) if "--ab" in sys.argv else dict(kernel=kernel_times())
    out_dir = os.environ.get("ADMM_OUT_DIR", "bench_out")
    os.makedirs(out_dir, exist_ok=True)
    name = "time_metrics_ab.json" if "--ab" in sys.argv else "time_metrics.json"
    json.dump(res, open(os.path.join(out_dir, name), "w"), indent=1)
