"""Setup timing of filtered back projection: event-timed
averages of the ramp filter (admm_fbp_filter) and of the plain adjoint (admm_project_adj) on the
same sinogram, one process, warm-up first, repeated launches between two events."""
import json
import os
import sys

import numpy as np
import torch

sys.path[:0] = ["distributed-inverse-problem-admm_amd", "."]
from admm_hip import ParallelBeamGeometry, RayTransform, ramp_filter  # noqa: E402
from admm_hip.fbp import fbp_scale  # noqa: E402


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


out = []
for N, angles, reps in ((512, 1536, 20), (2048, 6144, 5)):
    for dtype in ("float32", "float64"):
        geom = ParallelBeamGeometry(N, angles)
        A = RayTransform(geom, dtype, 0)
        tdt = torch.float64 if dtype == "float64" else torch.float32
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)
        sino = torch.randn((1, geom.m), generator=gen, device="cuda", dtype=tdt)
        rec = dict(N=N, angles=angles, dtype=dtype, reps=reps)
        for filt in ("ram-lak", "hann"):
            rec[f"filter_ms_{filt}"] = round(timed(lambda: ramp_filter(sino, geom, filt, fbp_scale(geom), dtype), reps), 4)
        rec["adjoint_ms"] = round(timed(lambda: A.T @ sino, reps), 4)
        rec["filter_over_adjoint"] = round(rec["filter_ms_ram-lak"] / rec["adjoint_ms"], 3)
        # useful work of the direct convolution: one float64 fma per (row, j, k)
        rec["filter_gfma_per_s"] = round(angles * N * N / rec["filter_ms_ram-lak"] / 1e6, 1)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del sino, A
        torch.cuda.empty_cache()
out_dir = os.environ.get("ADMM_OUT_DIR", "bench_out")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "time_fbp.json"), "w"), indent=1)
