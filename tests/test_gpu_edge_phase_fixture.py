"""GPU: the edge-phase side kernels give bit for bit what tests/golden/edge_phase_parent.json holds
-- recorded on an MI355X (tests/golden/make_parent_golden.py) from the library before its
block reduction, row-sum kernel and projection body were folded into one each (csrc/common.hpp,
k_bound_project<RELAXED>).  Every float64 sum is compared as its bit pattern, every output array
by its SHA-256 digest.  The other files hold these sums to 1e-13 / 1e-11 only; here the shapes also
reach the second pass of the row-sum kernel's strided loop (more than 256 block slots per row).

Inputs come from the seeded helpers of test_gpu_bounds.py, test_gpu_relax.py and metrics_ref.py."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest
import torch

import metrics_ref as mr
from admm_hip.bounds import BoundProjector, Bounds
from admm_hip.geometry import current_stream_handle
from admm_hip.metrics import Scorer
from test_gpu_bounds import _kernel_case
from test_gpu_relax import _edge_case, _relaxed

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_phase_parent.json")
FIXTURE_NOTES = dict(
    inputs="seeded: test_gpu_bounds._kernel_case, test_gpu_relax._edge_case, metrics_ref.phantom "
           "(test_gpu_edge_phase_fixture.run_case)",
    sums="float64 bit patterns, big-endian hex, row-major")
ALPHA = 1.6
# pixels: under one block; one block + a 65-pixel tail; 257 blocks, so that thread 0 of the row-sum
# kernel takes a second slot
PIXELS = (169, 1089, 262145)
CASES = (
    [dict(entry="bound_project", n=n, nimg=v, form=f, alpha=a)
     for a in (None, ALPHA) for n in PIXELS for v in (1, 3) for f in ("scalar", "maps")]
    + [dict(entry="consensus_relaxed", n=n, graph=g, weighted=w, alpha=ALPHA, split=s)
       for n in PIXELS[1:] for g in ("ring3", "star17") for w in (False, True) for s in (False, True)]
    # N = 11: one window; 43: 3 x 2 tiles; 368: 23 x 12 = 276 tiles, more than 256
    + [dict(entry="image_metrics", N=N, nimg=2, mask=m) for N in (11, 43, 368) for m in (False, True)]
)


def case_id(c):
    return "-".join(f"{k}={v}" for k, v in c.items())


def _hex(a):
    """float64 values as their bit patterns, row-major."""
    return [struct.pack(">d", float(v)).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _project_case(n, nimg, form):
    """_kernel_case; a pixel count that is no square (its maps form is a side x side support mask)
    takes the scalar form's images with maps drawn per pixel."""
    side = int(round(n ** 0.5))
    if form == "scalar" or side * side == n:
        return _kernel_case(n, nimg, form)
    _, _, _, x, w, f = _kernel_case(n, nimg, "scalar")
    rng = np.random.default_rng([1, n, nimg])
    sup = rng.random(n) < 0.8  # hi = 0 outside the support, where lo = 0 pins the pixel
    B = Bounds(0.0, 2.0, np.where(sup, rng.uniform(-0.5, 0.2, n), -1.0), np.where(sup, 1.0, 0.0))
    assert np.all(np.less_equal(*B.arrays(n)))
    return (B, *B.arrays(n), x, w, f)


def run_case(c, dev):
    """One case through the loaded library: {"sums": [hex, ...], "sha256": {array name: digest}}."""
    if c["entry"] == "bound_project":
        B, _, _, x, w, f = _project_case(c["n"], c["nimg"], c["form"])
        pr = BoundProjector(B, c["n"], dev, c["nimg"])
        xd, wd, fd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, w, f))
        s = pr.run(xd, wd, fd, current_stream_handle(dev), alpha=c["alpha"])
        torch.cuda.synchronize()
        return dict(sums=_hex(s.cpu().numpy()), sha256=dict(w=_sha(wd.cpu().numpy()), f=_sha(fd.cpu().numpy())))
    if c["entry"] == "consensus_relaxed":
        st, E = _edge_case(c["n"], c["graph"], weighted=c["weighted"], seed=int(c["weighted"]))
        ranges = [(0, E // 2), (E // 2, E)] if c["split"] else [(0, E)]
        got = _relaxed(st, E, c["alpha"], dev, ranges)
        names = ("y", "z", "y_b") if c["weighted"] else ("y", "z")
        return dict(sums=_hex(got["edge_stats"]), sha256={k: _sha(got[k]) for k in names})
    N = c["N"]
    pairs = [mr.phantom(N, 0.05, seed=1000 * N + v) for v in range(c["nimg"])]
    i, j = np.mgrid[0:N, 0:N]
    mask = (((i - (N - 1) / 2.0) ** 2 + (j - (N - 1) / 2.0) ** 2) <= (0.45 * N) ** 2) if c["mask"] else None
    sc = Scorer(pairs[0][0], 1.0, mask, device=dev.index)
    x = torch.from_numpy(np.stack([p[1].reshape(-1) for p in pairs])).to(dev)
    return dict(sums=_hex(sc.sums(x).cpu().numpy()), sha256={})


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    return {case_id(r["case"]): r for r in doc["cases"]}


def test_fixture_holds_every_case(recorded):
    assert len(CASES) == 24 + 16 + 6
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)
    for r in recorded.values():
        assert r["sums"] and all(len(h) == 16 for h in r["sums"])


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_is_bitwise_the_parents(cuda, recorded, c):
    want = recorded[case_id(c)]
    got = run_case(c, cuda)
    assert got["sums"] == want["sums"]
    assert got["sha256"] == want["sha256"]
