"""GPU: the x-update gives bit for bit what tests/golden/x_update_parent.json holds -- recorded on
an MI355X (tests/golden/make_parent_golden.py) from the library before its element-wise kernels
(k_gather, k_transpose, k_start_reuse, k_cg_update, k_tv_update) were folded onto one thread map,
one LDS tile and one transposed store.  x, d and e are compared by their SHA-256 digests, every
node statistic as its bit pattern.  test_gpu_state_update.py holds the same updates to the oracle
within a rounding bar only; here a changed operation order in any of the kernels shows.

The states are those of test_gpu_state_update.py (its _batch and _read, state_ref.case_problem and
random_state): N = 33 .. 65 (one and two 64-wide TV tile columns), V = 1 .. 11 (ragged chunks,
work-group counts that are no multiple of 8), every (rounds, CG steps) pair of the cases up to the
ring overflow (2, 9).  Added: the full direction ring, cg_iters = kMaxCgRing = 8, and
admm_project_fwd on three images (k_transpose at the operator API's widths)."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import state_ref as sr
from admm_hip.geometry import ParallelBeamGeometry, RayTransform
from test_gpu_edge_phase_fixture import _hex, _sha, case_id
from test_gpu_state_update import DTYPES, _batch, _read

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x_update_parent.json")
FIXTURE_NOTES = dict(
    inputs="seeded: state_ref.case_problem / random_state (test_gpu_x_update_fixture.run_case)",
    sums="node_stats as float64 bit patterns, big-endian hex, row-major; x, d, e as SHA-256 of float64")
# cg_iters = 8 fills the direction ring (no state_ref case has more than 5 steps below the overflow
# at 9); compared with the recording only, so the seed needs none of state_ref's conditions
FULL_RING = sr.Case(33, 3, "ring", 2, 8, "iso", 12, "1", "midpoint", False, 1)
BY_ID = {sr.case_id(c): c for c in sr.UPDATE_CASES + sr.REUSE_CASES + [FULL_RING]}
PROJECT = dict(N=33, a_per=12, nimg=3)
CASES = (
    [dict(entry="update", case=sr.case_id(c), dtype=t) for c in sr.UPDATE_CASES + [FULL_RING] for t in DTYPES]
    + [dict(entry="reuse", case=sr.case_id(c), dtype=t) for c in sr.REUSE_CASES for t in DTYPES]
    + [dict(entry="project_fwd", **PROJECT, dtype=t) for t in DTYPES]
)


@contextlib.contextmanager
def _mirror(mode):
    """ADMM_FWD_MIRROR as the case wants it (None: unset), restored afterwards."""
    old = os.environ.pop("ADMM_FWD_MIRROR", None)
    if mode is not None:
        os.environ["ADMM_FWD_MIRROR"] = mode
    try:
        yield
    finally:
        os.environ.pop("ADMM_FWD_MIRROR", None)
        if old is not None:
            os.environ["ADMM_FWD_MIRROR"] = old


def run_case(c, dev):
    """One case through the loaded library: {"sums": [hex, ...], "sha256": {array name: digest}}."""
    if c["entry"] == "project_fwd":
        with _mirror(None):
            A = RayTransform(ParallelBeamGeometry(c["N"], c["a_per"]), c["dtype"], dev.index)
            x = np.random.default_rng([7, c["N"], c["nimg"]]).standard_normal((c["nimg"], c["N"] * c["N"]))
            y = A.apply(torch.from_numpy(x).to(dev))
            torch.cuda.synchronize()
        return dict(sums=[], sha256=dict(sino=_sha(y.cpu().numpy())))
    case = BY_ID[c["case"]]
    with _mirror(case.mirror):
        P = sr.case_problem(case, c["dtype"])
        nb = _batch(case, c["dtype"], P, keep_x=c["entry"] == "reuse")
        sr.random_state(nb, case.seed)
        nb.node_update()
        if c["entry"] == "reuse":  # the second update starts from the first one's A^T (A x - b)
            sr.random_state(nb, case.seed + 1000, keep_x=True)
            nb.node_update()
        got = _read(nb)
    return dict(sums=_hex(got["stats"]), sha256={k: _sha(got[k]) for k in ("x", "d", "e")})


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    return {case_id(r["case"]): r for r in doc["cases"]}


def test_fixture_holds_every_case(recorded):
    assert len(sr.UPDATE_CASES) == 21 and len(sr.REUSE_CASES) == 4
    assert len(CASES) == 2 * (21 + 1) + 2 * 4 + 2 == 54
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)
    for r in recorded.values():
        if r["case"]["entry"] == "project_fwd":
            assert sorted(r["sha256"]) == ["sino"]
        else:
            assert len(r["sums"]) == 6 * BY_ID[r["case"]["case"]].V and all(len(h) == 16 for h in r["sums"])
            assert sorted(r["sha256"]) == ["d", "e", "x"]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_is_bitwise_the_parents(cuda, recorded, c):
    want = recorded[case_id(c)]
    got = run_case(c, cuda)
    assert got["sums"] == want["sums"]
    assert got["sha256"] == want["sha256"]
