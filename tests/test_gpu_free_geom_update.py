"""GPU: one x-update of a node batch on the free geometries (tests/free_geom.py) from a random,
non-smooth ADMM state against the float64 oracle -- x, d, e per pixel and the six statistics per
node, by test_gpu_state_update.py's comparison and bars (1e-9 for float64 samples; float32
samples 4 x the case's float32 yardstick).  The cases (state_ref.FREE_UPDATE_CASES) put the
solver's fused projector kernels -- k_fwdg / k_fwd_combine with their data-term epilogue, the
mirror kernels, the ungrouped k_fwd, and k_back's H epilogue -- on n_det != N, an asymmetric
detector, the full circle, odd counts, several tiles and ray chunks, and the geometry without a
grouped plan; test_state_ref_cpu.py holds the cases' conditions on the oracle alone.

Run with ``-s`` to see every case's device / yardstick ratios.
"""
import pytest
import torch

import free_geom
import state_ref as sr
from admm_hip.solver import NodeBatch
from test_gpu_state_update import _bars, _compare, _read, _set_mirror, _untouched

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", sr.FREE_UPDATE_CASES, ids=sr.case_id)
def test_update_from_random_state_on_free_geometry(cuda, monkeypatch, case, dtype):
    monkeypatch.delenv("ADMM_FWD_PLAN", raising=False)
    _set_mirror(monkeypatch, case.mirror)
    P = sr.case_problem(case, dtype)
    nb = NodeBatch(free_geom.BY_ID[case.geom], dtype, P["plan"], P["b"], P["q_fn"], sr.RHO, sr.LAM, sr.MU,
                   case.tv_iters, case.cg_iters, case.tv_kind, P["ph"], 0, fusion=case.fusion, Wi_list=P["W"],
                   derive_z=case.derive_z)
    # mirror mode where the case names it; none of the other geometries is eligible
    assert nb.mirror == (case.mirror == "1")
    grouped = bool(nb.fwd_plans())
    assert grouped == (case.geom != "nofit")  # nofit: the ungrouped forward kernel
    q0 = nb.q.clone()
    st = sr.random_state(nb, case.seed)
    nb.node_update()
    got = _read(nb)
    ref = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
    bars, yard = _bars(case, dtype, P, st, ref)
    _compare(dtype, case, dtype, got, ref, bars, yard)
    _untouched(nb, st)
    assert torch.equal(nb.q, q0)
