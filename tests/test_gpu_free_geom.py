"""GPU: the projectors and the forward plans on free geometries (tests/free_geom.py): detectors
with n_det != N, off-centre, inside or off the image, angle ranges over the full circle, limited,
starting below 0 or past pi, odd counts, a single bin, and the geometry whose row windows do not
fit the grouped forward kernel (fits = false: the ungrouped k_fwd).

* Operator path (admm_project_fwd, admm_project_adj, admm_column_norms_sq) against
  oracle.geometry.joseph_matrix of the same geometry, on the values the GPU saw, at
  test_gpu_projector.py's gates: 2e-6 (float32 samples) / 1e-12 (float64) relative Frobenius,
  2e-6 for the column norms; <Ax, y> = <x, A^T y> of the device's own results in float64
  accumulation.  The detector that misses the image gives exact zeros.
* Forward plans: a 5-node batch bound with ADMM_FWD_PLAN=0..5 runs bitwise the same two ADMM
  iterations; on the detector that misses the image every forced plan binds (the clipped plans
  have no blocks there and fall back) and the x-update is the oracle's with A = 0.
* A node's result does not depend on its batch's size (1, 2, 3, 4, 8 nodes), bitwise.
"""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

import free_geom
import state_ref as sr
from admm_hip.geometry import RayTransform
from admm_hip.plan import make_plan
from admm_hip.solver import NodeBatch
from oracle.geometry import ellipse_phantom, joseph_matrix
from test_gpu_state_update import _bars, _compare

pytestmark = pytest.mark.gpu

TOL = {"float32": 2e-6, "float64": 1e-12}  # test_gpu_projector.py's gates
DTYPES = ["float32", "float64"]
ELLIPSE = [[1.0, 0.25, 0.1, 0.45, -0.2, 30.0]]  # off-centre, rotated


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


@functools.lru_cache(maxsize=None)
def matrix(gid):
    """The float64 Joseph matrix of a free geometry, made once and left unchanged."""
    return joseph_matrix(free_geom.BY_ID[gid].oracle())


def _tdt(dtype):
    return torch.float64 if dtype == "float64" else torch.float32


# ----------------------------------------------------------------------------
# operator path
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", free_geom.GEOMS, ids=free_geom.IDS)
def test_forward_adjoint_match_oracle(cuda, g, dtype):
    A = matrix(g.id)
    op = RayTransform(g, dtype)
    assert op.shape == A.shape
    rng = np.random.default_rng(g.N * 100 + g.n_det)
    X = rng.standard_normal((3, g.n))
    X[0] = ellipse_phantom(g.N, ELLIPSE, 2).ravel()
    Yi = rng.standard_normal((2, g.m))
    Xt, Yt = torch.as_tensor(X, dtype=_tdt(dtype)), torch.as_tensor(Yi, dtype=_tdt(dtype))
    Xs, Ys = Xt.double().numpy(), Yt.double().numpy()  # the values the GPU actually saw
    Y = (op @ Xt.to(cuda)).double().cpu().numpy()
    Z = (op.T @ Yt.to(cuda)).double().cpu().numpy()
    assert Y.shape == (3, g.m) and Z.shape == (2, g.n)
    if g.id == "missed":  # no ray meets the image: exact zeros, every call ADMM_OK (no exception)
        assert A.nnz == 0 and not Y.any() and not Z.any()
        return
    ef = [rel(Y[v], A @ Xs[v]) for v in range(3)]
    ea = [rel(Z[v], A.T @ Ys[v]) for v in range(2)]
    print(f"\nOPERATOR {g.id} {dtype}: forward {max(ef):.2e} adjoint {max(ea):.2e}")
    assert max(ef) < TOL[dtype], ef
    assert max(ea) < TOL[dtype], ea
    # <A x, y> = <x, A^T y> of the device's results.  Each side is within the gate of the exact
    # product, so by Cauchy-Schwarz the two differ by at most tol (|Ax| |y| + |x| |A^T y|).
    for v in range(2):
        lhs, rhs = float(np.dot(Y[v], Ys[v])), float(np.dot(Xs[v], Z[v]))
        bound = TOL[dtype] * (np.linalg.norm(Y[v]) * np.linalg.norm(Ys[v]) + np.linalg.norm(Xs[v]) * np.linalg.norm(Z[v]))
        assert abs(lhs - rhs) <= bound, (v, lhs, rhs, bound)


@pytest.mark.parametrize("g", free_geom.GEOMS, ids=free_geom.IDS)
def test_column_norms_match_oracle(cuda, g):
    A = matrix(g.id)
    W = np.maximum(np.asarray(A.multiply(A).sum(axis=0)).ravel(), 1e-12)
    Wg = RayTransform(g).column_norms_sq()
    assert Wg.shape == (g.n,)
    print(f"\nCOLNORMS {g.id}: {rel(Wg, W):.2e}")
    assert rel(Wg, W) < 2e-6
    if g.id == "missed":
        assert np.all(Wg == 1e-12)


# ----------------------------------------------------------------------------
# forward plans and batch size
# ----------------------------------------------------------------------------
def _problem(gid, V, graph, dtype, iters=(2, 3)):
    case = sr._f(gid, V, graph, iters, None, "stored")
    return case, sr.case_problem(case, dtype)


def _bind(case, dtype, P):
    return NodeBatch(free_geom.BY_ID[case.geom], dtype, P["plan"], P["b"], P["q_fn"], sr.RHO, sr.LAM, sr.MU,
                     case.tv_iters, case.cg_iters, case.tv_kind, P["ph"], 0, fusion=case.fusion, Wi_list=P["W"],
                     derive_z=case.derive_z)


def _trajectory(nb, iters=2):
    out = []
    for _ in range(iters):
        nb.node_update()
        nb.consensus()
        torch.cuda.synchronize()
        out += [nb.x_ext.cpu().numpy().copy(), nb.node_stats.cpu().numpy().copy(), nb.edge_stats.cpu().numpy().copy(),
                nb.y.cpu().numpy().copy(), nb.z.cpu().numpy().copy()]
    return out


def _active(nb):
    return [p["plan"] for p in nb.fwd_plans() if p["active"]]


@pytest.mark.parametrize("gid,dtype,mirror", [("wide", "float32", "1"), ("wide", "float32", "0"), ("wide", "float64", "0"),
                                              ("shifted", "float32", None), ("shifted", "float64", None),
                                              ("tiles", "float32", None), ("tiles", "float64", None)])
def test_forward_plans_bitwise_equal(cuda, monkeypatch, gid, dtype, mirror):
    """As test_gpu_admm.py::test_forward_plans_bitwise_equal on the standard geometry: the plans
    only redistribute rays over blocks, every (segment, ray) partial is the same sum."""
    if mirror is None:
        monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    else:
        monkeypatch.setenv("ADMM_FWD_MIRROR", mirror)
    case, P = _problem(gid, 5, "ring", dtype)
    runs = []
    for plan in range(6):
        monkeypatch.setenv("ADMM_FWD_PLAN", str(plan))
        nb = _bind(case, dtype, P)
        assert nb.mirror == (mirror == "1")
        have = {p["plan"] for p in nb.fwd_plans()}
        assert {0, 1} <= have
        if not nb.mirror and plan in have:  # (mirror mode binds the half geometry's plan)
            assert _active(nb) == [plan]
        runs.append(_trajectory(nb))
    assert np.any(runs[0][0] != 0.0)
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_missed_detector_binds_under_every_forced_plan(cuda, monkeypatch, dtype):
    """Detector [3, 5]: the clipped plans 3-5 have groups and no blocks.  Forced, they fall back
    to the free choice instead of launching a grid of 0 blocks; A = 0, so A^T b = 0 exactly and
    the x-update is the oracle's with the zero matrix (bitwise the same under every plan)."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    case = sr.MISSED_CASE
    P = sr.case_problem(case, dtype)
    assert P["A"].nnz == 0
    outs = []
    for plan in (None, 0, 1, 2, 3, 4, 5):
        if plan is None:
            monkeypatch.delenv("ADMM_FWD_PLAN", raising=False)
        else:
            monkeypatch.setenv("ADMM_FWD_PLAN", str(plan))
        nb = _bind(case, dtype, P)
        blocks = {p["plan"]: p["blocks"] for p in nb.fwd_plans()}
        assert [blocks[p] for p in (3, 4, 5)] == [0, 0, 0]
        act = _active(nb)
        assert len(act) == 1 and blocks[act[0]] > 0
        if plan in (0, 1, 2):
            assert act == [plan]
        assert not nb.atb.cpu().numpy().any()
        st = sr.random_state(nb, case.seed)
        nb.node_update()
        torch.cuda.synchronize()
        outs.append((nb.x_ext[:nb.V].cpu().numpy().copy(), nb.d.cpu().numpy().copy(), nb.e.cpu().numpy().copy(),
                     nb.node_stats.cpu().numpy().copy()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)
    ref = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
    x, d, e, stats = outs[0]
    bars, yard = _bars(case, dtype, P, st, ref)
    # MSE_SINO = |0 - b|^2 has no float32 rounding at all here (b is read exactly), so its
    # yardstick is 0; what remains is the order of a float64 sum of m = 1024 exact squares,
    # at most m 2^-53 = 1.1e-13 relative
    bars["stats"][0] = max(bars["stats"][0], 1e-12)
    _compare(dtype + " missed", case, dtype, {"x": x, "d": d, "e": e, "stats": stats}, ref, bars, yard)
    for k in range(nb.V):  # A x = 0: the data term is |b|^2 whatever x is
        assert abs(stats[k, 0] - float(np.sum(P["b"][k] ** 2))) <= 1e-12 * stats[k, 0]


@pytest.mark.parametrize("gid,dtype,mirror", [("wide", "float32", "1"), ("wide", "float64", "1"),
                                              ("shifted", "float32", None), ("shifted", "float64", None)])
def test_result_independent_of_batch_size(cuda, monkeypatch, gid, dtype, mirror):
    """Node 0 of an edgeless graph in batches of 1, 2, 3, 4 and 8 nodes (every node-interleave
    width): bitwise the same image and statistics after two x-updates, as
    test_gpu_mirror.py::test_mirror_result_independent_of_batch_size on the standard geometry."""
    monkeypatch.delenv("ADMM_FWD_PLAN", raising=False)
    if mirror is None:
        monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    else:
        monkeypatch.setenv("ADMM_FWD_MIRROR", mirror)
    res = {}
    for V in (1, 2, 3, 4, 8):
        case, P = _problem(gid, V, "none", dtype, iters=(4, 3))
        if res:
            assert np.array_equal(P["b"][0], b0)
        b0 = P["b"][0]
        nb = _bind(case, dtype, P)
        assert nb.mirror == (mirror == "1")
        nb.node_update()
        nb.node_update()
        torch.cuda.synchronize()
        res[V] = (nb.x_ext[0].cpu().numpy().copy(), nb.node_stats[0].cpu().numpy().copy())
    assert np.any(res[1][0] != 0.0)
    for V, r in res.items():
        assert np.array_equal(r[0], res[1][0]), V
        assert np.array_equal(r[1], res[1][1]), V
