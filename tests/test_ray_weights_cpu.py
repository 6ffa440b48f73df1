"""CPU: the per-ray weights of the data term (1/2 sum_r w_r (A x - b)_r^2) without a GPU.

* the library exports the two new entry points, ABI 9 as before;
* tests/weights_ref.py: the duck-typed adjoint and the row-scaled matrix pose the same problem, and
  with w = 1 both are bitwise state_ref.oracle_update;
* the conditions of the weighted x-update cases of test_gpu_a_ray_weights.py hold on the oracle;
* ``admm_hip.data.transmission_data``;
* argument errors raise before any device work.
"""
import inspect
import math

import networkx as nx
import numpy as np
import pytest
import torch

import state_ref as sr
import weights_ref as wr
from admm_hip import _lib
from admm_hip.geometry import ParallelBeamGeometry, RayTransform
from admm_hip.plan import make_plan
from oracle.geometry import Geometry, joseph_matrix


def test_library_exports_the_weight_entry_points():
    lib = _lib.load()
    for name in ("admm_batch_set_ray_weights", "admm_column_norms_sq_weighted"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert lib.admm_abi_version() == _lib.ABI_VERSION == 9
    # no context: rejected before any HIP call
    assert lib.admm_batch_set_ray_weights(None, None, None) == -3
    assert lib.admm_column_norms_sq_weighted(None, None, None, None) == -1


def _one_node(seed=2):
    N, a_per = 33, 12
    case = sr.Case(N, 1, "none", 2, 3, "iso", a_per, None, "midpoint", False, seed)
    P = wr.case_problem(case, "float64")
    st = sr.host_state(P["plan"], P["n"], seed)
    return case, P, st


def test_duck_typed_and_row_scaled_references_agree():
    case, P, st = _one_node()
    w = P["w"]
    assert np.mean(w[0] == 0.0) > 0.1 and w[0].max() > 1.5
    a = wr.oracle_update_weighted(st, P["plan"], P["A"], P["b"], w, P["q_fn"], P["prm"], "midpoint", phantom=P["ph"])
    b = wr.oracle_update_row_scaled(st, P["plan"], P["A"], P["b"], {0: np.sqrt(w[0])}, P["q_fn"], P["prm"],
                                    "midpoint", phantom=P["ph"])
    gmin, um = sr.conditions(a, case.N, "iso", sr.LAM / sr.MU)
    assert gmin >= sr.GMIN and um >= sr.UMARGIN, (gmin, um)
    for k in ("x", "d", "e"):
        assert sr.field_err(a[k], b[k])[0] <= 1e-12, (k, sr.field_err(a[k], b[k]))
    assert sr.stat_err(a["stats"], b["stats"]).max() <= 1e-12, sr.stat_err(a["stats"], b["stats"])
    # the weights matter: the unweighted update is another one
    plain = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], "midpoint", phantom=P["ph"])
    assert sr.field_err(a["x"], plain["x"])[0] > 1e-3


def test_unit_weights_are_bitwise_the_plain_oracle():
    case, P, st = _one_node()
    m = P["A"].shape[0]
    plain = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], "midpoint", phantom=P["ph"])
    one = {0: np.ones(m)}
    for dtype in (np.float64, np.float32):
        A = P["A"] if dtype == np.float64 else sr.as_f32_matrix(P["A"])
        # (float32 samples: sinograms that are float32 numbers, as state_ref.sinograms makes them)
        b = {g: v.astype(dtype).astype(np.float64) for g, v in P["b"].items()}
        ref = sr.oracle_update(st, P["plan"], A, b, P["q_fn"], P["prm"], "midpoint", dtype=dtype, phantom=P["ph"])
        a = wr.oracle_update_weighted(st, P["plan"], A, b, one, P["q_fn"], P["prm"], "midpoint", dtype=dtype,
                                      phantom=P["ph"])
        for k in ("x", "d", "e"):
            assert np.array_equal(a[k], ref[k]), (dtype, k)
        assert np.array_equal(a["stats"][:, 1:], ref["stats"][:, 1:])
        # (MSE_SINO: the same sum, np.dot of (1, s * s) against np.dot of (s, s))
        assert np.allclose(a["stats"][:, 0], ref["stats"][:, 0], rtol=1e-14, atol=0.0)
    b = wr.oracle_update_row_scaled(st, P["plan"], P["A"], P["b"], one, P["q_fn"], P["prm"], "midpoint",
                                    phantom=P["ph"])
    for k in ("x", "d", "e", "stats"):
        assert np.array_equal(b[k], plain[k]), k


def test_row_scaling_is_exact_for_the_whole_run_weights():
    s = wr.s_weights(6, 16, [0, 1], 3)
    assert set(np.unique(np.concatenate([s[0], s[1]]))) == set(wr.S_VALUES) and not np.array_equal(s[0], s[1])
    w32 = (s[0] * s[0]).astype(np.float32)
    assert np.array_equal(np.sqrt(w32.astype(np.float64)), s[0])
    A = joseph_matrix(Geometry(16, 6))
    A2, b2 = wr.row_scaled(A, np.ones(A.shape[0]), s[0])
    assert np.array_equal(A2.indices, A.indices) and np.array_equal(b2, s[0])
    assert np.array_equal(np.asarray(A2.sum(axis=1)).ravel() == 0.0, s[0] == 0.0)


def test_weighted_cases_cover_every_value():
    cs = wr.WEIGHT_CASES
    assert {c.N for c in cs} == {33, 64} and {c.V for c in cs} == {1, 3, 5, 8, 11}
    assert {(c.N, c.V) for c in cs} >= {(33, 11), (64, 11), (33, 8), (64, 8)}
    assert {(c.tv_iters, c.cg_iters) for c in cs} == {(1, 1), (2, 3)}
    assert {c.tv_kind for c in cs} == {"iso", "aniso"}
    assert {(c.a_per % 2, c.mirror) for c in cs} == {(0, "1"), (0, "0"), (1, None)}
    assert len({sr.case_id(c) for c in cs}) == len(cs)
    w = wr.ray_weights(12, 33, [0, 1], 1, "float32")
    for g in (0, 1):
        wg = w[g].reshape(12, 33)
        assert wg.min() == 0.0 and 1.9 < wg.max() <= 2.0 and 0.1 < np.mean(wg == 0.0) < 0.3
        assert np.any(np.all(wg == 0.0, axis=1)) and np.any(np.all(wg == 0.0, axis=0))
        assert np.array_equal(wg, wg.astype(np.float32))
    assert not np.array_equal(w[0], w[1])


@pytest.mark.parametrize("case,dwf,reuse",
                         [(c, 1.0, False) for c in wr.WEIGHT_CASES] + [(c, 1.0, True) for c in wr.WEIGHT_REUSE_CASES]
                         + [(wr.KFWD_CASE, wr.KFWD_DWF, False)],
                         ids=lambda v: sr.case_id(v) if isinstance(v, sr.Case) else str(v))
def test_weighted_case_conditions_hold_on_the_oracle(case, dwf, reuse):
    """min |Kx| >= 1e-3 and no final u within 1e-6 of the shrink threshold (state_ref.conditions),
    so G2 and the shrink are far from their discontinuities at the weighted cases' seeds."""
    P = wr.case_problem(case, "float64", dwf)
    run = lambda s: wr.oracle_update_weighted(s, P["plan"], P["A"], P["b"], P["w"], P["q_fn"], P["prm"],  # noqa: E731
                                              case.fusion, phantom=P["ph"])
    st = sr.host_state(P["plan"], P["n"], case.seed, case.fusion, case.derive_z)
    up = run(st)
    gmin, um = sr.conditions(up, case.N, case.tv_kind, sr.LAM / sr.MU)
    assert gmin >= sr.GMIN and um >= sr.UMARGIN, (gmin, um)
    if reuse:
        up2 = run(sr.continue_state(st, up, **sr.rerandomised(P["plan"], P["n"], case)))
        gmin, um = sr.conditions(up2, case.N, case.tv_kind, sr.LAM / sr.MU)
        assert gmin >= sr.GMIN and um >= sr.UMARGIN, (gmin, um)


# --------------------------------------------------------------------------------------
# transmission data
# --------------------------------------------------------------------------------------
def test_transmission_data():
    from admm_hip.data import transmission_data
    I0, val = 50.0, 1.5
    sino = torch.full((400, 250), val, dtype=torch.float64)
    out = []
    for _ in range(2):
        g = torch.Generator()
        g.manual_seed(7)
        out.append(transmission_data(sino, I0, generator=g))
    (b, w), (b2, w2) = out
    assert torch.equal(b, b2) and torch.equal(w, w2)  # seeded: repeatable
    g = torch.Generator()
    g.manual_seed(8)
    assert not torch.equal(transmission_data(sino, I0, generator=g)[1], w)
    assert b.shape == sino.shape and w.shape == sino.shape and b.dtype == sino.dtype
    assert bool(torch.all(w >= 0)) and bool(torch.all(torch.isfinite(w)))
    # counts / I0 ~ Poisson(lam) / I0, lam = I0 exp(-val): mean exp(-val), variance exp(-val) / I0
    n = w.numel()
    mean, se = math.exp(-val), (math.exp(-val) / I0 / n) ** 0.5
    assert abs(float(w.mean()) - mean) <= 5.0 * se, (float(w.mean()), mean, se)
    counts = w * I0
    assert bool(torch.all(torch.abs(counts - torch.round(counts)) < 1e-9))
    # rays that counted nothing: w = 0 and b = log(I0), finite
    dark = torch.full((2000,), 9.0, dtype=torch.float32)
    g.manual_seed(9)
    bd, wd = transmission_data(dark, 20.0, generator=g)
    assert bd.dtype == torch.float32 and int((wd == 0).sum()) > 1000
    assert bool(torch.all(torch.isfinite(bd)))
    assert bool(torch.all(bd[wd == 0] == torch.log(torch.tensor(20.0))))
    with pytest.raises(ValueError):
        transmission_data(dark, 0.0)


# --------------------------------------------------------------------------------------
# argument errors, before any device work (this process has no GPU)
# --------------------------------------------------------------------------------------
N_, A_ = 16, 6
M_ = N_ * A_


def _bad_weights():
    neg = np.ones(M_)
    neg[5] = -1e-3
    nan = np.ones(M_)
    nan[7] = np.nan
    inf = np.ones((A_, N_))
    inf[1, 2] = np.inf
    return [("negative", neg, ">= 0"), ("nan", nan, "finite"), ("inf", inf, "finite"),
            ("length", np.ones(M_ + 1), "entries"), ("tensor", -torch.ones(M_), ">= 0")]


@pytest.mark.parametrize("name,w,msg", _bad_weights(), ids=[b[0] for b in _bad_weights()])
def test_bad_weights_raise_before_device_work(name, w, msg):
    from admm_hip.admm import run_admm
    from admm_hip.data import make_precisions
    from admm_hip.solver import NodeBatch
    from block_5_node_problem import build_node_problem
    from block_6_admm_loop_ver2 import decentralized_admm
    ops = [RayTransform(ParallelBeamGeometry(N_, A_), "float32", 0) for _ in range(2)]
    sin = [np.zeros(M_)] * 2
    G = nx.path_graph(2)
    W = [np.ones(N_ * N_)] * 2
    q = lambda i, j: np.ones(N_ * N_)  # noqa: E731
    with pytest.raises(ValueError, match=msg):
        run_admm(ops, sin, G, W, q, N_, ray_weights=w, verbose=False, write_params=False)
    with pytest.raises(ValueError, match=msg):
        decentralized_admm(ops, sin, G, W, q, N_, ray_weights=[None, w], verbose=False, write_params=False)
    with pytest.raises(ValueError, match=msg):
        NodeBatch(ops[0].geom, "float32", make_plan(G, 2), sin, q, 1.0, 0.1, 1.0, ray_weights=[w, None])
    with pytest.raises(ValueError, match=msg):
        make_precisions(ops, ray_weights=w)
    with pytest.raises(ValueError, match=msg):
        ops[0].column_norms_sq(ray_weights=w)
    with pytest.raises(ValueError, match=msg):
        build_node_problem(ops[0], sin[0], 1.0, [np.zeros(N_ * N_)], N_, 0.1, [np.ones(N_ * N_)], ray_weights=w)


def test_matrix_operators_reject_weights_before_device_work():
    from admm_hip.admm import run_admm
    from admm_hip.data import make_precisions
    from admm_hip.matrix import MatrixOperator
    from block_5_node_problem import build_node_problem
    A = joseph_matrix(Geometry(N_, A_))
    w = np.ones(M_)
    G = nx.path_graph(2)
    q = lambda i, j: np.ones(N_ * N_)  # noqa: E731
    with pytest.raises(ValueError, match="sqrt"):
        run_admm([A, A], [np.zeros(M_)] * 2, G, [np.ones(N_ * N_)] * 2, q, N_, ray_weights=w, verbose=False,
                 write_params=False)
    op = MatrixOperator(A, N_, "float32", 0)
    with pytest.raises(ValueError, match="sqrt"):
        op.column_norms_sq(ray_weights=w)
    with pytest.raises(ValueError, match="sqrt"):
        make_precisions([op], ray_weights=w)
    with pytest.raises(ValueError, match="sqrt"):
        build_node_problem(op, np.zeros(M_), 1.0, [np.zeros(N_ * N_)], N_, 0.1, [np.ones(N_ * N_)], ray_weights=w)


def test_ray_weights_keyword_is_trailing_and_defaults_to_none():
    import block_5_node_problem
    import block_6_admm_loop
    import block_6_admm_loop_ver2
    from admm_hip.admm import run_admm
    from admm_hip.data import make_precisions
    from admm_hip.groups import RankGroups
    from admm_hip.solver import NodeBatch
    for fn in (block_5_node_problem.build_node_problem, block_6_admm_loop.decentralized_admm,
               block_6_admm_loop_ver2.decentralized_admm, run_admm, make_precisions, RankGroups.__init__,
               NodeBatch.__init__, RayTransform.column_norms_sq):
        prm = inspect.signature(fn).parameters
        assert list(prm)[-1] == "ray_weights" and prm["ray_weights"].default is None, fn


def test_node_ray_weights_forms():
    from admm_hip.solver import node_ray_weights
    w = np.linspace(0.0, 2.0, M_)
    assert node_ray_weights(None, [0, 1], M_) is None
    assert node_ray_weights([None, None], [0, 1], M_) is None
    one = node_ray_weights(w.reshape(A_, N_), [3, 4], M_)  # one array: every node
    assert set(one) == {3, 4} and np.array_equal(one[3], w) and one[3].dtype == np.float64
    per = node_ray_weights([None, torch.as_tensor(w), 2 * w], [1, 2], M_)
    assert set(per) == {1, 2} and np.array_equal(per[2], 2 * w)
    assert set(node_ray_weights([w, None, None], [0, 1, 2], M_)) == {0}
    assert node_ray_weights([w, None, None], [1, 2], M_) is None  # this batch's nodes have none
