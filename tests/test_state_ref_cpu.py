"""CPU: keeps tests/state_ref.py honest without a GPU.

* ``consensus_ref`` reproduces the oracle's literal two-dual edge update on a random state;
* ``oracle_update`` from the zero state is the node update that
  test_gpu_fullsize.test_fullsize_single_node_update_vs_oracle compares the device with;
* the conditions under which the random-state x-update cases hold G2 and the shrink tight
  (state_ref.conditions) hold for every case of test_gpu_state_update.py and of the free-geometry
  tests (test_gpu_free_geom_update.py, test_gpu_free_geom.py), on the float64 oracle.
"""
import networkx as nx
import numpy as np
import pytest

import state_ref as sr
from admm_hip.plan import make_plan
from oracle import admm as oadmm
from oracle import node_solver as ons
from oracle.geometry import Geometry, joseph_matrix


@pytest.mark.parametrize("weighted", [False, True])
def test_consensus_ref_matches_literal_edge_update(weighted):
    V, n = 6, 50
    G = nx.cycle_graph(V)
    G.add_edge(0, 3)
    rng = np.random.default_rng(5)
    edges = oadmm.canonical_edges(G)
    x = rng.standard_normal((V, n))
    y = rng.standard_normal((len(edges), n))
    yb = rng.standard_normal((len(edges), n)) if weighted else -y
    z_old = rng.standard_normal((len(edges), n))
    W = [np.exp(rng.standard_normal(n)) for _ in range(V)]
    yd = {}
    for k, (a, b) in enumerate(edges):
        yd[(a, b, a)], yd[(a, b, b)] = y[k], yb[k]
    zl, yl = oadmm.edge_update_literal(G, list(x), yd, None, W if weighted else None)
    zn, yn, ybn, stats = sr.consensus_ref(x, y, yb if weighted else None, z_old, np.stack(W), edges,
                                          "weighted" if weighted else "midpoint")
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))  # noqa: E731
    for k, (a, b) in enumerate(edges):
        assert rel(zn[k], zl[(a, b)]) <= 1e-15
        assert rel(yn[k], yl[(a, b, a)]) <= 1e-15
        # the higher endpoint's dual: stored (weighted), or -y' up to rounding (single-y form)
        assert rel(ybn[k] if weighted else -yn[k], yl[(a, b, b)]) <= (1e-15 if weighted else 1e-14)
        want = [float(np.sum((x[a] - zl[(a, b)]) ** 2)), float(np.sum((x[b] - zl[(a, b)]) ** 2)),
                float(np.sum((zl[(a, b)] - z_old[k]) ** 2))]
        assert np.allclose(stats[k], want, rtol=1e-13, atol=0.0)


def test_oracle_update_from_zero_state_is_the_plain_node_update():
    N, a_per = 24, 24
    n = N * N
    plan = make_plan(nx.path_graph(2), 2)
    A = joseph_matrix(Geometry(N, a_per))
    b, ph = sr.sinograms(A, N, plan.local_nodes, 3, "float32")
    _, q_fn = sr.precisions(n, 2, 3)
    prm = ons.NodeParams(rho=2.0, lam=0.02, mu=0.2, tv_iters=2, cg_iters=3)
    zero = {"x_ext": np.zeros((2, n)), "d": np.zeros((2, 2, n)), "e": np.zeros((2, 2, n)),
            "y": np.zeros((1, n)), "y_b": None, "z": np.zeros((1, n)), "x_prev": None}
    got = sr.oracle_update(zero, plan, A, b, q_fn, prm, "midpoint", phantom=ph)
    q = q_fn(0, 1)
    st = ons.NodeState.zeros(n)
    dg = ons.node_update(A, A.T @ b[0], b[0], q, np.zeros(n), [(q, np.zeros(n))], st, N, prm)
    assert np.array_equal(got["x"][0], st.x) and np.any(st.x != 0.0)
    assert np.array_equal(got["d"][0, 0], st.dx) and np.array_equal(got["e"][0, 1], st.ey)
    assert got["stats"][0, 0] == dg.mse_sino and got["stats"][0, 1] == dg.g_norm ** 2
    assert got["stats"][0, 4] == float(np.sum((st.x - ph) ** 2))


def test_random_state_is_reproducible_and_keeps_x():
    plan = make_plan(nx.cycle_graph(3), 3)
    a = sr.host_state(plan, 25, 4, "weighted", False)
    b = sr.host_state(plan, 25, 4, "weighted", False, x_ext=np.ones((3, 25)))
    assert all(np.array_equal(a[k], b[k]) for k in ("d", "e", "y", "y_b", "z"))
    assert np.array_equal(b["x_ext"], np.ones((3, 25))) and a["x_prev"] is None
    c = sr.host_state(plan, 25, 5, "midpoint", True)
    assert c["z"] is None and c["y_b"] is None and not np.array_equal(c["x_ext"], a["x_ext"])


def test_update_cases_cover_every_value():
    cs = sr.UPDATE_CASES
    assert {c.N for c in cs} == {33, 47, 64, 65}
    assert {c.V for c in cs} == {1, 3, 4, 5, 8, 11}
    assert {(c.tv_iters, c.cg_iters) for c in cs} == {(1, 1), (1, 5), (2, 3), (3, 2), (4, 3), (2, 9)}
    assert {c.tv_kind for c in cs} == {"iso", "aniso"}
    assert {(c.a_per % 2, c.mirror) for c in cs} == {(0, "1"), (0, "0"), (1, None)}
    assert {(c.fusion, c.derive_z) for c in cs} == {("midpoint", True), ("midpoint", False), ("weighted", False)}
    assert {(c.graph, c.V) for c in cs} >= {("star", 5), ("path", 3), ("ring", 3), ("ring", 8)}
    assert len({sr.case_id(c) for c in cs}) == len(cs)
    assert {(c.N, c.V) for c in sr.REUSE_CASES} == {(33, 3), (33, 8), (65, 3), (65, 8)}


@pytest.mark.parametrize("case", sr.UPDATE_CASES + sr.REUSE_CASES + [sr.HALO_CASE] + sr.FREE_UPDATE_CASES + [sr.MISSED_CASE],
                         ids=sr.case_id)
def test_case_conditions_hold_on_the_oracle(case):
    """After the update min |Kx| >= 1e-3 (aniso: min(|gx|, |gy|)) wherever the differences
    exist, so G2 is far from its discontinuity, and no final u lies within 1e-6 of the shrink
    threshold."""
    P = sr.halo_problem("float64") if case is sr.HALO_CASE else sr.case_problem(case, "float64")
    st = sr.host_state(P["plan"], P["n"], case.seed, case.fusion, case.derive_z)
    up = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
    gmin, um = sr.conditions(up, case.N, case.tv_kind, sr.LAM / sr.MU)
    assert gmin >= sr.GMIN and um >= sr.UMARGIN, (gmin, um)
    if case in sr.REUSE_CASES:  # the second update, from the continued state, as well
        st2 = sr.continue_state(st, up, **sr.rerandomised(P["plan"], P["n"], case))
        up2 = sr.oracle_update(st2, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
        gmin, um = sr.conditions(up2, case.N, case.tv_kind, sr.LAM / sr.MU)
        assert gmin >= sr.GMIN and um >= sr.UMARGIN, (gmin, um)
