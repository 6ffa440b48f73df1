"""GPU: one consensus of a node batch from a random state against state_ref.consensus_ref.

Every consensus kernel -- k_consensus<false> (stored z), k_consensus<true> (weighted),
k_consensus_derived<16 / 64 / 128> and k_consensus_derived_direct at the x_ext row counts on
either side of each boundary, admm_consensus_range -- with z, y (y_b, x_prev) per pixel and
RA2, RB2, DZ2 per edge.  Midpoint results are bitwise (no operation of theirs can be contracted
or reordered), weighted ones within 2 ulp, the statistics within 1e-13 of the math.fsum value
(a fixed-order float64 tree over <= 1369 terms stays hundreds of ulp inside that).
N = 13 and 37: 169 and 1369 pixels, multiples of neither 64 nor 1024; 2 angles per node (the
projector is not run).
"""
import networkx as nx
import numpy as np
import pytest
import torch

import state_ref as sr
from admm_hip.geometry import ParallelBeamGeometry
from admm_hip.plan import make_plan
from admm_hip.solver import NodeBatch

pytestmark = pytest.mark.gpu

A_PER = 2
SIZES = [13, 37]
STAT_BAR = 1e-13


def _batch(N, plan, V_total, fusion="midpoint", derive_z=False, seed=1):
    n = N * N
    rng = np.random.default_rng([seed, 5])
    b = {g: rng.standard_normal(A_PER * N) for g in plan.local_nodes}
    W, q_fn = sr.precisions(n, V_total, seed)
    nb = NodeBatch(ParallelBeamGeometry(N, A_PER), "float32", plan, b, q_fn, sr.RHO, sr.LAM, sr.MU, 1, 1, "iso",
                   None, 0, fusion=fusion, Wi_list=W, derive_z=derive_z)
    w = np.stack([W[g] for g in plan.local_nodes + plan.halo_nodes])
    return nb, w


def _edges(plan):
    return list(zip(plan.edge_a_row, plan.edge_b_row))


def _np(t):
    return t.detach().cpu().numpy().copy()


def _check_stats(got, want):
    rel = np.abs(got - want) / want
    e, c = np.unravel_index(int(np.argmax(rel)), rel.shape)
    assert rel[e, c] <= STAT_BAR, (f"edge slot {e} {('RA2', 'RB2', 'DZ2')[c]}: {got[e, c]!r} vs fsum "
                                   f"{want[e, c]!r}, relative {rel[e, c]:.2e}")


def _first_diff(a, b):
    at = np.argwhere(a != b)
    return None if len(at) == 0 else (tuple(int(i) for i in at[0]), len(at))


STORED_GRAPHS = [("path", 2), ("ring", 3), ("ring", 4), ("ring", 5), ("ring", 16), ("ring", 17), ("star", 5)]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("graph,V", STORED_GRAPHS, ids=[f"{g}{v}" for g, v in STORED_GRAPHS])
def test_stored_midpoint_consensus_bitwise(cuda, graph, V, N):
    plan = make_plan(sr.graph_of(graph, V), V)
    nb, w = _batch(N, plan, V)
    st = sr.random_state(nb, 3)
    nb.consensus()
    torch.cuda.synchronize()
    E = len(plan.stored_edges)
    zn, yn, _, stats = sr.consensus_ref(st["x_ext"], st["y"], None, st["z"], None, _edges(plan), "midpoint")
    assert _first_diff(_np(nb.z)[:E], zn) is None, ("z (slot, pixel), count", _first_diff(_np(nb.z)[:E], zn))
    assert _first_diff(_np(nb.y)[:E], yn) is None, ("y (slot, pixel), count", _first_diff(_np(nb.y)[:E], yn))
    assert np.array_equal(_np(nb.x_ext), st["x_ext"])
    _check_stats(_np(nb.edge_stats)[:E], stats)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("graph,V", [("ring", 5), ("star", 5), ("ring", 17)])
def test_weighted_consensus_within_2_ulp(cuda, graph, V, N):
    plan = make_plan(sr.graph_of(graph, V), V)
    nb, w = _batch(N, plan, V, fusion="weighted")
    st = sr.random_state(nb, 4)
    nb.consensus()
    torch.cuda.synchronize()
    E = len(plan.stored_edges)
    zn, yn, ybn, stats = sr.consensus_ref(st["x_ext"], st["y"], st["y_b"], st["z"], w, _edges(plan), "weighted")
    worst = {}
    for name, got, want in (("z", nb.z, zn), ("y", nb.y, yn), ("y_b", nb.y_b, ybn)):
        u = sr.ulps(_np(got)[:E], want)
        worst[name] = float(u.max())
    print(f"\nWEIGHTED {graph}{V} N={N}: worst ulp " + " ".join(f"{k}={v:.1f}" for k, v in worst.items()))
    assert max(worst.values()) <= 2.0, worst
    assert np.array_equal(_np(nb.x_ext), st["x_ext"])
    _check_stats(_np(nb.edge_stats)[:E], stats)


DERIVED = [("ring", r) for r in (16, 17, 64, 65, 128, 129)] + [("complete", 17)]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("graph,V", DERIVED, ids=[f"{g}{v}" for g, v in DERIVED])
def test_derived_consensus_bitwise(cuda, graph, V, N):
    """n_xext = V rows: 16 | 17, 64 | 65, 128 | 129 sit on either side of each LDS tier's limit
    (the last takes the direct kernel); the complete graph on 17 nodes has 136 edges, so one LDS
    row serves many edges and the edge loop runs 8 strides of 16 with a remainder of 8."""
    plan = make_plan(sr.graph_of(graph, V), V)
    nb, _ = _batch(N, plan, V, derive_z=True)
    assert nb.z is None and plan.n_xext == V
    st = sr.random_state(nb, 5)
    nb.consensus()
    torch.cuda.synchronize()
    E = len(plan.stored_edges)
    assert E == (136 if graph == "complete" else V)
    z_old = np.stack([sr.z_of(st, plan, k) for k in range(E)])
    zn, yn, _, stats = sr.consensus_ref(st["x_ext"], st["y"], None, z_old, None, _edges(plan), "derived")
    assert _first_diff(_np(nb.y)[:E], yn) is None, ("y (slot, pixel), count", _first_diff(_np(nb.y)[:E], yn))
    assert np.array_equal(_np(nb.x_prev), st["x_ext"]) and np.array_equal(_np(nb.x_ext), st["x_ext"])
    for k in (0, E - 1):  # z as every kernel forms it now: the midpoint of the new x_prev rows
        assert np.array_equal(_np(nb.z_of(k)), zn[k])
    _check_stats(_np(nb.edge_stats)[:E], stats)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("k", [0, 1, 4, 9])
def test_consensus_range_pieces_equal_one_consensus(cuda, k, N):
    V = E = 9
    plan = make_plan(nx.cycle_graph(V), V)
    whole, _ = _batch(N, plan, V)
    parts, _ = _batch(N, plan, V)
    st = sr.random_state(whole, 6)
    sr.random_state(parts, 6)
    for nb in (whole, parts):
        nb.edge_stats.fill_(-1.0)
    whole.consensus()
    rows = 1 + max(plan.edge_a_row[:k] + plan.edge_b_row[:k]) if k else 1  # the smallest bound accepted
    if k:
        with pytest.raises(ValueError):
            parts.consensus_range(0, k, rows - 1)
    parts.consensus_range(0, k, rows)
    torch.cuda.synchronize()
    # slots outside [0, k) untouched by the first call
    assert np.array_equal(_np(parts.z)[k:], st["z"][k:]) and np.array_equal(_np(parts.y)[k:], st["y"][k:])
    assert np.all(_np(parts.edge_stats)[k:] == -1.0)
    parts.consensus_range(k, E, plan.n_xext)
    torch.cuda.synchronize()
    for name in ("z", "y", "edge_stats"):
        assert torch.equal(getattr(parts, name), getattr(whole, name)), name
    zn, yn, _, stats = sr.consensus_ref(st["x_ext"], st["y"], None, st["z"], None, _edges(plan), "midpoint")
    assert np.array_equal(_np(whole.z), zn) and np.array_equal(_np(whole.y), yn)
    _check_stats(_np(whole.edge_stats), stats)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("edge", ["stored", "derived", "weighted"])
def test_halo_rows_are_read_and_no_image_row_is_written(cuda, edge, N):
    """Rank 0 of 2 (nodes 0-3 of 8): a ring over nodes 0, 2, 3, ..., 7 leaves local node 1 without
    an edge and brings the images of nodes 4 and 7 in as halo rows 4 and 5, which the test fills
    itself; edge_b rows >= V are read, and no row of x_ext -- node 1's, which no stored edge
    touches, included -- changes."""
    G = nx.Graph()
    G.add_nodes_from(range(8))
    ring = [0, 2, 3, 4, 5, 6, 7]
    G.add_edges_from(zip(ring, ring[1:] + ring[:1]))
    plan = make_plan(G, 8, world=2, rank=0)
    assert plan.V == 4 and plan.halo_nodes == [4, 7] and max(plan.edge_b_row) >= plan.V
    assert 1 not in plan.edge_a_row + plan.edge_b_row
    fusion = "weighted" if edge == "weighted" else "midpoint"
    nb, w = _batch(N, plan, 8, fusion=fusion, derive_z=(edge == "derived"))
    st = sr.random_state(nb, 7)
    nb.consensus()
    torch.cuda.synchronize()
    E = len(plan.stored_edges)
    z_old = np.stack([sr.z_of(st, plan, k) for k in range(E)])
    zn, yn, ybn, stats = sr.consensus_ref(st["x_ext"], st["y"], st["y_b"], z_old, w, _edges(plan),
                                          "derived" if edge == "derived" else fusion)
    assert np.array_equal(_np(nb.x_ext), st["x_ext"])
    if edge == "weighted":
        for got, want in ((nb.z, zn), (nb.y, yn), (nb.y_b, ybn)):
            assert sr.ulps(_np(got)[:E], want).max() <= 2.0
    else:
        assert np.array_equal(_np(nb.y)[:E], yn)
        if edge == "stored":
            assert np.array_equal(_np(nb.z)[:E], zn)
        else:
            assert np.array_equal(_np(nb.x_prev), st["x_ext"])
    _check_stats(_np(nb.edge_stats)[:E], stats)
