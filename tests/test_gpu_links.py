"""GPU: unreliable links (admm_consensus_gated, links.Gate, NodeBatch(links=...), run_admm's ``links``;
references: tests/links_ref.py on tests/relax_ref.py and the unchanged oracle).

* the gated edge kernel alone, gates all up / all down / alternating / one edge up, alpha 1.0 and 1.6: y', z'
  bitwise a NumPy restatement (weighted fusion within 2 ulp), down edges keep their bits and report DZ2 = 0,
  the sums against math.fsum, rows outside [e0, e1) untouched, two ranges = one call;
* an edge with an endpoint row outside x_ext is left alone, up or down;
* through NodeBatch: an all-up gate is bitwise admm_consensus, at alpha 1.6 bitwise Relaxer.run_edges; a
  change of rho rescales the duals of down edges too;
* whole runs against links_ref.gated_admm at the project's gates (plain, relaxed, bounds, weighted fusion, an
  outage window); pipelined = per-iteration, streams=2 and two gloo ranks bitwise one rank;
* links=None and 1.0 are the run without the keyword; derived z is refused.

Run with ``-s`` to see every case's measured errors.
"""
import os

import networkx as nx
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import links_ref as lr
import state_ref as sr
from admm_hip import links as lk
from admm_hip.geometry import ParallelBeamGeometry, current_stream_handle
from admm_hip.links import Gate
from admm_hip.plan import make_plan
from admm_hip.relax import Relaxer
from admm_hip.solver import NodeBatch
from oracle.geometry import Geometry, joseph_matrix
from test_gpu_bounds import (RUN_APER, RUN_ITERS, RUN_KW, RUN_N, RUN_TOL, RUN_V, SUM_TOL, _free_port, _np, _run,
                             _run_problem, bits, rel)
from test_gpu_relax import GRAPHS, SENTINEL, SIZES, _batch, _device, _edge_case, _host, _same

pytestmark = pytest.mark.gpu

ALPHAS = [1.0, 1.6]


def _gates(E):
    """The gate rows of the kernel tests: all up, all down, alternating, one edge up."""
    one = np.zeros(E, dtype=bool)
    one[E // 2] = True
    return {"all-up": np.ones(E, dtype=bool), "all-down": np.zeros(E, dtype=bool),
            "alternating": np.arange(E) % 2 == 0, "one-up": one}


def _gated(st, E, up, alpha, dev, ranges):
    ns = _device(st, dev)
    g = Gate(np.asarray(up, dtype=bool).reshape(1, E), range(E), st["x_ext"].shape[1], dev, alpha)
    for e0, e1 in ranges:
        g.run_edges(ns, e0, e1, current_stream_handle(dev))
    return _host(ns)


def _check_sums(got, want, up):
    """RA2, RB2 of every edge and DZ2 of the up edges within SUM_TOL of fsum, none of them vacuous; DZ2 of a
    down edge is +0.0 exactly.  Returns the largest relative error."""
    cmp = np.ones_like(want, dtype=bool)
    cmp[~up, 2] = False
    assert np.all(want[cmp] > 0)
    assert np.all(got[~up, 2] == 0.0) and not np.any(np.signbit(got[~up, 2]))
    err = float(np.max(np.abs(got[cmp] - want[cmp]) / want[cmp]))
    assert err <= SUM_TOL, err
    return err


# --------------------------------------------------------------------------------------
# 1. the gated edge kernel alone
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("n", SIZES)
def test_gated_edges_are_bitwise_the_numpy_restatement(cuda, n, graph, alpha):
    st, E = _edge_case(n, graph)
    worst = 0.0
    for name, up in _gates(E).items():
        got = _gated(st, E, up, alpha, cuda, [(0, E)])
        yn, zn, _, sums = lr.edge_ref(st["x_ext"], st["y"], st["z"], st["edge_a"], st["edge_b"], up, alpha)
        assert _same(got["z"], zn), (name, int(np.sum(bits(got["z"]) != bits(zn))))
        assert _same(got["y"], yn), (name, int(np.sum(bits(got["y"]) != bits(yn))))
        assert _same(got["y"][~up], st["y"][~up]) and _same(got["z"][~up], st["z"][~up]), name  # down: kept
        if up.any():
            assert not _same(got["z"][up], st["z"][up]), name  # up: updated
        worst = max(worst, _check_sums(got["edge_stats"], sums, up))
        for k in ("x_ext", "edge_a", "edge_b"):  # only read
            assert np.array_equal(got[k], st[k]), (name, k)
        # two calls [0, k) + [k, E) are one call, statistics included
        if E > 1:
            k = E // 2
            two = _gated(st, E, up, alpha, cuda, [(0, k), (k, E)])
            assert all(_same(two[f], got[f]) for f in ("y", "z", "edge_stats")), name
        # a call owns rows [e0, e1) and nothing else
        e0, e1 = (1, E - 1) if E >= 3 else (0, 1)
        part = _gated(st, E, up, alpha, cuda, [(e0, e1)])
        out = np.r_[0:e0, e1:E]
        for f in ("y", "z", "edge_stats"):
            assert _same(part[f][e0:e1], got[f][e0:e1]) and _same(part[f][out], st[f][out]), (name, f)
        assert np.all(part["edge_stats"][out] == SENTINEL)
    print(f"\nGATED n={n} {graph} alpha={alpha}: sums rel err max {worst:.1e}")


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("n", SIZES)
def test_gated_weighted_edges_within_2_ulp(cuda, n, graph, alpha):
    st, E = _edge_case(n, graph, weighted=True, seed=1)
    worst, err = {}, 0.0
    for name, up in _gates(E).items():
        got = _gated(st, E, up, alpha, cuda, [(0, E)])
        yn, zn, ybn, sums = lr.edge_ref(st["x_ext"], st["y"], st["z"], st["edge_a"], st["edge_b"], up, alpha,
                                        y_b=st["y_b"], W=st["w"])
        for k, want in (("z", zn), ("y", yn), ("y_b", ybn)):
            worst[k] = max(worst.get(k, 0.0), float(sr.ulps(got[k], want).max()))
            assert _same(got[k][~up], st[k][~up]), (name, k)  # down: y, z and y_b keep their bits exactly
        err = max(err, _check_sums(got["edge_stats"], sums, up))
        for k in ("x_ext", "w", "edge_a", "edge_b"):
            assert np.array_equal(got[k], st[k]), (name, k)
    print(f"\nGATED WEIGHTED n={n} {graph} alpha={alpha}: worst ulp " + " ".join(f"{k}={v:.1f}" for k, v in worst.items())
          + f"; sums rel err max {err:.1e}")
    assert max(worst.values()) <= 2.0, worst


# --------------------------------------------------------------------------------------
# 2. an edge that points outside x_ext
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("is_up", [True, False], ids=["up", "down"])
def test_an_edge_with_a_row_outside_x_ext_is_left_alone(cuda, is_up, alpha):
    """The kernel reads no row at or past n_rows: such an edge keeps y and z, and its sums are NaN, whatever its
    gate.  (The tensor holds one row more than the view handed in, so even the refused row exists.)"""
    st, E = _edge_case(1089, "ring3")
    ns = _device(st, cuda)
    full = torch.cat([ns.x_ext, torch.ones((1, 1089), dtype=torch.float64, device=cuda)])
    ns.x_ext = full[:3]
    ns.edge_b = torch.tensor([1, 3, 2], dtype=torch.int32, device=cuda)
    up = np.array([True, is_up, False])
    g = Gate(up.reshape(1, E), range(E), 1089, cuda, alpha)
    g.run_edges(ns, 0, E, current_stream_handle(cuda))
    got = _host(ns)
    assert _same(got["y"][1], st["y"][1]) and _same(got["z"][1], st["z"][1]) and np.isnan(got["edge_stats"][1]).all()
    yn, zn, _, sums = lr.edge_ref(st["x_ext"], st["y"], st["z"], st["edge_a"], st["edge_b"], up, alpha)
    for e in (0, 2):
        assert _same(got["z"][e], zn[e]) and _same(got["y"][e], yn[e])
        assert np.max(np.abs(got["edge_stats"][e, :2] - sums[e, :2]) / sums[e, :2]) <= SUM_TOL
    with pytest.raises(ValueError):
        g.run_edges(ns, 0, E + 1, current_stream_handle(cuda))
    with pytest.raises(ValueError):
        g.set_row(1)


# --------------------------------------------------------------------------------------
# 3. through NodeBatch
# --------------------------------------------------------------------------------------
def _fields(fusion):
    return ("y", "z") + (("y_b",) if fusion == "weighted" else ())


def _snap(nb, fusion):
    torch.cuda.synchronize()
    return {k: getattr(nb, k).cpu().numpy().copy() for k in _fields(fusion) + ("edge_stats",)}


@pytest.mark.parametrize("fusion", ["midpoint", "weighted"])
@pytest.mark.parametrize("N", [13, 33])
def test_an_all_up_gate_is_bitwise_the_ungated_batch(cuda, N, fusion):
    plan = make_plan(sr.graph_of("ring", 5), 5)
    E = len(plan.stored_edges)
    ones = np.ones((2, E), dtype=bool)
    # alpha = 1: admm_consensus
    nb = _batch(N, plan, 5, fusion=fusion)
    assert nb.gate is None
    sr.random_state(nb, 3)
    nb.consensus()
    want = _snap(nb, fusion)
    gb = _batch(N, plan, 5, fusion=fusion, links=ones)
    assert gb.gate is not None and gb.relaxer is None and gb.gate.alpha == 1.0
    st = sr.random_state(gb, 3)
    gb.gate.set_row(1)
    gb.consensus()
    got = _snap(gb, fusion)
    for k in _fields(fusion):
        assert _same(got[k], want[k]), k
        assert not _same(got[k], st[k])  # (the update did something)
    # (two fixed-order sums of the same terms, each within SUM_TOL of the exact sum)
    assert np.max(np.abs(got["edge_stats"] - want["edge_stats"]) / want["edge_stats"]) <= 2 * SUM_TOL
    # alpha = 1.6: Relaxer.run_edges
    sr.random_state(nb, 4)
    Relaxer(1.6, N * N, E, cuda).run_edges(nb, 0, E, current_stream_handle(cuda))
    want = _snap(nb, fusion)
    gb = _batch(N, plan, 5, fusion=fusion, links=ones, relaxation=1.6)
    assert gb.gate.alpha == 1.6
    sr.random_state(gb, 4)
    gb.consensus()
    got = _snap(gb, fusion)
    for k in _fields(fusion) + ("edge_stats",):  # (the same sums code: bitwise too)
        assert _same(got[k], want[k]), k


def test_consensus_range_goes_through_the_gate_and_set_rho_reaches_down_edges(cuda):
    plan = make_plan(sr.graph_of("ring", 5), 5)
    E = len(plan.stored_edges)
    table = np.array([[True, False, True, False, True], [False] * 5])
    nb = _batch(13, plan, 5, links=table)
    st = sr.random_state(nb, 5)
    nb.consensus()
    whole = _snap(nb, "midpoint")
    sr.random_state(nb, 5)
    nb.consensus_range(0, 2, plan.n_xext)
    nb.consensus_range(2, E, plan.n_xext)
    parts = _snap(nb, "midpoint")
    up = table[0][np.asarray(plan.stored_edges)]
    for k in ("y", "z", "edge_stats"):
        assert _same(parts[k], whole[k]), k
    assert _same(whole["z"][~up], st["z"][~up]) and not _same(whole["z"][up], st["z"][up])
    # the dual's scale belongs to rho, not to the link: a down edge's y is rescaled like any other
    nb.gate.set_row(1)
    nb.set_rho(2.0 * sr.RHO)
    nb.consensus()
    after = _snap(nb, "midpoint")
    assert _same(after["y"], 0.5 * whole["y"]) and _same(after["z"], whole["z"])
    assert np.all(after["edge_stats"][:, 2] == 0.0)


# --------------------------------------------------------------------------------------
# 4. whole runs: 4-node ring, N = 33, 12 angles per node, 10 iterations
# --------------------------------------------------------------------------------------
EDGE_HIST = ("primal", "dual", "obj_total")
BOUND_HIST = EDGE_HIST + ("bound_primal", "bound_dual", "bound_violation")
LINKS = {"p": 0.6, "seed": 0}
VARIANTS = {
    "plain": dict(links=LINKS, bounds=None, keys=EDGE_HIST),
    "relaxed": dict(links=LINKS, bounds=None, relaxation=1.6, keys=EDGE_HIST),
    "bounds": dict(links=LINKS, bounds=(0.0, 1.0), keys=BOUND_HIST),
    "weighted": dict(links=LINKS, bounds=None, fusion="weighted", keys=EDGE_HIST),
    "outage": dict(links={"outages": [(0, 1, 2, 6), (0, 3, 8, None)]}, bounds=None, keys=EDGE_HIST),
}


def _table(links, iters=RUN_ITERS, V=RUN_V):
    t = lk.schedule(nx.cycle_graph(V), iters, links)
    assert t.any() and not t.all()  # both up and down entries
    return t


@pytest.fixture(scope="module")
def run_ref():
    """{(dtype, variant): (x, history)} of links_ref on the Joseph matrix and the device's sinograms."""
    cache = {}

    def get(dtype, variant):
        if (dtype, variant) not in cache:
            ops, ph, sinos, Wi, Q = _run_problem(dtype)
            A = joseph_matrix(Geometry(RUN_N, RUN_APER))
            b = [_np(s).reshape(-1) for s in sinos]
            v = VARIANTS[variant]
            x, _, h = lr.gated_admm([A] * RUN_V, b, nx.cycle_graph(RUN_V), Q, RUN_N, _table(v["links"]),
                                    alpha=v.get("relaxation", 1.0), fusion=v.get("fusion", "midpoint"),
                                    Wi_list=[_np(w) for w in Wi], bounds=v["bounds"], max_iters=RUN_ITERS,
                                    phantom_true=_np(ph), **RUN_KW)
            cache[(dtype, variant)] = (np.stack(x), {k: np.asarray(h[k]) for k in v["keys"]})
        return cache[(dtype, variant)]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gated_run_matches_reference(cuda, monkeypatch, run_ref, dtype, variant):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    via = "dropin" if variant == "plain" else "run_admm"
    x, h, full = _run(dtype, via=via, **VARIANTS[variant])
    xo, ho = run_ref(dtype, variant)
    errs = {"images": rel(x, xo), **{k: rel(h[k], ho[k]) for k in ho}}
    print(f"\nGATED RUN {dtype} {variant}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert len(h["primal"]) == RUN_ITERS and "links" not in full
    t = _table(VARIANTS[variant]["links"])
    assert full["links_up"] == lk.links_up(t).tolist() and full["link_age_max"] == lk.link_age_max(t).tolist()
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)


# --------------------------------------------------------------------------------------
# 5. equivalences
# --------------------------------------------------------------------------------------
def test_pipelined_and_per_iteration_histories_are_equal(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    keys = BOUND_HIST + ("bound_pri_per_node", "pri_per_node", "dual_per_node", "links_up", "link_age_max")
    xa, ha, _ = _run("float32", iters=4, keys=keys, links=LINKS)
    xb, hb, _ = _run("float32", iters=4, keys=keys, links=LINKS, pipeline=False)
    assert np.array_equal(xa, xb)
    for k in keys:
        assert np.array_equal(ha[k], hb[k]), k
    _table(LINKS, 4)


@pytest.mark.parametrize("variant", ["bounds", "weighted"])
def test_streams_split_is_bitwise_one_batch(cuda, monkeypatch, variant):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}
    v = VARIANTS[variant]
    _table(LINKS, 3, 8)
    x1, h1, _ = _run("float64", V=8, iters=3, inspect=lambda rg: seen.setdefault(1, len(rg.batches)), **v)
    x2, h2, _ = _run("float64", V=8, iters=3, streams=2, inspect=lambda rg: seen.setdefault(2, len(rg.batches)), **v)
    assert seen == {1: 1, 2: 2}
    assert np.array_equal(x1, x2)
    for k in v["keys"]:
        assert np.array_equal(h1[k], h2[k]), k


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = {}
        for overlap in ("1", "0"):
            os.environ["ADMM_EXCHANGE_OVERLAP"] = overlap
            seen = {}
            x, h, _ = _run("float32", iters=4, links=LINKS, relaxation=1.6, keys=BOUND_HIST,
                           inspect=lambda rg: seen.update(overlaps=rg.overlaps_exchange))
            out[overlap] = (x, h, seen["overlaps"])
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_one_rank_bitwise(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EXCHANGE_OVERLAP", raising=False)
    x1, h1, _ = _run("float32", iters=4, links=LINKS, relaxation=1.6, keys=BOUND_HIST)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in range(2):
        for overlap in ("1", "0"):
            x2, h2, overlaps = res[r][overlap]
            assert overlaps  # (the run can overlap: the range calls are what "1" exercises)
            assert np.array_equal(x1, x2), (r, overlap)
            for k in h1:
                assert np.array_equal(h1[k], h2[k]), (k, r, overlap)


# --------------------------------------------------------------------------------------
# 6. off is off
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [None, (0.0, 1.0)], ids=["plain", "bounds"])
def test_none_and_one_are_the_run_without_the_keyword(cuda, monkeypatch, bounds):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = []
    look = lambda rg: seen.append([nb.gate for nb in rg.batches])  # noqa: E731
    x0, _, h0 = _run("float32", iters=3, bounds=bounds, keys=())
    for value in (None, 1.0, {"p": 1.0}, {"outages": [(0, 1, 3, 5)]}):  # (the window lies past the run)
        x, _, h = _run("float32", iters=3, bounds=bounds, keys=(), links=value, inspect=look)
        assert np.array_equal(x, x0) and set(h) == set(h0)
        for k in h0:
            assert np.array_equal(np.asarray(h[k]), np.asarray(h0[k]), equal_nan=True), k
    assert seen == [[None]] * 4  # no table, no scratch either
    # and a gated run is another run, with two more keys: the host arithmetic on its table
    xg, _, hg = _run("float32", iters=3, bounds=bounds, keys=(), links=LINKS, inspect=look)
    assert seen[-1][0] is not None
    assert rel(xg, x0) > 1e-3 and set(hg) == set(h0) | {"links_up", "link_age_max"}
    t = _table(LINKS, 3)
    assert hg["links_up"] == t.sum(axis=1).tolist() and hg["link_age_max"] == lk.link_age_max(t).tolist()
    # an explicit all-up table is used as it is: through the gate, the same images
    xa, _, ha = _run("float32", iters=3, bounds=bounds, keys=(), links=np.ones((3, RUN_V), dtype=bool))
    assert np.array_equal(xa, x0) and ha["links_up"] == [RUN_V] * 3 and ha["link_age_max"] == [0] * 3


# --------------------------------------------------------------------------------------
# 7. the refusals
# --------------------------------------------------------------------------------------
def test_links_with_derived_z_are_refused(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    with pytest.raises(ValueError, match="stored z"):
        _run("float32", iters=2, bounds=None, links=LINKS, edge_state="derived")
    monkeypatch.setenv("ADMM_EDGE_STATE", "derived")
    with pytest.raises(ValueError, match="stored z"):
        _run("float32", iters=2, bounds=None, links=LINKS)
    monkeypatch.delenv("ADMM_EDGE_STATE")
    # the HBM rule's derived choice, in the run and in a batch of its own
    import admm_hip.groups as groups
    import admm_hip.solver as solver
    monkeypatch.setattr(groups, "z_is_stored", lambda *a, **k: False)
    with pytest.raises(ValueError, match="links need stored z.*stored-z rule"):
        _run("float32", iters=2, bounds=None, links=LINKS)
    monkeypatch.setattr(solver, "z_is_stored", lambda *a, **k: False)
    plan = make_plan(sr.graph_of("ring", 3), 3)
    mk = lambda **kw: NodeBatch(ParallelBeamGeometry(13, 2), "float32", plan, {g: np.zeros(26) for g in range(3)},  # noqa: E731
                                sr.precisions(169, 3, 1)[1], sr.RHO, sr.LAM, sr.MU, 1, 1, "iso", None, 0,
                                links=np.zeros((2, 3), dtype=bool), **kw)
    with pytest.raises(ValueError, match="links need stored z.*stored-z rule"):
        mk()
    with pytest.raises(ValueError, match="stored z"):
        mk(derive_z=True)
