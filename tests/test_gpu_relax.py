"""GPU: over-relaxation (admm_consensus_relaxed, admm_bound_project_relaxed, NodeBatch(relaxation=...),
run_admm's ``relaxation``; references: tests/relax_ref.py on the unchanged oracle).

* the edge kernel alone: z' and y' bitwise a NumPy restatement, the three sums against math.fsum, rows
  outside [e0, e1) untouched, two ranges = one call; weighted fusion within 2 ulp;
* alpha = 1 through the low-level wrapper: bitwise admm_consensus / admm_bound_project;
* the relaxed projection: bitwise its restatement, batch-position invariance;
* whole runs against relax_ref.relaxed_admm at the project's gates (plain, bounds, weighted fusion);
  pipelined = per-iteration, streams=2 and two gloo ranks bitwise one rank;
* relaxation=None and 1.0 are the run without the keyword.

Run with ``-s`` to see every case's measured errors.
"""
import os
from types import SimpleNamespace

import networkx as nx
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import bounds_ref as br
import relax_ref as rr
import state_ref as sr
from admm_hip.bounds import BoundProjector
from admm_hip.geometry import ParallelBeamGeometry, current_stream_handle
from admm_hip.plan import make_plan
from admm_hip.relax import Relaxer
from admm_hip.solver import NodeBatch
from oracle.geometry import Geometry, joseph_matrix
from test_gpu_bounds import (RUN_APER, RUN_ITERS, RUN_KW, RUN_N, RUN_TOL, RUN_V, SUM_TOL, _free_port, _kernel_case, _np,
                             _run, _run_problem, bits, rel)

pytestmark = pytest.mark.gpu

ALPHAS = [0.5, 1.6, 1.8]
SIZES = [169, 1089, 4096]  # less than one block, one block + a 65-pixel tail, exactly four blocks
GRAPHS = {
    "edge": (2, [(0, 1)]),
    "ring3": (3, [(0, 1), (1, 2), (0, 2)]),
    "star17": (17, [(0, k) for k in range(1, 17)]),
    "complete6": (6, [(a, b) for a in range(6) for b in range(a + 1, 6)]),
}
SENTINEL = 7.0  # edge_stats before a call: rows the call does not own keep it


# --------------------------------------------------------------------------------------
# 1. the edge kernel alone
# --------------------------------------------------------------------------------------
def _edge_case(n, graph, weighted=False, seed=0):
    R, edges = GRAPHS[graph]
    E = len(edges)
    rng = np.random.default_rng([seed, n, E])
    st = dict(x_ext=rng.standard_normal((R, n)), y=rng.standard_normal((E, n)), z=rng.standard_normal((E, n)),
              y_b=rng.standard_normal((E, n)) if weighted else None,
              w=rng.uniform(0.5, 2.0, (R, n)) if weighted else None,
              edge_a=np.array([a for a, _ in edges], dtype=np.int32),
              edge_b=np.array([b for _, b in edges], dtype=np.int32),
              edge_stats=np.full((E, 3), SENTINEL))
    return st, E


def _device(st, dev):
    """The host state as an object with NodeBatch's tensor names (what Relaxer.run_edges reads)."""
    return SimpleNamespace(**{k: None if v is None else torch.from_numpy(v.copy()).to(dev) for k, v in st.items()})


def _host(ns):
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in vars(ns).items()}


def _relaxed(st, E, alpha, dev, ranges):
    ns = _device(st, dev)
    rx = Relaxer(alpha, st["x_ext"].shape[1], E, dev)
    for e0, e1 in ranges:
        rx.run_edges(ns, e0, e1, current_stream_handle(dev))
    return _host(ns)


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _stat_err(got, want):
    return float(np.max(np.abs(got - want) / want))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("n", SIZES)
def test_relaxed_edges_are_bitwise_the_numpy_restatement(cuda, n, graph, alpha):
    st, E = _edge_case(n, graph)
    got = _relaxed(st, E, alpha, cuda, [(0, E)])
    yn, zn, _, sums = rr.edge_ref(st["x_ext"], st["y"], st["z"], st["edge_a"], st["edge_b"], alpha)
    assert _same(got["z"], zn), int(np.sum(bits(got["z"]) != bits(zn)))
    assert _same(got["y"], yn), int(np.sum(bits(got["y"]) != bits(yn)))
    err = _stat_err(got["edge_stats"], sums)
    print(f"\nEDGES n={n} {graph} alpha={alpha}: sums rel err max {err:.1e}")
    assert np.all(sums > 0) and err <= SUM_TOL
    for k in ("x_ext", "edge_a", "edge_b"):  # only read
        assert np.array_equal(got[k], st[k]), k
    # two calls [0, k) + [k, E) are one call, statistics included
    if E > 1:
        k = E // 2
        two = _relaxed(st, E, alpha, cuda, [(0, k), (k, E)])
        assert all(_same(two[f], got[f]) for f in ("y", "z", "edge_stats"))
    # a call owns rows [e0, e1) and nothing else
    e0, e1 = (1, E - 1) if E >= 3 else (0, 1)
    part = _relaxed(st, E, alpha, cuda, [(e0, e1)])
    out = np.r_[0:e0, e1:E]
    for f in ("y", "z", "edge_stats"):
        assert _same(part[f][e0:e1], got[f][e0:e1]) and _same(part[f][out], st[f][out]), f


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("n", SIZES)
def test_relaxed_weighted_edges_within_2_ulp(cuda, n, graph, alpha):
    st, E = _edge_case(n, graph, weighted=True, seed=1)
    got = _relaxed(st, E, alpha, cuda, [(0, E)])
    yn, zn, ybn, sums = rr.edge_ref(st["x_ext"], st["y"], st["z"], st["edge_a"], st["edge_b"], alpha, y_b=st["y_b"],
                                    W=st["w"])
    worst = {k: float(sr.ulps(got[k], want).max()) for k, want in (("z", zn), ("y", yn), ("y_b", ybn))}
    err = _stat_err(got["edge_stats"], sums)
    print(f"\nWEIGHTED n={n} {graph} alpha={alpha}: worst ulp " + " ".join(f"{k}={v:.1f}" for k, v in worst.items())
          + f"; sums rel err max {err:.1e}")
    assert max(worst.values()) <= 2.0, worst
    assert err <= SUM_TOL
    for k in ("x_ext", "w", "edge_a", "edge_b"):
        assert np.array_equal(got[k], st[k]), k


def test_an_edge_with_a_row_outside_x_ext_is_left_alone(cuda):
    """The kernel reads no row at or past n_rows: such an edge keeps y and z, and its sums are NaN.
    (The tensor holds one row more than the view handed in, so even the refused row exists.)"""
    st, E = _edge_case(1089, "ring3")
    ns = _device(st, cuda)
    full = torch.cat([ns.x_ext, torch.ones((1, 1089), dtype=torch.float64, device=cuda)])
    ns.x_ext = full[:3]
    ns.edge_b = torch.tensor([1, 3, 2], dtype=torch.int32, device=cuda)
    Relaxer(1.6, 1089, E, cuda).run_edges(ns, 0, E, current_stream_handle(cuda))
    got = _host(ns)
    assert _same(got["y"][1], st["y"][1]) and _same(got["z"][1], st["z"][1]) and np.isnan(got["edge_stats"][1]).all()
    yn, zn, _, sums = rr.edge_ref(st["x_ext"], st["y"], st["z"], st["edge_a"], st["edge_b"], 1.6)
    for e in (0, 2):
        assert _same(got["z"][e], zn[e]) and _same(got["y"][e], yn[e])
    with pytest.raises(ValueError):
        Relaxer(1.6, 1089, E, cuda).run_edges(ns, 0, E + 1, current_stream_handle(cuda))


# --------------------------------------------------------------------------------------
# 2. alpha = 1 through the low-level wrapper is the unrelaxed kernel
# --------------------------------------------------------------------------------------
def _batch(N, plan, V_total, fusion="midpoint", seed=1, **kw):
    n, a_per = N * N, 2
    rng = np.random.default_rng([seed, 5])
    b = {g: rng.standard_normal(a_per * N) for g in plan.local_nodes}
    W, q_fn = sr.precisions(n, V_total, seed)
    return NodeBatch(ParallelBeamGeometry(N, a_per), "float32", plan, b, q_fn, sr.RHO, sr.LAM, sr.MU, 1, 1, "iso", None,
                     0, fusion=fusion, Wi_list=W, derive_z=False, **kw)


@pytest.mark.parametrize("fusion", ["midpoint", "weighted"])
@pytest.mark.parametrize("N", [13, 33])
def test_alpha_one_is_bitwise_admm_consensus(cuda, N, fusion):
    plan = make_plan(sr.graph_of("ring", 5), 5)
    nb = _batch(N, plan, 5, fusion=fusion)
    E = len(plan.stored_edges)
    sr.random_state(nb, 3)
    nb.consensus()
    torch.cuda.synchronize()
    want = {k: getattr(nb, k).cpu().numpy().copy() for k in ("y", "z") + (("y_b",) if fusion == "weighted" else ())}
    st = sr.random_state(nb, 3)
    assert nb.relaxer is None
    Relaxer(1.0, N * N, E, cuda).run_edges(nb, 0, E, current_stream_handle(cuda))
    torch.cuda.synchronize()
    for k, v in want.items():
        assert _same(getattr(nb, k).cpu().numpy(), v), k
        assert not _same(v, st[k])  # (the update did something)


def test_alpha_one_projection_is_bitwise_admm_bound_project(cuda):
    n, nimg = 1089, 3
    rng = np.random.default_rng(11)
    x, w, f = rng.standard_normal((nimg, n)), rng.standard_normal((nimg, n)), 0.3 * rng.standard_normal((nimg, n))
    B = _kernel_case(n, nimg, "maps")[0]
    out = {}
    for alpha in (None, 1.0):
        pr = BoundProjector(B, n, cuda, nimg)
        xd, wd, fd = (torch.from_numpy(a.copy()).to(cuda) for a in (x, w, f))
        s = pr.run(xd, wd, fd, current_stream_handle(cuda), alpha=alpha)
        torch.cuda.synchronize()
        out[alpha] = (wd.cpu().numpy(), fd.cpu().numpy(), s.cpu().numpy().copy())
    for a, b in zip(out[None], out[1.0]):
        assert _same(a, b)


# --------------------------------------------------------------------------------------
# 3. the relaxed projection
# --------------------------------------------------------------------------------------
def _project(B, x, w, f, alpha, dev):
    pr = BoundProjector(B, x.shape[1], dev, x.shape[0])
    xd, wd, fd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, w, f))
    s = Relaxer(alpha, x.shape[1], 1, dev).run_bounds(pr, xd, wd, fd, current_stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), torch.from_numpy(np.ascontiguousarray(x)))  # x is only read
    return wd.cpu().numpy(), fd.cpu().numpy(), s.cpu().numpy().copy()


@pytest.mark.parametrize("form", ["scalar", "maps"])
@pytest.mark.parametrize("nimg", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_relaxed_projection_is_bitwise_the_numpy_restatement(cuda, n, nimg, form):
    B, l, h, x, w, f = _kernel_case(n, nimg, form)
    for alpha in (1.6, 0.5):
        wn, fn, sums = _project(B, x, w, f, alpha, cuda)
        wr_, fr_, sr_ = rr.project_ref(x, w, f, l, h, alpha)
        assert _same(wn, wr_), int(np.sum(bits(wn) != bits(wr_)))
        assert _same(fn, fr_), int(np.sum(bits(fn) != bits(fr_)))
        assert np.all(wn >= l) and np.all(wn <= h)
        err = _stat_err(sums, sr_)
        print(f"\nRELAXED PROJ n={n} nimg={nimg} {form} alpha={alpha}: sums rel err max {err:.1e}")
        assert np.all(sr_ > 0) and err <= SUM_TOL
        assert not _same(wn, br.project_ref(x, w, f, l, h)[0])  # and it is not the plain projection


def test_a_relaxed_images_outputs_do_not_depend_on_batch_position(cuda):
    n, nimg = 1089, 8
    B, l, h, x, w, f = _kernel_case(n, nimg, "maps", seed=1)
    full = _project(B, x, w, f, 1.6, cuda)
    for v in (0, 3, 7):  # alone
        one = _project(B, x[v:v + 1], w[v:v + 1], f[v:v + 1], 1.6, cuda)
        for a, b in zip(one, full):
            assert _same(a[0], b[v]), v
    perm = [5, 0, 7, 2]  # other positions in a smaller batch
    sub = _project(B, x[perm], w[perm], f[perm], 1.6, cuda)
    for k, v in enumerate(perm):
        for a, b in zip(sub, full):
            assert _same(a[k], b[v]), v


# --------------------------------------------------------------------------------------
# 4. whole runs: 4-node ring, N = 33, 12 angles per node, alpha = 1.6, 10 iterations
# --------------------------------------------------------------------------------------
ALPHA = 1.6
EDGE_HIST = ("primal", "dual", "obj_total")
BOUND_HIST = EDGE_HIST + ("bound_primal", "bound_dual", "bound_violation")
VARIANTS = {
    "plain": dict(bounds=None, keys=EDGE_HIST),
    "bounds": dict(bounds=(0.0, 1.0), keys=BOUND_HIST),
    "weighted": dict(bounds=None, fusion="weighted", keys=EDGE_HIST),
}


@pytest.fixture(scope="module")
def run_ref():
    """{(dtype, variant): (x, history)} of relax_ref on the Joseph matrix and the device's sinograms."""
    cache = {}

    def get(dtype, variant):
        if (dtype, variant) not in cache:
            ops, ph, sinos, Wi, Q = _run_problem(dtype)
            A = joseph_matrix(Geometry(RUN_N, RUN_APER))
            b = [_np(s).reshape(-1) for s in sinos]
            v = VARIANTS[variant]
            x, _, h = rr.relaxed_admm([A] * RUN_V, b, nx.cycle_graph(RUN_V), Q, RUN_N, alpha=ALPHA,
                                      fusion=v.get("fusion", "midpoint"), Wi_list=[_np(w) for w in Wi],
                                      bounds=v["bounds"], max_iters=RUN_ITERS, phantom_true=_np(ph), **RUN_KW)
            cache[(dtype, variant)] = (np.stack(x), {k: np.asarray(h[k]) for k in v["keys"]})
        return cache[(dtype, variant)]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_relaxed_run_matches_reference(cuda, monkeypatch, run_ref, dtype, variant):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    via = "dropin" if variant == "plain" else "run_admm"
    x, h, full = _run(dtype, via=via, relaxation=ALPHA, **VARIANTS[variant])
    xo, ho = run_ref(dtype, variant)
    errs = {"images": rel(x, xo), **{k: rel(h[k], ho[k]) for k in ho}}
    print(f"\nRELAXED RUN {dtype} {variant}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert len(h["primal"]) == RUN_ITERS and "relaxation" not in full
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)


def test_relaxed_run_differs_from_the_plain_run_and_converges_faster(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    x0, h0, _ = _run("float64", bounds=None, keys=EDGE_HIST)
    x1, h1, _ = _run("float64", bounds=None, keys=EDGE_HIST, relaxation=ALPHA)
    print(f"\nRELAXED vs PLAIN after {RUN_ITERS}: primal {h0['primal'][-1]:.3e} -> {h1['primal'][-1]:.3e}, "
          f"dual {h0['dual'][-1]:.3e} -> {h1['dual'][-1]:.3e}")
    assert rel(x1, x0) > 1e-3
    assert h1["primal"][-1] < h0["primal"][-1]


def test_pipelined_and_per_iteration_histories_are_equal(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    keys = BOUND_HIST + ("bound_pri_per_node", "pri_per_node")
    xa, ha, _ = _run("float32", iters=4, keys=keys, relaxation=ALPHA)
    xb, hb, _ = _run("float32", iters=4, keys=keys, relaxation=ALPHA, pipeline=False)
    assert np.array_equal(xa, xb)
    for k in keys:
        assert np.array_equal(ha[k], hb[k]), k


@pytest.mark.parametrize("variant", ["bounds", "weighted"])
def test_streams_split_is_bitwise_one_batch(cuda, monkeypatch, variant):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}
    v = VARIANTS[variant]
    x1, h1, _ = _run("float64", V=8, iters=3, relaxation=ALPHA, inspect=lambda rg: seen.setdefault(1, len(rg.batches)),
                     **v)
    x2, h2, _ = _run("float64", V=8, iters=3, relaxation=ALPHA, streams=2,
                     inspect=lambda rg: seen.setdefault(2, len(rg.batches)), **v)
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
            x, h, _ = _run("float32", iters=4, relaxation=ALPHA, keys=BOUND_HIST,
                           inspect=lambda rg: seen.update(overlaps=rg.overlaps_exchange))
            out[overlap] = (x, h, seen["overlaps"])
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_one_rank_bitwise(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EXCHANGE_OVERLAP", raising=False)
    x1, h1, _ = _run("float32", iters=4, relaxation=ALPHA, keys=BOUND_HIST)
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
# 5. off is off; the refusals
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [None, (0.0, 1.0)], ids=["plain", "bounds"])
def test_none_and_one_are_the_run_without_the_keyword(cuda, monkeypatch, bounds):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = []
    look = lambda rg: seen.append([nb.relaxer for nb in rg.batches])  # noqa: E731
    x0, _, h0 = _run("float32", iters=3, bounds=bounds, keys=())
    for value in (None, 1.0):
        x, _, h = _run("float32", iters=3, bounds=bounds, keys=(), relaxation=value, inspect=look)
        assert np.array_equal(x, x0) and set(h) == set(h0)
        for k in h0:
            assert np.array_equal(np.asarray(h[k]), np.asarray(h0[k]), equal_nan=True), k
    assert seen == [[None], [None]]  # no scratch either


def test_relaxation_with_derived_z_is_refused(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    with pytest.raises(ValueError, match="stored z"):
        _run("float32", iters=1, bounds=None, relaxation=ALPHA, edge_state="derived")
    monkeypatch.setenv("ADMM_EDGE_STATE", "derived")
    with pytest.raises(ValueError, match="stored z"):
        _run("float32", iters=1, bounds=None, relaxation=ALPHA)
    monkeypatch.delenv("ADMM_EDGE_STATE")
    # the HBM rule's derived choice, in the run and in a batch of its own
    import admm_hip.groups as groups
    import admm_hip.solver as solver
    monkeypatch.setattr(groups, "z_is_stored", lambda *a, **k: False)
    with pytest.raises(ValueError, match="stored-z rule"):
        _run("float32", iters=1, bounds=None, relaxation=ALPHA)
    monkeypatch.setattr(solver, "z_is_stored", lambda *a, **k: False)
    plan = make_plan(sr.graph_of("ring", 3), 3)
    mk = lambda **kw: NodeBatch(ParallelBeamGeometry(13, 2), "float32", plan, {g: np.zeros(26) for g in range(3)},  # noqa: E731
                                sr.precisions(169, 3, 1)[1], sr.RHO, sr.LAM, sr.MU, 1, 1, "iso", None, 0,
                                relaxation=ALPHA, **kw)
    with pytest.raises(ValueError, match="stored-z rule"):
        mk()
    with pytest.raises(ValueError, match="stored z"):
        mk(derive_z=True)
