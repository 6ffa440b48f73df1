"""GPU: residual-balancing rho and the scale-free stop test (admm_node_norms, admm_batch_set_rho,
NodeBatch.set_rho / node_norms, run_admm's ``adapt_rho`` / ``eps_abs`` / ``eps_rel``; references:
tests/penalty_ref.py on the unchanged oracle).

* the norms kernel alone: its three sums against math.fsum at the bar of the other fixed-order sums,
  +0 for an isolated node, invariance to batch position and stride, inputs untouched, a NaN row for an
  out-of-range slot;
* set_rho: the next update is bitwise a freshly built batch's (float32 / float64, ray weights, bounds,
  keep_x on and off), and the weights survive;
* whole runs against penalty_ref.adaptive_admm at the project's gates (plain, bounds + relaxation,
  weighted fusion), ``rho_history`` exactly; a run with tolerances stops where the reference stops;
  streams=2 and two gloo ranks bitwise one rank;
* the three keywords at None are the run without them.

Run with ``-s`` to see every case's measured errors.
"""
import os

import networkx as nx
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import bounds_ref as br
import penalty_ref as pr
import state_ref as sr
from admm_hip.geometry import ParallelBeamGeometry, current_stream_handle
from admm_hip.penalty import NORM_KEYS, NodeNorms
from admm_hip.plan import make_plan
from admm_hip.solver import NodeBatch
from oracle.geometry import Geometry, joseph_matrix
from test_gpu_bounds import RUN_TOL, SUM_TOL, _free_port, _np, bits, rel

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------
# 1. the norms kernel alone
# --------------------------------------------------------------------------------------
SIZES = [1, 169, 1025, 4096]  # one pixel, less than one block, one block + 1 pixel, exactly four blocks
E_REAL = 6
# incidences per image: 0 (an isolated node), 1, 2 and 5 real edges; "+c": a constraint-style slot follows
COUNTS = {1: [(5, True)], 3: [(0, False), (2, True), (5, False)],
          8: [(0, False), (1, False), (2, False), (5, False), (1, True), (0, True), (5, True), (2, True)]}


def _norm_case(n, nimg, with_yb, seed=0):
    """Host arrays of one call: E_REAL edge rows then one constraint-style row per image (z row = w,
    y row = f, sign +1, last of its image's incidences); mixed signs on the real incidences."""
    rng = np.random.default_rng([seed, n, nimg, int(with_yb)])
    ES = E_REAL + nimg
    off, edge, sign = [0], [], []
    for v, (cnt, slot) in enumerate(COUNTS[nimg]):
        es = rng.permutation(E_REAL)[:cnt]
        sg = np.where(np.arange(cnt) % 2 == v % 2, 1, -1)  # alternating, starting either way
        edge += [int(e) for e in es] + ([E_REAL + v] if slot else [])
        sign += [int(s) for s in sg] + ([1] if slot else [])
        off.append(len(edge))
    return dict(x=rng.standard_normal((nimg, n)), y=rng.standard_normal((ES, n)), z=rng.standard_normal((ES, n)),
                y_b=rng.standard_normal((ES, n)) if with_yb else None, off=np.array(off, dtype=np.int32),
                edge=np.array(edge if edge else [0], dtype=np.int32), sign=np.array(sign if sign else [0], dtype=np.int32),
                n_edges=ES)


def _norms(c, dev, rows=None, pad=0):
    """The kernel's (nimg, 3) sums for case ``c``; ``rows``: only these images, in this order (their
    incidence lists rebuilt); ``pad``: x rows ``pad`` doubles apart more than n.  Also returns the device
    copies of the inputs after the call."""
    rows = list(range(c["x"].shape[0])) if rows is None else rows
    n = c["x"].shape[1]
    off, edge, sign = [0], [], []
    for v in rows:
        lo, hi = int(c["off"][v]), int(c["off"][v + 1])
        edge += c["edge"][lo:hi].tolist()
        sign += c["sign"][lo:hi].tolist()
        off.append(len(edge))
    t = lambda a, dt=torch.float64: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    wide = torch.full((len(rows), n + pad), 3.0, dtype=torch.float64, device=dev)
    wide[:, :n] = t(c["x"][rows])
    x = wide[:, :n]
    y, yb, z = t(c["y"]), t(c["y_b"]), t(c["z"])
    ti = lambda a: torch.tensor(a if len(a) else [0], dtype=torch.int32, device=dev)  # noqa: E731
    io, ie, isg = ti(off), ti(edge), ti(sign)
    nn = NodeNorms(n, len(rows), dev)
    out = nn.run(x, y, yb, z, io, ie, isg, c["n_edges"], current_stream_handle(dev))
    torch.cuda.synchronize()
    after = dict(x=x.cpu().numpy(), y=y.cpu().numpy(), z=z.cpu().numpy(), y_b=None if yb is None else yb.cpu().numpy())
    return out.cpu().numpy().copy(), after


def _sum_err(got, want):
    nz = want != 0.0
    return float(np.max(np.abs(got[nz] - want[nz]) / want[nz])) if nz.any() else 0.0


@pytest.mark.parametrize("with_yb", [False, True], ids=["midpoint", "y_b"])
@pytest.mark.parametrize("nimg", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_norms_match_the_numpy_restatement(cuda, n, nimg, with_yb):
    c = _norm_case(n, nimg, with_yb)
    got, after = _norms(c, cuda)
    want = pr.node_norms_ref(c["x"], c["y"], c["y_b"], c["z"], c["off"], c["edge"], c["sign"])
    err = _sum_err(got, want)
    print(f"\nNORMS n={n} nimg={nimg} y_b={with_yb}: sums rel err max {err:.1e}")
    assert err <= SUM_TOL and np.all(want[:, 0] > 0)
    for v, (cnt, slot) in enumerate(COUNTS[nimg]):
        if cnt == 0 and not slot:  # an isolated node: Z2 = U2 = +0 exactly
            assert got[v, 1] == 0.0 and got[v, 2] == 0.0 and not np.signbit(got[v, 1:]).any()
        else:
            assert want[v, 1] > 0 and want[v, 2] > 0
    for k in ("x", "y", "z", "y_b"):  # only read
        assert (c[k] is None and after[k] is None) or np.array_equal(bits(after[k]), bits(c[k])), k
    # y_b is read where the sign is negative, and only there
    if with_yb:
        other = pr.node_norms_ref(c["x"], c["y"], None, c["z"], c["off"], c["edge"], c["sign"])
        neg = [v for v in range(nimg) if (c["sign"][c["off"][v]:c["off"][v + 1]] < 0).any()]
        assert neg and all(other[v, 2] != want[v, 2] for v in neg)


@pytest.mark.parametrize("with_yb", [False, True], ids=["midpoint", "y_b"])
def test_an_images_norms_do_not_depend_on_batch_position_or_stride(cuda, with_yb):
    c = _norm_case(1025, 8, with_yb, seed=1)
    full, _ = _norms(c, cuda)
    for v in (0, 3, 6, 7):  # alone, and with a row stride that is no multiple of anything
        one, _ = _norms(c, cuda, rows=[v], pad=7)
        assert np.array_equal(bits(one[0]), bits(full[v])), v
    perm = [6, 0, 7, 3, 2]  # other positions in a smaller batch
    sub, _ = _norms(c, cuda, rows=perm, pad=1)
    for k, v in enumerate(perm):
        assert np.array_equal(bits(sub[k]), bits(full[v])), v


@pytest.mark.parametrize("slot", [-1, "n_edges"])
def test_an_out_of_range_slot_gives_a_nan_row_and_leaves_the_neighbours(cuda, slot):
    """The kernel dereferences no slot outside [0, n_edges): that image's sums are NaN.  (The tensors
    hold one row more than n_edges says, so even the refused row exists.)"""
    c = _norm_case(1025, 8, False, seed=2)
    want = pr.node_norms_ref(c["x"], c["y"], None, c["z"], c["off"], c["edge"], c["sign"])
    bad = dict(c, edge=c["edge"].copy(), n_edges=c["n_edges"] - 1)  # the last row exists but is out of range
    v = 3  # five incidences: the third is the bad one
    bad["edge"][c["off"][v] + 2] = -1 if slot == -1 else bad["n_edges"]
    last = c["n_edges"] - 1
    assert all(last not in c["edge"][c["off"][u]:c["off"][u + 1]] for u in range(8) if u != 7)
    got, _ = _norms(bad, cuda)
    assert np.isnan(got[v]).all()
    assert np.isnan(got[7]).all()  # image 7's constraint-style slot is the row n_edges now excludes
    for u in (0, 1, 2, 4, 5, 6):
        assert _sum_err(got[u:u + 1], want[u:u + 1]) <= SUM_TOL and not np.isnan(got[u]).any(), u


def test_node_norms_wrapper_refuses_wrong_shapes(cuda):
    nn = NodeNorms(169, 2, cuda)
    t = lambda *s: torch.zeros(s, dtype=torch.float64, device=cuda)  # noqa: E731
    io = torch.zeros(3, dtype=torch.int32, device=cuda)
    s = current_stream_handle(cuda)
    with pytest.raises(ValueError, match="x must be"):
        nn.run(t(3, 169), t(1, 169), None, t(1, 169), io, io, io, 1, s)
    with pytest.raises(ValueError, match="x must be"):
        nn.run(t(2, 338)[:, ::2], t(1, 169), None, t(1, 169), io, io, io, 1, s)
    with pytest.raises(ValueError, match="hold 2 rows"):
        nn.run(t(2, 169), t(1, 169), None, t(2, 169), io, io, io, 2, s)
    with pytest.raises(ValueError, match="inc_off"):
        nn.run(t(2, 169), t(1, 169), None, t(1, 169), io[:2], io, io, 1, s)


# --------------------------------------------------------------------------------------
# 2. set_rho: the next update is a freshly bound batch's, bitwise
# --------------------------------------------------------------------------------------
SET_N, SET_V, SET_APER = 13, 4, 3
STATE = ("x_ext", "d", "e", "y", "z")
SET_VARIANTS = {
    "plain": {},
    "weights": dict(ray_weights=True),
    "bounds": dict(bounds=(-0.25, 0.25)),
}


def _set_batch(dtype, rho, variant, keep_x):
    plan = make_plan(sr.graph_of("ring", SET_V), SET_V)
    rng = np.random.default_rng(5)
    b = {g: rng.standard_normal(SET_APER * SET_N) for g in plan.local_nodes}
    W, q_fn = sr.precisions(SET_N * SET_N, SET_V, 1)
    kw = dict(SET_VARIANTS[variant])
    if kw.pop("ray_weights", False):
        kw["ray_weights"] = [np.random.default_rng(9 + g).uniform(0.0, 2.0, SET_APER * SET_N) for g in range(SET_V)]
    return NodeBatch(ParallelBeamGeometry(SET_N, SET_APER), dtype, plan, b, q_fn, rho, sr.LAM, sr.MU, 2, 2, "iso", None, 0,
                     fusion="midpoint", Wi_list=W, keep_x=keep_x, derive_z=False, **kw)


def _read_update(nb):
    torch.cuda.synchronize()
    return {k: getattr(nb, k).cpu().numpy().copy() for k in ("x_ext", "d", "e", "node_stats")}


def _copy_state(dst, src):
    for k in STATE:
        getattr(dst, k).copy_(getattr(src, k))
    torch.cuda.synchronize()


@pytest.mark.parametrize("keep_x", [False, True], ids=["project", "keep_x"])
@pytest.mark.parametrize("variant", list(SET_VARIANTS))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_set_rho_then_update_is_bitwise_a_fresh_batch(cuda, monkeypatch, dtype, variant, keep_x):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    rho0, rho1 = 2.0, 0.5
    nb = _set_batch(dtype, rho0, variant, keep_x)
    for _ in range(2):  # warm state: two iterations
        nb.node_update()
        nb.consensus()
    torch.cuda.synchronize()
    y0, z0 = nb.y.clone(), nb.z.clone()
    assert float(y0.abs().max()) > 0
    nb.set_rho(rho1)
    assert nb.params["rho"] == rho1 and nb.cb.rho == rho1
    assert torch.equal(nb.y, y0 * (rho0 / rho1)) and torch.equal(nb.z, z0)  # the constraint rows f included
    fresh, old = _set_batch(dtype, rho1, variant, keep_x), _set_batch(dtype, rho0, variant, keep_x)
    _copy_state(fresh, nb)
    _copy_state(old, nb)
    for t in (nb, fresh, old):
        t.node_update()
    got, want = _read_update(nb), _read_update(fresh)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert not np.array_equal(_read_update(old)["x_ext"], want["x_ext"])  # and it is not the old rho's update
    # a second update (keep_x: the reuse start) stays bitwise
    nb.consensus()
    fresh.consensus()
    nb.node_update()
    fresh.node_update()
    got, want = _read_update(nb), _read_update(fresh)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert nb.set_rho(rho1) is None  # the same rho: nothing to do
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="rho"):
            nb.set_rho(bad)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_set_rho_back_and_forth_leaves_the_ray_weights_in_force(cuda, monkeypatch, dtype):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    nb = _set_batch(dtype, 2.0, "weights", True)
    nb.node_update()
    nb.consensus()
    nb.set_rho(8.0)
    nb.set_rho(2.0)
    fresh, plain = _set_batch(dtype, 2.0, "weights", True), _set_batch(dtype, 2.0, "plain", True)
    _copy_state(fresh, nb)
    _copy_state(plain, nb)
    for t in (nb, fresh, plain):
        t.node_update()
    got, want, unweighted = _read_update(nb), _read_update(fresh), _read_update(plain)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert not np.array_equal(got["x_ext"], unweighted["x_ext"])


# --------------------------------------------------------------------------------------
# 3. whole runs: 4-node ring, N = 33, 12 angles per node, sigma = 0.5, 10 iterations from rho_0 = 20
# --------------------------------------------------------------------------------------
RUN_N, RUN_V, RUN_APER, RUN_ITERS, RUN_NOISE, RUN_SEED = 33, 4, 12, 10, 0.5, 3
RHO0, LAM = 20.0, 0.02
GUARD = 1.05  # no decision of the reference may lie within this factor of its threshold
TOLS = dict(eps_abs=1e-4, eps_rel=3e-2)
TOL_ITERS = 12
EDGE_HIST = ("primal", "dual", "obj_total")
BOUND_HIST = EDGE_HIST + ("bound_primal", "bound_dual", "bound_violation")
VARIANTS = {
    "plain": dict(keys=EDGE_HIST),
    "bounds": dict(bounds=(0.0, 1.0), alpha=1.6, keys=BOUND_HIST),
    "weighted": dict(fusion="weighted", keys=EDGE_HIST),
}


def _problem(dtype, V=RUN_V):
    """Operators, phantom, precisions on the device; the sinograms made on the host (Joseph matrix,
    NumPy noise of RUN_SEED) so that the reference's decisions can be checked where the seed is chosen."""
    from admm_hip.data import make_precisions
    from admm_hip.solver import make_operators
    ops = make_operators(RUN_N, V, RUN_APER * V, dtype=dtype, device=0)
    A = joseph_matrix(Geometry(RUN_N, RUN_APER))
    ph = br.blocks_phantom(RUN_N)
    rng = np.random.default_rng(RUN_SEED)
    b = [A @ ph + RUN_NOISE * rng.standard_normal(A.shape[0]) for _ in range(V)]
    if dtype == "float32":  # the device and the reference read the same numbers
        b = [v.astype(np.float32).astype(np.float64) for v in b]
    Wi, Q = make_precisions(ops)
    return ops, A, ph, b, Wi, Q


def _run(dtype, variant="plain", V=RUN_V, iters=RUN_ITERS, adapt_rho=True, keys=None, **kw):
    from admm_hip.admm import run_admm
    ops, A, ph, b, Wi, Q = _problem(dtype, V)
    v = VARIANTS[variant]
    kw = dict(dict(lam_tv=LAM, rho=RHO0, eps_pri=0.0, eps_dual=0.0, max_iters=iters, verbose=False,
                   phantom_true=torch.from_numpy(ph.reshape(RUN_N, RUN_N)), write_params=False, bounds=v.get("bounds"),
                   fusion=v.get("fusion", "midpoint"), relaxation=v.get("alpha"), adapt_rho=adapt_rho), **kw)
    sinos = [s.reshape(RUN_APER, RUN_N) for s in b]
    x, h = run_admm(ops, sinos, nx.cycle_graph(V), Wi, Q, RUN_N, **kw)
    keys = v["keys"] if keys is None else keys
    return np.stack([_np(xi) for xi in x]), {k: np.asarray(h[k]) for k in keys}, h


def _robust(ratios):
    """A stop decision (every ratio residual / threshold < 1) no rounding can flip: some ratio is
    beyond GUARD, or all are below 1 / GUARD."""
    return max(ratios) >= GUARD or max(ratios) <= 1.0 / GUARD


@pytest.fixture(scope="module")
def run_ref():
    """{(dtype, variant, tolerances)}: (x, history) of penalty_ref.adaptive_admm on the Joseph matrix,
    after the assertion that none of its decisions is a close call."""
    cache = {}

    def get(dtype, variant, tols=False):
        key = (dtype, variant, tols)
        if key not in cache:
            ops, A, ph, b, Wi, Q = _problem(dtype)
            v = VARIANTS[variant]
            x, _, h = pr.adaptive_admm([A] * RUN_V, b, nx.cycle_graph(RUN_V), Q, RUN_N, adapt=True,
                                       alpha=v.get("alpha", 1.0), fusion=v.get("fusion", "midpoint"),
                                       Wi_list=[_np(w) for w in Wi], bounds=v.get("bounds"), lam_tv=LAM, rho=RHO0,
                                       max_iters=TOL_ITERS if tols else RUN_ITERS, phantom_true=ph,
                                       **(TOLS if tols else {}))
            for k, m1, m2 in h["margins"]:  # every balancing decision, on the reference
                assert not (1.0 / GUARD <= m1 <= GUARD) and not (1.0 / GUARD <= m2 <= GUARD), (k, m1, m2)
            if tols:
                r = np.hypot(h["primal"], h["bound_primal"]) if "bound_primal" in h else np.asarray(h["primal"])
                s = np.hypot(h["dual"], h["bound_dual"]) if "bound_dual" in h else np.asarray(h["dual"])
                for k in range(len(r)):
                    assert _robust((r[k] / h["eps_pri_history"][k], s[k] / h["eps_dual_history"][k])), k
            cache[key] = (np.stack(x), {k: np.asarray(h[k]) for k in h if k != "margins"})
        return cache[key]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_adaptive_run_matches_reference(cuda, monkeypatch, run_ref, dtype, variant):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    x, h, full = _run(dtype, variant)
    xo, ho = run_ref(dtype, variant)
    errs = {"images": rel(x, xo), **{k: rel(h[k], ho[k]) for k in h}}
    print(f"\nADAPTIVE RUN {dtype} {variant}: rho {list(full['rho_history'])}; "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert full["rho_history"] == list(ho["rho_history"]) and len(set(full["rho_history"][:4])) > 1
    assert len(h["primal"]) == RUN_ITERS and not set(NORM_KEYS) & set(full)
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)


@pytest.mark.parametrize("variant", ["plain", "bounds"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_run_with_tolerances_stops_where_the_reference_stops(cuda, monkeypatch, run_ref, dtype, variant):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    # eps_pri / eps_dual are not consulted: values that would stop the absolute test at once
    x, h, full = _run(dtype, variant, iters=TOL_ITERS, keys=VARIANTS[variant]["keys"] + NORM_KEYS, eps_pri=1e9,
                      eps_dual=1e9, **TOLS)
    xo, ho = run_ref(dtype, variant, tols=True)
    stop = len(ho["primal"])
    errs = {"images": rel(x, xo), **{k: rel(h[k], ho[k]) for k in h}}
    print(f"\nTOLERANCE RUN {dtype} {variant}: stops after {len(h['primal'])} (reference {stop}) of {TOL_ITERS}; "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert 1 < stop < TOL_ITERS and len(h["primal"]) == stop
    assert full["rho_history"] == list(ho["rho_history"])
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)


def test_tolerances_alone_keep_rho_and_the_fixed_rho_trajectory(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    keys = EDGE_HIST + ("pri_per_node", "dual_per_node")
    x0, h0, _ = _run("float32", iters=4, adapt_rho=None, keys=keys)
    x1, h1, full = _run("float32", iters=4, adapt_rho=None, keys=keys, eps_abs=1e-12, eps_rel=1e-12)
    assert "rho_history" not in full and all(len(full[k]) == 4 for k in NORM_KEYS)
    assert np.array_equal(x0, x1)
    for k in keys:
        assert np.array_equal(h0[k], h1[k]), k


@pytest.mark.parametrize("variant", ["bounds", "weighted"])
def test_streams_split_is_bitwise_one_batch(cuda, monkeypatch, variant):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}
    keys = VARIANTS[variant]["keys"] + NORM_KEYS + ("rho_history",)
    kw = dict(V=8, iters=4, keys=keys, eps_abs=1e-12, eps_rel=1e-12)
    x1, h1, _ = _run("float64", variant, inspect=lambda rg: seen.setdefault(1, len(rg.batches)), **kw)
    x2, h2, _ = _run("float64", variant, streams=2, inspect=lambda rg: seen.setdefault(2, len(rg.batches)), **kw)
    assert seen == {1: 1, 2: 2} and len(set(h1["rho_history"])) > 1
    assert np.array_equal(x1, x2)
    for k in keys:
        assert np.array_equal(h1[k], h2[k]), k


RANK_KEYS = BOUND_HIST + NORM_KEYS + ("rho_history",)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, h, _ = _run("float32", "bounds", iters=4, keys=RANK_KEYS, eps_abs=1e-12, eps_rel=1e-12)
        q.put((rank, (x, h)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_one_rank_bitwise(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EXCHANGE_OVERLAP", raising=False)
    x1, h1, _ = _run("float32", "bounds", iters=4, keys=RANK_KEYS, eps_abs=1e-12, eps_rel=1e-12)
    assert len(set(h1["rho_history"])) > 1
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
        x2, h2 = res[r]
        assert np.array_equal(x1, x2), r
        for k in h1:
            assert np.array_equal(h1[k], h2[k]), (k, r)


# --------------------------------------------------------------------------------------
# 4. off is off; the refusals
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "bounds"])
def test_none_is_the_run_without_the_keywords(cuda, monkeypatch, variant):
    from admm_hip.admm import run_admm
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    ops, A, ph, b, Wi, Q = _problem("float32")
    v = VARIANTS[variant]
    kw = dict(lam_tv=LAM, rho=RHO0, eps_pri=0.0, eps_dual=0.0, max_iters=3, verbose=False, write_params=False,
              phantom_true=torch.from_numpy(ph.reshape(RUN_N, RUN_N)), bounds=v.get("bounds"))
    args = (ops, [s.reshape(RUN_APER, RUN_N) for s in b], nx.cycle_graph(RUN_V), Wi, Q, RUN_N)
    seen = []
    look = lambda rg: seen.append([(nb.norms, nb.norm_stats, rg.stop_norms) for nb in rg.batches])  # noqa: E731
    x0, h0 = run_admm(*args, **kw)
    x, h = run_admm(*args, adapt_rho=None, eps_abs=None, eps_rel=None, inspect=look, **kw)
    assert set(h) == set(h0) and not {"rho_history", *NORM_KEYS} & set(h)
    assert all(np.array_equal(_np(a), _np(c)) for a, c in zip(x, x0))
    for k in h0:
        assert np.array_equal(np.asarray(h[k]), np.asarray(h0[k]), equal_nan=True), k
    assert seen == [[(None, None, False)]]  # no scratch either
    _, hf = run_admm(*args, adapt_rho=False, **kw)
    assert set(hf) == set(h0)


def test_tolerances_with_derived_z_are_refused_and_adapt_rho_is_not(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    with pytest.raises(ValueError, match="stored z"):
        _run("float32", iters=1, adapt_rho=None, edge_state="derived", **TOLS)
    import admm_hip.groups as groups
    with monkeypatch.context() as m:
        m.setattr(groups, "z_is_stored", lambda *a, **k: False)
        with pytest.raises(ValueError, match="eps_abs / eps_rel need stored z.*stored-z rule"):
            _run("float32", iters=1, adapt_rho=None, **TOLS)
    # balancing alone runs on derived z, with the same decisions and (to rounding) the same run
    seen = []
    xs, hs, fs = _run("float64", iters=5)
    xd, hd, fd = _run("float64", iters=5, edge_state="derived", inspect=lambda rg: seen.append(rg.derive_z))
    assert seen == [True] and fd["rho_history"] == fs["rho_history"] and len(set(fd["rho_history"])) > 1
    assert rel(xd, xs) < 1e-9 and rel(hd["primal"], hs["primal"]) < 1e-9
