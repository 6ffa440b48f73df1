"""GPU: bound constraints lo <= x <= hi (admm_bound_project, NodeBatch(bounds=...), run_admm's
``bounds`` / ``bound_weight`` / ``return_feasible``; references: tests/bounds_ref.py on the
unchanged oracle).

* the kernel alone: w' and f' bitwise a NumPy restatement (planted ties, neighbours of the bounds,
  +-0), the three sums against math.fsum, batch / position / stride invariance;
* one x-update from a random warm state with random w, f, q_c, per pixel and per statistic, with
  the bars of test_gpu_state_update.py;
* a whole run against bounds_ref at the project's gates, pipelined = per-iteration, streams=2 and
  two gloo ranks bitwise one rank, a start from FBP, feasible images;
* an infinite box on the device; the error paths.

Run with ``-s`` to see every case's measured errors.
"""
import math
import os
import socket

import networkx as nx
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import bounds_ref as br
import state_ref as sr
from admm_hip.bounds import BoundProjector, Bounds, check_bounds
from admm_hip.geometry import ParallelBeamGeometry, current_stream_handle
from admm_hip.solver import NodeBatch
from oracle.geometry import Geometry, joseph_matrix
from test_gpu_state_update import _compare, _read, _set_mirror

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
RUN_TOL = {"float32": 1e-5, "float64": 1e-9}
SUM_TOL = 1e-13  # the consensus tests' bar for a fixed-order float64 sum against math.fsum


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _np(v):
    return v.detach().cpu().numpy().astype(np.float64) if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)


# --------------------------------------------------------------------------------------
# 1. the kernel alone
# --------------------------------------------------------------------------------------
def _form(form, n, rng):
    """The checked box of a bound form for n = side^2 pixels."""
    side = int(round(math.sqrt(n)))
    if form == "scalar":
        return check_bounds((0.0, 1.0), side)
    if form == "lo-only":
        return check_bounds((0.0, math.inf), side)
    if form == "hi-only":
        return check_bounds((None, 1.0), side)
    sup = np.zeros((side, side), dtype=bool)  # a support mask: hi = 0 outside, with lo = 0 the pixel is pinned
    sup[side // 5: side - side // 6, side // 7: side - side // 4] = True
    sup = sup.reshape(-1)
    sup[:8] = True  # (the planted pixels keep an interval)
    lo_map = np.where(sup, rng.uniform(-0.5, 0.2, n), -1.0)  # under the scalar lo = 0 on part of the support
    lo_map[6:8] = -1.0  # (l = 0 at the planted +-0)
    # scalars and maps together: the kernel takes the max / min of both
    B = Bounds(0.0, 2.0, lo_map, np.where(sup, 1.0, 0.0))
    assert np.all(np.less_equal(*B.arrays(n)))
    return B


def _kernel_case(n, nimg, form, seed=0):
    rng = np.random.default_rng([seed, n, nimg])
    B = _form(form, n, rng)
    l, h = B.arrays(n)
    x = rng.uniform(-1.0, 2.0, (nimg, n))
    f = 0.3 * rng.standard_normal((nimg, n))
    w = rng.uniform(-0.5, 1.5, (nimg, n))
    # planted in every image's first pixels: t = x + f exactly a tie, a neighbour of a bound, +-0
    for v in range(nimg):
        tgt = [l[0], h[1], np.nextafter(l[2], -np.inf), np.nextafter(l[3], np.inf), np.nextafter(h[4], -np.inf),
               np.nextafter(h[5], np.inf), 0.0, -0.0]
        own = [l[0], h[1], l[2], l[3], h[4], h[5], 0.0, 0.0]  # the bound each one is planted at
        for p, t in enumerate(tgt):
            if np.isfinite(own[p]):  # (a side that is off has no tie to plant)
                x[v, p], f[v, p] = t, (-0.0 if np.signbit(t) else 0.0)
    return B, l, h, x, w, f


def _project(B, x, w, f, dev):
    """One projection through BoundProjector of host arrays; returns host w', f', sums."""
    n = x.shape[1]
    pr = BoundProjector(B, n, dev, x.shape[0])
    xd, wd, fd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, w, f))
    s = pr.run(xd, wd, fd, current_stream_handle(dev))
    torch.cuda.synchronize()
    return wd.cpu().numpy(), fd.cpu().numpy(), s.cpu().numpy().copy()


@pytest.mark.parametrize("form", ["scalar", "lo-only", "hi-only", "maps"])
@pytest.mark.parametrize("nimg", [1, 3, 8])
@pytest.mark.parametrize("n", [169, 1089, 4096])
def test_projection_is_bitwise_the_numpy_restatement(cuda, n, nimg, form):
    B, l, h, x, w, f = _kernel_case(n, nimg, form)
    wn, fn, sums = _project(B, x, w, f, cuda)
    wr_, fr_, sr_ = br.project_ref(x, w, f, l, h)
    assert np.array_equal(bits(wn), bits(wr_)), int(np.sum(bits(wn) != bits(wr_)))
    assert np.array_equal(bits(fn), bits(fr_)), int(np.sum(bits(fn) != bits(fr_)))
    assert np.all(wn >= l) and np.all(wn <= h)
    if form in ("scalar", "maps"):  # t = -0 with l = 0 stays -0, and f' = -0 - -0 = +0
        assert np.all(np.signbit(wn[:, 7])) and not np.any(np.signbit(wn[:, 6])) and not np.any(np.signbit(fn[:, 7]))
        assert np.all(wn[:, 2] == l[2]) and np.all(fn[:, 2] < 0) and np.all(wn[:, 5] == h[5]) and np.all(fn[:, 5] > 0)
        assert np.all(wn[:, 3] == np.nextafter(l[3], np.inf)) and np.all(wn[:, 4] == np.nextafter(h[4], -np.inf))
    err = np.abs(sums - sr_) / np.maximum(np.abs(sr_), 1e-300)
    print(f"\nPROJ n={n} nimg={nimg} {form}: sums rel err max {err.max():.1e}")
    assert np.all(sr_ > 0) and err.max() <= SUM_TOL, err


@pytest.mark.parametrize("form", ["scalar", "maps"])
def test_an_images_outputs_do_not_depend_on_batch_position_or_strides(cuda, form):
    n, nimg = 1089, 8  # odd rows: 8-byte aligned only
    B, l, h, x, w, f = _kernel_case(n, nimg, form, seed=1)
    full = _project(B, x, w, f, cuda)
    for v in (0, 3, 7):  # alone
        one = _project(B, x[v:v + 1], w[v:v + 1], f[v:v + 1], cuda)
        for a, b in zip(one, full):
            assert np.array_equal(bits(a[0]), bits(b[v])), v
    perm = [5, 0, 7, 2]  # other positions in a smaller batch
    sub = _project(B, x[perm], w[perm], f[perm], cuda)
    for k, v in enumerate(perm):
        for a, b in zip(sub, full):
            assert np.array_equal(bits(a[k]), bits(b[v])), v
    # strided views: x rows n + 7 apart, w and f rows n + 13 apart (every second row odd-aligned)
    pr = BoundProjector(B, n, cuda, nimg)
    xb = torch.full((nimg, n + 7), 9.0, dtype=torch.float64, device=cuda)
    wb = torch.full((nimg, n + 13), 9.0, dtype=torch.float64, device=cuda)
    fb = torch.full((nimg, n + 13), 9.0, dtype=torch.float64, device=cuda)
    xb[:, :n], wb[:, :n], fb[:, :n] = (torch.from_numpy(a).to(cuda) for a in (x, w, f))
    s = pr.run(xb[:, :n], wb[:, :n], fb[:, :n], current_stream_handle(cuda))
    torch.cuda.synchronize()
    assert np.array_equal(bits(wb[:, :n].cpu().numpy()), bits(full[0]))
    assert np.array_equal(bits(fb[:, :n].cpu().numpy()), bits(full[1]))
    assert np.array_equal(bits(s.cpu().numpy()), bits(full[2]))
    assert torch.all(wb[:, n:] == 9.0) and torch.all(fb[:, n:] == 9.0) and torch.all(xb[:, n:] == 9.0)  # the gaps
    assert torch.equal(xb[:, :n].cpu(), torch.from_numpy(x))  # x is only read


def test_projection_argument_errors(cuda):
    import ctypes as C

    from admm_hip import _lib
    lib = _lib.load()
    need = C.c_longlong()
    assert lib.admm_bound_project_work(1089, 3, C.byref(need)) == 0 and need.value == 3 * 2 * 3
    assert lib.admm_bound_project_work(0, 3, C.byref(need)) != 0
    assert lib.admm_bound_project_work(1089, 0, C.byref(need)) != 0
    x, w, f = (torch.zeros((2, 64), dtype=torch.float64, device=cuda) for _ in range(3))
    work, out = (torch.zeros(6, dtype=torch.float64, device=cuda) for _ in range(2))
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    z = C.c_void_p(0)
    s = C.c_void_p(current_stream_handle(cuda))
    ok = (p(x), 64, p(w), p(f), 64, z, z, 0.0, 1.0, 64, 2, p(work), p(out), s)
    # every call below is refused before any launch
    for i, bad in ((0, z), (2, z), (3, z), (11, z), (12, z), (1, 63), (4, 63), (7, 2.0), (7, float("nan")), (10, 0)):
        args = list(ok)
        args[i] = bad
        assert lib.admm_bound_project(*args) != 0, i
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------
# 2. one x-update from random warm states: random w, f, q_c
# --------------------------------------------------------------------------------------
def _batch(case, dtype, P, keep_x=False):
    geom = ParallelBeamGeometry(case.N, case.a_per)
    nb = NodeBatch(geom, dtype, P["plan"], P["b"], P["q_fn"], sr.RHO, sr.LAM, sr.MU, case.tv_iters, case.cg_iters,
                   case.tv_kind, P["ph"], 0, fusion="midpoint", Wi_list=P["W"], keep_x=keep_x, derive_z=False,
                   bounds=br.UPDATE_BOUNDS)
    if case.mirror is not None:
        assert nb.mirror == (case.mirror == "1")
    E, V = len(P["plan"].stored_edges), P["plan"].V
    assert nb.y.shape[0] == nb.z.shape[0] == E + V and nb.cb.n_edges == E + V
    assert nb.edge_a[E:E + V].tolist() == nb.edge_b[E:E + V].tolist() == list(range(V))
    return nb


def _oracle(P, A, dtype=np.float64):
    return lambda s: br.oracle_update_bounded(s, P["plan"], A, P["b"], P["q_fn"], P["W"], P["prm"], dtype=dtype,
                                              phantom=P["ph"])


def _bars(dtype, ref, run32):
    if dtype == "float64":
        return {"x": sr.F64_BAR, "d": sr.F64_BAR, "e": sr.F64_BAR, "stats": np.full(6, sr.F64_BAR)}, None
    y = sr.yardstick(ref, run32())
    return {k: sr.F32_FACTOR * v for k, v in y.items()}, y


def _only_read(nb, st, q0):
    """What the x-update must only read: y and z (the w and f rows included), q -- bitwise."""
    torch.cuda.synchronize()
    assert np.array_equal(nb.y.cpu().numpy(), st["y"]) and np.array_equal(nb.z.cpu().numpy(), st["z"])
    assert torch.equal(nb.q, q0)
    assert np.array_equal(nb.x_ext[nb.V:].cpu().numpy(), st["x_ext"][nb.V:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", br.BOUND_CASES, ids=sr.case_id)
def test_bounded_update_from_random_state(cuda, monkeypatch, case, dtype):
    _set_mirror(monkeypatch, case.mirror)
    P = sr.case_problem(case, dtype)
    nb = _batch(case, dtype, P)
    q0 = nb.q.clone()
    st = br.random_state(nb, case.seed)
    nb.node_update()
    got = _read(nb)
    ref = _oracle(P, P["A"])(st)
    bars, yard = _bars(dtype, ref, lambda: _oracle(P, sr.as_f32_matrix(P["A"]), np.float32)(st))
    _compare(dtype + " bounded", case, dtype, got, ref, bars, yard)
    _only_read(nb, st, q0)
    # D includes q_c, in the reference's order
    E = len(P["plan"].stored_edges)
    k = P["plan"].V - 1
    D = np.zeros(P["n"])
    for s in range(P["plan"].inc_off[k], P["plan"].inc_off[k + 1]):
        D += P["q_fn"](P["plan"].local_nodes[k], P["plan"].inc_nbr[s])
    D += P["W"][P["plan"].local_nodes[k]]
    assert np.array_equal(nb.dsum[k].cpu().numpy(), D) and E + k < nb.z.shape[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", br.BOUND_REUSE_CASES, ids=sr.case_id)
def test_bounded_reuse_start(cuda, monkeypatch, case, dtype):
    """ADMM_BATCH_KEEP_X: the second update starts from the first one's A^T (A x - b) and reads the
    constraint incidence in k_start_reuse."""
    _set_mirror(monkeypatch, case.mirror)
    P = sr.case_problem(case, dtype)
    nb = _batch(case, dtype, P, keep_x=True)
    q0 = nb.q.clone()
    st0 = br.random_state(nb, case.seed)
    nb.node_update()
    st1 = br.random_state(nb, case.seed + 1000, keep_x=True)
    nb.node_update()
    got = _read(nb)
    _only_read(nb, st1, q0)
    two = lambda run: run(sr.continue_state(st0, run(st0), **br.rerandomised(P["plan"], P["n"], case)))  # noqa: E731
    ref = two(_oracle(P, P["A"]))
    bars, yard = _bars(dtype, ref, lambda: two(_oracle(P, sr.as_f32_matrix(P["A"]), np.float32)))
    _compare(dtype + " bounded reuse", case, dtype, got, ref, bars, yard)


def test_set_precisions_keeps_q_c_and_recomputes_d(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    case = br.BOUND_CASES[1]
    P = sr.case_problem(case, "float64")
    nb = _batch(case._replace(mirror=None), "float64", P)
    plan = P["plan"]
    qc0, d0 = nb.q[nb.n_qslots:].clone(), nb.dsum.clone()
    qs = [2.0 * P["q_fn"](g, plan.inc_nbr[s]) for k, g in enumerate(plan.local_nodes)
          for s in range(plan.inc_off[k], plan.inc_off[k + 1])]
    nb.set_precisions(qs)
    assert torch.equal(nb.q[nb.n_qslots:], qc0)
    want = 2.0 * (d0 - qc0) + qc0
    assert float((nb.dsum - want).abs().max()) < 1e-12 and not torch.equal(nb.dsum, d0)
    st = br.random_state(nb, 3)
    nb.node_update()
    q2 = lambda i, j: 2.0 * P["q_fn"](i, j)  # noqa: E731
    ref = br.oracle_update_bounded(st, plan, P["A"], P["b"], q2, P["W"], P["prm"], phantom=P["ph"])
    assert sr.field_err(_read(nb)["x"], ref["x"])[0] <= sr.F64_BAR


# --------------------------------------------------------------------------------------
# 3. whole run: 4-node ring, N = 33, 12 angles per node, bounds [0, 1], 10 iterations
# --------------------------------------------------------------------------------------
# (the sparse-view, noisy regime: a phantom in {0, 1} and noise sigma = 0.5, so that the unconstrained
# images leave the box and about half of w's pixels end on a bound)
RUN_N, RUN_V, RUN_APER, RUN_ITERS, RUN_NOISE = 33, 4, 12, 10, 0.5
HIST = ("primal", "dual", "bound_primal", "bound_dual", "bound_violation")
RUN_KW = dict(lam_tv=0.02, rho=2.0, eps_pri=0.0, eps_dual=0.0)


def _run_problem(dtype, V=RUN_V):
    from admm_hip.data import make_precisions, make_sinograms
    from admm_hip.solver import make_operators
    ops = make_operators(RUN_N, V, RUN_APER * V, dtype=dtype, device=0)
    ph = torch.from_numpy(br.blocks_phantom(RUN_N).reshape(RUN_N, RUN_N))
    sinos = make_sinograms(ops, ph, RUN_NOISE, seed=1000)
    Wi, Q = make_precisions(ops)
    return ops, ph, sinos, Wi, Q


def _run(dtype, V=RUN_V, iters=RUN_ITERS, via="run_admm", bounds=(0.0, 1.0), keys=HIST, **kw):
    ops, ph, sinos, Wi, Q = _run_problem(dtype, V)
    args = (ops, sinos, nx.cycle_graph(V), Wi, Q, RUN_N)
    kw = dict(RUN_KW, max_iters=iters, verbose=False, phantom_true=ph, write_params=False, bounds=bounds, **kw)
    if via == "dropin":
        from block_6_admm_loop_ver2 import decentralized_admm
        x, h = decentralized_admm(*args, **kw)
    else:
        from admm_hip.admm import run_admm
        x, h = run_admm(*args, **kw)
    return np.stack([_np(xi) for xi in x]), {k: np.asarray(h[k]) for k in keys}, h


@pytest.fixture(scope="module")
def run_ref():
    """{dtype: (x, w, history)} of bounds_ref on the Joseph matrix and the device's sinograms."""
    cache = {}

    def get(dtype, x_init=None, key=None):
        key = key or dtype
        if key not in cache:
            ops, ph, sinos, Wi, Q = _run_problem(dtype)
            A = joseph_matrix(Geometry(RUN_N, RUN_APER))
            b = [_np(s).reshape(-1) for s in sinos]
            x, w, f, h = br.bounded_admm([A] * RUN_V, b, nx.cycle_graph(RUN_V), Q, [_np(v) for v in Wi], RUN_N,
                                         (0.0, 1.0), max_iters=RUN_ITERS, phantom_true=_np(ph), x_init=x_init,
                                         **RUN_KW)
            cache[key] = (np.stack(x), np.stack(w), {k: np.asarray(h[k]) for k in HIST + ("obj_total",)})
        return cache[key]
    return get


@pytest.mark.parametrize("via", ["run_admm", "dropin"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bounded_run_matches_reference(cuda, monkeypatch, run_ref, dtype, via):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    x, h, full = _run(dtype, via=via, keys=HIST + ("obj_total",))
    xo, wo, ho = run_ref(dtype)
    on = float(np.mean((wo == 0.0) | (wo == 1.0)))
    errs = {"images": rel(x, xo), **{k: rel(h[k], ho[k]) for k in ho}}
    print(f"\nRUN {dtype} {via}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" | reference pixels on a bound {on:.2f}, violation {ho['bound_violation'][0]:.3f} -> "
          f"{ho['bound_violation'][-1]:.3f}")
    assert on > 0.25  # the constraint is active on a large part of the image
    assert len(full["bound_pri_per_node"]) == RUN_ITERS and full["bound_pri_per_node"][0].shape == (RUN_V,)
    assert math.isclose(math.sqrt(float(np.sum(full["bound_violation_per_node"][-1]))), full["bound_violation"][-1])
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pipelined_and_per_iteration_histories_are_equal(cuda, monkeypatch, dtype):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    keys = HIST + ("obj_total", "bound_pri_per_node", "bound_violation_per_node", "psnr_mean")
    xa, ha, _ = _run(dtype, iters=4, keys=keys, metrics=("psnr",))
    xb, hb, _ = _run(dtype, iters=4, keys=keys, metrics=("psnr",), pipeline=False)
    assert np.array_equal(xa, xb)
    for k in keys:
        assert np.array_equal(ha[k], hb[k]), k
    assert ha["bound_primal"].shape == (4,) and np.all(ha["bound_primal"] > 0)


def test_stop_test_waits_for_the_constraint(cuda, monkeypatch):
    """The run stops at the first iteration at which the edge residuals and the constraint's pass."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    _, hb, _ = _run("float64", iters=6)

    eps_p = 1.0001 * float(hb["primal"][3])
    ok = (hb["primal"] < eps_p) & (hb["bound_primal"] < eps_p)
    first = int(np.argmax(ok))
    print(f"\nSTOP: eps_pri={eps_p:.3e} primal={hb['primal']} bound_primal={hb['bound_primal']} first={first}")
    assert ok.any()
    _, h, _ = _run("float64", iters=6, eps_pri=eps_p, eps_dual=1e9)
    assert len(h["primal"]) == first + 1, (len(h["primal"]), first)
    assert np.array_equal(h["bound_primal"], hb["bound_primal"][: first + 1])


def test_streams_split_is_bitwise_one_batch(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}
    x1, h1, _ = _run("float64", V=8, iters=3, inspect=lambda rg: seen.setdefault(1, len(rg.batches)))
    x2, h2, _ = _run("float64", V=8, iters=3, streams=2, inspect=lambda rg: seen.setdefault(2, len(rg.batches)))
    assert seen == {1: 1, 2: 2}
    assert np.array_equal(x1, x2)
    for k in HIST:
        assert np.array_equal(h1[k], h2[k]), k


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, h, _ = _run("float32", iters=4, return_feasible=True)
        q.put((rank, (x, h)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_one_rank_bitwise(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    x1, h1, _ = _run("float32", iters=4, return_feasible=True)
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


def test_run_from_fbp_matches_reference(cuda, monkeypatch, run_ref):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    from admm_hip.fbp import fbp
    dtype = "float64"
    ops, ph, sinos, Wi, Q = _run_problem(dtype)
    start = [_np(fbp(ops[g], sinos[g].reshape(-1), "ram-lak")).reshape(-1) for g in range(RUN_V)]
    assert min(float(s.min()) for s in start) < 0.0  # the start itself leaves the box: w = clip(x) matters
    x, h, _ = _run(dtype, x_init="fbp")
    xo, wo, ho = run_ref(dtype, x_init=start, key="fbp")
    errs = {"images": rel(x, xo), **{k: rel(h[k], ho[k]) for k in HIST}}
    print("\nRUN fbp start: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)
    x0, _, _ = run_ref(dtype)
    assert rel(x, x0) > 1e-3  # and the start matters after 10 iterations


@pytest.mark.parametrize("dtype", DTYPES)
def test_feasible_images_lie_in_the_box_exactly(cuda, monkeypatch, run_ref, dtype):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}

    def inspect(rg):
        nb = rg.batches[0]
        seen["w"], seen["x"] = nb.w_bound.cpu().numpy().copy(), nb.x_local.cpu().numpy().copy()

    w, _, _ = _run(dtype, return_feasible=True, inspect=inspect)
    x, _, _ = _run(dtype)
    assert w.min() >= 0.0 and w.max() <= 1.0 and (w == 0.0).any() and (w == 1.0).any()
    assert x.min() < 0.0  # x itself is only feasible in the limit
    assert np.array_equal(w, seen["w"]) and np.array_equal(x, seen["x"])
    assert rel(w, run_ref(dtype)[1]) < RUN_TOL[dtype]
    wt, _, _ = _run(dtype, return_feasible=True, return_tensors=True)
    assert np.array_equal(wt, w)


# --------------------------------------------------------------------------------------
# 4. an infinite box; a support mask; the error paths
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_box_keeps_f_zero_and_w_equal_to_x(cuda, monkeypatch, dtype):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}

    def inspect(rg):
        nb = rg.batches[0]
        seen.update(w=nb.w_bound.cpu().numpy(), f=nb.f_bound.cpu().numpy(), x=nb.x_local.cpu().numpy())

    _, h, _ = _run(dtype, iters=4, bounds=(-math.inf, math.inf), inspect=inspect)
    assert not bits(seen["f"]).any()  # +0 in every bit
    assert np.array_equal(bits(seen["w"]), bits(seen["x"])) and seen["x"].min() < 0.0
    assert not h["bound_violation"].any() and not h["bound_primal"].any()
    seen2 = {}
    _run(dtype, iters=4, bounds=(None, None), inspect=lambda rg: seen2.update(x=rg.batches[0].x_local.cpu().numpy()))
    assert np.array_equal(seen["x"], seen2["x"])


def test_support_mask_pins_the_outside_to_zero(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    yy, xx = np.mgrid[:RUN_N, :RUN_N]
    sup = ((yy - 16) ** 2 + (xx - 16) ** 2 <= 15 ** 2).astype(np.float64)
    w, h, _ = _run("float32", iters=5, bounds=(0.0, torch.from_numpy(sup)), return_feasible=True)
    out = sup.reshape(-1) == 0
    assert not w[:, out].any() and w.min() >= 0.0 and w[:, ~out].max() > 0.5
    assert h["bound_violation"][-1] < h["bound_violation"][0]


def test_unsupported_combinations_raise_value_error(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    for kw in (dict(edge_state="derived"), dict(fusion="weighted"), dict(bounds=(1.0, 0.0)),
               dict(bounds=(0.0, np.full(RUN_N * RUN_N, np.nan))), dict(bound_weight=-1.0)):
        with pytest.raises(ValueError):
            _run("float32", iters=1, **kw)
    monkeypatch.setenv("ADMM_EDGE_STATE", "derived")
    with pytest.raises(ValueError, match="stored z"):
        _run("float32", iters=1)
    monkeypatch.delenv("ADMM_EDGE_STATE")
    with pytest.raises(ValueError):
        _run("float32", iters=1, bounds=None, return_feasible=True)
    # the batch itself refuses them too, and the HBM rule's derived choice
    case = br.BOUND_CASES[1]
    P = sr.case_problem(case, "float32")
    mk = lambda **kw: NodeBatch(ParallelBeamGeometry(case.N, case.a_per), "float32", P["plan"], P["b"], P["q_fn"],  # noqa: E731
                                sr.RHO, sr.LAM, sr.MU, 2, 3, "iso", P["ph"], 0, Wi_list=P["W"], **kw)
    for kw in (dict(derive_z=True), dict(fusion="weighted"), dict(bound_weight=0.0)):
        with pytest.raises(ValueError):
            mk(bounds=(0.0, 1.0), **kw)
    with pytest.raises(ValueError):
        mk(bound_weight=2.0)  # without bounds
    import admm_hip.solver as solver
    monkeypatch.setattr(solver, "z_is_stored", lambda *a, **k: False)
    with pytest.raises(ValueError, match="stored-z rule"):
        mk(bounds=(0.0, 1.0))


def test_no_bounds_means_no_slot_no_column_no_key(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}

    def inspect(rg):
        nb = rg.batches[0]
        seen.update(rows=nb.z.shape[0], E=len(nb.plan.stored_edges), n_edges=nb.cb.n_edges, proj=nb.projector,
                    width=rg.node_stat_width, q=nb.q.shape[0])

    _, _, h = _run("float32", iters=2, bounds=None, keys=("primal",), inspect=inspect)
    assert seen["rows"] == seen["E"] == seen["n_edges"] == RUN_V and seen["proj"] is None and seen["width"] == 6
    assert not set(br.BOUND_KEYS) & set(h)
    _, _, hb = _run("float32", iters=2, keys=("primal",), inspect=inspect)
    assert seen["rows"] == seen["n_edges"] == 2 * RUN_V and seen["width"] == 9 and set(br.BOUND_KEYS) <= set(hb)
