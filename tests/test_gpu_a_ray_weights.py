"""GPU: per-ray weights of the data term, 1/2 sum_r w_r (A x - b)_r^2 (admm_batch_set_ray_weights,
admm_column_norms_sq_weighted; references: tests/weights_ref.py on the unchanged oracle).

* one x-update from a random warm state per pixel and per statistic, with the bars of
  test_gpu_state_update.py (float64 1e-9; float32 4 x the case's float32-emulation yardstick), over
  padded lanes, a second lane block, more than one chunk, mirror on / off / an odd angle count,
  the ungrouped k_fwd, iso / aniso, and the keep_x start of a second update;
* w = 1 is bitwise the unweighted batch, statistics included, over two updates;
* bitwise invariances: the batch width, the other nodes' weights, clearing the weights, a re-bind
  by set_precisions;
* A^T (w b) and the weighted column norms against the Joseph matrix;
* a whole run (run_admm and the decentralized_admm drop-in) against the oracle on row-scaled
  matrices, and two gloo ranks on one GPU against one rank, bitwise;
* a node with every second view zeroed against a batch on the geometry of the remaining views.

Run with ``-s`` to see every case's device / yardstick ratios.
"""
import math
import os
import socket

import networkx as nx
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import state_ref as sr
import weights_ref as wr
from admm_hip.geometry import ParallelBeamGeometry, RayTransform
from admm_hip.plan import make_plan
from admm_hip.solver import NodeBatch
from oracle.geometry import Geometry, joseph_matrix
from test_gpu_state_update import _compare, _read, _set_mirror, _untouched

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
PROJ_TOL = {"float32": 2e-6, "float64": 1e-12}  # tests/test_gpu_projector.py
RUN_TOL = {"float32": 1e-5, "float64": 1e-9}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def _batch(case, dtype, P, w, keep_x=False, dwf=1.0, plan=None, b=None):
    geom = ParallelBeamGeometry(case.N, case.a_per, dwf)
    plan = plan or P["plan"]
    wl = None if w is None else [w.get(g) for g in range(max(plan.local_nodes) + 1)]
    nb = NodeBatch(geom, dtype, plan, b or P["b"], P["q_fn"], sr.RHO, sr.LAM, sr.MU, case.tv_iters, case.cg_iters,
                   case.tv_kind, P["ph"], 0, fusion=case.fusion, Wi_list=P["W"], keep_x=keep_x,
                   derive_z=case.derive_z, ray_weights=wl)
    if case.mirror is not None and dwf == 1.0:
        assert nb.mirror == (case.mirror == "1")
    return nb


def _bars(case, dtype, P, ref, run32):
    if dtype == "float64":
        return {"x": sr.F64_BAR, "d": sr.F64_BAR, "e": sr.F64_BAR, "stats": np.full(6, sr.F64_BAR)}, None
    y = sr.yardstick(ref, run32())
    return {k: sr.F32_FACTOR * v for k, v in y.items()}, y


def _oracle(P, case, A, dtype=np.float64):
    return lambda s: wr.oracle_update_weighted(s, P["plan"], A, P["b"], P["w"], P["q_fn"], P["prm"], case.fusion,
                                               dtype=dtype, phantom=P["ph"])


# --------------------------------------------------------------------------------------
# 5. one x-update per pixel
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", wr.WEIGHT_CASES, ids=sr.case_id)
def test_weighted_update_from_random_state(cuda, monkeypatch, case, dtype):
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, dtype)
    nb = _batch(case, dtype, P, P["w"])
    st = sr.random_state(nb, case.seed)
    nb.node_update()
    got = _read(nb)
    ref = _oracle(P, case, P["A"])(st)
    bars, yard = _bars(case, dtype, P, ref, lambda: _oracle(P, case, sr.as_f32_matrix(P["A"]), np.float32)(st))
    _compare(dtype + " weighted", case, dtype, got, ref, bars, yard)
    _untouched(nb, st)
    # the weights change the answer: the unweighted oracle is far outside the bars
    plain = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
    assert sr.field_err(got["x"], plain["x"])[0] > 1e-3


@pytest.mark.parametrize("dtype", DTYPES)
def test_weighted_update_through_the_ungrouped_forward(cuda, monkeypatch, dtype):
    """A detector four times the image's width at 64^2: no angle-group plan fits the grouped forward
    projector's windows (admm_fwd_plan_info reports none), so the bound batch projects with k_fwd."""
    case = wr.KFWD_CASE
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, dtype, wr.KFWD_DWF)
    nb = _batch(case, dtype, P, P["w"], dwf=wr.KFWD_DWF)
    assert nb.fwd_plans() == [] and not nb.mirror
    st = sr.random_state(nb, case.seed)
    nb.node_update()
    got = _read(nb)
    ref = _oracle(P, case, P["A"])(st)
    bars, yard = _bars(case, dtype, P, ref, lambda: _oracle(P, case, sr.as_f32_matrix(P["A"]), np.float32)(st))
    _compare(dtype + " weighted k_fwd", case, dtype, got, ref, bars, yard)
    _untouched(nb, st)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unweighted_update_through_the_ungrouped_forward(cuda, monkeypatch, dtype):
    """The same batch without weights: the unweighted k_fwd (MODE 0 in the CG, MODE 1 for the residual and
    its statistics) against the unweighted oracle, with the same bars."""
    case = wr.KFWD_CASE
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, dtype, wr.KFWD_DWF)
    nb = _batch(case, dtype, P, None, dwf=wr.KFWD_DWF)
    assert nb.fwd_plans() == [] and not nb.mirror
    st = sr.random_state(nb, case.seed)
    nb.node_update()
    got = _read(nb)

    def run(A, dt):
        return sr.oracle_update(st, P["plan"], A, P["b"], P["q_fn"], P["prm"], case.fusion, dtype=dt, phantom=P["ph"])

    ref = run(P["A"], np.float64)
    bars, yard = _bars(case, dtype, P, ref, lambda: run(sr.as_f32_matrix(P["A"]), np.float32))
    _compare(dtype + " k_fwd", case, dtype, got, ref, bars, yard)
    _untouched(nb, st)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", wr.WEIGHT_REUSE_CASES, ids=sr.case_id)
def test_weighted_reuse_start(cuda, monkeypatch, case, dtype):
    """ADMM_BATCH_KEEP_X: the second update starts from the first one's A^T W (A x - b)."""
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, dtype)
    nb = _batch(case, dtype, P, P["w"], keep_x=True)
    st0 = sr.random_state(nb, case.seed)
    nb.node_update()
    st1 = sr.random_state(nb, case.seed + 1000, keep_x=True)
    nb.node_update()
    got = _read(nb)
    _untouched(nb, st1)
    two = lambda run: run(sr.continue_state(st0, run(st0), **sr.rerandomised(P["plan"], P["n"], case)))  # noqa: E731
    ref = two(_oracle(P, case, P["A"]))
    bars, yard = _bars(case, dtype, P, ref, lambda: two(_oracle(P, case, sr.as_f32_matrix(P["A"]), np.float32)))
    _compare(dtype + " weighted reuse", case, dtype, got, ref, bars, yard)


# --------------------------------------------------------------------------------------
# 6. w = 1 is bitwise the unweighted batch
# --------------------------------------------------------------------------------------
def _two_updates(nb, case):
    out = []
    sr.random_state(nb, case.seed)
    nb.node_update()
    out.append(_read(nb))
    sr.random_state(nb, case.seed + 1000, keep_x=True)
    nb.node_update()
    out.append(_read(nb))
    return out


def _assert_bitwise(a, b, what):
    for k in ("x", "d", "e", "stats"):
        assert np.array_equal(a[k], b[k]), (what, k, float(np.max(np.abs(a[k] - b[k]))))


@pytest.mark.parametrize("dtype,N,V,a_per,mirror", [("float32", 64, 8, 24, "1"), ("float64", 33, 3, 12, None)],
                         ids=["float32-mirror-64-V8", "float64-33-V3"])
@pytest.mark.parametrize("keep_x", [False, True], ids=["fresh", "keep_x"])
def test_unit_weights_are_bitwise_the_unweighted_batch(cuda, monkeypatch, dtype, N, V, a_per, mirror, keep_x):
    case = sr.Case(N, V, "ring", 2, 3, "iso", a_per, mirror, "midpoint", False, 5)
    if mirror is None:
        monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    else:
        monkeypatch.setenv("ADMM_FWD_MIRROR", mirror)
    P = sr.case_problem(case, dtype)
    ones = {g: np.ones(a_per * N) for g in range(V)}
    plain = _batch(case, dtype, P, None, keep_x=keep_x)
    unit = _batch(case, dtype, P, ones, keep_x=keep_x)
    assert plain.ray_weights is None and unit.ray_weights is not None
    assert torch.equal(plain.atb, unit.atb)
    a, b = _two_updates(plain, case), _two_updates(unit, case)
    assert np.any(a[1]["x"] != 0.0) and np.all(a[1]["stats"][:, 0] > 0.0)
    for i in range(2):
        _assert_bitwise(a[i], b[i], f"update {i}")


# --------------------------------------------------------------------------------------
# 7. invariances, bitwise
# --------------------------------------------------------------------------------------
def _isolated(dtype, N, a_per, V, nodes, w, seed, state):
    """A batch of the edgeless nodes ``nodes`` (sinograms, weights and state rows of those nodes of
    a V-node problem), one update; returns its outputs."""
    case = sr.Case(N, len(nodes), "none", 2, 3, "iso", a_per, None, "midpoint", False, seed)
    P = sr.case_problem(case._replace(V=V), dtype)
    plan = make_plan(nx.empty_graph(len(nodes)), len(nodes))
    b = {k: P["b"][g] for k, g in enumerate(nodes)}
    wk = None if w is None else {k: w[g] for k, g in enumerate(nodes) if g in w}
    nb = _batch(case, dtype, P, wk, plan=plan, b=b)
    nb.x_ext.copy_(torch.from_numpy(state["x_ext"][nodes]))
    nb.d.copy_(torch.from_numpy(state["d"][nodes]))
    nb.e.copy_(torch.from_numpy(state["e"][nodes]))
    nb.node_update()
    return _read(nb)


@pytest.mark.parametrize("dtype", DTYPES)
def test_result_does_not_depend_on_batch_width_or_other_nodes_weights(cuda, monkeypatch, dtype):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)  # the defaults: float32 mirrors, float64 does not
    N, a_per, V, seed, g = 33, 12, 8, 4, 2
    w = wr.ray_weights(a_per, N, range(V), seed, dtype)
    state = sr.host_state(make_plan(nx.empty_graph(V), V), N * N, seed)
    alone = _isolated(dtype, N, a_per, V, [g], w, seed, state)
    assert np.any(alone["x"] != state["x_ext"][g])
    for width in (5, 8):
        nodes = list(range(width))
        got = _isolated(dtype, N, a_per, V, nodes, w, seed, state)
        for k in ("x", "d", "e", "stats"):
            assert np.array_equal(got[k][g], alone[k][0]), (width, k)
    # other nodes' weights: all but node g's replaced (and one node's dropped: w = 1 there)
    w2 = wr.ray_weights(a_per, N, range(V), seed + 1, dtype)
    w2[g] = w[g]
    del w2[0]
    got = _isolated(dtype, N, a_per, V, list(range(5)), w2, seed, state)
    for k in ("x", "d", "e", "stats"):
        assert np.array_equal(got[k][g], alone[k][0]), ("other weights", k)
    assert not np.array_equal(got["x"][1], _isolated(dtype, N, a_per, V, [1], w, seed, state)["x"][0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_clearing_restores_unweighted_and_set_precisions_keeps_weights(cuda, monkeypatch, dtype):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    case = sr.Case(33, 3, "ring", 2, 3, "iso", 12, None, "midpoint", False, 6)
    P = wr.case_problem(case, dtype)

    def run(nb):
        sr.random_state(nb, case.seed)
        nb.node_update()
        return _read(nb)

    plain_nb = _batch(case, dtype, P, None)
    plain = run(plain_nb)
    nb = _batch(case, dtype, P, P["w"])
    atb_w = nb.atb.clone()
    weighted = run(nb)
    assert not torch.equal(atb_w, plain_nb.atb) and not np.array_equal(weighted["x"], plain["x"])
    # set_precisions re-binds (which drops the library's weights): the batch applies them again
    qs = [P["q_fn"](g, P["plan"].inc_nbr[s]) for k, g in enumerate(P["plan"].local_nodes)
          for s in range(P["plan"].inc_off[k], P["plan"].inc_off[k + 1])]
    nb.set_precisions(qs)
    _assert_bitwise(run(nb), weighted, "after set_precisions")
    assert torch.equal(nb.atb, atb_w)
    # NULL clears them: the unweighted results, A^T b included
    nb.set_ray_weights(None)
    assert nb.ray_weights is None and torch.equal(nb.atb, plain_nb.atb)
    _assert_bitwise(run(nb), plain, "after clearing")
    # and setting them again gives the weighted results again
    nb.set_ray_weights([P["w"][g] for g in range(3)])
    assert torch.equal(nb.atb, atb_w)
    _assert_bitwise(run(nb), weighted, "after setting again")


# --------------------------------------------------------------------------------------
# 8. A^T (w b) and the weighted column norms
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,a_per,mirror", [(33, 12, "1"), (33, 9, None), (64, 24, "1"), (64, 24, "0"), (64, 9, None)])
def test_atb_and_weighted_column_norms_match_the_joseph_matrix(cuda, monkeypatch, N, a_per, mirror, dtype):
    _set_mirror(monkeypatch, mirror)
    case = sr.Case(N, 3, "ring", 1, 1, "iso", a_per, mirror, "midpoint", False, 7)
    P = wr.case_problem(case, dtype)
    A = P["A"]
    nb = _batch(case, dtype, P, P["w"])
    atb = nb.atb.cpu().numpy()
    op = RayTransform(ParallelBeamGeometry(N, a_per), dtype)
    W1 = op.column_norms_sq()
    assert np.array_equal(op.column_norms_sq(ray_weights=np.ones(a_per * N)), W1)
    A2 = A.multiply(A).T.tocsr()
    for g in range(3):
        b = np.asarray(P["b"][g], dtype=np.float64)
        e = rel(atb[g], A.T @ (P["w"][g] * b))
        assert e < PROJ_TOL[dtype], ("atb", g, e)
        Wg = op.column_norms_sq(ray_weights=P["w"][g].reshape(a_per, N))
        e = rel(Wg, np.maximum(A2 @ P["w"][g], 1e-12))
        assert e < PROJ_TOL[dtype], ("column norms", g, e)
    assert np.all(op.column_norms_sq(ray_weights=np.zeros(a_per * N)) == 1e-12)


def test_make_precisions_with_weights(cuda):
    from admm_hip.data import make_precisions
    N, a_per = 33, 12
    ops = [RayTransform(ParallelBeamGeometry(N, a_per), "float32", 0) for _ in range(3)]
    w = wr.ray_weights(a_per, N, range(3), 2, "float32")
    Wp, _ = make_precisions(ops)
    Ww, Q = make_precisions(ops, ray_weights=[w[0], None, w[2]])
    assert np.array_equal(Ww[1], Wp[1]) and not np.array_equal(Ww[0], Wp[0]) and not np.array_equal(Ww[0], Ww[2])
    assert np.array_equal(Ww[0], ops[0].column_norms_sq(ray_weights=w[0]))
    assert np.array_equal(Q(0, 2), np.maximum(0.5 * (Ww[0] + Ww[2]), 1e-12))
    assert Q.qslot_key(0, 1) != Q.qslot_key(2, 1) and Q.qslot_key(0, 2) == Q.qslot_key(2, 0)


# --------------------------------------------------------------------------------------
# 9. whole run
# --------------------------------------------------------------------------------------
RUN_N, RUN_V, RUN_ANGLES, RUN_ITERS = 64, 4, 96, 3
HIST = ("primal", "dual", "obj_total", "mse_sino_total")


def _run_problem(dtype):
    from admm_hip.data import make_precisions, make_sinograms, shepp_logan
    from admm_hip.solver import make_operators
    ops = make_operators(RUN_N, RUN_V, RUN_ANGLES, dtype=dtype, device=0)
    ph = shepp_logan(RUN_N)
    sinos = make_sinograms(ops, ph, 0.005, seed=1000)
    s = wr.s_weights(RUN_ANGLES // RUN_V, RUN_N, range(RUN_V), 3)
    w = [s[g] * s[g] for g in range(RUN_V)]
    Wi, Q = make_precisions(ops, ray_weights=w)
    return ops, ph, sinos, s, w, Wi, Q


def _run_weighted(dtype, via="dropin", group=None):
    ops, ph, sinos, s, w, Wi, Q = _run_problem(dtype)
    kw = dict(lam_tv=0.02, rho=2.0, max_iters=RUN_ITERS, eps_pri=0.0, eps_dual=0.0, verbose=False,
              phantom_true=ph, write_params=False, group=group, ray_weights=w)
    if via == "dropin":
        from block_6_admm_loop_ver2 import decentralized_admm
        x, h = decentralized_admm(ops, sinos, nx.cycle_graph(RUN_V), Wi, Q, RUN_N, **kw)
    else:
        from admm_hip.admm import run_admm
        x, h = run_admm(ops, sinos, nx.cycle_graph(RUN_V), Wi, Q, RUN_N, **kw)
    return np.stack(x), {k: np.asarray(h[k]) for k in HIST}


@pytest.fixture(scope="module")
def run_oracle():
    """{dtype: (images, history)} of the oracle on diag(s_g) A and s_g b_g, computed once per dtype."""
    from oracle import admm as oadmm
    cache = {}

    def get(dtype):
        if dtype not in cache:
            ops, ph, sinos, s, w, Wi, Q = _run_problem(dtype)
            A = joseph_matrix(Geometry(RUN_N, RUN_ANGLES // RUN_V))
            scaled = [wr.row_scaled(A, sinos[g].double().cpu().numpy().reshape(-1), s[g]) for g in range(RUN_V)]
            xo, ho = oadmm.decentralized_admm([a for a, _ in scaled], [b for _, b in scaled], nx.cycle_graph(RUN_V),
                                              Q, RUN_N, lam_tv=0.02, rho=2.0, max_iters=RUN_ITERS, eps_pri=0.0,
                                              eps_dual=0.0, phantom_true=ph.numpy())
            cache[dtype] = (np.stack(xo), {k: np.asarray(ho[k]) for k in HIST})
        return cache[dtype]
    return get


@pytest.mark.parametrize("via", ["run_admm", "dropin"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_weighted_run_matches_row_scaled_oracle(cuda, monkeypatch, run_oracle, dtype, via):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    x, h = _run_weighted(dtype, via)
    xo, ho = run_oracle(dtype)
    errs = {"images": rel(x, xo), **{k: rel(h[k], ho[k]) for k in HIST}}
    print(f"\nRUN {dtype} {via}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)


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
        q.put((rank, _run_weighted("float32")))
    finally:
        dist.destroy_process_group()


def test_weighted_two_ranks_on_one_gpu_match_one_rank_bitwise(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    x1, h1 = _run_weighted("float32")
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
# 10. a node with every second view zeroed = the geometry of the remaining views
# --------------------------------------------------------------------------------------
def test_zeroed_views_equal_the_geometry_of_the_remaining_views(cuda, monkeypatch):
    """2a angles (u + 1/2) pi / 2a with w = 0 on the odd u: the even ones are the a angles
    (t + 1/2) pi / a - pi / 4a of ParallelBeamGeometry(N, a, angle_min=-pi/4a, angle_max=pi-pi/4a)."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    N, a, V, seed = 33, 6, 3, 8
    case = sr.Case(N, V, "ring", 2, 3, "iso", 2 * a, None, "midpoint", False, seed)
    P = sr.case_problem(case, "float64")
    keep = np.zeros((2 * a, N))
    keep[0::2] = 1.0
    full = _batch(case, "float64", P, {g: keep.reshape(-1) for g in range(V)})
    st = sr.random_state(full, seed)
    full.node_update()
    got = _read(full)
    off = math.pi / (4 * a)
    half_geom = ParallelBeamGeometry(N, a, 1.0, -off, math.pi - off)
    b_half = {g: np.asarray(P["b"][g]).reshape(2 * a, N)[0::2].reshape(-1) for g in range(V)}
    half = NodeBatch(half_geom, "float64", P["plan"], b_half, P["q_fn"], sr.RHO, sr.LAM, sr.MU, case.tv_iters,
                     case.cg_iters, case.tv_kind, P["ph"], 0)
    assert half.ray_weights is None
    sr.random_state(half, seed)
    half.node_update()
    want = _read(half)
    assert rel(full.atb.cpu().numpy(), half.atb.cpu().numpy()) < 1e-9
    for k in ("x", "d", "e"):
        assert sr.field_err(got[k], want[k])[0] <= 1e-9, (k, sr.field_err(got[k], want[k]))
    assert sr.stat_err(got["stats"], want["stats"]).max() <= 1e-9, sr.stat_err(got["stats"], want["stats"])
    # and the zeroed views matter
    plain = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
    assert sr.field_err(got["x"], plain["x"])[0] > 1e-3
