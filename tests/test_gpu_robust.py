"""GPU: the Huber data term by reweighted rays (admm_huber_weights, admm_batch_update_ray_weights,
run_admm(robust=delta); references: tests/robust_ref.py).

* the kernel against its NumPy restatement: w_out bitwise, counts equal, the loss within 1e-12 relative
  (nonnegative terms, m <= 2049: a fixed-order float64 sum lies within m 2^-53 = 2.3e-13 of the exact
  one), an image alone bitwise the image in a batch;
* admm_batch_update_ray_weights: the next x-update is bitwise that of a batch given the same weights by
  admm_batch_set_ray_weights;
* admm_batch_refresh_kept: the kept start formed again, bitwise the kept start when the weights are
  the same;
* run_admm(robust=inf) is bitwise the run without the keyword;
* run_admm(robust=0.3) against robust_ref.irls_run at the whole-run gates (1e-9 float64, 1e-5 float32
  samples);
* the zinger case: the Huber run ends near the clean-data run, the plain run does not;
* pipelined / read-back, one / two streams, two batches / each alone: bitwise.

Run with ``-s`` to see the measured figures.
"""
import math

import networkx as nx
import numpy as np
import pytest
import torch

import robust_ref as rr
import state_ref as sr
import weights_ref as wr
from admm_hip import huber_weights
from admm_hip.geometry import ParallelBeamGeometry, RayTransform
from admm_hip.solver import NodeBatch
from test_gpu_state_update import _read, _set_mirror

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
TDT = {"float32": torch.float32, "float64": torch.float64}
NDT = {"float32": np.float32, "float64": np.float64}
RUN_TOL = {"float32": 1e-5, "float64": 1e-9}  # the whole-run gates
LOSS_TOL = 1e-12


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


# --------------------------------------------------------------------------------------
# the kernel
# --------------------------------------------------------------------------------------
def _rays(dtype, nimg, m, seed):
    rng = np.random.default_rng([seed, nimg, m])
    ax = rng.standard_normal((nimg, m)).astype(NDT[dtype])
    b = (ax.astype(np.float64) + 0.4 * rng.standard_normal((nimg, m))).astype(NDT[dtype])
    b[:, 0] = 0
    ax[:, 0] = NDT[dtype](rr.DELTA)  # |r| = (T)delta: at the threshold with float64, just beyond with float32
    w = rng.uniform(0.0, 2.0, (nimg, m)).astype(NDT[dtype])
    w[rng.random((nimg, m)) < 0.1] = 0
    return ax, b, w


@pytest.mark.parametrize("delta", [rr.DELTA, math.inf], ids=["delta0.3", "inf"])
@pytest.mark.parametrize("with_w", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_its_restatement(cuda, dtype, with_w, delta):
    worst = 0.0
    for m in (1, 255, 1024, 1025, 2049):
        for nimg in (1, 3):
            ax, b, w = _rays(dtype, nimg, m, 7)
            if not with_w:
                w = None
            dev = lambda a: None if a is None else torch.from_numpy(a).to(cuda)  # noqa: E731
            wo, loss, cnt = huber_weights(dev(ax), dev(b), delta, dev(w))
            assert wo.dtype == TDT[dtype] and tuple(wo.shape) == (nimg, m) and loss.dtype == torch.float64
            wo, loss, cnt = wo.cpu().numpy(), loss.cpu().numpy(), cnt.cpu().numpy()
            for v in range(nimg):
                rw, rl, rc = rr.huber_weights_ref(ax[v], b[v], delta, None if w is None else w[v], NDT[dtype])
                assert np.array_equal(wo[v].view(np.uint8), rw.view(np.uint8)), (m, nimg, v)
                assert cnt[v] == rc, (m, nimg, v, cnt[v], rc)
                err = abs(loss[v] - rl) / max(rl, 1e-300)
                worst = max(worst, err)
                assert err <= LOSS_TOL, (m, nimg, v, loss[v], rl)
                # the image alone: bitwise the image in the batch
                o1, l1, c1 = huber_weights(dev(ax[v]), dev(b[v]), delta, None if w is None else dev(w[v]))
                assert tuple(o1.shape) == (m,) and np.array_equal(o1.cpu().numpy().view(np.uint8), wo[v].view(np.uint8))
                assert l1.cpu().numpy()[0] == loss[v] and c1.cpu().numpy()[0] == cnt[v]
            if delta == math.inf:
                want = np.ones_like(ax) if w is None else w
                assert np.array_equal(wo.view(np.uint8), want.view(np.uint8)) and not cnt.any()
            elif m > 1:
                assert cnt.sum() > 0
    print(f"\nKERNEL {dtype} w={with_w} delta={delta}: worst loss error {worst:.2e}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_masks_and_propagates_nan(cuda, dtype):
    ax, b, w = _rays(dtype, 2, 1025, 9)
    w[0, 5], w[1, 6] = 0, 1
    ax[0, 5], b[0, 5] = np.nan, np.inf   # masked: + 0, not counted
    ax[1, 6] = np.nan                    # unmasked: propagates
    wo, loss, cnt = (t.cpu().numpy() for t in huber_weights(*(torch.from_numpy(a).to(cuda) for a in (ax, b)),
                                                            rr.DELTA, torch.from_numpy(w).to(cuda)))
    r0 = rr.huber_weights_ref(ax[0], b[0], rr.DELTA, w[0], NDT[dtype])
    assert wo[0, 5] == 0 and not np.signbit(wo[0, 5]) and np.all(wo[0][w[0] == 0] == 0)
    assert np.array_equal(wo[0].view(np.uint8), r0[0].view(np.uint8)) and cnt[0] == r0[2]
    assert abs(loss[0] - r0[1]) <= LOSS_TOL * r0[1]
    r1 = rr.huber_weights_ref(ax[1], b[1], rr.DELTA, w[1], NDT[dtype])
    assert np.isnan(wo[1, 6]) and np.isnan(loss[1]) and cnt[1] == r1[2]
    assert np.array_equal(np.delete(wo[1], 6).view(np.uint8), np.delete(r1[0], 6).view(np.uint8))


def test_kernel_argument_errors(cuda):
    import ctypes as C
    from admm_hip import _lib
    lib = _lib.load()
    t = torch.zeros(8, dtype=torch.float64, device=cuda)
    o = torch.zeros(8, dtype=torch.float64, device=cuda)
    p = _lib.ptr
    ok = (p(t), p(t), None, p(o), _lib.ADMM_DTYPE_F64, 8, 1, 0.3, p(o), p(o), None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.admm_huber_weights(*a)

    assert call(_7=0.0) == -1 and call(_7=float("nan")) == -1 and call(_7=-1.0) == -1
    assert call(_0=None) == -1 and call(_3=None) == -1 and call(_8=None) == -1 and call(_9=None) == -1
    assert call(_3=p(t)) == -1 and call(_4=7) == -1 and call(_5=0) == -1 and call(_6=0) == -1 and call(_6=65536) == -1
    need = C.c_longlong()
    assert lib.admm_huber_weights_work(2049, 3, C.byref(need)) == 0 and need.value == 2 * 3 * 3
    assert lib.admm_batch_update_ray_weights(None, p(t), None) == -3
    with pytest.raises(ValueError):
        huber_weights(t, t, True)
    with pytest.raises(ValueError):
        huber_weights(t, t, 0.0)


# --------------------------------------------------------------------------------------
# admm_batch_update_ray_weights
# --------------------------------------------------------------------------------------
UPDATE_PATH = [
    (sr.Case(33, 3, "ring", 2, 3, "iso", 12, "1", "midpoint", False, 3), False),
    (sr.Case(64, 8, "ring", 2, 3, "iso", 24, "0", "midpoint", False, 3), False),
    (sr.Case(33, 3, "ring", 2, 3, "iso", 12, "1", "midpoint", False, 3), True),
]


def _batch(case, dtype, P, w, keep_x):
    geom = ParallelBeamGeometry(case.N, case.a_per)
    wl = None if w is None else [w.get(g) for g in range(case.V)]
    nb = NodeBatch(geom, dtype, P["plan"], P["b"], P["q_fn"], sr.RHO, sr.LAM, sr.MU, case.tv_iters, case.cg_iters,
                   case.tv_kind, P["ph"], 0, fusion=case.fusion, Wi_list=P["W"], keep_x=keep_x, derive_z=False,
                   ray_weights=wl)
    assert nb.mirror == (case.mirror == "1")
    return nb


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,keep_x", UPDATE_PATH,
                         ids=["33-V3-mirror", "64-V8-nomirror", "33-V3-mirror-keep_x"])
def test_updated_weights_are_bitwise_set_weights(cuda, monkeypatch, case, keep_x, dtype):
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, dtype)
    w_new = wr.ray_weights(case.a_per, case.N, range(case.V), case.seed + 50, dtype)
    t_new = torch.from_numpy(np.stack([w_new[g] for g in range(case.V)])).to(device=cuda, dtype=TDT[dtype])
    out = {}
    for how in ("update", "set"):
        nb = _batch(case, dtype, P, P["w"], keep_x)
        sr.random_state(nb, case.seed)
        nb.node_update()  # (keep_x: the batch now holds a kept A^T s of the old weights)
        first = _read(nb)
        if how == "update":
            nb.update_ray_weights(t_new)
        else:
            nb.set_ray_weights([w_new[g] for g in range(case.V)])
        sr.random_state(nb, case.seed + 1000, keep_x=True)
        nb.node_update()
        out[how] = (first, _read(nb), nb.atb.cpu().numpy())
    for k in ("x", "d", "e", "stats"):
        assert np.array_equal(out["update"][0][k], out["set"][0][k]), ("first", k)
        assert np.array_equal(out["update"][1][k], out["set"][1][k]), (k, float(np.max(np.abs(
            out["update"][1][k] - out["set"][1][k]))))
    assert np.array_equal(out["update"][2], out["set"][2])
    # and the new weights matter
    assert not np.array_equal(out["update"][1]["x"], out["update"][0]["x"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_refreshed_kept_start_is_bitwise_the_kept_start(cuda, monkeypatch, dtype):
    """keep_x: update_ray_weights with the weights the batch has, then refresh_kept_start -- the next
    update is bitwise that of a batch whose weights were never touched (both start from the kept
    A^T s); without the refresh it projects x again and differs."""
    case = UPDATE_PATH[2][0]
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, dtype)
    t_same = torch.from_numpy(np.stack([P["w"][g] for g in range(case.V)])).to(device=cuda, dtype=TDT[dtype])
    out = {}
    for how in ("untouched", "refreshed", "dropped"):
        nb = _batch(case, dtype, P, P["w"], True)
        sr.random_state(nb, case.seed)
        nb.node_update()
        stats = nb.node_stats.clone()
        if how != "untouched":
            nb.update_ray_weights(t_same)
        if how == "refreshed":
            nb.refresh_kept_start()
            assert torch.equal(nb.node_stats, stats)  # the refresh leaves the statistics alone
            with pytest.raises(Exception):
                nb.refresh_kept_start()  # nothing left to refresh
        sr.random_state(nb, case.seed + 1000, keep_x=True)
        nb.node_update()
        out[how] = _read(nb)
    for k in ("x", "d", "e", "stats"):
        assert np.array_equal(out["refreshed"][k], out["untouched"][k]), k
    assert sr.field_err(out["dropped"]["x"], out["untouched"]["x"])[0] < RUN_TOL[dtype]


def test_refresh_needs_a_dropped_kept_start(cuda, monkeypatch):
    case = UPDATE_PATH[0][0]
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, "float64")
    from admm_hip import _lib
    lib = _lib.load()
    assert lib.admm_batch_refresh_kept(None, None) == -3
    for keep_x in (False, True):
        nb = _batch(case, "float64", P, P["w"], keep_x)
        sr.random_state(nb, case.seed)
        nb.node_update()
        assert lib.admm_batch_refresh_kept(nb.ctx.h, None) == -3  # nothing was dropped
        nb.update_ray_weights(nb.ray_weights.clone())
        assert lib.admm_batch_refresh_kept(nb.ctx.h, None) == (0 if keep_x else -3)
    nb = _batch(case, "float64", P, P["w"], True)
    nb.update_ray_weights(nb.ray_weights.clone())  # no update yet: no kept samples of x
    assert lib.admm_batch_refresh_kept(nb.ctx.h, None) == -3


def test_update_needs_weights(cuda, monkeypatch):
    case = UPDATE_PATH[0][0]
    _set_mirror(monkeypatch, case.mirror)
    P = wr.case_problem(case, "float64")
    nb = _batch(case, "float64", P, None, False)
    t = torch.ones_like(nb.b)
    with pytest.raises(ValueError):
        nb.update_ray_weights(t)
    from admm_hip import _lib
    assert nb.lib.admm_batch_update_ray_weights(nb.ctx.h, _lib.ptr(t), None) == -3  # ADMM_E_STATE
    nb2 = _batch(case, "float64", P, P["w"], False)
    assert nb2.lib.admm_batch_update_ray_weights(nb2.ctx.h, None, None) == -1
    with pytest.raises(ValueError):
        nb2.update_ray_weights(torch.ones((case.V, 5), dtype=torch.float64, device=cuda))


# --------------------------------------------------------------------------------------
# whole runs
# --------------------------------------------------------------------------------------
def _run(case, dtype, P, iters, b=None, seen=None, **kw):
    from admm_hip.admm import run_admm
    ops = [RayTransform(ParallelBeamGeometry(case.N, case.a_per), dtype, 0) for _ in range(case.V)]
    b = P["b"] if b is None else b
    prm = P["prm"]

    def inspect(rg):
        if case.mirror is not None:
            assert all(nb.mirror == (case.mirror == "1") for nb in rg.batches)
        if seen is not None:
            seen.append(len(rg.batches))

    x, h = run_admm(ops, [b[g] for g in range(case.V)], sr.graph_of(case.graph, case.V), P["W"], P["q_fn"], case.N,
                    lam_tv=prm.lam, rho=prm.rho, mu=prm.mu, tv_iters=prm.tv_iters, cg_iters=prm.cg_iters,
                    tv_kind=case.tv_kind, max_iters=iters, eps_pri=0.0, eps_dual=0.0, verbose=False,
                    phantom_true=P["ph"], write_params=False, inspect=inspect, **kw)
    return np.stack(x), h


def _same_history(h, g, keys=None):
    for k in (keys or h):
        assert np.array_equal(np.asarray(h[k]), np.asarray(g[k]), equal_nan=True), k


INF_CASE = sr.Case(33, 4, "ring", 2, 3, "iso", 12, None, "midpoint", False, 4)


@pytest.mark.parametrize("weights", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_delta_is_bitwise_the_plain_run(cuda, monkeypatch, dtype, weights):
    """run_admm(robust=inf) against the run without the keyword, 3 iterations: the images and every
    history key of the plain run bitwise, no outlier.

    run_admm binds its batches with ADMM_BATCH_KEEP_X, so the plain run's later x-updates start from the
    kept A^T (A x - b); after a refresh of the weights the loop forms it again with the update's own
    epilogue launches (admm_batch_refresh_kept), so with weights that never move both runs take the same
    start from the same bits."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    P = wr.case_problem(INF_CASE, dtype)
    kw = dict(ray_weights=[P["w"][g] for g in range(INF_CASE.V)]) if weights else {}
    x0, h0 = _run(INF_CASE, dtype, P, 3, **kw)
    x1, h1 = _run(INF_CASE, dtype, P, 3, robust=math.inf, **kw)
    assert "robust_loss_total" not in h0 and len(h1["robust_loss_total"]) == 3
    diffs = {k: float(np.max(np.nan_to_num(np.abs(np.asarray(h0[k], dtype=np.float64)
                                                  - np.asarray(h1[k], dtype=np.float64))))) for k in h0}
    print(f"\nINF {dtype} weights={weights}: images max diff {np.max(np.abs(x0 - x1)):.3e} "
          f"(rel {rel(x1, x0):.2e}); history max diffs " + " ".join(f"{k}={v:.2e}" for k, v in diffs.items() if v))
    assert h1["robust_outliers_total"] == [0.0, 0.0, 0.0]
    assert all(np.all(np.asarray(v) >= 0) for v in h1["robust_loss_per_node"])
    assert np.array_equal(x0, x1)
    _same_history(h0, h1)


@pytest.mark.parametrize("weights", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_delta_is_bitwise_without_the_kept_start(cuda, monkeypatch, dtype, weights):
    """The same two runs on batches bound without ADMM_BATCH_KEEP_X (every update projects x): the
    all-ones weights given at setup, the refresh and A^T (omega b) formed again change no bit."""
    from admm_hip.groups import RankGroups
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    case = INF_CASE
    P = wr.case_problem(case, dtype)
    ops = [RayTransform(ParallelBeamGeometry(case.N, case.a_per), dtype, 0) for _ in range(case.V)]
    w = [P["w"][g] for g in range(case.V)] if weights else None
    out = {}
    for robust in (False, True):
        rg = RankGroups(ops, sr.graph_of(case.graph, case.V), case.V, 1, 0, [P["b"][g] for g in range(case.V)],
                        P["q_fn"], sr.RHO, sr.LAM, sr.MU, case.tv_iters, case.cg_iters, case.tv_kind, P["ph"],
                        Wi_list=P["W"], keep_x=False, ray_weights=w)
        if robust:
            rg.enable_robust(math.inf)
        seen = []
        for k in range(3):
            rg.node_update()
            if robust:
                rg.reweight(True)
            rg.exchange_consensus()
            nb = rg.batches[0]
            seen.append([t.cpu().numpy().copy() for t in (nb.x_local, nb.d, nb.e, nb.node_stats, nb.y, nb.z, nb.atb)])
        if robust:
            sums = rg.batches[0].huber.sums.cpu().numpy()
            assert np.all(sums[:, 1] == 0) and np.all(sums[:, 0] > 0)
        out[robust] = seen
    for k in range(3):
        for a, b in zip(out[False][k], out[True][k]):
            assert np.array_equal(a, b), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", rr.PARITY_RUNS, ids=rr.parity_id)
def test_run_matches_the_reweighted_reference(cuda, monkeypatch, p, dtype):
    name, every, weights = p
    P = rr.parity_problem(name, dtype, weights)
    case = P["case"]
    _set_mirror(monkeypatch, case.mirror)
    ref = rr.parity_reference(name, every, weights, dtype)
    kw = dict(ray_weights=[P["w"][g] for g in range(case.V)]) if weights else {}
    x, h = _run(case, dtype, P, rr.PARITY_ITERS, robust={"delta": rr.DELTA, "every": every}, **kw)
    errs = {"images": rel(x, ref["x"]), "primal": rel(h["primal"], ref["primal"]),
            "robust_loss_total": rel(h["robust_loss_total"], ref["loss_total"])}
    got = np.stack(h["robust_outliers_per_node"])
    want = np.stack(ref["outliers"])
    room = 0 if dtype == "float64" else rr.near_threshold(ref, rr.DELTA, rr.COUNT_MARGIN)
    print(f"\nPARITY {rr.parity_id(p)} {dtype}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" outliers {got.sum(axis=1).tolist()} ref {want.sum(axis=1).tolist()} room {room}")
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)
    assert float(np.abs(got - want).sum()) <= room
    assert h["robust_outliers_total"] == [float(s) for s in got.sum(axis=1)]
    assert np.allclose(h["robust_loss_total"], [float(np.sum(v)) for v in h["robust_loss_per_node"]], rtol=1e-15)


def test_zinger_case_through_run_admm(cuda, monkeypatch):
    """3 % of the rays off by +-3, float64 samples: the Huber run's final image error is <= 0.75 x the
    plain run's and <= 1.06 x the clean-data run's (the reference's 0.70 and 1.05 plus the parity gate's
    room)."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    P = rr.zinger_problem()
    case = P["case"]

    def err(b, **kw):
        x, h = _run(case, "float64", P, rr.Z_ITERS, b=b, **kw)
        return math.sqrt(float(np.sum((x - P["ph"][None, :]) ** 2)) / case.V), h

    plain, _ = err(P["b_zinger"])
    clean, _ = err(P["b"])
    robust, h = err(P["b_zinger"], robust=rr.DELTA)
    R = rr.zinger_runs()
    print(f"\nZINGER plain {plain:.4f} clean {clean:.4f} robust {robust:.4f}: ratios {robust / plain:.4f} "
          f"{robust / clean:.4f} (reference {R['robust']['img_err'][-1] / R['plain']['img_err'][-1]:.4f} "
          f"{R['robust']['img_err'][-1] / R['clean']['img_err'][-1]:.4f}); outliers {h['robust_outliers_total']}")
    assert robust <= 0.75 * plain
    assert robust <= 1.06 * clean
    assert h["robust_outliers_total"][-1] == float(R["robust"]["outliers"][-1].sum())


# --------------------------------------------------------------------------------------
# loop forms, bitwise
# --------------------------------------------------------------------------------------
ROBUST_HIST = ("robust_loss_per_node", "robust_loss_total", "robust_outliers_per_node", "robust_outliers_total")


def test_pipelined_and_read_back_loops_agree(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    P = sr.case_problem(INF_CASE, "float32")
    xa, ha = _run(INF_CASE, "float32", P, 4, robust={"delta": rr.DELTA, "every": 2, "until": 3}, pipeline=True)
    xb, hb = _run(INF_CASE, "float32", P, 4, robust={"delta": rr.DELTA, "every": 2, "until": 3}, pipeline=False)
    assert np.array_equal(xa, xb) and ha["robust_outliers_total"][-1] > 0
    _same_history(ha, hb)
    # every = 2: iteration 1 still runs with the caller's weights; every = 1 differs from there on
    xc, hc = _run(INF_CASE, "float32", P, 4, robust=rr.DELTA)
    assert hc["robust_loss_total"][0] == ha["robust_loss_total"][0]
    assert hc["robust_loss_total"][1] != ha["robust_loss_total"][1] and not np.array_equal(xa, xc)


def test_two_streams_agree_with_one(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    case = sr.Case(33, 8, "ring", 2, 3, "iso", 12, None, "midpoint", False, 5)
    P = sr.case_problem(case, "float64")
    seen = []
    xa, ha = _run(case, "float64", P, 3, robust=rr.DELTA, streams=1, seen=seen)
    xb, hb = _run(case, "float64", P, 3, robust=rr.DELTA, streams=2, seen=seen)
    assert seen == [1, 2]
    assert np.array_equal(xa, xb)
    _same_history(ha, hb)


def test_two_batches_agree_with_each_batch_alone(cuda, monkeypatch):
    """Six nodes, two 3-rings with 12 and 9 angles per node (two batches), against each ring's run."""
    from admm_hip.admm import run_admm
    from admm_hip.data import make_sinograms, shepp_logan
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    N, n = 33, 33 * 33
    ops = [RayTransform(ParallelBeamGeometry(N, a), "float64", 0) for a in (12, 12, 12, 9, 9, 9)]
    ph = shepp_logan(N)
    sinos = make_sinograms(ops, ph, 0.05, seed=11)
    W, q = sr.precisions(n, 6, 6)
    kw = dict(lam_tv=sr.LAM, rho=sr.RHO, mu=sr.MU, tv_iters=2, cg_iters=3, max_iters=3, eps_pri=0.0, eps_dual=0.0,
              verbose=False, phantom_true=ph, write_params=False, robust=rr.DELTA)
    seen = []
    G = nx.disjoint_union(nx.cycle_graph(3), nx.cycle_graph(3))
    x, h = run_admm(ops, sinos, G, W, q, N, inspect=lambda rg: seen.append(len(rg.batches)), **kw)
    assert seen == [2] and sum(h["robust_outliers_total"]) > 0
    for off in (0, 3):
        qs = lambda i, j, off=off: q(i + off, j + off)  # noqa: E731
        qs.qslot_key = lambda i, j, off=off: q.qslot_key(i + off, j + off)
        xs, hs = run_admm(ops[off:off + 3], sinos[off:off + 3], nx.cycle_graph(3), W[off:off + 3], qs, N, **kw)
        assert np.array_equal(np.stack(x)[off:off + 3], np.stack(xs)), off
        for k in ("robust_loss_per_node", "robust_outliers_per_node", "mse_sino_per_node"):
            assert np.array_equal(np.stack(h[k])[:, off:off + 3], np.stack(hs[k])), (off, k)


# --------------------------------------------------------------------------------------
# errors
# --------------------------------------------------------------------------------------
def test_matrix_operator_raises_before_device_work(cuda, monkeypatch):
    from admm_hip import admm
    from oracle.geometry import Geometry, joseph_matrix
    N = 16
    A = joseph_matrix(Geometry(N, 6))
    ops = [RayTransform(ParallelBeamGeometry(N, 6), "float64", 0), A.toarray()]

    def boom(*a, **k):
        raise AssertionError("device work before the argument check")

    monkeypatch.setattr(admm, "RankGroups", boom)
    W, q = sr.precisions(N * N, 2, 1)
    with pytest.raises(ValueError, match="explicit-matrix"):
        admm.run_admm(ops, [np.zeros(6 * N)] * 2, nx.path_graph(2), W, q, N, max_iters=1, verbose=False,
                      write_params=False, robust=0.3)
