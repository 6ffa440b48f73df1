"""GPU: one x-update of a node batch from a random, non-smooth ADMM state against the float64
oracle, per pixel and per statistic (tests/state_ref.py).

The solver's other tests start from x = d = e = y = z = 0 on a smooth phantom and judge
whole-image norms; a wrong incidence sign, q slot, border row, tile seam or node lane of a ragged
chunk can hide under those.  Here every output of one update is compared where it is:

* x, d, e per pixel (max-abs error relative to the oracle field's max-abs, the offending
  (node, i, j) reported) and each of the six node statistics of each node on its own;
* float64 samples within 1e-9; float32 samples within 4 x the float32
  rounding yardstick of the case (the float64 oracle against its own float32 emulation);
* the rows of the batch the update must not write, bitwise;
* the ADMM_BATCH_KEEP_X start (k_start_reuse) from a re-randomised state;
* the rounds override against a batch bound with that round count, bitwise;
* the shrink at its threshold and the CG's zero-denominator guards.

Run with ``-s`` to see every case's device / yardstick ratios.
"""
import math

import networkx as nx
import numpy as np
import pytest
import torch

import state_ref as sr
from admm_hip.geometry import ParallelBeamGeometry
from admm_hip.plan import make_plan
from admm_hip.solver import NodeBatch
from oracle import tv as otv

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]


def _set_mirror(monkeypatch, mirror):
    if mirror is None:
        monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    else:
        monkeypatch.setenv("ADMM_FWD_MIRROR", mirror)


def _batch(case, dtype, P, keep_x=False, tv_iters=None, plan=None):
    geom = ParallelBeamGeometry(case.N, case.a_per)
    nb = NodeBatch(geom, dtype, plan or P["plan"], P["b"], P["q_fn"], sr.RHO, sr.LAM, sr.MU,
                   case.tv_iters if tv_iters is None else tv_iters, case.cg_iters, case.tv_kind, P["ph"], 0,
                   fusion=case.fusion, Wi_list=P["W"], keep_x=keep_x, derive_z=case.derive_z)
    if case.mirror is not None:
        assert nb.mirror == (case.mirror == "1")
    return nb


def _read(nb):
    torch.cuda.synchronize()
    V = nb.V
    return {"x": nb.x_ext[:V].cpu().numpy().copy(), "d": nb.d.cpu().numpy().copy(), "e": nb.e.cpu().numpy().copy(),
            "stats": nb.node_stats.cpu().numpy().copy()}


def _bars(case, dtype, P, st, ref, st0=None):
    """The bars of a case: 1e-9 for float64 samples; for float32 samples 4 x the yardstick (the
    float32 emulation from the same state -- from ``st0`` through two updates for a reuse case)."""
    if dtype == "float64":
        return {"x": sr.F64_BAR, "d": sr.F64_BAR, "e": sr.F64_BAR, "stats": np.full(6, sr.F64_BAR)}, None
    A32 = sr.as_f32_matrix(P["A"])
    run = lambda s: sr.oracle_update(s, P["plan"], A32, P["b"], P["q_fn"], P["prm"], case.fusion,  # noqa: E731
                                     dtype=np.float32, phantom=P["ph"])
    if st0 is None:
        emu = run(st)
    else:
        emu = run(sr.continue_state(st0, run(st0), **sr.rerandomised(P["plan"], P["n"], case)))
    y = sr.yardstick(ref, emu)
    return {k: sr.F32_FACTOR * v for k, v in y.items()}, y


def _compare(tag, case, dtype, got, ref, bars, yard):
    """Per pixel and per statistic; prints the device / yardstick ratios, then asserts."""
    N = case.N
    errs, where = {}, {}
    for k in ("x", "d", "e"):
        errs[k], at = sr.field_err(got[k], ref[k])
        where[k] = (at[0],) + divmod(at[-1], N) + ((("x", "y")[at[1]],) if len(at) == 3 else ())
    serr = sr.stat_err(got["stats"], ref["stats"])
    if yard is not None:
        ratio = {k: errs[k] / yard[k] if yard[k] > 0 else (0.0 if errs[k] == 0 else math.inf) for k in errs}
        with np.errstate(divide="ignore", invalid="ignore"):
            smax = serr.max(axis=0)
            sratio = np.where(yard["stats"] > 0, smax / yard["stats"], np.where(smax > 0, np.inf, 0.0))
        print(f"\nRATIO {tag} {sr.case_id(case)}: " + " ".join(f"{k}={v:.2f}" for k, v in ratio.items()) + " | "
              + " ".join(f"{nm}={v:.2f}" for nm, v in zip(sr.STAT_NAMES, sratio)))
    else:
        print(f"\nERR64 {tag} {sr.case_id(case)}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()) + " | "
              + " ".join(f"{nm}={v:.1e}" for nm, v in zip(sr.STAT_NAMES, serr.max(axis=0))))
    for k in ("x", "d", "e"):
        assert errs[k] <= bars[k], (f"{tag} {k}: max-abs error {errs[k]:.3e} of the field's max-abs at "
                                    f"(node, i, j[, component]) = {where[k]}, bar {bars[k]:.3e}")
    for v in range(serr.shape[0]):
        for c, nm in enumerate(sr.STAT_NAMES):
            assert serr[v, c] <= bars["stats"][c], (f"{tag} node {v} {nm}: relative error {serr[v, c]:.3e}, "
                                                    f"bar {bars['stats'][c]:.3e}")


def _untouched(nb, st):
    """What an x-update only reads: x_ext rows >= V, y, y_b, z / x_prev, q -- bitwise as written."""
    torch.cuda.synchronize()
    V = nb.V
    assert np.array_equal(nb.x_ext[V:].cpu().numpy(), st["x_ext"][V:])
    for k in ("y", "y_b", "z", "x_prev"):
        if st[k] is not None:
            assert np.array_equal(getattr(nb, k).cpu().numpy(), st[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sr.UPDATE_CASES, ids=sr.case_id)
def test_update_from_random_state(cuda, monkeypatch, case, dtype):
    _set_mirror(monkeypatch, case.mirror)
    P = sr.case_problem(case, dtype)
    nb = _batch(case, dtype, P)
    q0 = nb.q.clone()
    st = sr.random_state(nb, case.seed)
    nb.node_update()
    got = _read(nb)
    ref = sr.oracle_update(st, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
    bars, yard = _bars(case, dtype, P, st, ref)
    _compare(dtype, case, dtype, got, ref, bars, yard)
    _untouched(nb, st)
    assert torch.equal(nb.q, q0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_update_leaves_halo_rows_alone(cuda, monkeypatch, dtype):
    """A batch with halo rows (rank 0 of 2 of an 8-ring; the test fills the halo images itself):
    the update reads z and y of the edges to them and writes only rows < V."""
    case = sr.HALO_CASE
    _set_mirror(monkeypatch, case.mirror)
    P = sr.halo_problem(dtype)
    plan = P["plan"]
    assert plan.V == 4 and plan.n_xext == 6
    nb = _batch(case, dtype, P)
    st = sr.random_state(nb, case.seed)
    nb.node_update()
    got = _read(nb)
    ref = sr.oracle_update(st, plan, P["A"], P["b"], P["q_fn"], P["prm"], case.fusion, phantom=P["ph"])
    bars, yard = _bars(case, dtype, P, st, ref)
    _compare(dtype + " halo", case, dtype, got, ref, bars, yard)
    _untouched(nb, st)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sr.REUSE_CASES, ids=sr.case_id)
def test_reuse_start_from_rerandomised_state(cuda, monkeypatch, case, dtype):
    """ADMM_BATCH_KEEP_X: the second update starts from the first one's A^T(Ax - b)
    (k_start_reuse) with new random d, e, y, z / x_prev around the kept x.  Against the oracle
    continued through the same two steps, and against a keep_x=False batch, which projects x
    again (same bars; not bitwise, A^T A x is formed differently)."""
    _set_mirror(monkeypatch, case.mirror)
    P = sr.case_problem(case, dtype)
    run = lambda s: sr.oracle_update(s, P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], case.fusion,  # noqa: E731
                                     phantom=P["ph"])
    out, st0 = {}, None
    for keep in (True, False):
        nb = _batch(case, dtype, P, keep_x=keep)
        st0 = sr.random_state(nb, case.seed)
        nb.node_update()
        st1 = sr.random_state(nb, case.seed + 1000, keep_x=True)
        nb.node_update()
        out[keep] = _read(nb)
        _untouched(nb, st1)
    ref = run(sr.continue_state(st0, run(st0), **sr.rerandomised(P["plan"], P["n"], case)))
    bars, yard = _bars(case, dtype, P, None, ref, st0=st0)
    _compare(dtype + " reuse", case, dtype, out[True], ref, bars, yard)
    _compare(dtype + " fresh", case, dtype, out[False], ref, bars, yard)
    _compare(dtype + " reuse-vs-fresh", case, dtype, out[True], out[False], bars, yard)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,R", [(4, 1), (2, 3)])
def test_rounds_override_is_bitwise_the_bound_round_count(cuda, monkeypatch, T, R, dtype):
    case = sr.Case(33, 3, "ring", T, 3, "iso", 12, "1", "midpoint", False, 3)
    _set_mirror(monkeypatch, case.mirror)
    P = sr.case_problem(case, dtype)
    out = []
    for bound, rounds in ((T, R), (R, None)):
        nb = _batch(case, dtype, P, tv_iters=bound)
        sr.random_state(nb, case.seed)
        nb.node_update(rounds=rounds)
        out.append(_read(nb))
    assert np.any(out[0]["x"] != 0.0)
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), (k, float(np.max(np.abs(out[0][k] - out[1][k]))))


def _planted(N, tau):
    """(pixel, ux, uy, exact): threshold and zero entries, spread over borders and interior.
    ``exact``: d' = 0 and e' = u hold exactly there."""
    up, dn = np.nextafter(tau, np.inf), np.nextafter(tau, -np.inf)
    vals = [(0.0, 0.0, True), (-0.0, 0.0, True), (0.0, -0.0, True), (-0.0, -0.0, True),
            (tau, 0.0, True), (-tau, 0.0, True), (0.0, tau, True), (0.0, -tau, True),
            (tau, -0.0, True), (-0.0, -tau, True),
            (up, 0.0, False), (-up, 0.0, False), (0.0, up, False), (0.0, -up, False),
            (dn, 0.0, True), (0.0, -dn, True),
            (1e-200, 1e-200, True), (-1e-200, 0.0, True), (0.0, 1e-200, True)]
    spots = [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1), (0, N // 2), (N // 2, 0), (N - 1, N // 2),
             (N // 2, N - 1), (N // 2, N // 2), (1, 1), (N - 2, N - 2), (7, 31), (8, 32), (15, 16), (16, 15),
             (31, 32), (32, 31), (3, 20), (20, 3)]
    assert len(spots) >= len(vals) and len(set(spots)) == len(spots)
    return [(i * N + j, ux, uy, ex) for (i, j), (ux, uy, ex) in zip(spots, vals)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lam", [0.02, 0.0])
@pytest.mark.parametrize("tv_kind", ["iso", "aniso"])
def test_exact_shrink_and_degenerate_cg(cuda, monkeypatch, tv_kind, lam, dtype):
    """x = 0, b = 0, no edges, d = e = U: r = p = 0, so pHp = rr = 0 (alpha = beta = 0 by the
    guards), x stays exactly 0 and u = U exactly.  d', e' against oracle.tv.shrink(U) within 2 ulp,
    and exactly (d' = 0, e' = U) at the planted zeros, thresholds and 1e-200 entries.
    lam = 0 (tau = 0, TV off) as well: for tau > 0 a shrink that took |u| = tau as active would
    still give (s - tau) / s = 0, bit for bit the same; at tau = 0 it divides 0 by 0 at u = 0."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    N, V, a_per = 33, 3, 12
    n = N * N
    mu = 0.2
    tau = lam / mu
    plan = make_plan(nx.empty_graph(V), V)
    ph = sr.shepp_logan(N).reshape(-1).astype(np.float64)
    b = {g: np.zeros(a_per * N) for g in range(V)}
    _, q_fn = sr.precisions(n, V, 1)
    nb = NodeBatch(ParallelBeamGeometry(N, a_per), dtype, plan, b, q_fn, 2.0, lam, mu, 3, 4, tv_kind, ph, 0)
    rng = np.random.default_rng(17)
    U = 0.2 * rng.standard_normal((V, 2, n))
    plants = _planted(N, tau)
    for v in range(V):
        for pix, ux, uy, _ in plants:
            U[v, 0, pix], U[v, 1, pix] = (ux, uy) if v != 1 else (uy, ux)
    nb.x_ext.zero_()
    nb.d.copy_(torch.from_numpy(U))
    nb.e.copy_(torch.from_numpy(U))
    nb.node_update(rounds=1)
    torch.cuda.synchronize()
    x, d, e = nb.x_ext.cpu().numpy(), nb.d.cpu().numpy(), nb.e.cpu().numpy()
    stats = nb.node_stats.cpu().numpy()
    assert np.all(x == 0.0), "x moved: the zero-denominator guards of the CG step"
    for name, a in (("d", d), ("e", e), ("node_stats", stats)):
        assert np.all(np.isfinite(a)), (name, "first non-finite entry at", tuple(np.argwhere(~np.isfinite(a))[0]))
    worst = 0.0
    for v in range(V):
        dx, dy = otv.shrink(U[v, 0], U[v, 1], tau, tv_kind)
        want_d = np.stack([dx, dy])
        want_e = U[v] - want_d
        if tau > 0:
            assert 0.2 < np.mean(want_d != 0.0) < 0.95  # shrink is active on part of the pixels
        with np.errstate(invalid="ignore"):
            ud = np.where(d[v] == want_d, 0.0, sr.ulps(d[v], want_d))
            ue = np.where(e[v] == want_e, 0.0, sr.ulps(e[v], want_e))
        worst = max(worst, float(ud.max()), float(ue.max()))
        assert ud.max() <= 2.0 and ue.max() <= 2.0, (v, float(ud.max()), float(ue.max()),
                                                     divmod(int(np.argmax(ud.max(axis=0))), N))
        for pix, _, _, exact in plants:
            if exact and tau > 0:
                assert np.all(d[v, :, pix] == 0.0), (v, divmod(pix, N), d[v, :, pix])
                assert np.array_equal(e[v, :, pix], U[v, :, pix]), (v, divmod(pix, N), e[v, :, pix])
        kte = mu * otv.div_t(e[v, 0], e[v, 1], N)
        sb, img = math.fsum(kte * kte), math.fsum(ph * ph)
        assert stats[v, 0] == 0.0 and stats[v, 1] == 0.0 and stats[v, 2] == 0.0 and stats[v, 3] == 0.0, stats[v]
        assert abs(stats[v, 4] - img) <= 1e-13 * img, (stats[v, 4], img)
        assert abs(stats[v, 5] - sb) <= 1e-13 * sb, (stats[v, 5], sb)
    print(f"\nSHRINK {tv_kind} lam={lam} {dtype}: worst d', e' error {worst:.2f} ulp")
