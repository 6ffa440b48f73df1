"""CPU: residual-balancing rho and the scale-free stop test -- the float64 restatement
(tests/penalty_ref.py on the unchanged oracle), the host-side checks and rules (admm_hip/penalty.py)
and the C entry points' argument checks.  No GPU.

(a) adaptive_admm with both features off is relax_ref.relaxed_admm bit for bit (midpoint, weighted,
    bounded and relaxed);
(b) on the 4-node ring at 16^2 (6 angles per node, sigma = 0.5, seed 3) fixed rho_0 = 0.05 and rho_0 = 20
    do not reach primal, dual < 1e-2 in 300 iterations; balancing from either does, in no more
    iterations than fixed rho = 1, and ends within 1e-3 of the rho = 1 images;
(c) a rho change keeps the unscaled dual rho y bitwise (factor 2);
(d) the scale-free test stops a problem and its 64-fold multiple at the same iteration; the absolute
    test does not;
(e) check_adapt_rho / balance / check_stop_tolerances / thresholds on planted values, run_admm's
    refusals before device work, the signature order, the drop-ins, the params file;
(f) admm_batch_set_rho, admm_node_norms and admm_node_norms_work refuse every bad argument before any
    HIP call.
"""
import ctypes as C
import inspect
import math

import networkx as nx
import numpy as np
import pytest

import penalty_ref as pr
import relax_ref as rr
from admm_hip import penalty as pen
from test_relax_cpu import KEYS, q_of, ring_problem, same_history
import bounds_ref as br


# --------------------------------------------------------------------------------------
# (a) off is the relaxed loop, bit for bit
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return ring_problem(12, 3, 6, 0.5, 5)


@pytest.mark.parametrize("variant", ["midpoint", "weighted", "bounds"])
def test_features_off_is_the_relaxed_loop(small, variant):
    ops, b, G, W, ph = small
    kw = dict(lam_tv=0.01, rho=2.0, max_iters=5, phantom_true=ph, alpha=1.6, Wi_list=W)
    if variant == "bounds":
        kw["bounds"] = (0.0, 1.0)
    else:
        kw["fusion"] = variant
    xo, wo, ho = rr.relaxed_admm(ops, b, G, q_of(W), 12, **kw)
    x, w, h = pr.adaptive_admm(ops, b, G, q_of(W), 12, adapt=None, eps_abs=None, eps_rel=None, **kw)
    assert set(h) == set(ho)
    assert all(np.array_equal(a, c) for a, c in zip(x, xo))
    assert (w is None) == (wo is None) and (w is None or all(np.array_equal(a, c) for a, c in zip(w, wo)))
    same_history(h, ho, KEYS + (br.BOUND_KEYS if variant == "bounds" else ()))
    # and with a feature on it is another run with more keys
    x2, _, h2 = pr.adaptive_admm(ops, b, G, q_of(W), 12, adapt=dict(ratio=1.5), eps_abs=1e-9, eps_rel=1e-9, **kw)
    assert set(h2) - set(h) == {"rho_history", "margins"} | set(pr.NORM_KEYS)
    assert len(set(h2["rho_history"])) > 1 and not np.array_equal(x2[0], x[0])


# --------------------------------------------------------------------------------------
# (b) convergence: the 16^2 ring, 300 iterations
# --------------------------------------------------------------------------------------
TOL, ITERS = 1e-2, 300


@pytest.fixture(scope="module")
def ring16():
    return ring_problem(16, 4, 6, 0.5, 3)


@pytest.fixture(scope="module")
def tuned(ring16):
    ops, b, G, W, ph = ring16
    x, _, h = pr.adaptive_admm(ops, b, G, q_of(W), 16, lam_tv=0.01, rho=1.0, max_iters=ITERS)
    return np.stack(x), rr.iters_to(h, TOL)


@pytest.mark.parametrize("rho0", [0.05, 20.0])
def test_balancing_from_a_bad_rho_beats_the_tuned_rho(ring16, tuned, rho0):
    ops, b, G, W, ph = ring16
    x1, k1 = tuned
    kw = dict(lam_tv=0.01, rho=rho0, max_iters=ITERS)
    xf, _, hf = pr.adaptive_admm(ops, b, G, q_of(W), 16, **kw)
    xa, _, ha = pr.adaptive_admm(ops, b, G, q_of(W), 16, adapt=True, **kw)
    kf, ka = rr.iters_to(hf, TOL), rr.iters_to(ha, TOL)
    rh = np.asarray(ha["rho_history"])
    changes = int(np.sum(rh[1:] != rh[:-1]))
    df = float(np.linalg.norm(np.stack(xf) - x1) / np.linalg.norm(x1))
    da = float(np.linalg.norm(np.stack(xa) - x1) / np.linalg.norm(x1))
    print(f"\nRING16 rho_0={rho0}: iterations to primal, dual < {TOL}: fixed rho=1 {k1}, fixed rho_0 {kf}, "
          f"balanced {ka} ({changes} changes, final rho {rh[-1]}); images vs rho=1 after {ITERS}: fixed rel {df:.2e}, "
          f"balanced rel {da:.2e}")
    assert k1 is not None and kf is None
    assert ka is not None and ka <= k1, (ka, k1)
    assert da < 1e-3 and da < df
    assert 1 <= changes <= 8 and len(rh) == ITERS and rh[0] == rho0


# --------------------------------------------------------------------------------------
# (c) the dual rescale
# --------------------------------------------------------------------------------------
def test_a_rho_change_keeps_the_unscaled_dual_bitwise(small):
    ops, b, G, W, ph = small
    trace = []
    pr.adaptive_admm(ops, b, G, q_of(W), 12, adapt=True, lam_tv=0.01, rho=16.0, max_iters=6, trace=trace)
    assert trace
    for k, old, new, before, after in trace:
        assert new in (old * 2.0, old / 2.0)
        for e in before:
            assert np.any(before[e] != 0.0)
            assert np.array_equal(new * after[e], old * before[e]), (k, e)
    # NodeBatch.set_rho's arithmetic: one multiplication by c = rho_old / rho_new
    y = np.random.default_rng(0).standard_normal(1000)
    for old, new in ((20.0, 10.0), (1.25, 2.5), (0.3, 0.6)):
        assert np.array_equal(new * (y * (old / new)), old * y)


# --------------------------------------------------------------------------------------
# (d) scale invariance of the stop test
# --------------------------------------------------------------------------------------
def test_scale_free_test_stops_a_scaled_problem_at_the_same_iteration(ring16):
    """b -> 64 b, lambda -> 64 lambda with the split-Bregman mu held fixed: x, z, y scale by 64 exactly
    (a power of two), so r, s and the relative thresholds do, and eps_abs = 0 stops both runs alike."""
    ops, b, G, W, ph = ring16
    stops = {}
    for c in (1.0, 64.0):
        kw = dict(lam_tv=0.01 * c, mu=0.1, rho=1.0)
        bs = [c * v for v in b]
        _, _, hb = pr.adaptive_admm(ops, bs, G, q_of(W), 16, eps_abs=0.0, eps_rel=1e-3, max_iters=150, **kw)
        _, _, ha = pr.adaptive_admm(ops, bs, G, q_of(W), 16, eps_pri=TOL, eps_dual=TOL, max_iters=150, **kw)
        stops[c] = (len(hb["primal"]), len(ha["primal"]), hb)
    print(f"\nSCALE: scale-free test stops at {stops[1.0][0]} / {stops[64.0][0]}, absolute test at "
          f"{stops[1.0][1]} / {stops[64.0][1]} (of 150)")
    assert stops[1.0][0] == stops[64.0][0] < 150
    assert stops[1.0][1] < 150 and stops[64.0][1] == 150
    for key in ("primal", "dual") + pr.NORM_KEYS:
        assert np.array_equal(64.0 * np.asarray(stops[1.0][2][key]), np.asarray(stops[64.0][2][key])), key


# --------------------------------------------------------------------------------------
# (e) host-side checks and rules
# --------------------------------------------------------------------------------------
def test_check_adapt_rho_accepts_and_completes():
    assert pen.check_adapt_rho(None, 1.0) is None and pen.check_adapt_rho(False, 1.0) is None
    assert pen.check_adapt_rho(None, float("nan")) is None  # off: rho is not looked at
    d = pen.check_adapt_rho(True, 2.0)
    assert d == dict(ratio=10.0, factor=2.0, every=1, until=None, rho_min=2.0 / 1024, rho_max=2.0 * 1024)
    assert pen.check_adapt_rho({}, 2.0) == d
    d = pen.check_adapt_rho(dict(ratio=np.float32(5), factor=3, every=np.int64(4), until=0, rho_min=2.0, rho_max=2.0), 2)
    assert d == dict(ratio=5.0, factor=3.0, every=4, until=0, rho_min=2.0, rho_max=2.0)
    assert all(type(d[k]) is float for k in ("ratio", "factor", "rho_min", "rho_max")) and type(d["every"]) is int


@pytest.mark.parametrize("bad", [
    1, "on", [("ratio", 10)], dict(rato=10), dict(ratio=1.0), dict(ratio=True), dict(ratio=float("nan")),
    dict(ratio=math.inf), dict(factor=1.0), dict(factor=0.5), dict(factor=False), dict(factor="2"), dict(every=0),
    dict(every=1.0), dict(every=True), dict(until=-1), dict(until=2.5), dict(until=True), dict(rho_min=0.0),
    dict(rho_min=2.0), dict(rho_max=0.5), dict(rho_max=math.inf), dict(rho_min=float("nan")), dict(rho_max=True)])
def test_check_adapt_rho_rejects(bad):
    with pytest.raises(ValueError):
        pen.check_adapt_rho(bad, 1.0)


@pytest.mark.parametrize("rho", [0.0, -1.0, math.inf, float("nan"), True, "1", None])
def test_check_adapt_rho_rejects_a_bad_rho(rho):
    with pytest.raises(ValueError):
        pen.check_adapt_rho(True, rho)


def test_balance_on_planted_values():
    cfg = pen.check_adapt_rho(True, 1.0)
    assert pen.balance(1.0, 11.0, 1.0, cfg, 0) == 2.0 and pen.balance(1.0, 1.0, 11.0, cfg, 0) == 0.5
    assert pen.balance(1.0, 10.0, 1.0, cfg, 0) == 1.0 and pen.balance(1.0, 1.0, 10.0, cfg, 0) == 1.0  # strict
    assert pen.balance(1.0, 1.0, 0.0, cfg, 0) == 2.0 and pen.balance(1.0, 0.0, 0.0, cfg, 0) == 1.0
    for r, s in ((math.nan, 1.0), (1.0, math.nan), (math.inf, 1.0), (1.0, math.inf)):
        assert pen.balance(1.0, r, s, cfg, 0) == 1.0
    assert pen.balance(1024.0, 11.0, 1.0, cfg, 0) == 1024.0 and pen.balance(1.0 / 1024, 1.0, 11.0, cfg, 0) == 1.0 / 1024
    c3 = pen.check_adapt_rho(dict(factor=3.0, ratio=2.0, rho_max=2.5, rho_min=0.4), 1.0)
    assert pen.balance(1.0, 3.0, 1.0, c3, 0) == 2.5 and pen.balance(1.0, 1.0, 3.0, c3, 0) == 0.4  # the clamps
    ce = pen.check_adapt_rho(dict(every=3, until=6), 1.0)
    fired = [k for k in range(12) if pen.balance(1.0, 11.0, 1.0, ce, k) != 1.0]
    assert fired == [2, 5]  # after iterations 3 and 6 (1-based), none after ``until``
    assert pen.balance(1.0, 11.0, 1.0, pen.check_adapt_rho(dict(until=0), 1.0), 0) == 1.0
    # the restatement agrees
    rng = np.random.default_rng(1)
    for k in range(200):
        r, s, rho = (float(v) for v in np.exp(rng.uniform(-6, 6, 3)))
        assert pen.balance(rho, r, s, ce, k) == pr.balance_ref(rho, r, s, ce, k)[0]


def test_check_stop_tolerances():
    assert pen.check_stop_tolerances(None, None) is None
    assert pen.check_stop_tolerances(1e-4, 1e-3) == (1e-4, 1e-3) and pen.check_stop_tolerances(0, 1e-3) == (0.0, 1e-3)
    assert pen.check_stop_tolerances(None, 1e-3) == (0.0, 1e-3) and pen.check_stop_tolerances(np.float32(0.5), None) == (0.5, 0.0)
    for bad in ((0.0, 0.0), (None, 0.0), (-1e-3, 1e-3), (1e-3, -1.0), (math.nan, 1e-3), (1e-3, math.inf), (True, 1e-3),
                (1e-3, False), ("1e-3", 1e-3), (1e-3, [1e-3])):
        with pytest.raises(ValueError):
            pen.check_stop_tolerances(*bad)
    pen.check_tolerance_run(None, "derived", "derived")
    pen.check_tolerance_run((0.0, 1e-3), None, "")
    pen.check_tolerance_run((0.0, 1e-3), "stored", "derived")
    for es, env in (("derived", ""), (None, "derived")):
        with pytest.raises(ValueError, match="stored z"):
            pen.check_tolerance_run((0.0, 1e-3), es, env)


def test_thresholds_on_planted_values():
    edges = [(0, 1), (1, 2), (0, 2), (2, 3)]
    assert pen.incidences(edges, 4, False).tolist() == [2, 2, 3, 1] and pen.incidences(edges, 4, True).tolist() == [3, 3, 4, 2]
    assert pen.incidences([], 1, False).tolist() == [0]
    ninc = np.array([2.0, 2.0, 3.0, 1.0])
    norms = np.array([[4.0, 9.0, 1.0], [0.0, 16.0, 0.0], [1.0, 0.0, 3.0], [9.0, 0.0, 0.0]])
    ep, ed, ax, bz, aty = pen.thresholds(0.5, 0.25, 100, ninc, norms, 3.0)
    assert ax == math.sqrt(2 * 4 + 3 * 1 + 9) and bz == 5.0 and aty == 3.0 * 2.0
    assert ep == math.sqrt(100 * 8) * 0.5 + 0.25 * 5.0 and ed == math.sqrt(100 * 4) * 0.5 + 0.25 * 6.0
    assert pen.thresholds(0.0, 1.0, 100, ninc, norms, 1.0)[:2] == (5.0, 2.0)  # max(||Ax||, ||Bz||): ||Bz|| here
    assert pen.thresholds(0.0, 1.0, 100, ninc, norms * [4.0, 1.0, 1.0], 1.0)[0] == 2 * math.sqrt(20)
    got, want = pen.thresholds(1e-4, 1e-3, 49, ninc, norms, 0.7), pr.thresholds_ref(1e-4, 1e-3, 49, ninc, norms, 0.7)
    assert np.allclose(got, want, rtol=1e-15, atol=0)


def test_node_norms_ref_on_planted_values():
    x = np.array([[1.0, 2.0], [3.0, 4.0], [0.5, 0.0]])
    y = np.array([[1.0, -2.0], [0.25, 8.0]])
    yb = np.array([[5.0, 5.0], [7.0, 7.0]])
    z = np.array([[2.0, 1.0], [3.0, 0.0]])
    off, edge, sign = [0, 2, 3, 3], [0, 1, 1], [1, -1, 1]
    got = pr.node_norms_ref(x, y, None, z, off, edge, sign)
    assert got.tolist() == [[5.0, 4.0 + 9.0 + 1.0, 0.75 ** 2 + 10.0 ** 2], [25.0, 9.0, 0.0625 + 64.0], [0.25, 0.0, 0.0]]
    got = pr.node_norms_ref(x, y, yb, z, off, edge, sign)
    assert got[0].tolist() == [5.0, 14.0, 8.0 ** 2 + 5.0 ** 2] and got[1].tolist() == [25.0, 9.0, 0.0625 + 64.0]


def test_run_admm_rejects_bad_keywords_before_any_device_work(monkeypatch):
    """The keyword checks come before the operators are touched: stand-in operators are enough."""
    from admm_hip.admm import run_admm
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    args = ([object()] * 3, [None] * 3, nx.cycle_graph(3), [None] * 3, None, 8)
    for kw in (dict(adapt_rho=1), dict(adapt_rho=dict(ratio=1.0)), dict(adapt_rho=dict(nope=1)),
               dict(adapt_rho=dict(factor=float("nan"))), dict(adapt_rho=True, rho=0.0),
               dict(adapt_rho=dict(every=True)), dict(adapt_rho=dict(rho_min=5.0), rho=1.0)):
        with pytest.raises(ValueError, match="adapt_rho"):
            run_admm(*args, verbose=False, **kw)
    for kw in (dict(eps_abs=0.0, eps_rel=0.0), dict(eps_abs=-1.0), dict(eps_rel=float("nan")), dict(eps_rel=True),
               dict(eps_abs=1e-3, eps_rel=float("inf"))):
        with pytest.raises(ValueError, match="eps_abs|eps_rel"):
            run_admm(*args, verbose=False, **kw)
    with pytest.raises(ValueError, match="stored z"):
        run_admm(*args, verbose=False, eps_rel=1e-3, edge_state="derived")
    monkeypatch.setenv("ADMM_EDGE_STATE", "derived")
    with pytest.raises(ValueError, match="stored z"):
        run_admm(*args, verbose=False, eps_rel=1e-3)
    # adapt_rho alone works with either edge state: the check passes and the stand-ins fail next
    with pytest.raises(ValueError, match="a matrix must be 2-D"):
        run_admm(*args, verbose=False, adapt_rho=True, edge_state="derived")


def test_need_stored_z_names_the_tolerances():
    from admm_hip.plan import need_stored_z
    need_stored_z(True, False, False, "run")
    need_stored_z(False, True, True, "run", True)
    with pytest.raises(ValueError, match="eps_abs / eps_rel need stored z.*stored-z rule"):
        need_stored_z(True, False, False, "run", True)
    assert inspect.signature(need_stored_z).parameters["tolerances"].default is False


def test_signature_order_and_dropins_forward_the_keywords():
    import block_6_admm_loop
    import block_6_admm_loop_ver2
    from admm_hip import admm
    new = ["adapt_rho", "eps_abs", "eps_rel"]
    names = list(inspect.signature(admm.run_admm).parameters)
    at = names.index("metrics_mask")
    assert names[at + 1:at + 4] == new and names[at + 4] == "relaxation"
    assert names[-5:] == ["relaxation", "bounds", "bound_weight", "return_feasible", "ray_weights"]
    for mod in (block_6_admm_loop, block_6_admm_loop_ver2):
        sig = inspect.signature(mod.decentralized_admm).parameters
        assert list(sig)[-8:-5] == new and list(sig)[-5] == "relaxation"
        assert all(sig[k].default is None for k in new) and all(k in mod.__doc__ for k in new)
        seen = {}

        def fake(*a, **kw):
            seen.update(kw)
            return [], {"primal": [], "dual": [], "obj_total": []}

        orig = mod.run_admm
        mod.run_admm = fake
        try:
            mod.decentralized_admm(None, None, None, None, None, 8, adapt_rho=dict(ratio=5.0), eps_abs=1e-4, eps_rel=1e-3)
        finally:
            mod.run_admm = orig
        assert seen["adapt_rho"] == dict(ratio=5.0) and seen["eps_abs"] == 1e-4 and seen["eps_rel"] == 1e-3
    for k in ("rho_history",) + pen.NORM_KEYS:
        assert k not in admm.HISTORY_KEYS + admm.EXTRA_KEYS
    assert pen.NORM_KEYS == pr.NORM_KEYS


def test_params_file_names_the_balancing_only_when_on(tmp_path):
    from admm_hip.admm import _write_params
    cfg = pen.check_adapt_rho(True, 20.0)
    _write_params(str(tmp_path / "off"), 20.0, 0.01, 4, 0.1, 10, 5)
    _write_params(str(tmp_path / "on"), 2.5, 0.01, 4, 0.1, 10, 5, None, (20.0, cfg, 3))
    off = (tmp_path / "off" / "admm_internal_params.txt").read_text()
    on = (tmp_path / "on" / "admm_internal_params.txt").read_text()
    assert "balancing" not in off.lower() and "rho = 20.0\n" in off
    assert "rho = 2.5\n" in on  # the rho the last iteration ran with
    line = [ln for ln in on.splitlines() if ln.startswith("Residual balancing")]
    assert len(line) == 1 and "rho_0 = 20.0" in line[0] and "ratio = 10.0" in line[0] and "changes = 3" in line[0]
    rest = lambda t: [ln for ln in t.splitlines() if not ln.startswith(("rho =", "Residual", "Date"))]  # noqa: E731
    assert rest(on) == rest(off)


# --------------------------------------------------------------------------------------
# (f) the C entry points refuse bad arguments before any HIP call
# --------------------------------------------------------------------------------------
def test_c_entry_points_refuse_bad_arguments():
    from admm_hip import _lib
    lib = _lib.load()
    buf = (C.c_double * 8)()  # a host address: the checks never read through a pointer
    p, z = C.c_void_p(C.addressof(buf)), C.c_void_p(0)

    def refused(fn, args, what, rc_want=-1):
        rc = fn(*args)
        msg = lib.admm_last_error()
        assert rc == rc_want and msg, (what, rc, msg)
        return msg

    for rho in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert b"rho" in refused(lib.admm_batch_set_rho, (z, rho, z), rho)
    assert b"no batch bound" in refused(lib.admm_batch_set_rho, (z, 1.0, z), "no ctx", _lib_state())

    need = C.c_longlong(-7)
    assert lib.admm_node_norms_work(1089, 3, C.byref(need)) == 0 and need.value == 3 * 2 * 3
    assert lib.admm_node_norms_work(1, 1, C.byref(need)) == 0 and need.value == 3
    for args in ((0, 3, C.byref(need)), (1089, 0, C.byref(need)), (1089, 65536, C.byref(need)), (1089, 3, None)):
        refused(lib.admm_node_norms_work, args, args[:2])

    #     x  xs  y  y_b z  n   nimg off edge sign ne work out stream
    ok = [p, 64, p, z, p, 64, 2, p, p, p, 3, p, p, z]
    bad = [(0, z, b"x is null"), (7, z, b"inc_off"), (11, z, b"work"), (12, z, b"out"), (2, z, b"y or z"),
           (4, z, b"y or z"), (8, z, b"inc_edge"), (9, z, b"inc_edge"), (10, -1, b"n_edges"), (5, 0, b"n must"),
           (6, 0, b"nimg"), (6, 65536, b"nimg"), (1, 63, b"x_stride")]
    for i, v, word in bad:
        args = list(ok)
        args[i] = v
        assert word in refused(lib.admm_node_norms, args, (i, v)), (i, v)


def _lib_state():
    return -3  # ADMM_E_STATE (include/admm_tomo.h)
