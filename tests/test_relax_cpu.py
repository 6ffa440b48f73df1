"""CPU: over-relaxation's float64 restatement (tests/relax_ref.py on the unchanged oracle), the
host-side argument checks (admm_hip/relax.py) and the C entry points' argument checks.  No GPU.

(a) relaxed_admm(alpha = 1) is the oracle's loop bit for bit (midpoint, weighted, bounded);
(b) on the 4-node ring at 16^2 (6 angles per node, sigma = 0.5, seed 3) alpha = 1.6 needs at most
    0.75 x the iterations of alpha = 1 to primal, dual < 1e-2 -- with bounds (0, 1) too -- and reaches
    the same images;
(c) check_relaxation / check_relaxed_run, run_admm's refusals before device work, the drop-ins;
(d) admm_consensus_relaxed, admm_consensus_relaxed_work and admm_bound_project_relaxed return -1 with a
    message for every bad argument, before any HIP call.
"""
import ctypes as C
import inspect
import math

import networkx as nx
import numpy as np
import pytest

import bounds_ref as br
import relax_ref as rr
from admm_hip.relax import check_relaxation, check_relaxed_run
from oracle.admm import decentralized_admm
from oracle.geometry import Geometry, joseph_matrix


def q_of(W):
    return lambda i, j: np.maximum(0.5 * (W[i] + W[j]), 1e-12)


def ring_problem(N, V, a_per, sigma, seed):
    A = joseph_matrix(Geometry(N, a_per))
    ph = br.blocks_phantom(N)
    rng = np.random.default_rng(seed)
    b = [A @ ph + sigma * rng.standard_normal(A.shape[0]) for _ in range(V)]
    W = [br.column_weights(A)] * V
    return [A] * V, b, nx.cycle_graph(V), W, ph


# --------------------------------------------------------------------------------------
# (a) alpha = 1 is the unrelaxed loop, bit for bit
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return ring_problem(12, 3, 6, 0.5, 5)


KEYS = ("primal", "dual", "obj_total", "pri_per_node", "dual_per_node", "mse_sino_total", "img_mse_total")


def same_history(h, ho, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(h[k]), np.asarray(ho[k])), k


@pytest.mark.parametrize("fusion", ["midpoint", "weighted"])
def test_alpha_one_is_the_oracle_loop(small, fusion):
    ops, b, G, W, ph = small
    kw = dict(lam_tv=0.01, rho=1.0, max_iters=6, phantom_true=ph)
    xo, ho = decentralized_admm(ops, b, G, q_of(W), 12, eps_pri=0.0, eps_dual=0.0, fusion=fusion, Wi_list=W, **kw)
    x, w, h = rr.relaxed_admm(ops, b, G, q_of(W), 12, alpha=1.0, fusion=fusion, Wi_list=W, **kw)
    assert w is None and set(h) == set(ho)
    assert all(np.array_equal(a, c) for a, c in zip(x, xo))
    same_history(h, ho)
    # and another alpha is another trajectory
    x2, _, _ = rr.relaxed_admm(ops, b, G, q_of(W), 12, alpha=1.6, fusion=fusion, Wi_list=W, **kw)
    assert max(float(np.max(np.abs(a - c))) for a, c in zip(x2, xo)) > 1e-3


def test_alpha_one_with_bounds_is_the_bounded_loop(small):
    ops, b, G, W, ph = small
    kw = dict(lam_tv=0.01, rho=1.0, max_iters=6, phantom_true=ph)
    xo, wo, _, ho = br.bounded_admm(ops, b, G, q_of(W), W, 12, (0.0, 1.0), **kw)
    x, w, h = rr.relaxed_admm(ops, b, G, q_of(W), 12, alpha=1.0, Wi_list=W, bounds=(0.0, 1.0), **kw)
    assert all(np.array_equal(a, c) for a, c in zip(x, xo)) and all(np.array_equal(a, c) for a, c in zip(w, wo))
    same_history(h, ho, KEYS + br.BOUND_KEYS)


def test_restatements_on_planted_values():
    """The operation order of the two restatements, on values whose roundings tell the orders apart."""
    x_ext = np.array([[1.0, 0.1, 3.0], [2.0, 0.7, -1.0]])
    y, z = np.array([[0.5, 1e-17, 0.25]]), np.array([[4.0, 0.3, 1.0]])
    a = 1.6
    om = 1.0 - a
    yn, zn, ybn, s = rr.edge_ref(x_ext, y, z, [0], [1], a)
    xha, xhb = a * x_ext[0] + om * z[0], a * x_ext[1] + om * z[0]
    assert ybn is None and np.array_equal(zn[0], ((xha + y[0]) + (xhb - y[0])) * 0.5)
    assert np.array_equal(yn[0], (y[0] + xha) - zn[0])
    assert s[0, 2] == math.fsum((zn[0] - z[0]) ** 2) and s[0, 0] == math.fsum((x_ext[0] - zn[0]) ** 2)
    # alpha = 1: the plain update
    yn1, zn1, _, _ = rr.edge_ref(x_ext, y, z, [0], [1], 1.0)
    assert np.array_equal(zn1[0], ((x_ext[0] + y[0]) + (x_ext[1] - y[0])) * 0.5)
    assert np.array_equal(yn1[0], y[0] + x_ext[0] - zn1[0])
    # the single-y invariant: xha - z' = -(xhb - z') up to rounding
    assert np.max(np.abs((xha - zn[0]) + (xhb - zn[0]))) < 1e-15
    # weighted: both duals move, W = 1 is the midpoint up to rounding
    W = np.ones((2, 3))
    yw, zw, ybw, _ = rr.edge_ref(x_ext, y, z, [0], [1], a, y_b=-y, W=W)
    assert np.allclose(zw, zn, rtol=0, atol=1e-15) and np.allclose(ybw, -yw, rtol=0, atol=1e-15)
    wn, fn, sums = rr.project_ref(x_ext, z.repeat(2, 0), y.repeat(2, 0), np.zeros(3), np.ones(3), a)
    t = (a * x_ext + om * z) + y
    assert np.array_equal(wn, br.clip(t, 0.0, 1.0)) and np.array_equal(fn, t - wn)
    assert sums[1, 2] == math.fsum((x_ext[1] - br.clip(x_ext[1], 0.0, 1.0)) ** 2)


# --------------------------------------------------------------------------------------
# (b) convergence: the 16^2 ring, 300 iterations
# --------------------------------------------------------------------------------------
TOL, ITERS, ALPHA = 1e-2, 300, 1.6


@pytest.fixture(scope="module")
def ring16():
    return ring_problem(16, 4, 6, 0.5, 3)


def test_relaxation_cuts_the_iterations_and_keeps_the_fixed_point(ring16):
    ops, b, G, W, ph = ring16
    kw = dict(lam_tv=0.01, rho=1.0, max_iters=ITERS)
    x1, _, h1 = rr.relaxed_admm(ops, b, G, q_of(W), 16, alpha=1.0, **kw)
    xr, _, hr = rr.relaxed_admm(ops, b, G, q_of(W), 16, alpha=ALPHA, **kw)
    k1, kr = rr.iters_to(h1, TOL), rr.iters_to(hr, TOL)
    d = float(np.linalg.norm(np.stack(xr) - np.stack(x1)) / np.linalg.norm(np.stack(x1)))
    print(f"\nRING16: iterations to primal, dual < {TOL}: alpha=1 {k1}, alpha={ALPHA} {kr}; images rel {d:.2e}")
    assert k1 is not None and kr is not None
    assert kr <= 0.75 * k1, (kr, k1)
    assert d < 1e-3


def test_relaxation_cuts_the_iterations_with_bounds(ring16):
    ops, b, G, W, ph = ring16
    keys = ("primal", "dual", "bound_primal", "bound_dual")
    # (the loops stop at the test's own tolerance: the count is the history's length)
    kw = dict(lam_tv=0.01, rho=1.0, max_iters=ITERS, Wi_list=W, bounds=(0.0, 1.0), eps_pri=TOL, eps_dual=TOL)
    _, _, h1 = rr.relaxed_admm(ops, b, G, q_of(W), 16, alpha=1.0, **kw)
    _, _, hr = rr.relaxed_admm(ops, b, G, q_of(W), 16, alpha=ALPHA, **kw)
    k1, kr = rr.iters_to(h1, TOL, keys), rr.iters_to(hr, TOL, keys)
    print(f"\nRING16 bounds (0, 1): iterations to all four residuals < {TOL}: alpha=1 {k1}, alpha={ALPHA} {kr}")
    assert k1 is not None and kr is not None and k1 == len(h1["primal"]) and kr == len(hr["primal"])
    assert kr <= 0.75 * k1, (kr, k1)


# --------------------------------------------------------------------------------------
# (c) host-side checks
# --------------------------------------------------------------------------------------
def test_check_relaxation_accepts_and_normalises():
    assert check_relaxation(None) is None
    assert check_relaxation(1.0) is None and check_relaxation(1) is None and check_relaxation(np.float64(1.0)) is None
    assert check_relaxation(1.6) == 1.6 and isinstance(check_relaxation(np.float32(1.5)), float)
    assert check_relaxation(0.5) == 0.5 and check_relaxation(np.nextafter(2.0, 0.0)) < 2.0
    assert check_relaxation(5e-324) > 0.0


@pytest.mark.parametrize("bad", [True, False, float("nan"), 0.0, -0.5, 2.0, 2.5, math.inf, -math.inf, "1.6", [1.6],
                                 1.6 + 0j],
                         ids=["True", "False", "nan", "0", "neg", "2", "2.5", "inf", "-inf", "str", "list", "complex"])
def test_check_relaxation_rejects(bad):
    with pytest.raises(ValueError):
        check_relaxation(bad)


def test_check_relaxed_run():
    check_relaxed_run(None, "derived", "derived")  # no relaxation: nothing to object to
    check_relaxed_run(1.6, None, "")
    check_relaxed_run(1.6, "stored", "derived")  # the argument overrides the environment
    with pytest.raises(ValueError, match="stored z"):
        check_relaxed_run(1.6, "derived", "")
    with pytest.raises(ValueError, match="stored z"):
        check_relaxed_run(1.6, None, "derived")


def test_run_admm_rejects_bad_relaxation_before_any_device_work(monkeypatch):
    """The keyword checks come before the operators are touched: stand-in operators are enough."""
    from admm_hip.admm import run_admm
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    args = ([object()] * 3, [None] * 3, nx.cycle_graph(3), [None] * 3, None, 8)
    for kw in (dict(relaxation=True), dict(relaxation=0.0), dict(relaxation=2.0), dict(relaxation=float("nan")),
               dict(relaxation=-1.0), dict(relaxation=1.6, edge_state="derived")):
        with pytest.raises(ValueError, match="relaxation"):
            run_admm(*args, verbose=False, **kw)
    monkeypatch.setenv("ADMM_EDGE_STATE", "derived")
    with pytest.raises(ValueError, match="stored z"):
        run_admm(*args, verbose=False, relaxation=1.6)


def test_dropins_forward_the_keyword():
    import block_6_admm_loop
    import block_6_admm_loop_ver2
    from admm_hip import admm
    # a keyword with default None after every older one, in front of the bounds group and ray_weights,
    # whose places at the end test_bounds_cpu.py and test_ray_weights_cpu.py fix
    names = list(inspect.signature(admm.run_admm).parameters)
    assert names[-5:] == ["relaxation", "bounds", "bound_weight", "return_feasible", "ray_weights"]
    assert inspect.signature(admm.run_admm).parameters["relaxation"].default is None
    for mod in (block_6_admm_loop, block_6_admm_loop_ver2):
        sig = inspect.signature(mod.decentralized_admm).parameters
        assert list(sig)[-5] == "relaxation" and sig["relaxation"].default is None
        assert "relaxation" in mod.__doc__
        seen = {}

        def fake(*a, **kw):
            seen.update(kw)
            return [], {"primal": [], "dual": [], "obj_total": []}

        orig = mod.run_admm
        mod.run_admm = fake
        try:
            mod.decentralized_admm(None, None, None, None, None, 8, relaxation=1.7)
        finally:
            mod.run_admm = orig
        assert seen["relaxation"] == 1.7
    assert "relaxation" not in admm.HISTORY_KEYS + admm.EXTRA_KEYS


def test_params_file_names_alpha_only_when_relaxed(tmp_path):
    from admm_hip.admm import _write_params
    _write_params(str(tmp_path / "off"), 1.0, 0.01, 4, 0.1, 10, 5)
    _write_params(str(tmp_path / "on"), 1.0, 0.01, 4, 0.1, 10, 5, 1.6)
    off = (tmp_path / "off" / "admm_internal_params.txt").read_text()
    on = (tmp_path / "on" / "admm_internal_params.txt").read_text()
    assert "relaxation" not in off.lower() and "Over-relaxation alpha = 1.6\n" in on
    assert [ln for ln in on.splitlines() if "relax" not in ln.lower() and "Date" not in ln] == \
           [ln for ln in off.splitlines() if "Date" not in ln]


# --------------------------------------------------------------------------------------
# (d) the C entry points refuse bad arguments before any HIP call
# --------------------------------------------------------------------------------------
def test_c_entry_points_refuse_bad_arguments():
    from admm_hip import _lib
    lib = _lib.load()
    buf = (C.c_double * 8)()  # a host address: the checks never read through a pointer
    p, z = C.c_void_p(C.addressof(buf)), C.c_void_p(0)
    nan, inf = float("nan"), math.inf

    def refused(fn, args, what):
        rc = fn(*args)
        msg = lib.admm_last_error()
        assert rc == -1 and msg, (what, rc, msg)
        return msg

    need = C.c_longlong(-7)
    assert lib.admm_consensus_relaxed_work(1089, 3, C.byref(need)) == 0 and need.value == 3 * 2 * 3
    assert lib.admm_consensus_relaxed_work(4096, 16, C.byref(need)) == 0 and need.value == 3 * 4 * 16
    for args in ((0, 3, C.byref(need)), (1089, -1, C.byref(need)), (1089, 3, None)):
        refused(lib.admm_consensus_relaxed_work, args, args[:2])

    #      x_ext n  rows y  y_b z  w  ea eb e0 e1 alpha work stats stream
    ok = [p, 64, 2, p, z, p, z, p, p, 0, 1, 1.6, p, p, z]
    bad = [(0, z, b"null"), (3, z, b"null"), (5, z, b"null"), (7, z, b"null"), (8, z, b"null"), (12, z, b"null"),
           (13, z, b"null"), (4, p, b"pair"), (6, p, b"pair"), (9, -1, b"e0"), (10, -1, b"e0"), (1, 0, b"n must"),
           (2, 0, b"n_rows"), (11, 0.0, b"alpha"), (11, 2.0, b"alpha"), (11, -1.0, b"alpha"), (11, nan, b"alpha"),
           (11, inf, b"alpha")]
    for i, v, word in bad:
        args = list(ok)
        args[i] = v
        assert word in refused(lib.admm_consensus_relaxed, args, (i, v)), (i, v)
    args = list(ok)
    args[9], args[10] = 2, 1  # e1 < e0
    refused(lib.admm_consensus_relaxed, args, "e1 < e0")
    args[9], args[10], args[11] = 1, 1, 1.6  # an empty range is legal and launches nothing
    assert lib.admm_consensus_relaxed(*args) == 0

    #      x  xs  w  f  ws  lo_map hi_map lo   hi   n   nimg alpha work out stream
    okb = [p, 64, p, p, 64, z, z, 0.0, 1.0, 64, 2, 1.6, p, p, z]
    badb = [(0, z), (2, z), (3, z), (12, z), (13, z), (1, 63), (4, 63), (7, 2.0), (7, nan), (8, nan), (9, 0), (10, 0),
            (10, 65536), (11, 0.0), (11, 2.0), (11, nan), (11, -inf)]
    for i, v in badb:
        args = list(okb)
        args[i] = v
        refused(lib.admm_bound_project_relaxed, args, (i, v))
