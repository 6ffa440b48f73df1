"""CPU: unreliable links -- the host-side checks and schedules (admm_hip/links.py), the float64 restatement
(tests/links_ref.py on the unchanged oracle) and the C entry points' argument checks.  No GPU.

(a) check_links: every argument error, and the values that normalise to None;
(b) schedule: deterministic, independent of how it is called, the pinned default_rng draw; max_age bounds
    every run of downs where there is no outage; outages override max_age; links_up / link_age_max;
(c) gated_admm with every edge up is relaxed_admm bit for bit (midpoint, weighted, bounded, relaxed), and
    links_ref.edge_ref on planted values;
(d) convergence on the reference alone: the 4-node ring at 16^2 of test_relax_cpu.py (6 angles per node,
    sigma = 0.5, seed 3).  Measured: the ungated reference needs K = 93 iterations to primal, dual < 1e-2;
    with p = 0.5, seed 0 the gated one needs 167 (1.80 K; seeds 1, 2: 174, 185), asserted <= 4 K: the
    expected 1 / p = 2 x slowdown, doubled for the variance of one draw.  Images after 4 K gated against 300
    ungated iterations: 1.9e-4 relative, asserted < 1e-3 -- the bar test_relax_cpu.py holds the reference's
    own two runs (alpha = 1 and 1.6, measured 3.0e-5) to on this problem;
(e) run_admm's refusals before device work, the drop-ins' pass-through, the params line;
(f) admm_consensus_gated / admm_consensus_gated_work return -1 with a message for every bad argument.
"""
import ctypes as C
import inspect
import math

import networkx as nx
import numpy as np
import pytest

import bounds_ref as br
import links_ref as lr
import relax_ref as rr
from admm_hip import links as lk
from oracle.admm import canonical_edges
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
# (a) check_links
# --------------------------------------------------------------------------------------
BAD = {
    "True": True, "False": False, "nan": float("nan"), "0": 0.0, "neg": -0.5, "1.5": 1.5, "inf": math.inf,
    "str": "0.5", "list": [0.5], "complex": 0.5 + 0j, "np.bool": np.True_,
    "unknown key": {"p": 0.5, "prob": 0.5}, "dict p bool": {"p": True}, "dict p nan": {"p": float("nan")},
    "dict p 0": {"p": 0.0}, "dict p > 1": {"p": 1.0001}, "max_age 0": {"p": 0.5, "max_age": 0},
    "max_age -1": {"p": 0.5, "max_age": -1}, "max_age 1.5": {"p": 0.5, "max_age": 1.5},
    "max_age bool": {"p": 0.5, "max_age": True}, "seed neg": {"p": 0.5, "seed": -1},
    "outage k1 = k0": {"outages": [(0, 1, 3, 3)]}, "outage k1 < k0": {"outages": [(0, 1, 3, 2)]},
    "outage short": {"outages": [(0, 1, 3)]}, "outage k0 neg": {"outages": [(0, 1, -1, 2)]},
    "outage not a list": {"outages": 5}, "int array": np.ones((4, 3), dtype=np.int64),
    "1-D array": np.ones(4, dtype=bool),
}


@pytest.mark.parametrize("bad", list(BAD.values()), ids=list(BAD))
def test_check_links_rejects(bad):
    with pytest.raises(ValueError, match="links"):
        lk.check_links(bad)


def test_check_links_accepts_and_normalises():
    assert lk.check_links(None) is None
    for one in (1.0, 1, np.float64(1.0), {"p": 1.0}, {}, {"p": 1.0, "seed": 7}, {"p": 1.0, "max_age": 3},
                {"p": 1, "outages": []}):
        assert lk.check_links(one) is None, one
    assert lk.check_links(0.5) == dict(p=0.5, seed=0, max_age=None, outages=())
    assert lk.check_links(np.float32(0.25))["p"] == 0.25
    assert lk.check_links(5e-324)["p"] > 0.0
    c = lk.check_links({"p": 0.7, "seed": 3, "max_age": 2, "outages": [(2, 1, 0, None), [0, 1, 4, 9]]})
    assert c == dict(p=0.7, seed=3, max_age=2, outages=((1, 2, 0, None), (0, 1, 4, 9)))
    assert lk.check_links({"outages": [(0, 1, 0, 1)]})["p"] == 1.0  # an outage alone is a schedule
    t = np.zeros((3, 2), dtype=bool)
    assert lk.check_links(t) is not None and np.array_equal(lk.check_links(t), t)


def test_check_links_run():
    lk.check_links_run(None, "derived", "derived")  # no links: nothing to object to
    cfg = lk.check_links(0.5)
    lk.check_links_run(cfg, None, "")
    lk.check_links_run(cfg, "stored", "derived")  # the argument overrides the environment
    with pytest.raises(ValueError, match="stored z"):
        lk.check_links_run(cfg, "derived", "")
    with pytest.raises(ValueError, match="stored z"):
        lk.check_links_run(np.zeros((2, 2), dtype=bool), None, "derived")


def test_need_stored_z_names_the_links():
    from admm_hip.plan import need_stored_z
    need_stored_z(False, False, False, "run", links=True)
    with pytest.raises(ValueError, match="links need stored z.*stored-z rule"):
        need_stored_z(True, False, False, "run", links=True)
    assert inspect.signature(need_stored_z).parameters["links"].default is False


# --------------------------------------------------------------------------------------
# (b) schedules
# --------------------------------------------------------------------------------------
GRAPHS = {"ring5": nx.cycle_graph(5), "star7": nx.star_graph(6), "complete6": nx.complete_graph(6),
          "er12": nx.gnp_random_graph(12, 0.4, seed=2)}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_edge_list_is_the_runs_edge_order(name):
    G = GRAPHS[name]
    from admm_hip.plan import make_plan
    assert lk.edge_list(G) == canonical_edges(G) == make_plan(G, G.number_of_nodes()).edges


@pytest.mark.parametrize("name", list(GRAPHS))
def test_schedule_is_the_pinned_draw(name):
    G = GRAPHS[name]
    E = G.number_of_edges()
    for p, seed in ((0.5, 0), (0.8, 3), (0.05, 11)):
        want = np.random.default_rng([seed, 0x4C4E4B53]).random((40, E)) < p
        for value in ({"p": p, "seed": seed}, {"p": np.float64(p), "seed": np.int64(seed), "max_age": None,
                                                "outages": ()}):
            got = lk.schedule(G, 40, value)
            assert got.dtype == np.bool_ and got.shape == (40, E) and np.array_equal(got, want)
        if seed == 0:
            assert np.array_equal(lk.schedule(G, 40, p), want)  # a bare p is seed 0
    # twice the same; not a function of earlier calls; both values occur
    a, b = lk.schedule(G, 40, 0.5), lk.schedule(G, 40, 0.5)
    assert np.array_equal(a, b) and a is not b and a.any() and not a.all()
    assert not np.array_equal(a, lk.schedule(G, 40, {"p": 0.5, "seed": 1}))
    assert lk.schedule(G, 40, None).all() and lk.schedule(G, 40, 1.0).all() and lk.schedule(G, 40, {"p": 1.0}).all()


def test_schedule_takes_an_array_as_it_is():
    G = GRAPHS["ring5"]
    t = np.random.default_rng(4).random((12, 5)) < 0.5
    got = lk.schedule(G, 10, t)
    assert np.array_equal(got, t[:10]) and not np.shares_memory(got, t)
    for bad in (t[:, :4], np.zeros((12, 6), dtype=bool), t[:9]):
        with pytest.raises(ValueError, match="links"):
            lk.schedule(G, 10, bad)
    import torch
    assert np.array_equal(lk.schedule(G, 12, torch.from_numpy(t)), t)


def _down_runs(col):
    """Lengths of the maximal runs of False in a bool column."""
    runs, cur = [], 0
    for v in col:
        if v:
            if cur:
                runs.append(cur)
            cur = 0
        else:
            cur += 1
    if cur:
        runs.append(cur)
    return runs


@pytest.mark.parametrize("max_age", [1, 2, 5])
def test_max_age_bounds_every_run_of_downs(max_age):
    G = GRAPHS["complete6"]
    free = lk.schedule(G, 200, {"p": 0.2, "seed": 5})
    assert max(max(_down_runs(free[:, e])) for e in range(free.shape[1])) > 5  # the draw alone does not
    t = lk.schedule(G, 200, {"p": 0.2, "seed": 5, "max_age": max_age})
    longest = max(max(_down_runs(t[:, e]), default=0) for e in range(t.shape[1]))
    assert longest == max_age  # bounded, and the bound is reached
    assert np.all(t | ~free)  # forcing only ever raises an edge
    assert np.array_equal(lk.link_age_max(t) <= max_age, np.ones(200, dtype=bool))


def test_outages_override_max_age_and_name_edges():
    G = GRAPHS["ring5"]
    edges = lk.edge_list(G)
    c04, c12 = edges.index((0, 4)), edges.index((1, 2))
    cfg = {"p": 0.5, "seed": 2, "max_age": 2, "outages": [(4, 0, 3, 20), (1, 2, 25, None)]}
    t = lk.schedule(G, 40, cfg)
    base = lk.schedule(G, 40, {"p": 0.5, "seed": 2, "max_age": 2})
    assert not t[3:20, c04].any() and not t[25:, c12].any()  # down for the whole window, max_age or not
    mask = np.ones_like(t)
    mask[3:20, c04] = False
    mask[25:, c12] = False
    assert np.array_equal(t[mask], base[mask])  # and nothing else moved
    assert max(_down_runs(t[:, c04])) >= 17
    others = [e for e in range(5) if e not in (c04, c12)]
    assert max(max(_down_runs(t[:, e]), default=0) for e in others) <= 2
    assert lk.schedule(G, 3, {"outages": [(0, 1, 10, 20)]}).all()  # a window past the run
    for bad in ((0, 2, 0, 5), (0, 5, 0, 5), (3, 3, 0, 5)):
        with pytest.raises(ValueError, match="no edge"):
            lk.schedule(G, 40, {"outages": [bad]})


def test_history_arithmetic():
    t = np.array([[1, 1, 1], [0, 1, 0], [0, 0, 1], [0, 1, 1], [1, 1, 1], [0, 0, 0]], dtype=bool)
    assert lk.links_up(t).tolist() == [3, 1, 1, 2, 3, 0]
    assert lk.link_age_max(t).tolist() == [0, 1, 2, 3, 0, 1]
    assert lk.link_age_max(np.zeros((3, 2), dtype=bool)).tolist() == [1, 2, 3]  # never updated: from the start
    assert lk.links_up(np.ones((4, 7), dtype=bool)).tolist() == [7] * 4
    assert lk.LINK_KEYS == ("links_up", "link_age_max")


# --------------------------------------------------------------------------------------
# (c) the restatement
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return ring_problem(12, 3, 6, 0.5, 5)


KEYS = ("primal", "dual", "obj_total", "pri_per_node", "dual_per_node", "mse_sino_total", "img_mse_total")


@pytest.mark.parametrize("variant", ["midpoint", "weighted", "bounds", "relaxed", "relaxed-weighted"])
def test_all_up_is_relaxed_admm_bit_for_bit(small, variant):
    ops, b, G, W, ph = small
    kw = dict(lam_tv=0.01, rho=1.0, max_iters=6, phantom_true=ph, Wi_list=W,
              alpha=1.6 if variant.startswith("relaxed") else 1.0,
              fusion="weighted" if variant.endswith("weighted") else "midpoint",
              bounds=(0.0, 1.0) if variant == "bounds" else None)
    xo, wo, ho = rr.relaxed_admm(ops, b, G, q_of(W), 12, **kw)
    x, w, h = lr.gated_admm(ops, b, G, q_of(W), 12, np.ones((6, 3), dtype=bool), **kw)
    assert set(h) == set(ho) and (w is None) == (wo is None)
    assert all(np.array_equal(a, c) for a, c in zip(x, xo))
    if w is not None:
        assert all(np.array_equal(a, c) for a, c in zip(w, wo))
    for k in KEYS + (br.BOUND_KEYS if variant == "bounds" else ()):
        assert np.array_equal(np.asarray(h[k]), np.asarray(ho[k])), k
    # and a table with downs is another trajectory, whose down edges report no dual residual
    t = lk.schedule(G, 6, {"p": 0.5, "seed": 1})
    assert t.any() and not t.all()
    x2, _, h2 = lr.gated_admm(ops, b, G, q_of(W), 12, t, **kw)
    assert max(float(np.max(np.abs(a - c))) for a, c in zip(x2, xo)) > 1e-3
    k_all_down = [k for k in range(6) if not t[k].any()]
    assert all(h2["dual"][k] == 0.0 for k in k_all_down)


def test_edge_ref_on_planted_values():
    x_ext = np.array([[1.0, 0.1, 3.0], [2.0, 0.7, -1.0], [0.5, 0.25, 4.0]])
    y, z = np.array([[0.5, 1e-17, 0.25], [1.0, 2.0, 3.0]]), np.array([[4.0, 0.3, 1.0], [0.0, -1.0, 2.0]])
    ea, eb = [0, 1], [1, 2]
    for alpha in (1.0, 1.6):
        yr, zr, _, sr_ = rr.edge_ref(x_ext, y, z, ea, eb, alpha)
        yn, zn, ybn, s = lr.edge_ref(x_ext, y, z, ea, eb, [True, False], alpha)
        assert ybn is None
        assert np.array_equal(yn[0], yr[0]) and np.array_equal(zn[0], zr[0]) and np.array_equal(s[0], sr_[0])
        assert np.array_equal(yn[1], y[1]) and np.array_equal(zn[1], z[1])
        assert s[1, 0] == math.fsum((x_ext[1] - z[1]) ** 2) and s[1, 1] == math.fsum((x_ext[2] - z[1]) ** 2)
        assert s[1, 2] == 0.0 and not np.signbit(s[1, 2])
        up = lr.edge_ref(x_ext, y, z, ea, eb, [True, True], alpha)
        assert all(np.array_equal(a, c) for a, c in zip((up[0], up[1], up[3]), (yr, zr, sr_)))
    # the single-y invariant survives a partial update: y_a' + y_b' = 0 edge by edge, for any prior state
    yw, zw, ybw, _ = lr.edge_ref(x_ext, y, z, ea, eb, [False, True], 1.0, y_b=-y, W=np.ones((3, 3)))
    assert np.array_equal(ybw[0], -y[0]) and np.array_equal(yw[0], y[0])
    assert np.max(np.abs(yw[1] + ybw[1])) < 1e-14


# --------------------------------------------------------------------------------------
# (d) convergence, on the reference alone
# --------------------------------------------------------------------------------------
TOL, ITERS, P, SEED = 1e-2, 300, 0.5, 0


def test_half_the_links_reach_the_same_point_within_four_times_the_iterations():
    ops, b, G, W, ph = ring_problem(16, 4, 6, 0.5, 3)
    kw = dict(lam_tv=0.01, rho=1.0)
    x1, _, h1 = rr.relaxed_admm(ops, b, G, q_of(W), 16, alpha=1.0, max_iters=ITERS, **kw)
    K = rr.iters_to(h1, TOL)
    assert K is not None  # the tolerance is one the ungated reference reaches
    t = lk.schedule(G, 4 * K, {"p": P, "seed": SEED})
    assert 0.4 < t.mean() < 0.6
    xg, _, hg = lr.gated_admm(ops, b, G, q_of(W), 16, t, max_iters=4 * K, **kw)
    kg = rr.iters_to(hg, TOL)
    d = float(np.linalg.norm(np.stack(xg) - np.stack(x1)) / np.linalg.norm(np.stack(x1)))
    print(f"\nRING16 links p={P} seed={SEED}: iterations to primal, dual < {TOL}: all up {K}, gated {kg} "
          f"(ratio {kg / K if kg else float('nan'):.2f}); images rel {d:.2e}")
    assert kg is not None and kg <= 4 * K, (kg, K)
    assert kg > K  # (and half the links do cost iterations)
    assert d < 1e-3


# --------------------------------------------------------------------------------------
# (e) run_admm, the drop-ins, the params file
# --------------------------------------------------------------------------------------
def test_run_admm_rejects_bad_links_before_any_device_work(monkeypatch):
    """The keyword checks come before the operators are touched: stand-in operators are enough."""
    from admm_hip.admm import run_admm
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    args = ([object()] * 3, [None] * 3, nx.cycle_graph(3), [None] * 3, None, 8)
    for value in (True, float("nan"), 0.0, -0.1, 1.5, {"q": 1}, {"p": 0.5, "max_age": 0},
                  {"outages": [(0, 1, 2, 2)]}, {"outages": [(0, 1, 4, 2)]}, {"outages": [(0, 3, 0, 2)]},
                  np.ones((10, 2), dtype=bool), np.ones((9, 3), dtype=bool)):
        with pytest.raises(ValueError, match="links"):
            run_admm(*args, verbose=False, max_iters=10, links=value)
    for value in (0.5, {"outages": [(0, 1, 0, 2)]}, np.zeros((10, 3), dtype=bool)):
        with pytest.raises(ValueError, match="links need stored z"):
            run_admm(*args, verbose=False, max_iters=10, links=value, edge_state="derived")
    monkeypatch.setenv("ADMM_EDGE_STATE", "derived")
    with pytest.raises(ValueError, match="links need stored z"):
        run_admm(*args, verbose=False, max_iters=10, links=0.5)
    # what normalises to None is not refused for derived z: it is the run without the keyword, which goes on
    # to the operators (stand-ins here)
    for value in (None, 1.0, {"p": 1.0}, {"outages": [(0, 1, 10, 12)]}):
        with pytest.raises(ValueError, match="a matrix must be 2-D"):
            run_admm(*args, verbose=False, max_iters=10, links=value)


def test_dropins_forward_the_keyword():
    import block_6_admm_loop
    import block_6_admm_loop_ver2
    from admm_hip import admm
    import admm_hip
    assert admm_hip.links is lk
    p = inspect.signature(admm.run_admm).parameters
    assert p["links"].default is None and list(p).index("links") > list(p).index("phantom_true")
    for mod, last_ref in ((block_6_admm_loop, "scs_save_every_chunks"), (block_6_admm_loop_ver2, "phantom_true")):
        sig = inspect.signature(mod.decentralized_admm).parameters
        assert sig["links"].default is None and list(sig).index("links") > list(sig).index(last_ref)
        assert "links" in mod.__doc__ and "link_age_max" in mod.__doc__
        seen = {}

        def fake(*a, **kw):
            seen.update(kw)
            return [], {"primal": [], "dual": [], "obj_total": []}

        orig = mod.run_admm
        mod.run_admm = fake
        try:
            mod.decentralized_admm(None, None, None, None, None, 8, links={"p": 0.7})
        finally:
            mod.run_admm = orig
        assert seen["links"] == {"p": 0.7}
    assert not set(lk.LINK_KEYS) & set(admm.HISTORY_KEYS + admm.EXTRA_KEYS)


def test_params_file_names_the_schedule_only_when_gated(tmp_path):
    from admm_hip.admm import _write_params
    G = nx.cycle_graph(4)
    cfg = lk.check_links({"p": 0.6, "max_age": 3, "outages": [(0, 1, 2, 5)]})
    line = lk.describe(cfg, lk.schedule(G, 10, cfg))
    assert "\n" not in line and "p = 0.6" in line and "max_age = 3" in line and "(0, 1, 2, 5)" in line
    t = np.zeros((10, 4), dtype=bool)
    assert "explicit table 10 x 4" in lk.describe(t, t) and "up fraction = 0.0000" in lk.describe(t, t)
    _write_params(str(tmp_path / "off"), 1.0, 0.01, 4, 0.1, 10, 5)
    _write_params(str(tmp_path / "on"), 1.0, 0.01, 4, 0.1, 10, 5, links=line)
    off = (tmp_path / "off" / "admm_internal_params.txt").read_text()
    on = (tmp_path / "on" / "admm_internal_params.txt").read_text()
    assert "links" not in off.lower() and line + "\n" in on
    assert [ln for ln in on.splitlines() if "links" not in ln.lower() and "Date" not in ln] == \
           [ln for ln in off.splitlines() if "Date" not in ln]


# --------------------------------------------------------------------------------------
# (f) the C entry points refuse bad arguments before any HIP call
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
    assert lib.admm_consensus_gated_work(1089, 3, C.byref(need)) == 0 and need.value == 3 * 2 * 3
    assert lib.admm_consensus_gated_work(4096, 16, C.byref(need)) == 0 and need.value == 3 * 4 * 16
    assert lib.admm_consensus_gated_work(169, 0, C.byref(need)) == 0 and need.value == 3
    for args in ((0, 3, C.byref(need)), (1089, -1, C.byref(need)), (1089, 3, None)):
        refused(lib.admm_consensus_gated_work, args, args[:2])

    #      x_ext n  rows y  y_b z  w  ea eb e0 e1 alpha up work stats stream
    ok = [p, 64, 2, p, z, p, z, p, p, 0, 1, 1.0, p, p, p, z]
    bad = [(0, z, b"null"), (3, z, b"null"), (5, z, b"null"), (7, z, b"null"), (8, z, b"null"), (12, z, b"up is null"),
           (13, z, b"null"), (14, z, b"null"), (4, p, b"pair"), (6, p, b"pair"), (9, -1, b"e0"), (10, -1, b"e0"),
           (1, 0, b"n must"), (2, 0, b"n_rows"), (11, 0.0, b"alpha"), (11, 2.0, b"alpha"), (11, -1.0, b"alpha"),
           (11, nan, b"alpha"), (11, inf, b"alpha")]
    for i, v, word in bad:
        args = list(ok)
        args[i] = v
        assert word in refused(lib.admm_consensus_gated, args, (i, v)), (i, v)
    args = list(ok)
    args[9], args[10] = 2, 1  # e1 < e0
    refused(lib.admm_consensus_gated, args, "e1 < e0")
    for alpha in (1.0, 1.6):  # an empty range is legal and launches nothing
        args[9], args[10], args[11] = 1, 1, alpha
        assert lib.admm_consensus_gated(*args) == 0
