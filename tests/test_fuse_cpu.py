"""CPU: the fixed-point fusion arithmetic as tests/fuse_ref.py restates it -- the
reference the GPU tests hold the device to bit for bit, so its own properties are checked here:
order independence, the error bound against exact rational arithmetic, the edge cases of the shift,
and that the planted cancellation really separates it from a float64 partial-sum implementation.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import fuse_ref as fr

N_PIX = 1089
CANCEL, ZERO = 5, 7  # the planted pixels


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def case(V, seed=0, n=N_PIX):
    """(x, w) with the planted cancellation 1e8, -1e8, 1e-8 at pixel 5 and an all-zero pixel 7."""
    rng = np.random.default_rng([seed, V, n])
    x = rng.normal(size=(V, n))
    w = rng.uniform(0.5, 2.0, size=(V, n))
    if V >= 3:
        x[:, CANCEL] = 0.0
        x[0, CANCEL], x[1, CANCEL], x[2, CANCEL] = 1e8, -1e8, 1e-8
        w[:3, CANCEL] = 1.0
    x[:, ZERO] = 0.0
    return x, w


def groupings(V, rng):
    """Partitions and permutations of range(V): all at once, one by one, two halves, a shuffled split."""
    perm = rng.permutation(V)
    out = [[np.arange(V)], [np.array([i]) for i in range(V)], [perm]]
    if V > 1:
        k = max(1, V // 3)
        out += [[np.arange(V // 2), np.arange(V // 2, V)], [perm[:k], perm[k:]], [np.arange(V)[::-1]]]
    return out


@pytest.mark.parametrize("V", [1, 3, 8, 17, 64])
def test_bits_do_not_depend_on_order_or_grouping(V):
    x, w = case(V)
    rng = np.random.default_rng(V)
    base_u = fr.fuse(x, None, spread=True)
    base_w = fr.fuse(x, w, spread=True)
    s0 = fr.fixed_sum(w * x)[1]
    S0 = fr.fixed_sum(w * x)[2]
    assert np.abs(S0).max() < 2 ** 62
    for parts in groupings(V, rng):
        assert sorted(np.concatenate(parts).tolist()) == list(range(V))
        _, s, S = fr.fixed_sum(w * x, parts=parts)
        assert s == s0 and np.array_equal(S, S0)
        for got, want in ((fr.fuse(x, None, parts=parts, spread=True), base_u),
                          (fr.fuse(x, w, parts=parts, spread=True), base_w)):
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.all(base_u[0][ZERO] == 0.0) and base_u[1][ZERO] == 0.0


@pytest.mark.parametrize("V", [1, 3, 8, 17, 64])
def test_error_against_exact_rationals_is_within_the_bound(V):
    """|xbar - exact| <= V 2^-s / Dn + 4 * 2^-53 |exact| at every pixel, exact = (sum_i t_i) / (sum_i w_i) in
    rational arithmetic over the float64 terms t_i = w_i * x_i the rule sums: each q is within half a grid
    step 2^-s of its term, the conversion, the ldexp, the division and Dn's own rounding are four roundings
    of 2^-53 relative at the most."""
    x, w = case(V)
    t = w * x
    xbar = fr.fuse(x, w)
    _, s, _ = fr.fixed_sum(t)
    worst = 0.0
    for p in range(N_PIX):
        num = sum(Fraction(float(v)) for v in t[:, p])
        den = sum(Fraction(float(v)) for v in w[:, p])
        exact = num / den
        err = abs(Fraction(float(xbar[p])) - exact)
        bar = Fraction(V) * Fraction(2) ** (-s) / den + 4 * Fraction(2) ** -53 * abs(exact)
        assert err <= bar, (V, p, float(err), float(bar))
        worst = max(worst, float(err / (Fraction(float(np.abs(t).max())) / den)))
    print(f"\nV={V}: s={s}, worst error {worst:.2e} of B / Dn")
    # uniform weights: Dn is exactly V
    xu = fr.fuse(x, None)
    su = fr.fixed_sum(x)[1]
    for p in range(0, N_PIX, 9):
        exact = sum(Fraction(float(v)) for v in x[:, p]) / V
        assert abs(Fraction(float(xu[p])) - exact) <= Fraction(V) * Fraction(2) ** (-su) / V \
            + 2 * Fraction(2) ** -53 * abs(exact)


def test_shift_edge_cases():
    assert fr.shift(0.0, 4) == 0
    assert fr.shift(5e-324, 4) == 1132
    assert fr.shift(1.7e308, 64) == -969
    assert fr.shift(1.0, 1) == 60 and fr.shift(1.0, 2) == 59 and fr.shift(1.0, 3) == 58 and fr.shift(0.75, 4) == 59
    # B = 0: the sum is +0 everywhere
    out, s, S = fr.fixed_sum(np.zeros((3, 5)))
    assert s == 0 and not S.any() and np.array_equal(bits(out), bits(np.zeros(5)))
    # a subnormal B: the terms are exact multiples of the grid, so the sum is exact
    t = np.array([[5e-324, 1.5e-323], [1e-323, -5e-324]])
    out, s, _ = fr.fixed_sum(t)
    assert s == fr.shift(1.5e-323, 2) and np.array_equal(out, t[0] + t[1])
    # near DBL_MAX: no overflow in q (|q| <= 2^(61 - L)); a sum beyond the double range is +inf
    big = np.array([[1.7e308, 1.0e308], [-1.7e308, 1.0e308], [1e300, -1e300]])
    out, s, S = fr.fixed_sum(big, V_total=64)
    assert s == -969 and np.abs(S).max() < 2 ** 62
    assert out[0] == np.ldexp(np.rint(np.ldexp(1e300, s)), -s) and out[1] == np.inf
    # V_total larger than the images present only moves the shift
    a = fr.fixed_sum(t, V_total=2)
    b = fr.fixed_sum(t, V_total=1000)
    assert b[1] == a[1] - 9 and np.array_equal(a[0], b[0])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_term_makes_every_output_nan(bad):
    x, w = case(8)
    x[3, 100] = bad
    for wt in (None, w):
        xbar, sp = fr.fuse(x, wt, spread=True)
        assert np.isnan(xbar).all() and np.isnan(sp).all()
        assert np.isnan(fr.dev2(x, xbar)).all()
    assert fr.absmax(x) == math.inf


def test_the_planted_cancellation_separates_float64_partial_sums():
    """Two groupings of a plain float64 sum differ at the planted pixel, the fixed-point sums do not: the GPU
    invariance tests cannot be passed by an implementation that adds float64 partial sums."""
    x, w = case(8)
    t = (w * x)[:, CANCEL]
    one = ((t[0] + t[1]) + t[2]) + float(np.sum(t[3:]))  # nodes 0 .. 7 in order
    two = (t[0] + t[2]) + (t[1] + float(np.sum(t[3:])))  # {0, 2} and {1, 3 ..} as two partial sums
    assert one == 1e-8 and two != one and bits(one) != bits(two)  # (1e8 + 1e-8 rounds to a neighbour of 1e8)
    parts = [np.array([0, 2]), np.array([1, 3, 4, 5, 6, 7])]
    a, b = fr.fixed_sum(w * x), fr.fixed_sum(w * x, parts=parts)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2])
    # the grid keeps 1e-8 beside 1e8 to within its step
    assert a[1] == fr.shift(float(np.abs(w * x).max()), 8)
    assert abs(a[0][CANCEL] - 1e-8) <= 8 * 2.0 ** -a[1]


def test_uniform_fusion_splits_the_error_into_bias_and_consensus():
    """sum_i |x_i - x*|^2 = V |xbar - x*|^2 + sum_i |x_i - xbar|^2 within 1e-13 relative."""
    rng = np.random.default_rng(3)
    V, n = 5, 169
    x, star = rng.normal(size=(V, n)), rng.normal(size=n)
    xbar = fr.fuse(x, None)
    lhs = float(np.sum(fr.dev2(x, star)))
    rhs = V * float(fr.dev2(xbar[None], star)[0]) + float(np.sum(fr.dev2(x, xbar)))
    assert abs(lhs - rhs) <= 1e-13 * lhs, abs(lhs - rhs) / lhs


def test_check_fuse_and_the_keyword_surface():
    """Host-side argument checks (no device work) and the drop-ins' forwarding of the two keywords."""
    import inspect

    import networkx as nx

    import block_6_admm_loop
    import block_6_admm_loop_ver2
    from admm_hip import Fuser, check_fuse, fuse_images  # noqa: F401  (the public names)
    from admm_hip.admm import run_admm
    assert check_fuse(None) is None and check_fuse("uniform") == "uniform" and check_fuse("precision") == "precision"
    for bad in ("median", "Uniform", "", 1, True, ("uniform",), ["precision"]):
        with pytest.raises(ValueError, match="fuse"):
            check_fuse(bad)
    # the keyword checks come before the operators are touched: stand-in operators are enough
    args = ([object()] * 3, [None] * 3, nx.cycle_graph(3), None, None, 8)
    for kw in (dict(fuse="median"), dict(fuse=True), dict(fuse_out={}), dict(fuse="uniform", fuse_out=[]),
               dict(fuse="precision")):  # (precision without Wi_list)
        with pytest.raises(ValueError, match="fuse"):
            run_admm(*args, verbose=False, **kw)
    assert inspect.signature(run_admm).parameters["fuse"].default is None
    for mod in (block_6_admm_loop, block_6_admm_loop_ver2):
        sig = inspect.signature(mod.decentralized_admm).parameters
        assert sig["fuse"].default is None and sig["fuse_out"].default is None
        assert "consensus_err" in mod.__doc__ and "fuse_out" in mod.__doc__
        seen = {}

        def fake(*a, **kw):
            seen.update(kw)
            return [], {"primal": [], "dual": [], "obj_total": []}
        out = {}
        real, mod.run_admm = mod.run_admm, fake
        try:
            mod.decentralized_admm([], [], None, [], None, 8, fuse="precision", fuse_out=out)
        finally:
            mod.run_admm = real
        assert seen["fuse"] == "precision" and seen["fuse_out"] is out
