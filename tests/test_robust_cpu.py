"""CPU: the host side of run_admm(robust=delta) and the references of tests/robust_ref.py -- argument
checks, the reference's own properties, and the conditions the GPU cases of test_gpu_robust.py rest on
(no parity ray at the threshold; the zinger case's gain on the float64 reference)."""
import inspect
import math

import numpy as np
import pytest
import torch

import robust_ref as rr
from admm_hip import table
from admm_hip.robust import ROBUST_KEYS, ROBUST_STATS, applies, check_robust

DTYPES = [np.float32, np.float64]


# --------------------------------------------------------------------------------------
# host checks
# --------------------------------------------------------------------------------------
def test_check_robust_accepts():
    assert check_robust(None) is None
    assert check_robust(0.3) == dict(delta=0.3, every=1, until=None)
    assert check_robust(2) == dict(delta=2.0, every=1, until=None)
    assert check_robust(math.inf) == dict(delta=math.inf, every=1, until=None)
    assert check_robust(np.float32(0.5))["delta"] == 0.5
    assert check_robust({"delta": 0.3, "every": 2, "until": 7}) == dict(delta=0.3, every=2, until=7)
    assert check_robust({"delta": math.inf, "until": 0}) == dict(delta=math.inf, every=1, until=0)


@pytest.mark.parametrize("bad", [True, False, float("nan"), 0, 0.0, -1.0, -math.inf, "0.3", [0.3], {}, {"every": 2},
                                 {"delta": 0.3, "evry": 2}, {"delta": True}, {"delta": float("nan")},
                                 {"delta": 0.0}, {"delta": 0.3, "every": 0}, {"delta": 0.3, "every": 1.5},
                                 {"delta": 0.3, "every": True}, {"delta": 0.3, "until": -1},
                                 {"delta": 0.3, "until": 2.0}])
def test_check_robust_rejects(bad):
    with pytest.raises(ValueError):
        check_robust(bad)


def test_applies_rule():
    cfg = check_robust({"delta": 1.0, "every": 2, "until": 5})
    assert [applies(cfg, k) for k in range(8)] == [False, True, False, True, False, False, False, False]
    assert all(applies(check_robust(1.0), k) for k in range(5))
    assert [applies(cfg, k) for k in range(8)] == [rr.applies(k, 2, 5) for k in range(8)]


def test_run_admm_and_dropins_take_the_keyword():
    from admm_hip.admm import run_admm
    import block_6_admm_loop
    import block_6_admm_loop_ver2
    for fn in (run_admm, block_6_admm_loop.decentralized_admm, block_6_admm_loop_ver2.decentralized_admm):
        p = inspect.signature(fn).parameters["robust"]
        assert p.default is None


def test_bad_values_raise_before_any_operator_is_touched():
    from admm_hip.admm import run_admm
    for bad in (True, float("nan"), -0.3, {"delta": 0.3, "every": 0}, {"delta": 0.3, "k": 1}):
        with pytest.raises(ValueError):
            run_admm([object()], [None], None, None, None, 8, robust=bad)


def test_table_block_and_keys():
    assert table.ORDER.index("robust") == table.ORDER.index("norms") + 1
    assert ROBUST_STATS == 2 and len(ROBUST_KEYS) == 4
    cols = table.NodeColumns()
    cols.add("fuse", 2, lambda nb: [], ("consensus_err",))
    cols.add("robust", ROBUST_STATS, lambda nb: [], ROBUST_KEYS)
    assert [b.name for b in cols.blocks] == ["core", "robust", "fuse"]


def test_recorder_records_the_block():
    from admm_hip._lib import EDGE_STATS, NODE_STATS
    from admm_hip.admm import _Recorder
    cols = table.NodeColumns()
    cols.add("robust", ROBUST_STATS, lambda nb: [], ROBUST_KEYS)
    hist = {}
    rec = _Recorder(hist, cols, [(0, 1)], 2, 0.01, False, None)
    ns = np.zeros((2, NODE_STATS + ROBUST_STATS))
    ns[:, NODE_STATS] = (1.5, 2.25)
    ns[:, NODE_STATS + 1] = (3.0, 4.0)
    rec(0, ns, np.zeros((1, EDGE_STATS)), 1.0)
    assert hist["robust_loss_total"] == [3.75] and hist["robust_outliers_total"] == [7.0]
    assert np.array_equal(hist["robust_loss_per_node"][0], [1.5, 2.25])
    assert np.array_equal(hist["robust_outliers_per_node"][0], [3.0, 4.0])


def test_add_zingers_is_seeded_and_hits_the_fraction():
    from admm_hip.data import add_zingers
    s = torch.linspace(0.0, 1.0, 20000, dtype=torch.float32).reshape(100, 200)
    a, hit = add_zingers(s, 0.03, 3.0, generator=torch.Generator().manual_seed(5))
    b, hit2 = add_zingers(s, 0.03, 3.0, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b) and torch.equal(hit, hit2) and a.dtype == s.dtype and a.shape == s.shape
    assert 0.02 < hit.double().mean().item() < 0.04
    d = (a - s)[hit]
    assert torch.all((d - 3.0).abs().minimum((d + 3.0).abs()) < 1e-6) and torch.equal(a[~hit], s[~hit])
    assert (d > 0).any() and (d < 0).any()
    assert not add_zingers(s, 0.0, 3.0)[1].any()
    with pytest.raises(ValueError):
        add_zingers(s, 1.5, 3.0)


# --------------------------------------------------------------------------------------
# the reference's own properties
# --------------------------------------------------------------------------------------
def _rays(dtype, m=2049, seed=3):
    rng = np.random.default_rng([seed, 5])
    ax = rng.standard_normal(m).astype(dtype)
    b = (ax.astype(np.float64) + 0.4 * rng.standard_normal(m)).astype(dtype)
    w = rng.uniform(0.0, 2.0, m).astype(dtype)
    w[rng.random(m) < 0.1] = 0
    return ax, b, w


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_delta_gives_the_weights_back(dtype):
    ax, b, w = _rays(dtype)
    wo, loss, cnt = rr.huber_weights_ref(ax, b, math.inf, None, dtype)
    assert wo.dtype == dtype and np.array_equal(wo, np.ones_like(ax)) and cnt == 0
    r = (ax - b).astype(np.float64)
    assert loss == math.fsum(0.5 * (np.abs(r) * np.abs(r)))
    wo, loss, cnt = rr.huber_weights_ref(ax, b, math.inf, w, dtype)
    assert np.array_equal(wo.view(np.uint8), w.view(np.uint8)) and cnt == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_rays_give_zero_whatever_they_hold(dtype):
    ax, b, w = _rays(dtype)
    ref = rr.huber_weights_ref(ax, b, rr.DELTA, w, dtype)
    ax2, b2 = ax.copy(), b.copy()
    dead = w == 0
    ax2[dead] = np.nan
    b2[np.flatnonzero(dead)[::2]] = np.inf
    got = rr.huber_weights_ref(ax2, b2, rr.DELTA, w, dtype)
    assert np.all(got[0][dead] == 0) and not np.any(np.signbit(got[0][dead]))
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and got[2] == ref[2]
    live = ~dead
    assert ref[2] == np.count_nonzero(np.abs((ax - b).astype(np.float64))[live] > rr.DELTA) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_is_continuous_at_the_threshold_and_loss_is_the_closed_form(dtype):
    d = 0.3
    b = np.zeros(5, dtype=dtype)
    at = dtype(d)
    ax = np.array([np.nextafter(at, dtype(0)), at, np.nextafter(at, dtype(1)), 2 * at, -4 * at], dtype=dtype)
    wo, loss, cnt = rr.huber_weights_ref(ax, b, float(at), None, dtype)
    assert wo[0] == 1 and wo[1] == 1 and 1 - wo[2] <= 2 * np.finfo(dtype).eps
    assert wo[3] == dtype(0.5) and wo[4] == dtype(0.25) and cnt == 3
    ax, b, w = _rays(dtype)
    r = (ax - b).astype(np.float64)
    for ww in (None, w):
        _, loss, _ = rr.huber_weights_ref(ax, b, d, ww, dtype)
        want = rr.huber_closed_form(r, d, ww)
        assert abs(loss - want) <= 1e-13 * want
    # the value and the majoriser's slope: h r = psi'(r)
    wo, _, _ = rr.huber_weights_ref(ax, b, d, None, dtype)
    assert np.allclose(wo.astype(np.float64) * r, np.clip(r, -d, d), rtol=4 * np.finfo(dtype).eps, atol=0)


def test_a_nan_residual_propagates():
    ax = np.array([0.1, np.nan, 2.0])
    wo, loss, cnt = rr.huber_weights_ref(ax, np.zeros(3), 0.3, np.ones(3), np.float64)
    assert np.isnan(wo[1]) and math.isnan(loss) and cnt == 1 and wo[0] == 1.0


# --------------------------------------------------------------------------------------
# conditions on the GPU cases
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("p", rr.PARITY_RUNS, ids=rr.parity_id)
def test_parity_runs_have_no_ray_at_the_threshold(p, dtype):
    run = rr.parity_reference(p[0], p[1], p[2], dtype)
    assert rr.near_threshold(run, rr.DELTA, rr.PARITY_MARGIN) == 0
    # and the threshold matters: rays beyond it in every iteration, fewer as the run proceeds
    tot = [int(c.sum()) for c in run["outliers"]]
    assert tot[-1] > 0 and tot[0] > tot[-1]
    if p[2]:  # masked rays are never counted
        assert np.any(run["base"] == 0)


def test_every_two_differs_from_every_one_only_after_the_second_iteration():
    a = rr.parity_reference("ring33", 1, False, "float64")
    b = rr.parity_reference("ring33", 2, False, "float64")
    assert a["loss_total"][0] == b["loss_total"][0] and a["loss_total"][1] != b["loss_total"][1]


def test_zinger_case_on_the_reference():
    """The float64 reference on the zinger case: the plain run's image error grows, the Huber run ends at
    <= 0.70 x the plain run's and <= 1.05 x the clean-data run's (measured with this seed: 0.651 and
    1.0002; on clean data delta = 0.3 costs 0.04 %)."""
    R = rr.zinger_runs()
    plain, clean, robust = (R[k]["img_err"] for k in ("plain", "clean", "robust"))
    print(f"\nzinger: plain {plain[3]:.3f} -> {plain[-1]:.3f}, clean {clean[-1]:.3f}, robust {robust[-1]:.3f}; "
          f"ratios {robust[-1] / plain[-1]:.4f}, {robust[-1] / clean[-1]:.4f}; clean-data cost "
          f"{R['robust_clean']['img_err'][-1] / clean[-1] - 1:.2e}")
    assert plain[-1] > plain[3]
    assert robust[-1] <= 0.70 * plain[-1]
    assert robust[-1] <= 1.05 * clean[-1]
    assert R["robust_clean"]["img_err"][-1] <= 1.01 * clean[-1]
    assert rr.near_threshold(R["robust"], rr.DELTA, rr.PARITY_MARGIN) == 0  # the GPU run's counts are the reference's
    # the rays the last iteration counts are the planted ones, to a few
    P = rr.zinger_problem()
    planted = sum(int(np.count_nonzero(P["b_zinger"][g] != P["b"][g])) for g in P["plan"].local_nodes)
    assert abs(int(R["robust"]["outliers"][-1].sum()) - planted) <= 0.1 * planted
