"""CPU: the float64 restatement of PSNR / SSIM (tests/metrics_ref.py) pinned by closed forms, and
the argument errors of admm_hip.metrics and run_admm(metrics=...) raised before any device work
(this file runs on a machine without a GPU)."""
import math
import os
import sys

import networkx as nx
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as mr  # noqa: E402

from admm_hip import image_metrics, psnr, ssim  # noqa: E402
from admm_hip.admm import EXTRA_KEYS, HISTORY_KEYS, run_admm  # noqa: E402
from block_6_admm_loop_ver2 import decentralized_admm  # noqa: E402

U = 2.0 ** -53


def test_taps_are_normalised_and_symmetric():
    w = mr.taps()
    assert w.shape == (11,) and abs(w.sum() - 1.0) <= 4 * U
    assert np.array_equal(w, w[::-1])
    assert w[5] / w[0] == pytest.approx(math.exp(25.0 / 4.5), rel=1e-14)


@pytest.mark.parametrize("N", [11, 12, 33])
def test_ssim_of_an_image_with_itself_is_one(N):
    _, x = mr.phantom(N, 0.3, seed=N)
    m = mr.ssim_map(x, x, 1.0)
    assert m.shape == (N - 10, N - 10)
    assert np.array_equal(m, np.ones_like(m))  # numerator and denominator are the same expressions
    assert mr.ssim(x, x, 1.0) == 1.0


@pytest.mark.parametrize("a,b", [(0.25, 0.75), (0.5, 0.5), (0.0, 1.0), (0.3, 0.9)])
def test_two_constant_images(a, b):
    """Zero variances: S = (2ab + c1) / (a^2 + b^2 + c1).  The window sum of a constant a is
    a * (sum of the 121 weights), which is 1 only up to rounding, so E[x^2] - mu^2 is not 0 but at
    most ~ 2 * 121 u a^2 (u = 2^-53; 121-term sums): relative to c2 = 9e-4 that bounds the
    deviation of the contrast factor by 4 * 121 u (a^2 + b^2) / c2, < 1.2e-10 here; measured: 0
    to 2e-13."""
    N, L = 16, 1.0
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    got = mr.ssim_map(np.full((N, N), a), np.full((N, N), b), L)
    tol = 4 * 121 * U * (a * a + b * b) / c2 + 8 * U
    assert np.max(np.abs(got - want)) <= tol * max(want, 1.0)


@pytest.mark.parametrize("N", [11, 23, 40])
def test_ssim_is_symmetric(N):
    ref, x = mr.phantom(N, 0.2, seed=N)
    assert np.array_equal(mr.ssim_map(x, ref, 1.0), mr.ssim_map(ref, x, 1.0))


def test_constant_offset_leaves_only_the_luminance_factor():
    """x + c against x: the (co)variances of both are those of x, the contrast factor is 1 and
    SSIM is the mean of (2 mx my + c1) / (mx^2 + my^2 + c1), my = mx + c."""
    N, c, L = 31, 0.25, 1.0
    ref, _ = mr.phantom(N)
    c1 = (0.01 * L) ** 2
    mx = mr._direct(ref)
    my = mx + c
    lum = (2 * mx * my + c1) / (mx * mx + my * my + c1)
    # the variances cancel to ~ 121 u (|x| + c)^2 against c2 = 9e-4: 2e-11 is 10x that
    assert abs(mr.ssim(ref + c, ref, L) - float(np.mean(lum))) <= 2e-11
    assert float(np.mean(lum)) < 0.95  # the offset is visible


@pytest.mark.parametrize("N", [11, 12, 33, 43, 64, 97])
def test_separable_and_direct_orders_agree(N):
    """Two float64 orders of the same window sums, in-range disk + box phantom plus noise:
    <= 1e-12 (measured <= 4e-14)."""
    for noise in (0.0, 0.05, 0.5):
        ref, x = mr.phantom(N, noise, seed=N)
        d = np.max(np.abs(mr.ssim_map(x, ref, 1.0) - mr.ssim_map_separable(x, ref, 1.0)))
        assert d <= 1e-12, (N, noise, d)


def test_psnr_restatement_is_the_reference_formula():
    ref, x = mr.phantom(20, 0.1, seed=3)
    mse = np.mean((x - ref) ** 2)
    assert mr.psnr(x, ref, 2.0) == pytest.approx(20.0 * np.log10(2.0) - 10.0 * np.log10(mse), rel=1e-14)
    assert mr.psnr(ref, ref, 1.0) == float("inf")


# --- argument errors before any device work ---------------------------------------------------

@pytest.mark.parametrize("fn", [image_metrics, psnr, ssim])
def test_data_range_must_be_positive(fn):
    ref, x = mr.phantom(16, 0.1)
    for L in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            fn(x, ref, data_range=L)


def test_small_and_mismatched_images_are_rejected():
    with pytest.raises(ValueError, match="N >= 11"):
        image_metrics(np.zeros((10, 10)), np.zeros((10, 10)), data_range=1.0)
    with pytest.raises(ValueError, match="N >= 11"):
        image_metrics(np.zeros(100), np.zeros(100), data_range=1.0)
    ref = np.zeros((16, 16))
    for bad in (np.zeros((15, 15)), np.zeros((3, 255)), np.zeros((2, 16, 15)), np.zeros(250), np.zeros((0, 256))):
        with pytest.raises(ValueError):
            image_metrics(bad, ref, data_range=1.0)
    with pytest.raises(ValueError, match="ref"):
        image_metrics(np.zeros((2, 256)), np.zeros((2, 256)), data_range=1.0)
    with pytest.raises(ValueError, match="mask"):
        image_metrics(ref, ref, data_range=1.0, mask=np.ones((15, 15)))
    edge = np.zeros((16, 16), dtype=bool)
    edge[:5] = True  # pixels, but none in the valid region
    with pytest.raises(ValueError, match="valid"):
        image_metrics(ref, ref, data_range=1.0, mask=edge)


def _run_args(N=16, V=3):
    A = [np.zeros((4, N * N))] * V
    return (A, [np.zeros(4)] * V, nx.cycle_graph(V), [np.ones(N * N)] * V, lambda i, j: np.ones(N * N), N)


@pytest.mark.parametrize("run", [run_admm, decentralized_admm])
def test_run_admm_metric_arguments_fail_before_device_work(run):
    kw = dict(verbose=False, write_params=False)
    ph = np.zeros((16, 16))
    with pytest.raises(ValueError, match="phantom_true"):
        run(*_run_args(), metrics=("psnr", "ssim"), **kw)
    with pytest.raises(ValueError, match="phantom_true"):
        run(*_run_args(), metrics="ssim", **kw)
    with pytest.raises(ValueError, match="subset"):
        run(*_run_args(), metrics=("psnr", "mse"), phantom_true=ph, **kw)
    with pytest.raises(ValueError, match="data_range"):
        run(*_run_args(), metrics=("psnr",), phantom_true=ph, data_range=0.0, **kw)
    with pytest.raises(ValueError, match="mask"):
        run(*_run_args(), metrics=("psnr",), phantom_true=ph, metrics_mask=np.ones(7), **kw)
    with pytest.raises(ValueError, match="N >= 11"):
        run(*_run_args(N=8), metrics=("ssim",), phantom_true=np.zeros((8, 8)), **kw)


def test_history_key_tuples_are_unchanged():
    assert len(HISTORY_KEYS) == 13 and EXTRA_KEYS == ("sb_res_history", "inner_updates_history")
    assert not any("psnr" in k or "ssim" in k for k in HISTORY_KEYS + EXTRA_KEYS)
