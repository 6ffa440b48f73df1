"""Float64 NumPy restatement of admm_hip.metrics (PSNR of the reference's helper,
/root/reference/test_final_integration.py:41-45; SSIM of Wang et al. 2004 as skimage's
structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=L)).

``ssim_map`` is a direct 2-D window sum: 121 shifted slices of the image weighted by the outer
product of the 1-D Gaussian taps, added in row-major tap order -- deliberately not the separable
(rows, then columns) order a kernel would use.  ``ssim_map_separable`` is that other order, kept to
measure how far two float64 orders of the same sums differ.
"""
import math

import numpy as np

R = 5
WIN = 2 * R + 1
SIGMA = 1.5


def taps():
    """The 11 Gaussian taps, normalised to sum 1."""
    k = np.arange(WIN, dtype=np.float64) - R
    w = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


def _direct(f):
    """Window sum of the (N, N) field at the valid centres: (N - 10, N - 10)."""
    N = f.shape[0]
    v = N - 2 * R
    w2 = np.outer(taps(), taps())
    out = np.zeros((v, v))
    for a in range(WIN):
        for b in range(WIN):
            out += w2[a, b] * f[a:a + v, b:b + v]
    return out


def _separable(f):
    N = f.shape[0]
    v = N - 2 * R
    w = taps()
    h = np.zeros((N, v))
    for b in range(WIN):
        h += w[b] * f[:, b:b + v]
    out = np.zeros((v, v))
    for a in range(WIN):
        out += w[a] * h[a:a + v, :]
    return out


def _map(x, y, L, win):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] != x.shape[1] or x.shape != y.shape or x.shape[0] < WIN:
        raise ValueError("two equal (N, N) images with N >= 11")
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my = win(x), win(y)
    vx = win(x * x) - mx * mx
    vy = win(y * y) - my * my
    vxy = win(x * y) - mx * my
    return ((2.0 * mx * my + c1) * (2.0 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim_map(x, y, L):
    """SSIM at the valid centres 5 <= i, j <= N - 6: (N - 10, N - 10)."""
    return _map(x, y, L, _direct)


def ssim_map_separable(x, y, L):
    return _map(x, y, L, _separable)


def _valid_mask(mask, N):
    if mask is None:
        return np.ones((N - 2 * R, N - 2 * R), dtype=bool)
    return np.asarray(mask).reshape(N, N)[R:N - R, R:N - R] != 0


def ssim(x, y, L, mask=None, separable=False):
    """Mean SSIM over the valid centres (under ``mask``)."""
    m = (ssim_map_separable if separable else ssim_map)(x, y, L)
    keep = _valid_mask(mask, m.shape[0] + 2 * R)
    return math.fsum(m[keep].tolist()) / int(keep.sum())


def sse(x, y, mask=None):
    """sum (x - y)^2 over the masked pixels, correctly rounded (math.fsum)."""
    d = (np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)).ravel()
    if mask is not None:
        d = d[np.asarray(mask).ravel() != 0]
    return math.fsum((d * d).tolist())


def psnr(x, y, L, mask=None):
    """test_final_integration.py:41-45 with the mean taken over the masked pixels."""
    n = np.asarray(x).size if mask is None else int((np.asarray(mask) != 0).sum())
    mse = sse(x, y, mask) / n
    if mse == 0:
        return float("inf")
    return 20.0 * math.log10(L) - 10.0 * math.log10(mse)


def phantom(N, noise=0.0, seed=0):
    """(reference, image): a disk plus a box in [0, 1] and the same with Gaussian noise added."""
    i, j = np.mgrid[0:N, 0:N]
    c = (N - 1) / 2.0
    ref = 0.6 * (((i - c) ** 2 + (j - c) ** 2) <= (0.4 * N) ** 2)
    ref = ref + 0.4 * ((np.abs(i - 0.4 * N) <= 0.12 * N) & (np.abs(j - 0.55 * N) <= 0.2 * N))
    rng = np.random.default_rng(seed)
    return ref, ref + noise * rng.standard_normal((N, N))
