"""CPU: the ramp filter's taps, the float64 restatement of filtered back projection that the
GPU tests compare against (pinned here by the analytic sinogram of a disk), and the argument
checks of admm_fbp_filter, which run before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from admm_hip import _lib
from admm_hip.fbp import FILTERS, fbp_scale, filter_taps
from admm_hip.geometry import ParallelBeamGeometry
from oracle.geometry import Geometry, ellipse_radon, joseph_matrix

DISK = [[1.0, 0.5, 0.5, 0.0, 0.0, 0.0]]  # density 1, radius 0.5, centred


def fbp_restatement(geom: Geometry, sino, filt: str) -> np.ndarray:
    """NumPy float64 FBP: q = c tau (row * h) per angle, then the Joseph matrix's transpose."""
    n = geom.n_det
    tau = geom.h_det
    c = (np.pi / geom.n_angles) * tau / geom.h ** 2
    h = filter_taps(filt, n, tau)
    sym = np.concatenate([h[:0:-1], h])
    rows = np.asarray(sino, dtype=np.float64).reshape(geom.n_angles, n)
    q = np.stack([c * tau * np.convolve(r, sym)[n - 1:2 * n - 1] for r in rows])
    return joseph_matrix(geom).T @ q.ravel()


def disk_means(img, N):
    xc = -1.0 + (np.arange(N) + 0.5) * (2.0 / N)
    r = np.hypot(xc[:, None], xc[None, :])
    img = np.asarray(img, dtype=np.float64).reshape(N, N)
    return float(img[r < 0.35].mean()), float(img[(r > 0.65) & (r < 0.9)].mean())


@pytest.mark.parametrize("n_det", [64, 1024])
def test_ramlak_taps(n_det):
    tau = 2.0 / n_det
    h = filter_taps("ram-lak", n_det, tau)
    assert h.dtype == np.float64 and h.shape == (n_det,)
    assert np.all(h[2::2] == 0.0)
    assert h[0] == 1.0 / (4.0 * tau * tau)
    assert np.allclose(h[1::2], -1.0 / (np.pi ** 2 * np.arange(1, n_det, 2) ** 2 * tau ** 2), rtol=1e-15)
    # the ramp has no DC response: h[0] + 2 sum_{k>=1} h[k] -> 0; the odd-k tail of sum 1/k^2 beyond
    # n is < 1/(2n), so the truncated sum is within (2/pi^2)/(2n) < 1/n of 0 in units of 1/tau^2
    for name in FILTERS:
        t = filter_taps(name, n_det, tau)
        assert abs(t[0] + 2.0 * t[1:].sum()) * tau * tau < 1.0 / n_det, name


def test_hann_and_shepp_logan_taps():
    n, tau = 37, 0.03
    rl = filter_taps("ram-lak", n + 1, tau)
    hn = filter_taps("hann", n, tau)
    left = np.concatenate([rl[1:2], rl[:n - 1]])
    assert np.array_equal(hn, 0.5 * rl[:n] + 0.25 * (left + rl[1:n + 1]))
    sl = filter_taps("shepp-logan", n, tau)
    assert np.isclose(sl[0], 2.0 / (np.pi ** 2 * tau ** 2), rtol=1e-15)
    assert np.allclose(sl, -2.0 / (np.pi ** 2 * tau ** 2 * (4.0 * np.arange(n) ** 2 - 1.0)), rtol=1e-15)
    with pytest.raises(ValueError):
        filter_taps("cosine", n, tau)
    with pytest.raises(ValueError):
        filter_taps("hann", n, 0.0)


def test_scale_matches_restatement_constants():
    g = ParallelBeamGeometry(48, 37, 1.5)
    o = Geometry(48, 37, 1.5)
    assert np.isclose(fbp_scale(g), (np.pi / 37) * o.h_det / o.h ** 2, rtol=1e-15)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("N,angles,dwf", [(64, 96, 1.0), (64, 96, 1.5), (48, 37, 1.0)])
def test_restatement_reconstructs_disk(N, angles, dwf, filt):
    """The scale c = dtheta tau / h^2: FBP of the analytic disk sinogram is ~1 inside, ~0 outside."""
    geom = Geometry(N, angles, dwf)
    img = fbp_restatement(geom, ellipse_radon(geom, DISK), filt)
    inner, outer = disk_means(img, N)
    print(N, angles, dwf, filt, inner, outer)
    assert abs(inner - 1.0) < 0.01, inner
    assert abs(outer) < 0.005, outer


def test_filter_argument_checks_without_gpu_work():
    lib = _lib.load()
    assert lib.admm_abi_version() == 9  # additive entry point: no ABI bump
    a = np.zeros(64, dtype=np.float32)
    b = np.zeros(64, dtype=np.float32)
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)

    def call(sino=pa, out=pb, dtype=0, n_angles=1, n_det=64, nimg=1, tau=0.1, scale=1.0, filt=0):
        rc = lib.admm_fbp_filter(sino, out, dtype, n_angles, n_det, nimg, tau, scale, filt, None)
        return rc, lib.admm_last_error().decode()

    for kw, word in ((dict(sino=None), "sino"), (dict(out=None), "out"), (dict(out=pa), "alias"),
                     (dict(n_det=0), "n_det"), (dict(n_det=4097), "n_det"), (dict(filt=3), "filter"),
                     (dict(filt=-1), "filter"), (dict(dtype=2), "dtype"), (dict(n_angles=0), "n_angles"),
                     (dict(nimg=0), "nimg"), (dict(n_angles=1 << 10, nimg=1 << 10, n_det=2048), "nimg"),
                     (dict(tau=0.0), "det_spacing"), (dict(tau=float("nan")), "det_spacing")):
        rc, msg = call(**kw)
        assert rc == -1, kw
        assert word in msg, (kw, msg)
    rc, msg = call(out=pa)
    assert "out" in msg and "sino" in msg
