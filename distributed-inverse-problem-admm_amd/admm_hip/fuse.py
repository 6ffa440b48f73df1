"""The network-fused image and the consensus error (scope row f11).

A decentralized run ends with one image per graph node.  What one publishes is their fusion

    xbar = (sum_i W_i x_i) / (sum_i W_i)        per pixel, over ALL graph nodes

-- the precision-weighted mean (``fuse="precision"``, W = Wi_list; ADMM_Algo.pdf eq.(2)'s rule applied to
the whole network) or the plain mean (``"uniform"``) -- and what one monitors is the consensus error
||x_i - xbar||, the graph-independent agreement measure, with the per-pixel weighted standard deviation
across nodes (``spread``) as a cheap uncertainty map.

The sums over nodes run across device batches, streams and ranks, so they are fixed-point
(csrc/fuse.hip; include/admm_tomo.h states the arithmetic): exact in int64, hence bitwise the same in
any order and grouping.  Their resolution is 2 V^2 B 2^-61 absolute, B the largest term of the whole
network -- one wild pixel coarsens every pixel's grid.

``Fuser`` owns one batch's kernel scratch and enqueues the four entry points; ``fuse_images`` is the
standalone function; ``run_admm(fuse=...)`` goes through groups.RankGroups.enable_fuse / fuse_images.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .geometry import current_stream_handle, default_device

FUSE_MODES = ("uniform", "precision")
TERM_WX, TERM_W, TERM_WD2 = 0, 1, 2  # admm_fuse_absmax / admm_fuse_accumulate `mode`
FUSE_KEYS = ("consensus_err", "consensus_err_per_node", "fused_img_mse")
FUSE_SCALARS = 1  # rank-replicated scalars ahead of the fused metrics: |xbar - phantom|^2


def check_fuse(fuse):
    """None, "uniform" or "precision"; anything else raises ValueError.  Host work only."""
    if fuse is None:
        return None
    if not isinstance(fuse, str) or fuse not in FUSE_MODES:
        raise ValueError(f"fuse must be None or one of {FUSE_MODES}, got {fuse!r}")
    return fuse


_p = _lib.ptr


def _rows(t, nimg, n, what):
    if t.dtype != torch.float64 or t.dim() != 2 or tuple(t.shape) != (nimg, n) or t.stride(1) != 1 or \
            (nimg > 1 and t.stride(0) < n):
        raise ValueError(f"{what} must be a float64 ({nimg}, {n}) device tensor with unit inner stride and rows "
                         f"that do not overlap, got {tuple(t.shape)} {t.dtype}")
    return int(t.stride(0)) if nimg > 1 else n


class FixedSum:
    """One fixed-point sum of n pixels in flight: the int64 accumulator S and the one double B."""

    def __init__(self, n: int, device):
        self.acc = torch.zeros(int(n), dtype=torch.int64, device=device)
        self.bmax = torch.zeros(1, dtype=torch.float64, device=device)

    def zero_(self):
        self.acc.zero_()
        self.bmax.zero_()
        return self


class Fuser:
    """The fusion kernels on batches of up to ``nimg`` images of ``n`` pixels on ``device``: the scratch of
    the absmax and deviation launches (used one after the other on one stream) and the (nimg,) deviations."""

    def __init__(self, n: int, nimg: int, device):
        self.lib = _lib.load()
        self.n, self.nimg = int(n), int(nimg)
        self.dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        need = max(_lib.work_size(fn, self.n, self.nimg)
                   for fn in ("admm_fuse_absmax_work", "admm_fuse_deviation_work"))
        self.work = torch.empty(need, dtype=torch.float64, device=self.dev)  # one scratch serves both launches
        self.dev2 = torch.zeros(self.nimg, dtype=torch.float64, device=self.dev)

    def new_sum(self) -> FixedSum:
        return FixedSum(self.n, self.dev)

    def _terms(self, x, w, mean, mode):
        if mode not in (TERM_WX, TERM_W, TERM_WD2):
            raise ValueError(f"mode must be 0, 1 or 2, got {mode!r}")
        lead = x if x is not None else w
        if lead is None:
            raise ValueError("x and w are both None")
        nimg = lead.shape[0]
        if not 1 <= nimg <= self.nimg:
            raise ValueError(f"the batch holds {nimg} images, the scratch is for 1 .. {self.nimg}")
        xs = _rows(x, nimg, self.n, "x") if x is not None else self.n
        ws = _rows(w, nimg, self.n, "w") if w is not None else self.n
        if mean is not None and (mean.dtype != torch.float64 or mean.numel() != self.n or not mean.is_contiguous()):
            raise ValueError(f"mean must be a contiguous float64 tensor of {self.n} pixels")
        return nimg, xs, ws

    def absmax(self, x, w, mean, mode: int, fs: FixedSum, stream: int | None = None) -> None:
        """fs.bmax <- max(fs.bmax, max |term|) over the rows of ``x`` (``w``: their weights or None)."""
        nimg, xs, ws = self._terms(x, w, mean, mode)
        s = current_stream_handle(self.dev) if stream is None else stream
        _lib.check(self.lib.admm_fuse_absmax(_p(x), xs, _p(w), ws, _p(mean), self.n, nimg, mode, _p(self.work),
                                             _p(fs.bmax), C.c_void_p(s)), "admm_fuse_absmax")

    def accumulate(self, x, w, mean, mode: int, fs: FixedSum, v_total: int, stream: int | None = None) -> None:
        """fs.acc += the rows' quantised terms at the shift of fs.bmax (the B of all ``v_total`` nodes)."""
        nimg, xs, ws = self._terms(x, w, mean, mode)
        s = current_stream_handle(self.dev) if stream is None else stream
        _lib.check(self.lib.admm_fuse_accumulate(_p(x), xs, _p(w), ws, _p(mean), self.n, nimg, mode, _p(fs.bmax),
                                                 int(v_total), _p(fs.acc), C.c_void_p(s)), "admm_fuse_accumulate")

    def finish(self, num: FixedSum, den: FixedSum | None, v_total: int, out, root: bool = False,
               stream: int | None = None):
        """out <- num / den per pixel (``den`` None: / v_total), ``root``: its square root."""
        if out.dtype != torch.float64 or out.numel() != self.n or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float64 tensor of {self.n} pixels")
        s = current_stream_handle(self.dev) if stream is None else stream
        _lib.check(self.lib.admm_fuse_finish(_p(num.acc), _p(num.bmax), _p(den.acc if den else None),
                                             _p(den.bmax if den else None), int(v_total), self.n, int(bool(root)),
                                             _p(out), C.c_void_p(s)), "admm_fuse_finish")
        return out

    def deviation(self, x, mean, out=None, stream: int | None = None):
        """out (default ``dev2``) [v] <- sum_p (x_v[p] - mean[p])^2 of the rows of ``x``."""
        nimg, xs, _ = self._terms(x, None, mean, TERM_WX)
        out = self.dev2[:nimg] if out is None else out
        if out.dtype != torch.float64 or out.numel() != nimg or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float64 tensor of {nimg} entries")
        s = current_stream_handle(self.dev) if stream is None else stream
        _lib.check(self.lib.admm_fuse_deviation(_p(x), xs, _p(mean), self.n, nimg, _p(self.work), _p(out),
                                                C.c_void_p(s)), "admm_fuse_deviation")
        return out


def _stack(images, what):
    """``images`` ((V, n), (V, N, N) or a list of images; array or tensor) as (is a tensor, (V, ...) data)."""
    if isinstance(images, (list, tuple)):
        if not images:
            raise ValueError(f"{what} holds no image")
        if isinstance(images[0], torch.Tensor):
            return True, torch.stack([torch.as_tensor(im) for im in images])
        return False, np.stack([np.asarray(im) for im in images])
    if isinstance(images, torch.Tensor):
        return True, images
    return False, np.asarray(images)


def _device_rows(data, V, n, dev):
    t = data if isinstance(data, torch.Tensor) else torch.as_tensor(data)
    t = t.to(device=dev, dtype=torch.float64).reshape(V, n)
    return t if t.stride(1) == 1 and (V == 1 or t.stride(0) >= n) else t.contiguous()


def fuse_images(images, weights=None, spread=False, deviations=False):
    """The fusion xbar = (sum_i w_i x_i) / (sum_i w_i) of ``images`` -- (V, n), (V, N, N) or a list of V
    images, array or tensor -- with ``weights`` None (the plain mean) or of the same shape, finite and > 0
    (checked on the host for host inputs; the caller's promise for device tensors).  Returns xbar shaped
    like one image, and with ``spread`` / ``deviations`` a tuple (xbar[, spread][, dev2]): the per-pixel
    weighted standard deviation across the images and the (V,) vector |x_i - xbar|^2.  Arrays come back as
    arrays, tensors as device tensors.  The sums over images are fixed-point (csrc/fuse.hip): the result
    does not depend on the order of the images, and it is bitwise what ``run_admm(fuse=...)`` forms from
    the same images.  A NaN or infinite image or weight makes every output NaN."""
    is_t, x = _stack(images, "images")
    if x.ndim not in (2, 3) or x.shape[0] < 1:
        raise ValueError(f"images must be (V, n) or (V, N, N), got shape {tuple(x.shape)}")
    shape1 = tuple(x.shape[1:])
    V, n = int(x.shape[0]), int(np.prod(shape1))
    w = None
    if weights is not None:
        w_t, w = _stack(weights, "weights")
        if w.ndim < 2 or w.shape[0] != V or int(np.prod(tuple(w.shape[1:]))) != n:
            raise ValueError(f"weights have shape {tuple(w.shape)}, the images {tuple(x.shape)}")
        if not (w_t and w.is_cuda):
            wh = w.numpy() if w_t else w
            if not (np.all(np.isfinite(wh)) and np.all(wh > 0)):
                raise ValueError("weights must be finite and > 0")
    dev = None
    for t in (x, w):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            dev = t.device
            break
    dev = torch.device("cuda", default_device()) if dev is None else dev
    with torch.cuda.device(dev):
        xd = _device_rows(x, V, n, dev)
        wd = _device_rows(w, V, n, dev) if w is not None else None
        fz = Fuser(n, V, dev)
        mean = torch.empty(n, dtype=torch.float64, device=dev)
        den = None
        if wd is not None:
            den = fixed_sum(fz, [(None, wd)], None, TERM_W, V)
        num = fixed_sum(fz, [(xd, wd)], None, TERM_WX, V)
        fz.finish(num, den, V, mean)
        out = [mean.view(shape1)]
        if spread:
            var = fixed_sum(fz, [(xd, wd)], mean, TERM_WD2, V)
            out.append(fz.finish(var, den, V, torch.empty_like(mean), root=True).view(shape1))
        if deviations:
            out.append(fz.deviation(xd, mean).clone())
    if not is_t:
        out = [t.cpu().numpy() for t in out]
    return out[0] if len(out) == 1 else tuple(out)


def fixed_sum(fz: Fuser, parts, mean, mode: int, v_total: int, fs: FixedSum | None = None) -> FixedSum:
    """fixed_sum of the terms ``mode`` over ``parts`` = [(x rows, w rows or None)] on the current stream, one
    process: every part's absmax, then every part's accumulate."""
    fs = fz.new_sum() if fs is None else fs.zero_()
    for x, w in parts:
        fz.absmax(x, w, mean, mode, fs)
    for x, w in parts:
        fz.accumulate(x, w, mean, mode, fs, v_total)
    return fs
