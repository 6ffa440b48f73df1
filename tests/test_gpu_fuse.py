"""GPU: the network-fused image and the consensus error (csrc/fuse.hip, admm_hip/fuse.py, run_admm's
``fuse`` / ``fuse_out``; reference: tests/fuse_ref.py, whose own properties tests/test_fuse_cpu.py checks).

* the kernels alone: xbar, the spread and the int64 sums S bitwise fuse_ref (planted cancellation, an
  all-zero pixel, +-0, a subnormal term), dev2 against math.fsum, inputs untouched; one call = chained
  calls = a permutation, bitwise; dev2 independent of batch position and stride; the NaN rule; a
  v_total larger than the images present; the argument errors;
* whole runs against fuse_ref on the reference loop's images at the project's gates, and bitwise against
  the standalone ``fuse_images`` of the returned images;
* every fuse value array_equal across pipelined / per-iteration, streams=2, two operator groups and two
  gloo ranks;
* fuse=None is the run without the keyword; the combinations with the other keywords.

Run with ``-s`` to see every case's measured errors.
"""
import ctypes as C
import math
import os

import networkx as nx
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fuse_ref as fr
import relax_ref as rr
from admm_hip import _lib, fuse_images
from admm_hip.fuse import TERM_W, TERM_WD2, TERM_WX, Fuser, fixed_sum
from admm_hip.geometry import current_stream_handle
from oracle.geometry import Geometry, joseph_matrix
from test_gpu_bounds import (RUN_APER, RUN_KW, RUN_N, RUN_TOL, RUN_V, SUM_TOL, _free_port, _np, _run, _run_problem,
                             bits, rel)

pytestmark = pytest.mark.gpu

SIZES = [169, 1089, 4096]  # less than one block, one block + a 65-pixel tail, exactly four blocks
NIMGS = [1, 3, 8, 17]  # one image, less than a load group, two groups, four groups + one
CANCEL, ZERO, SIGNED, TINY = 5, 7, 9, 11  # the planted pixels


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------
# 1. the kernels alone
# --------------------------------------------------------------------------------------
def _case(n, nimg, weighted, seed=0):
    rng = np.random.default_rng([seed, n, nimg])
    x = rng.standard_normal((nimg, n))
    w = rng.uniform(0.5, 2.0, (nimg, n)) if weighted else None
    if nimg >= 3:  # 1e8 - 1e8 + 1e-8: a float64 sum keeps or loses the 1e-8 depending on its order
        x[:, CANCEL] = 0.0
        x[0, CANCEL], x[1, CANCEL], x[2, CANCEL] = 1e8, -1e8, 1e-8
        if weighted:
            w[:3, CANCEL] = 1.0
    x[:, ZERO] = 0.0
    x[:, SIGNED] = np.where(np.arange(nimg) % 2 == 1, -0.0, 0.0)
    x[:, TINY] = 0.0
    x[0, TINY] = 5e-324
    return x, w


def _upload(a, idx, pad, dev):
    """Rows ``idx`` of ``a`` on the device; ``pad`` > 0: as a view of rows n + pad doubles apart."""
    rows = np.ascontiguousarray(a[idx])
    if not pad:
        return torch.from_numpy(rows).to(dev)
    buf = torch.full((rows.shape[0], rows.shape[1] + pad), 9.0, dtype=torch.float64, device=dev)
    buf[:, : rows.shape[1]] = torch.from_numpy(rows).to(dev)
    return buf[:, : rows.shape[1]]


def _device(x, w, dev, parts=None, V_total=None, pad=0):
    """The four kernels through Fuser on host arrays, the images in the chained calls ``parts``: host S,
    xbar, spread and dev2 (in the images' own order), after checking that the inputs were only read."""
    V, n = x.shape
    V_total = V if V_total is None else V_total
    parts = [np.arange(V)] if parts is None else parts
    fz = Fuser(n, max(len(p) for p in parts), dev)
    xs = [_upload(x, p, pad, dev) for p in parts]
    ws = [_upload(w, p, pad + 6 if pad else 0, dev) if w is not None else None for p in parts]
    den = fixed_sum(fz, [(None, wd) for wd in ws], None, TERM_W, V_total) if w is not None else None
    num = fixed_sum(fz, list(zip(xs, ws)), None, TERM_WX, V_total)
    mean = fz.finish(num, den, V_total, torch.empty(n, dtype=torch.float64, device=dev))
    var = fixed_sum(fz, list(zip(xs, ws)), mean, TERM_WD2, V_total)
    spread = fz.finish(var, den, V_total, torch.empty(n, dtype=torch.float64, device=dev), root=True)
    dev2 = np.empty(V)
    for p, xd in zip(parts, xs):
        dev2[p] = fz.deviation(xd, mean).cpu().numpy()
    torch.cuda.synchronize()
    for p, xd, wd in zip(parts, xs, ws):  # only read, gaps of a strided view included
        assert _same(xd.cpu().numpy(), x[p])
        assert wd is None or _same(wd.cpu().numpy(), w[p])
        if pad:
            assert torch.all(xd.as_strided((len(p), pad), (n + pad, 1), n) == 9.0)
    return dict(S=num.acc.cpu().numpy(), xbar=mean.cpu().numpy(), spread=spread.cpu().numpy(), dev2=dev2)


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weights"])
@pytest.mark.parametrize("nimg", NIMGS)
@pytest.mark.parametrize("n", SIZES)
def test_fusion_is_bitwise_the_numpy_restatement(cuda, n, nimg, weighted):
    x, w = _case(n, nimg, weighted)
    want_x, want_s = fr.fuse(x, w, spread=True)
    _, s, S = fr.fixed_sum(x if w is None else w * x)
    for pad in (0, 7):  # contiguous rows; rows n + 7 (weights n + 13) apart: every second one odd-aligned
        got = _device(x, w, cuda, pad=pad)
        assert np.array_equal(got["S"], S), int(np.sum(got["S"] != S))
        assert _same(got["xbar"], want_x), int(np.sum(bits(got["xbar"]) != bits(want_x)))
        assert _same(got["spread"], want_s), int(np.sum(bits(got["spread"]) != bits(want_s)))
        ref = fr.dev2(x, want_x)
        err = float(np.max(np.abs(got["dev2"] - ref) / np.maximum(ref, 1e-300))) if nimg > 1 else 0.0
        print(f"\nFUSE n={n} nimg={nimg} {'w' if weighted else 'u'} pad={pad}: s={s} dev2 rel err max {err:.1e}")
        if nimg > 1:
            assert np.all(ref > 0) and err <= SUM_TOL
        else:  # one image: xbar is the image (the grid is finer than its pixels' own), dev2 = 0 or tiny
            assert np.all(got["dev2"] <= 1e-25 * n)
    assert want_x[ZERO] == 0.0 and want_s[ZERO] == 0.0 and not np.signbit(want_x[SIGNED])
    if nimg >= 3 and not weighted:
        assert abs(want_x[CANCEL] * nimg - 1e-8) <= nimg * 2.0 ** -s


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weights"])
@pytest.mark.parametrize("nimg", [3, 8, 17])
def test_chained_calls_and_permutations_give_the_same_bits(cuda, nimg, weighted):
    n = 1089
    x, w = _case(n, nimg, weighted, seed=1)
    one = _device(x, w, cuda)
    rng = np.random.default_rng(nimg)
    perm = rng.permutation(nimg)
    k = max(1, nimg // 3)
    splits = {"two": [np.arange(k), np.arange(k, nimg)],
              "three": [np.array([0, 2]), np.array([1]), np.arange(3, nimg)] if nimg > 3 else
              [np.array([0, 2]), np.array([1])],
              "permuted": [perm], "permuted halves": [perm[: nimg // 2], perm[nimg // 2:]]}
    for name, parts in splits.items():
        got = _device(x, w, cuda, parts=parts)
        assert np.array_equal(got["S"], one["S"]), name
        for key in ("xbar", "spread", "dev2"):
            assert _same(got[key], one[key]), (name, key)
    # ({0, 2} | {1, ...} is the grouping for which float64 partial sums lose the planted 1e-8: test_fuse_cpu)


def test_an_images_deviation_does_not_depend_on_batch_position_or_stride(cuda):
    n, nimg = 1089, 8
    x, w = _case(n, nimg, True, seed=2)
    mean = torch.from_numpy(fr.fuse(x, w)).to(cuda)
    fz = Fuser(n, nimg, cuda)
    full = fz.deviation(torch.from_numpy(x).to(cuda), mean).cpu().numpy().copy()
    for v in (0, 3, 7):
        assert _same(fz.deviation(torch.from_numpy(x[v:v + 1].copy()).to(cuda), mean).cpu().numpy(), full[v:v + 1])
    perm = [5, 0, 7, 2]
    assert _same(fz.deviation(torch.from_numpy(x[perm]).to(cuda), mean).cpu().numpy(), full[perm])
    assert _same(fz.deviation(_upload(x, np.arange(nimg), 7, cuda), mean).cpu().numpy(), full)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weights"])
def test_one_non_finite_term_makes_every_output_nan(cuda, weighted, bad):
    x, w = _case(1089, 8, weighted)
    x[6, 1000] = bad
    got = _device(x, w, cuda, parts=[np.arange(5), np.arange(5, 8)])
    for key in ("xbar", "spread", "dev2"):
        assert np.isnan(got[key]).all(), key
    if weighted:  # a bad weight too
        x, w = _case(1089, 8, True)
        w[2, 3] = bad
        got = _device(x, w, cuda)
        assert np.isnan(got["xbar"]).all() and np.isnan(got["spread"]).all()


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weights"])
def test_a_larger_v_total_gives_the_references_shift(cuda, weighted):
    """The multi-rank case seen from one rank: 3 of 64 nodes."""
    x, w = _case(1089, 3, weighted, seed=3)
    got = _device(x, w, cuda, V_total=64)
    want_x, want_s = fr.fuse(x, w, V_total=64, spread=True)
    _, s, S = fr.fixed_sum(x if w is None else w * x, V_total=64)
    assert s == fr.fixed_sum(x if w is None else w * x)[1] - 4
    assert np.array_equal(got["S"], S) and _same(got["xbar"], want_x) and _same(got["spread"], want_s)


def test_argument_errors_are_refused_before_any_launch(cuda):
    lib = _lib.load()
    need = C.c_longlong()
    assert lib.admm_fuse_absmax_work(1089, 3, C.byref(need)) == 0 and need.value == 2 * 3
    assert lib.admm_fuse_deviation_work(4096, 17, C.byref(need)) == 0 and need.value == 4 * 17
    for fn in (lib.admm_fuse_absmax_work, lib.admm_fuse_deviation_work):
        assert fn(0, 3, C.byref(need)) != 0 and fn(1089, 0, C.byref(need)) != 0 and fn(1089, 65536, C.byref(need)) != 0
        assert fn(1089, 3, None) != 0
    x, w = (torch.ones((2, 64), dtype=torch.float64, device=cuda) for _ in range(2))
    m, out = (torch.zeros(64, dtype=torch.float64, device=cuda) for _ in range(2))
    work, b = torch.zeros(8, dtype=torch.float64, device=cuda), torch.zeros(1, dtype=torch.float64, device=cuda)
    acc = torch.zeros(64, dtype=torch.int64, device=cuda)
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    z = C.c_void_p(0)
    s = C.c_void_p(current_stream_handle(cuda))
    INV = -1  # ADMM_E_INVALID
    calls = {
        "admm_fuse_absmax": ((p(x), 64, p(w), 64, p(m), 64, 2, 0, p(work), p(b), s),
                             [(0, z), (8, z), (9, z), (1, 63), (3, 63), (5, 0), (6, 0), (6, 65536), (7, 3), (7, -1)]),
        "admm_fuse_accumulate": ((p(x), 64, p(w), 64, p(m), 64, 2, 0, p(b), 2, p(acc), s),
                                 [(0, z), (8, z), (10, z), (1, 63), (3, 63), (5, 0), (6, 0), (7, 3), (9, 0), (9, 1),
                                  (9, 2 ** 30 + 1)]),
        "admm_fuse_finish": ((p(acc), p(b), p(acc), p(b), 2, 64, 0, p(out), s),
                             [(0, z), (1, z), (2, z), (3, z), (7, z), (4, 0), (4, 2 ** 30 + 1), (5, 0)]),
        "admm_fuse_deviation": ((p(x), 64, p(m), 64, 2, p(work), p(out), s),
                                [(0, z), (2, z), (5, z), (6, z), (1, 63), (3, 0), (4, 0), (4, 65536)]),
    }
    for name, (ok, bads) in calls.items():
        for i, bad in bads:
            args = list(ok)
            args[i] = bad
            assert getattr(lib, name)(*args) == INV, (name, i)
            assert len(lib.admm_last_error()) > 0
    args = list(calls["admm_fuse_absmax"][0])  # mode 2 needs m
    args[4], args[7] = z, 2
    assert lib.admm_fuse_absmax(*args) == INV and b"m is null" in lib.admm_last_error()
    torch.cuda.synchronize()
    assert float(b.item()) == 0.0 and not acc.any() and not out.any()  # nothing ran
    for name, (ok, _) in calls.items():  # and the unmodified calls are accepted
        assert getattr(lib, name)(*ok) == 0, name
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        fuse_images(np.ones((2, 9)), np.zeros((2, 9)))
    with pytest.raises(ValueError):
        fuse_images(np.ones((2, 9)), np.ones((3, 9)))


def test_fuse_images_accepts_lists_arrays_and_tensors(cuda):
    x, w = _case(1089, 3, True, seed=4)
    want_x, want_s = fr.fuse(x, w, spread=True)
    a = fuse_images(x.reshape(3, 33, 33), w.reshape(3, 33, 33), spread=True, deviations=True)
    assert a[0].shape == (33, 33) and a[1].shape == (33, 33) and a[2].shape == (3,)
    assert _same(a[0].reshape(-1), want_x) and _same(a[1].reshape(-1), want_s)
    b = fuse_images([torch.from_numpy(r).to(cuda) for r in x], list(w))  # device images, host weights
    assert isinstance(b, torch.Tensor) and b.is_cuda and _same(b.cpu().numpy(), want_x)
    c = fuse_images(x, deviations=True)
    assert _same(c[0], fr.fuse(x)) and c[1].shape == (3,)


# --------------------------------------------------------------------------------------
# 2. whole runs: 4-node ring, N = 33, 12 angles per node, sigma = 0.5, 6 iterations
# --------------------------------------------------------------------------------------
ITERS = 6
KEYS = ("consensus_err", "consensus_err_per_node", "fused_img_mse")
MKEYS = KEYS + ("fused_psnr", "fused_ssim")


def _fused_run(dtype, fuse, keys=KEYS, **kw):
    """test_gpu_bounds._run without bounds and with ``fuse``: (images, fuse histories, fuse_out, history)."""
    fo = {}
    kw.setdefault("iters", ITERS)
    x, h, full = _run(dtype, bounds=kw.pop("bounds", None), keys=keys, fuse=fuse, fuse_out=fo, **kw)
    return x, h, {k: _np(v) for k, v in fo.items()}, full


def _equal_runs(a, b, what):
    xa, ha, fa, _ = a
    xb, hb, fb, _ = b
    assert np.array_equal(xa, xb), what
    assert set(ha) == set(hb) and set(fa) == set(fb) == {"image", "spread"}
    for k in ha:
        assert np.array_equal(ha[k], hb[k]), (what, k)
    for k in fa:
        assert _same(fa[k], fb[k]), (what, k)


@pytest.fixture(scope="module")
def ref_images():
    """{dtype: the reference loop's images after ITERS iterations} on the Joseph matrix and the device's
    sinograms (relax_ref with alpha = 1 is oracle.admm's loop), computed once."""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            ops, ph, sinos, Wi, Q = _run_problem(dtype)
            A = joseph_matrix(Geometry(RUN_N, RUN_APER))
            x, _, _ = rr.relaxed_admm([A] * RUN_V, [_np(s).reshape(-1) for s in sinos], nx.cycle_graph(RUN_V), Q, RUN_N,
                                      alpha=1.0, max_iters=ITERS, phantom_true=_np(ph), **RUN_KW)
            cache[dtype] = (np.stack(x), np.stack([_np(w).reshape(-1) for w in Wi]), _np(ph).reshape(-1))
        return cache[dtype]
    return get


@pytest.mark.parametrize("fuse", ["uniform", "precision"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fused_run_matches_reference_and_the_standalone_function(cuda, monkeypatch, ref_images, dtype, fuse):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    via = "dropin" if fuse == "uniform" else "run_admm"
    x, h, fo, full = _fused_run(dtype, fuse, keys=MKEYS + ("img_mse_total",), via=via, metrics=("psnr", "ssim"))
    xo, W, ph = ref_images(dtype)
    wo = W if fuse == "precision" else None
    want = fr.fuse(xo, wo)
    cons = math.sqrt(float(np.sum(fr.dev2(xo, want))))
    errs = {"images": rel(x, xo), "xbar": rel(fo["image"].reshape(-1), want),
            "consensus_err": rel(h["consensus_err"][-1], cons)}
    print(f"\nFUSED RUN {dtype} {fuse}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" | consensus_err {h['consensus_err'][0]:.3e} -> {h['consensus_err'][-1]:.3e}, |xbar| "
          f"{np.linalg.norm(want):.3e}")
    assert all(len(h[k]) == ITERS for k in MKEYS) and h["consensus_err_per_node"].shape == (ITERS, RUN_V)
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)
    # bitwise: the standalone function on the returned images
    ops, pht, sinos, Wi, Q = _run_problem(dtype)
    xbar, sp, d2 = fuse_images(list(x), Wi if fuse == "precision" else None, spread=True, deviations=True)
    assert _same(fo["image"].reshape(-1), _np(xbar).reshape(-1))
    assert _same(fo["spread"].reshape(-1), _np(sp).reshape(-1))
    assert _same(h["consensus_err_per_node"][-1], np.sqrt(_np(d2)))
    assert h["consensus_err"][-1] == math.sqrt(float(np.sum(_np(d2))))
    assert np.all(fo["spread"] >= 0) and fo["image"].shape == (RUN_N, RUN_N)
    # the fused image's scores are the public metrics of the returned fused image
    from admm_hip.metrics import psnr, ssim
    assert h["fused_psnr"][-1] == float(psnr(fo["image"], pht)[0])
    assert h["fused_ssim"][-1] == float(ssim(fo["image"], pht)[0])
    assert rel(h["fused_img_mse"][-1], float(fr.dev2(fo["image"].reshape(1, -1), ph)[0])) <= SUM_TOL
    if fuse == "uniform":  # sum_i |x_i - x*|^2 = V |xbar - x*|^2 + sum_i |x_i - xbar|^2, every iteration
        rhs = RUN_V * h["fused_img_mse"] + h["consensus_err"] ** 2
        gap = float(np.max(np.abs(h["img_mse_total"] - rhs) / h["img_mse_total"]))
        print(f"identity gap {gap:.1e}")
        assert gap <= 1e-10


# --------------------------------------------------------------------------------------
# 3. invariance: every fuse value is array_equal however the nodes are grouped
# --------------------------------------------------------------------------------------
def test_pipelined_and_per_iteration_runs_are_equal(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    for fuse in ("uniform", "precision"):
        a = _fused_run("float32", fuse, keys=MKEYS, iters=4, metrics=("psnr", "ssim"))
        b = _fused_run("float32", fuse, keys=MKEYS, iters=4, metrics=("psnr", "ssim"), pipeline=False)
        _equal_runs(a, b, fuse)
        assert a[1]["consensus_err"].shape == (4,) and np.all(a[1]["consensus_err"] > 0)


def test_streams_split_is_bitwise_one_batch(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = {}
    a = _fused_run("float32", "precision", keys=MKEYS, V=16, iters=3, metrics=("psnr", "ssim"),
                   inspect=lambda rg: seen.setdefault(1, len(rg.batches)))
    b = _fused_run("float32", "precision", keys=MKEYS, V=16, iters=3, metrics=("psnr", "ssim"), streams=2,
                   inspect=lambda rg: seen.setdefault(2, len(rg.batches)))
    assert seen == {1: 1, 2: 2}
    _equal_runs(a, b, "streams")


def _two_group_run(**kw):
    """A 4-node ring whose nodes have 13, 13, 12, 12 angles: two operator groups, so two device batches."""
    from admm_hip.admm import run_admm
    from admm_hip.data import make_precisions, make_sinograms
    from admm_hip.solver import make_operators
    import bounds_ref as br
    ops = make_operators(RUN_N, 4, 50, dtype="float32", device=0)
    assert [A.geom.n_angles for A in ops] == [13, 13, 12, 12]
    ph = torch.from_numpy(br.blocks_phantom(RUN_N).reshape(RUN_N, RUN_N))
    sinos = make_sinograms(ops, ph, 0.5, seed=1000)
    Wi, Q = make_precisions(ops)
    fo, seen = {}, {}
    x, h = run_admm(ops, sinos, nx.cycle_graph(4), Wi, Q, RUN_N, max_iters=3, verbose=False, phantom_true=ph,
                    write_params=False, fuse="precision", fuse_out=fo, metrics=("psnr",),
                    inspect=lambda rg: seen.update(batches=len(rg.batches)), **RUN_KW, **kw)
    assert seen["batches"] == 2
    run = (np.stack(x), {k: np.asarray(h[k]) for k in KEYS + ("fused_psnr",)}, {k: _np(v) for k, v in fo.items()}, h)
    return run, Wi, ph


def test_two_operator_groups_fuse_like_one_batch(cuda, monkeypatch):
    """Nodes with unequal angle counts cannot share a batch, so the one-batch side of the comparison is the
    standalone function (one batch of all four images) on the returned images; the two-batch run is also
    equal in its pipelined and per-iteration forms."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    a, Wi, ph = _two_group_run()
    b, _, _ = _two_group_run(pipeline=False)
    _equal_runs(a, b, "two groups")
    x, h, fo, _ = a
    xbar, sp, d2 = fuse_images(x, Wi, spread=True, deviations=True)
    assert _same(fo["image"].reshape(-1), _np(xbar)) and _same(fo["spread"].reshape(-1), _np(sp))
    assert _same(h["consensus_err_per_node"][-1], np.sqrt(_np(d2)))
    from admm_hip.metrics import psnr
    assert h["fused_psnr"][-1] == float(psnr(fo["image"], ph)[0])


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = {}
        for pipeline in (None, False):
            x, h, fo, _ = _fused_run("float32", "precision", keys=MKEYS, iters=4, metrics=("psnr", "ssim"),
                                     pipeline=pipeline)
            out[pipeline] = (x, h, fo, None)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_one_rank_bitwise(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    one = _fused_run("float32", "precision", keys=MKEYS, iters=4, metrics=("psnr", "ssim"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in range(2):
        for pipeline in (None, False):
            _equal_runs(one, res[r][pipeline], (r, pipeline))


# --------------------------------------------------------------------------------------
# 4. off is off; the combinations; the refusals
# --------------------------------------------------------------------------------------
def test_fuse_none_is_the_run_without_the_keyword(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    seen = []
    look = lambda rg: seen.append((rg.fuse_mode, rg.node_stat_width,  # noqa: E731
                                   [hasattr(nb, "fuser") for nb in rg.batches]))
    x0, _, h0 = _run("float32", iters=3, bounds=None, keys=(), metrics=("psnr",), inspect=look)
    x1, _, h1 = _run("float32", iters=3, bounds=None, keys=(), metrics=("psnr",), fuse=None, fuse_out=None,
                     inspect=look)
    assert np.array_equal(x0, x1) and set(h0) == set(h1)
    assert not [k for k in h1 if "fuse" in k or "consensus" in k]
    for k in h0:
        assert np.array_equal(np.asarray(h0[k]), np.asarray(h1[k]), equal_nan=True), k
    assert seen[0] == seen[1] and seen[0][0] is None and seen[0][2] == [False]
    # and with the keyword the images and the other histories are still those
    x2, _, h2 = _run("float32", iters=3, bounds=None, keys=(), metrics=("psnr",), fuse="precision")
    assert np.array_equal(x0, x2)
    for k in h0:
        assert np.array_equal(np.asarray(h0[k]), np.asarray(h2[k]), equal_nan=True), k
    assert set(h2) - set(h0) == set(KEYS) | {"fused_psnr"}


COMBOS = {
    "bounds-feasible": dict(bounds=(0.0, 1.0), return_feasible=True),
    "relaxation": dict(relaxation=1.6),
    "derived": dict(edge_state="derived"),
    "weighted": dict(fusion="weighted"),
}


@pytest.mark.parametrize("combo", list(COMBOS))
def test_combinations_run_and_stay_finite(cuda, monkeypatch, combo):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    monkeypatch.delenv("ADMM_EDGE_STATE", raising=False)
    x, h, fo, _ = _fused_run("float32", "precision", iters=2, **COMBOS[combo])
    for k in KEYS:
        assert np.all(np.isfinite(h[k])), k
    assert np.all(np.isfinite(fo["image"])) and np.all(np.isfinite(fo["spread"]))
    if combo == "bounds-feasible":  # a convex combination of box-feasible images: inside the box exactly
        assert np.all(x >= 0.0) and np.all(x <= 1.0)
        assert fo["image"].min() >= 0.0 and fo["image"].max() <= 1.0
        ops, ph, sinos, Wi, Q = _run_problem("float32")  # (the run clips the quotient's last ulp into the box)
        assert _same(fo["image"].reshape(-1), np.clip(_np(fuse_images(list(x), Wi)).reshape(-1), 0.0, 1.0))


def test_explicit_matrix_nodes_fuse(cuda):
    from admm_hip.data import make_precisions, shepp_logan
    from block_6_admm_loop_ver2 import decentralized_admm
    N = 32
    mats = [joseph_matrix(Geometry(N, a)).tocsr() for a in (33, 32, 31)]
    ph = shepp_logan(N).numpy().ravel()
    rng = np.random.default_rng(5)
    sinos = [(A @ ph + 0.005 * rng.standard_normal(A.shape[0])).astype(np.float32) for A in mats]
    Wi, Q = make_precisions(mats)
    fo = {}
    x, h = decentralized_admm(mats, sinos, nx.complete_graph(3), Wi, Q, N, lam_tv=0.02, rho=2.0, max_iters=2,
                              eps_pri=0.0, eps_dual=0.0, phantom_true=ph, verbose=False, write_params=False,
                              fuse="precision", fuse_out=fo)
    for k in KEYS:
        assert np.all(np.isfinite(np.asarray(h[k]))), k
    assert _same(fo["image"].reshape(-1), fuse_images(np.stack(x), np.stack([_np(w).reshape(-1) for w in Wi])))


def test_bad_fuse_values_raise_value_error(cuda):
    for bad in ("median", "Uniform", 1, True, ("uniform",)):
        with pytest.raises(ValueError, match="fuse"):
            _run("float32", iters=1, bounds=None, fuse=bad)
    with pytest.raises(ValueError, match="fuse_out"):
        _run("float32", iters=1, bounds=None, fuse_out={})
    with pytest.raises(ValueError, match="fuse_out"):
        _run("float32", iters=1, bounds=None, fuse="uniform", fuse_out=[])
