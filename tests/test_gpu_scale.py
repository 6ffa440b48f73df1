"""GPU: the self-scaling Huber threshold (admm_ray_quantile, admm_huber_weights_dev,
run_admm(robust={"scale": k}); references: tests/scale_ref.py).

* the quantile kernel against its NumPy restatement, bitwise (delta, a_k, cnt), on inputs chosen to break a
  radix select; an image alone bitwise the image in a batch; two calls in a row bitwise;
* admm_huber_weights_dev bitwise admm_huber_weights at the same thresholds, stride 1 and 3;
* run_admm(robust={"scale": ...}) against scale_ref.irls_scale_run at the whole-run gates (1e-9 float64,
  1e-5 float32 samples), the thresholds included;
* the zinger case at scale = 4: the bars of test_gpu_robust.py, the final thresholds the reference's;
* pipelined / read-back, one / two streams, two batches / each alone, delta_min = inf / robust = inf:
  bitwise.

Run with ``-s`` to see the measured figures.
"""
import math

import networkx as nx
import numpy as np
import pytest
import torch

import robust_ref as rr
import scale_ref as sc
import state_ref as sr
from admm_hip import huber_weights, ray_quantile
from admm_hip.geometry import ParallelBeamGeometry, RayTransform, current_stream_handle
from admm_hip.robust import RayQuantile
from test_gpu_robust import INF_CASE, _run, _same_history, rel
from test_gpu_state_update import _set_mirror

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
TDT = {"float32": torch.float32, "float64": torch.float64}
NDT = {"float32": np.float32, "float64": np.float64}
UDT = {"float32": np.uint32, "float64": np.uint64}
RUN_TOL = {"float32": 1e-5, "float64": 1e-9}  # the whole-run gates
MS = (1, 2, 3, 255, 1024, 1025, 2049, 4097)
QS = (0.0, 0.25, 0.5, 1.0)


# --------------------------------------------------------------------------------------
# the quantile kernel
# --------------------------------------------------------------------------------------
def _mask(rng, shape, dt):
    w = rng.uniform(0.5, 2.0, shape).astype(dt)
    w[rng.random(shape) < 0.1] = 0
    return w


def _inputs(kind, dtype, nimg, m, with_w):
    """(ax, b, w or None, c, floor) of the input class ``kind``; the residual is ax - b in the sample type."""
    dt, ut = NDT[dtype], UDT[dtype]
    rng = np.random.default_rng([len(kind), ord(kind[0]), ord(kind[-1]), nimg, m, int(with_w)])
    shape = (nimg, m)
    b = np.zeros(shape, dt)
    w = _mask(rng, shape, dt) if with_w else None
    c, floor = 1.4826 * 4.0, 0.0
    fi = np.finfo(dt)
    if kind == "normal":
        ax = rng.standard_normal(shape).astype(dt)
        b = (ax.astype(np.float64) + 0.4 * rng.standard_normal(shape)).astype(dt)
    elif kind == "ties":
        ax = np.full(shape, 0.75, dt)
    elif kind == "two":  # two values, the median rank on either side of the boundary
        ax = np.empty(shape, dt)
        for v in range(nimg):
            live = m if w is None else int(np.count_nonzero(w[v]))
            low = min(m, int(math.floor(0.5 * max(live - 1, 0))) + (v + m) % 2)
            row = np.where(np.arange(m) < low, 1.0, 2.0)
            ax[v] = rng.permutation(row) * rng.choice([-1.0, 1.0], m)
    elif kind == "lowbit":  # 1.0 and its next seven neighbours: the last pass decides
        ax = (np.array(1.0, dt).view(ut) + rng.integers(0, 8, shape).astype(ut)).view(dt)
    elif kind == "topexp":  # powers of two across the whole exponent range: the first pass decides
        e = rng.integers(fi.minexp, fi.maxexp, shape)
        ax = (np.ldexp(1.0, e) * rng.choice([-1.0, 1.0], shape)).astype(dt)
    elif kind == "mix":
        pool = np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, 3 * fi.smallest_subnormal, fi.tiny,
                         1.0, -1.5, fi.max, -fi.max, np.inf, -np.inf], dt)
        ax = pool[rng.integers(0, pool.size, shape)]
    elif kind == "nan":  # an unmasked NaN sorts last
        ax = rng.standard_normal(shape).astype(dt)
        ax[:, m // 2] = np.nan
        if w is not None:
            w[:, m // 2] = 1
    elif kind == "masked_junk":  # NaN and inf on masked rays only (without w: nothing is masked, plain rays)
        ax = rng.standard_normal(shape).astype(dt)
        if w is not None:
            dead = w == 0
            ax[dead] = np.nan
            b[dead & (rng.random(shape) < 0.5)] = np.inf
    elif kind == "all_masked":
        ax = rng.standard_normal(shape).astype(dt)
        w = np.zeros(shape, dt)
    elif kind == "one_unmasked":
        ax = rng.standard_normal(shape).astype(dt)
        w = np.zeros(shape, dt)
        w[np.arange(nimg), rng.integers(0, m, nimg)] = 2
    elif kind == "floor":  # c a_k < floor: the floor wins
        ax = rng.standard_normal(shape).astype(dt)
        c, floor = 1e-3, 10.0
    elif kind == "zero_median":  # more than half the rays with exactly zero residual
        ax = rng.standard_normal(shape).astype(dt)
        b = np.where(np.arange(m)[None, :] % 4 != 3, ax, b).astype(dt)  # three rays in four
    else:
        raise KeyError(kind)
    return ax, b, w, c, floor


KINDS = ["normal", "ties", "two", "lowbit", "topexp", "mix", "nan", "masked_junk", "all_masked", "one_unmasked",
         "floor", "zero_median"]


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(a).to(cuda)


def _same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), equal_nan=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantile_is_bitwise_its_restatement(cuda, dtype, kind):
    seen = {"finite": 0, "inf": 0}
    for m in MS:
        for nimg in (1, 3):
            for with_w in (False, True):
                ax, b, w, c, floor = _inputs(kind, dtype, nimg, m, with_w)
                for q in QS:
                    got = np.stack([t.cpu().numpy() for t in ray_quantile(_dev(ax, cuda), _dev(b, cuda), q,
                                                                          _dev(w, cuda), c, floor)], axis=1)
                    assert got.shape == (nimg, 3) and got.dtype == np.float64
                    for v in range(nimg):
                        want = sc.ray_quantile_ref(ax[v], b[v], q, c, floor, None if w is None else w[v], NDT[dtype])
                        assert _same(got[v], want), (m, nimg, with_w, q, v, got[v].tolist(), want)
                        assert not math.isnan(got[v, 0]) and got[v, 0] > 0  # never NaN, never <= 0
                        seen["finite" if math.isfinite(got[v, 0]) else "inf"] += 1
                    if kind == "nan" and q == 0.5:  # (a mask may leave a short row fewer than three rays)
                        some = got[:, 2] >= 3
                        assert np.all(np.isfinite(got[some, 0])) and np.all(np.isfinite(got[some, 1]))
                    if kind == "nan" and q == 1.0:
                        assert np.all(np.isnan(got[:, 1])) and np.all(np.isinf(got[:, 0]))
                    if kind == "all_masked":
                        assert _same(got, [[math.inf, 0.0, 0.0]] * nimg)
                    if kind == "one_unmasked":
                        assert np.all(got[:, 2] == 1)
                    if kind == "floor":
                        assert np.all(got[got[:, 2] > 0, 0] == 10.0)  # (a mask may leave a short row no ray)
                    if kind == "zero_median" and q == 0.5:
                        assert np.all(np.isinf(got[:, 0])) and np.all(got[:, 1] == 0)
    print(f"\nQUANTILE {dtype} {kind}: {seen}")
    if kind in ("normal", "ties", "two", "lowbit", "topexp", "floor", "one_unmasked", "masked_junk"):
        assert seen["finite"] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantile_alone_is_bitwise_the_image_in_a_batch(cuda, dtype):
    for m in (255, 1025, 4097, 8193, 16391):  # (8192 rays per sweep of the block: one, two, three sweeps)
        for with_w in (False, True):
            ax, b, w, c, floor = _inputs("normal", dtype, 3, m, with_w)
            full = torch.stack(ray_quantile(_dev(ax, cuda), _dev(b, cuda), 0.5, _dev(w, cuda), c, floor), 1)
            full = full.cpu().numpy()
            assert len({tuple(r) for r in full.tolist()}) == 3  # three different images
            for v in range(3):
                assert _same(full[v], sc.ray_quantile_ref(ax[v], b[v], 0.5, c, floor, None if w is None else w[v],
                                                          NDT[dtype])), (m, with_w, v)
            for v in (0, 2):  # either end of the batch
                one = torch.stack(ray_quantile(_dev(ax[v], cuda), _dev(b[v], cuda), 0.5,
                                               None if w is None else _dev(w[v], cuda), c, floor), 1).cpu().numpy()
                assert one.shape == (1, 3) and np.array_equal(one[0], full[v]), (m, with_w, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_quantile_calls_in_a_row_agree(cuda, dtype):
    """The same buffers twice, then other data and the first again: no state survives a call."""
    m, nimg = 8193, 3
    ax, b, w, c, floor = _inputs("normal", dtype, nimg, m, True)
    ax2 = _inputs("lowbit", dtype, nimg, m, True)[0]
    rq = RayQuantile(m, nimg, TDT[dtype], cuda)
    assert np.all(np.isinf(rq.out[:, 0].cpu().numpy()))  # before the first estimate: least squares
    s = current_stream_handle(torch.device(cuda))
    d = [_dev(a, cuda) for a in (ax, b, w, ax2)]
    first = rq.run(d[0], d[1], d[2], 0.5, c, floor, s).clone()
    second = rq.run(d[0], d[1], d[2], 0.5, c, floor, s).clone()
    other = rq.run(d[3], d[1], d[2], 0.5, c, floor, s).clone()
    third = rq.run(d[0], d[1], d[2], 0.5, c, floor, s).clone()
    assert torch.equal(first, second) and torch.equal(first, third) and not torch.equal(first, other)
    assert rq.delta.stride(0) == 3 and torch.equal(rq.delta, third[:, 0])


def test_quantile_argument_errors(cuda):
    import ctypes as C
    from admm_hip import _lib
    lib = _lib.load()
    t = torch.zeros(8, dtype=torch.float64, device=cuda)
    o = torch.zeros(3, dtype=torch.float64, device=cuda)
    p = _lib.ptr
    ok = (p(t), p(t), None, _lib.ADMM_DTYPE_F64, 8, 1, 0.5, 1.0, 0.0, None, p(o), None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.admm_ray_quantile(*a)

    assert call() == 0
    assert call(_0=None) == -1 and call(_1=None) == -1 and call(_10=None) == -1 and call(_3=7) == -1
    assert call(_4=0) == -1 and call(_4=2 ** 32) == -1 and call(_5=0) == -1 and call(_5=65536) == -1
    assert call(_6=-0.1) == -1 and call(_6=1.5) == -1 and call(_6=float("nan")) == -1
    assert call(_7=0.0) == -1 and call(_7=float("nan")) == -1 and call(_8=-1.0) == -1 and call(_8=float("nan")) == -1
    need = C.c_longlong(-1)
    assert lib.admm_ray_quantile_work(4097, 3, C.byref(need)) == 0 and need.value == 0
    assert lib.admm_ray_quantile_work(0, 3, C.byref(need)) == -1
    for bad in (dict(q=1.5), dict(c=0.0), dict(floor=-1.0), dict(q=True)):
        with pytest.raises(ValueError):
            ray_quantile(t, t, **bad)


# --------------------------------------------------------------------------------------
# admm_huber_weights_dev
# --------------------------------------------------------------------------------------
def _rays(dtype, nimg, m, seed):
    rng = np.random.default_rng([seed, nimg, m])
    ax = rng.standard_normal((nimg, m)).astype(NDT[dtype])
    b = (ax.astype(np.float64) + 0.4 * rng.standard_normal((nimg, m))).astype(NDT[dtype])
    return ax, b, _mask(rng, (nimg, m), NDT[dtype])


def _strided(values, stride, cuda):
    """A (k,) float64 device view with stride ``stride`` holding ``values``; the gaps hold NaN."""
    buf = torch.full((len(values), stride), math.nan, dtype=torch.float64, device=cuda)
    buf[:, 0] = torch.tensor(values, dtype=torch.float64)
    return buf[:, 0]


def _bits(t):
    return t.cpu().numpy().reshape(-1).view(np.uint8)


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("with_w", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_thresholds_are_bitwise_the_host_threshold(cuda, dtype, with_w, stride):
    for m in (255, 1025):
        ax, b, w = (_dev(a, cuda) for a in _rays(dtype, 3, m, 21))
        w = w if with_w else None
        for delta in (rr.DELTA, math.inf):
            want = [t.clone() for t in huber_weights(ax, b, delta, w)]
            got = huber_weights(ax, b, _strided([delta] * 3, stride, cuda), w)
            for g, h in zip(got, want):
                assert np.array_equal(_bits(g), _bits(h)), (m, delta)
            if delta == rr.DELTA:
                assert float(want[2].sum()) > 0
        # three different thresholds against three single-image calls
        deltas = [0.2, math.inf, 0.55]
        got = huber_weights(ax, b, _strided(deltas, stride, cuda), w)
        for v, dv in enumerate(deltas):
            one = huber_weights(ax[v], b[v], dv, None if w is None else w[v])
            assert np.array_equal(_bits(got[0][v]), _bits(one[0]))
            assert np.array_equal(_bits(got[1][v]), _bits(one[1][0]))
            assert np.array_equal(_bits(got[2][v]), _bits(one[2][0]))


def test_device_threshold_reads_the_quantile_in_place(cuda):
    """ray_quantile's kernel output feeds the Huber kernel without leaving the device: the thresholds'
    column of RayQuantile.out, stride 3."""
    m, nimg = 1025, 3
    ax, b, w = (_dev(a, cuda) for a in _rays("float32", nimg, m, 22))
    rq = RayQuantile(m, nimg, torch.float32, cuda)
    out = rq.run(ax, b, w, 0.5, 1.345 * 1.4826, 0.0, current_stream_handle(torch.device(cuda)))
    got = huber_weights(ax, b, rq.delta, w)
    for v, dv in enumerate(out[:, 0].cpu().tolist()):
        assert math.isfinite(dv) and dv > 0
        one = huber_weights(ax[v], b[v], dv, w[v])
        assert np.array_equal(_bits(got[0][v]), _bits(one[0])) and float(got[2][v]) == float(one[2][0]) > 0
        assert np.array_equal(_bits(got[1][v]), _bits(one[1][0]))


def test_device_threshold_argument_errors(cuda):
    from admm_hip import _lib
    lib = _lib.load()
    t = torch.zeros(8, dtype=torch.float64, device=cuda)
    o = torch.zeros(8, dtype=torch.float64, device=cuda)
    d = torch.ones(1, dtype=torch.float64, device=cuda)
    p = _lib.ptr
    ok = (p(t), p(t), None, p(o), _lib.ADMM_DTYPE_F64, 8, 1, p(d), 1, p(o), p(o), None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.admm_huber_weights_dev(*a)

    assert call(_7=None) == -1 and call(_8=0) == -1 and call(_0=None) == -1 and call(_3=None) == -1
    assert call(_7=p(o)) == -1 and call(_4=7) == -1 and call(_5=0) == -1 and call(_6=0) == -1
    with pytest.raises(ValueError):
        huber_weights(t, t, torch.ones(2, dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        huber_weights(t, t, torch.ones(1, dtype=torch.float32, device=cuda))


# --------------------------------------------------------------------------------------
# whole runs
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", sc.PARITY_RUNS, ids=sc.parity_id)
def test_run_matches_the_self_scaled_reference(cuda, monkeypatch, p, dtype):
    name, every, weights, until, scale = p
    P = rr.parity_problem(name, dtype, weights)
    case = P["case"]
    _set_mirror(monkeypatch, case.mirror)
    ref = sc.parity_reference(*p, dtype)
    kw = dict(ray_weights=[P["w"][g] for g in range(case.V)]) if weights else {}
    cfg = {"scale": scale, "every": every}
    if until is not None:
        cfg["until"] = until
    x, h = _run(case, dtype, P, sc.PARITY_ITERS, robust=cfg, **kw)
    assert len(h["robust_delta_per_node"]) == sc.PARITY_ITERS
    errs = {"images": rel(x, ref["x"]), "primal": rel(h["primal"], ref["primal"]),
            "robust_loss_total": rel(h["robust_loss_total"], ref["loss_total"]),
            "robust_delta_per_node": rel(np.stack(h["robust_delta_per_node"]), np.stack(ref["delta"]))}
    got = np.stack(h["robust_outliers_per_node"])
    want = np.stack(ref["outliers"])
    room = 0 if dtype == "float64" else sc.near_threshold(ref, sc.COUNT_MARGIN)
    print(f"\nPARITY {sc.parity_id(p)} {dtype}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" outliers {got.sum(axis=1).tolist()} ref {want.sum(axis=1).tolist()} room {room}")
    for k, v in errs.items():
        assert v < RUN_TOL[dtype], (k, v)
    assert float(np.abs(got - want).sum()) <= room
    assert h["robust_outliers_total"] == [float(s) for s in got.sum(axis=1)]
    if until is not None:  # frozen: the later thresholds are the last estimate's, bitwise
        d = np.stack(h["robust_delta_per_node"])
        assert np.array_equal(d[until:], np.repeat(d[until - 1][None], len(d) - until, axis=0))


def test_zinger_case_through_run_admm_at_scale_four(cuda, monkeypatch):
    """3 % of the rays off by +-3, float64 samples, nobody knowing delta: at scale = 4 the final image error
    is <= 0.75 x the plain run's and <= 1.06 x the clean-data run's (the reference: 0.6497 and 0.9990), and
    the final per-node thresholds are the reference's within 1e-9."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    P = rr.zinger_problem()
    case = P["case"]

    def err(b, **kw):
        x, h = _run(case, "float64", P, rr.Z_ITERS, b=b, **kw)
        return math.sqrt(float(np.sum((x - P["ph"][None, :]) ** 2)) / case.V), h

    plain, _ = err(P["b_zinger"])
    clean, _ = err(P["b"])
    robust, h = err(P["b_zinger"], robust={"scale": sc.SCALE})
    ref = sc.zinger_scale_runs()["scale4"]
    d_err = float(np.max(np.abs(h["robust_delta_per_node"][-1] - ref["delta"][-1]) / ref["delta"][-1]))
    print(f"\nZINGER scale 4: plain {plain:.4f} clean {clean:.4f} robust {robust:.4f}: ratios "
          f"{robust / plain:.4f} {robust / clean:.4f}; final delta {h['robust_delta_per_node'][-1].tolist()} "
          f"(reference {ref['delta'][-1].tolist()}, rel {d_err:.2e}); outliers {h['robust_outliers_total']}")
    assert robust <= 0.75 * plain
    assert robust <= 1.06 * clean
    assert d_err <= 1e-9
    assert h["robust_outliers_total"][-1] == float(ref["outliers"][-1].sum())


# --------------------------------------------------------------------------------------
# loop forms, bitwise
# --------------------------------------------------------------------------------------
CUT = {"scale": sc.TEXTBOOK}  # thresholds that cut within a few iterations from zero


def test_pipelined_and_read_back_loops_agree(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    P = sr.case_problem(INF_CASE, "float32")
    cfg = {"scale": sc.TEXTBOOK, "every": 2, "until": 3}
    xa, ha = _run(INF_CASE, "float32", P, 4, robust=cfg, pipeline=True)
    xb, hb = _run(INF_CASE, "float32", P, 4, robust=cfg, pipeline=False)
    assert np.array_equal(xa, xb) and ha["robust_outliers_total"][-1] > 0
    _same_history(ha, hb)
    d = np.stack(ha["robust_delta_per_node"])
    assert np.array_equal(d[3], d[2]) and not np.array_equal(d[2], d[1]) and np.all(np.isfinite(d))


def test_two_streams_agree_with_one(cuda, monkeypatch):
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    case = sr.Case(33, 8, "ring", 2, 3, "iso", 12, None, "midpoint", False, 5)
    P = sr.case_problem(case, "float64")
    seen = []
    xa, ha = _run(case, "float64", P, 3, robust=CUT, streams=1, seen=seen)
    xb, hb = _run(case, "float64", P, 3, robust=CUT, streams=2, seen=seen)
    assert seen == [1, 2] and sum(ha["robust_outliers_total"]) > 0
    assert np.array_equal(xa, xb)
    _same_history(ha, hb)


def test_two_batches_agree_with_each_batch_alone(cuda, monkeypatch):
    """Six nodes, two 3-rings with 12 and 9 angles per node (two batches), against each ring's run."""
    from admm_hip.admm import run_admm
    from admm_hip.data import make_sinograms, shepp_logan
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    N, n = 33, 33 * 33
    ops = [RayTransform(ParallelBeamGeometry(N, a), "float64", 0) for a in (12, 12, 12, 9, 9, 9)]
    ph = shepp_logan(N)
    sinos = make_sinograms(ops, ph, 0.05, seed=11)
    W, q = sr.precisions(n, 6, 6)
    kw = dict(lam_tv=sr.LAM, rho=sr.RHO, mu=sr.MU, tv_iters=2, cg_iters=3, max_iters=3, eps_pri=0.0, eps_dual=0.0,
              verbose=False, phantom_true=ph, write_params=False, robust=CUT)
    seen = []
    G = nx.disjoint_union(nx.cycle_graph(3), nx.cycle_graph(3))
    x, h = run_admm(ops, sinos, G, W, q, N, inspect=lambda rg: seen.append(len(rg.batches)), **kw)
    assert seen == [2] and sum(h["robust_outliers_total"]) > 0
    for off in (0, 3):
        qs = lambda i, j, off=off: q(i + off, j + off)  # noqa: E731
        qs.qslot_key = lambda i, j, off=off: q.qslot_key(i + off, j + off)
        xs, hs = run_admm(ops[off:off + 3], sinos[off:off + 3], nx.cycle_graph(3), W[off:off + 3], qs, N, **kw)
        assert np.array_equal(np.stack(x)[off:off + 3], np.stack(xs)), off
        for k in ("robust_loss_per_node", "robust_outliers_per_node", "robust_delta_per_node", "mse_sino_per_node"):
            assert np.array_equal(np.stack(h[k])[:, off:off + 3], np.stack(hs[k])), (off, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_floor_is_bitwise_the_infinite_delta(cuda, monkeypatch, dtype):
    """delta_min = +inf makes every threshold infinite: the run is bitwise run_admm(robust=inf) -- which
    test_gpu_robust.py shows to be bitwise the plain run -- on the images and every shared history key."""
    monkeypatch.delenv("ADMM_FWD_MIRROR", raising=False)
    P = sr.case_problem(INF_CASE, dtype)
    x0, h0 = _run(INF_CASE, dtype, P, 3, robust=math.inf)
    x1, h1 = _run(INF_CASE, dtype, P, 3, robust={"scale": 4.0, "delta_min": math.inf})
    assert "robust_delta_per_node" not in h0
    assert np.all(np.isinf(np.stack(h1["robust_delta_per_node"]))) and h1["robust_outliers_total"] == [0.0] * 3
    assert np.array_equal(x0, x1)
    _same_history(h0, h1)


def test_matrix_operator_raises_before_device_work(cuda, monkeypatch):
    from admm_hip import admm
    from oracle.geometry import Geometry, joseph_matrix
    N = 16
    A = joseph_matrix(Geometry(N, 6))
    ops = [RayTransform(ParallelBeamGeometry(N, 6), "float64", 0), A.toarray()]

    def boom(*a, **k):
        raise AssertionError("device work before the argument check")

    monkeypatch.setattr(admm, "RankGroups", boom)
    W, q = sr.precisions(N * N, 2, 1)
    with pytest.raises(ValueError, match="explicit-matrix"):
        admm.run_admm(ops, [np.zeros(6 * N)] * 2, nx.path_graph(2), W, q, N, max_iters=1, verbose=False,
                      write_params=False, robust={"scale": 4.0})
