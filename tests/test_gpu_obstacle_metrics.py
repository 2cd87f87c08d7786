"""Realised-path metrics against obstacle rows (scpqp_metrics_accumulate_obstacles,
include/scpqp_obstacles.h): nominal rows against the constant obstacles, bitwise; turning
rows with their own footprints against the fp64 mirror (tests/obstacle_mirror.py over
tests/metrics_mirror.py); the bad-row rule; batch splits and variant indices.

Integer outputs, infinities and the exact zeros of the gaps are compared exactly.  The
double-valued outputs differ from the mirror through sincos / sin / hypot and FMA
contraction, in the pose of the obstacle and in the gap.  Measured on an MI355X: the
largest |device - mirror| of the outputs in metres (gaps and margins, dense and
accumulated) over every test of this file is 1.4e-14 m (coordinates up to 30 m; the
16-vehicle case).  The tolerance is ten times that, and asserted to be below 1e-9 m.
sum_sq_xtrack is a sum of n squares e^2 in m^2 and is held to n d (2 max e + d) with d the
tolerance, as tests/test_gpu_metrics.py holds it (measured: 7.3e-12 m^2, 87 ticks).
"""
import math
import types

import numpy as np
import pytest
import torch

import metrics_mirror as MM
import obstacle_mirror as OM

pytestmark = pytest.mark.gpu

MEASURED_MAX_DIFF = 1.421e-14     # metres; see the module docstring
TOL = 10 * MEASURED_MAX_DIFF
assert TOL <= 1e-9
PI = math.pi
INT_FIELDS = ("argmin_gap_veh", "argmin_gap_obs", "first_collision_tick", "n_collision_ticks",
              "n_ticks_seen")
DBL_FIELDS = ("min_gap_veh", "min_gap_obs", "min_margin_veh", "min_margin_obs", "max_xtrack",
              "sum_sq_xtrack")
SHAPES = [(3, 2, 3, 5), (2, 16, 2, 44), (3, 1, 22, 41)]   # (B, n_veh, n_obst, K)
TICK0 = 120


def scenario(rng, nV, nO, span, dsafe=2.0):
    obstacles = [(rng.uniform(-span, span), rng.uniform(-span, span), rng.uniform(-PI, PI),
                  rng.uniform(0, 3), rng.uniform(1, 4), rng.uniform(0.5, 2)) for _ in range(nO)]
    return types.SimpleNamespace(
        nVeh=nV, nObst=nO, Length=list(rng.uniform(0.5, 2.0, nV)), Width=list(rng.uniform(0.4, 1.0, nV)),
        obstacles=[np.asarray(o, float) for o in obstacles],
        dsafeVehicles=np.full((nV, nV), dsafe) + 0.01 * np.arange(nV * nV).reshape(nV, nV),
        dsafeObstacles=np.full((nV, nO), dsafe) + 0.01 * np.arange(nV * nO).reshape(nV, nO),
        referenceTrajectories=[np.asarray([(-100.0, float(v)), (100.0, float(v))]) for v in range(nV)],
        tick_length=0.01)


def random_path(rng, B, nV, K, span):
    x = np.zeros((B, nV, K, 6))
    x[..., 0:2] = rng.uniform(-span, span, (B, nV, K, 2))
    x[..., 2] = rng.uniform(-PI, PI, (B, nV, K))
    x[..., 3:] = rng.normal(0, 1, (B, nV, K, 3))      # never read by the metrics
    return x


def turning_rows(rng, sc, B):
    """The scenario's obstacles with their own start, speed, footprint and turn rate per
    realisation."""
    rows = np.broadcast_to(OM.nominal_rows(sc)[None], (B, sc.nObst, 7)).copy()
    rows[..., 0:2] += rng.uniform(-1, 1, (B, sc.nObst, 2))
    rows[..., 3] = rng.uniform(0.0, 3.0, (B, sc.nObst))
    rows[..., 4] = rng.uniform(0.5, 4.0, (B, sc.nObst))
    rows[..., 5] = rng.uniform(0.3, 2.0, (B, sc.nObst))
    rows[..., 6] = rng.uniform(-0.8, 0.8, (B, sc.nObst))
    return rows


def case(shape, seed):
    B, nV, nO, K = shape
    rng = np.random.default_rng(seed)
    span = 3.0 if nV <= 2 else 14.0
    sc = scenario(rng, nV, nO, span)
    return sc, random_path(rng, B, nV, K, span), rng


def smallest_margin(base, rows, x, tick0):
    """The smallest |separation margin| over every rectangle pair and axis of the path, the
    obstacles posed by the realisation's rows (rows None: the constant obstacles)."""
    m = math.inf
    for b in range(x.shape[0]):
        Cn = base if rows is None else OM.RowConstants(base, rows[b])
        for k in range(x.shape[2]):
            rects = [MM._rect(x[b, v, k, 0], x[b, v, k, 1], x[b, v, k, 2], Cn.length[v], Cn.width[v])
                     for v in range(Cn.nV)]
            obs = [Cn.obstacle_rect(o, tick0 + k) for o in range(Cn.nO)]
            for v in range(Cn.nV):
                for other in rects[v + 1:] + obs:
                    m = min(m, min(abs(t) for t in MM.separation_margins(rects[v], other)))
    return m


def close(name, got, want, tol=None):
    tol = TOL if tol is None else tol
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, name
    special = np.isinf(want) | np.isinf(got)
    if "gap" in name:
        special |= (want == 0.0) | (got == 0.0)
    assert np.array_equal(got[special], want[special]), name
    d = float(np.abs(got[~special] - want[~special]).max()) if (~special).any() else 0.0
    print(f"max |device - mirror| {name}: {d:.3e}")
    assert d <= tol, (name, d)


def check_result(res, want, tag):
    for k in INT_FIELDS:
        assert np.array_equal(res[k].cpu().numpy(), want[k]), (tag, k)
    for k in DBL_FIELDS[:-1]:
        close(f"{tag}.{k}", res[k].cpu().numpy(), want[k])
    n, e = float(want["n_ticks_seen"].max()), float(want["max_xtrack"].max())
    close(f"{tag}.sum_sq_xtrack", res["sum_sq_xtrack"].cpu().numpy(), want["sum_sq_xtrack"],
          tol=max(n * TOL * (2 * e + TOL), 1e-300))


def same(a, b, tag):
    """Two result or dense dicts, bit for bit."""
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (tag, k)


def dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu)


# ---------------------------------------------------------------------------
# 1. nominal rows are the constant obstacles, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_nominal_rows_are_the_constant_obstacles_bitwise(gpu, shape):
    from scpqp import obstacles as OB
    from scpqp.metrics import PathMetrics
    B, nV, nO, K = shape
    sc, x, rng = case(shape, 31)
    x2 = random_path(rng, B, nV, K, 3.0 if nV <= 2 else 14.0)
    x2[:, :, 0] = x[:, :, -1]
    rows = OB.nominal(sc, B, device=gpu)
    out = {}
    for name, kw in (("const", {}), ("rows", dict(obstacles=rows))):
        pm = PathMetrics(sc, B, gpu)
        pm.reset(B)
        d1 = pm.accumulate(dev(x, gpu), TICK0, 0, dense=True, **kw)
        d2 = pm.accumulate(dev(x2, gpu), TICK0 + K - 1, 1, dense=True, **kw)
        out[name] = (d1, d2, pm.result())
        pm.close()
    for i, tag in enumerate(("dense call 1", "dense call 2", "accumulator")):
        same(out["const"][i], out["rows"][i], tag)
    res = out["rows"][2]
    assert torch.isfinite(res["min_gap_obs"]).all() and (res["n_ticks_seen"] == 2 * K - 1).all()
    go = out["rows"][0]["gap_obs"]
    assert tuple(go.shape) == (B, K, nV, nO) and (go > 0).any()


# ---------------------------------------------------------------------------
# 2. turning rows against the mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_turning_rows_match_the_mirror(gpu, shape):
    """Two consecutive calls (k_first 0, then 1 on the step that starts where the first
    ended), dense outputs of both, against the mirror with the obstacles posed by the rows.
    Realisation 0 drives its vehicle 0 into obstacle 0 at entry 2 of the second call: the
    vehicle's centre on the turned obstacle's centre, a gap of 0.0 and a collision tick."""
    from scpqp.metrics import PathMetrics
    B, nV, nO, K = shape
    sc, x1, rng = case(shape, 37)
    span = 3.0 if nV <= 2 else 14.0
    x2 = random_path(rng, B, nV, K, span)
    x2[:, :, 0] = x1[:, :, -1]
    rows = turning_rows(rng, sc, B)
    rows[0, 0, 6] = 0.7                                   # turned by more than 0.8 rad at the hit
    t1 = TICK0 + K - 1
    hit = t1 + 2
    px, py, ph = OM.pose(rows[0, 0], hit * sc.tick_length)
    assert ph - rows[0, 0, 2] > 0.8
    x2[0, 0, 2, 0:2] = (px, py)
    base = MM.Constants.of_scenario(sc)
    calls = [(x1, TICK0, 0), (x2, t1, 1)]
    margin = min(smallest_margin(base, rows, x, t0) for x, t0, _ in calls)
    print(f"smallest separation margin: {margin:.3e}")
    assert margin > 1e-6
    pm = PathMetrics(sc, B, gpu)
    pm.reset(B)
    r = dev(rows, gpu)
    dense = [pm.accumulate(dev(x, gpu), t0, kf, dense=True, obstacles=r) for x, t0, kf in calls]
    res = pm.result()
    torch.cuda.synchronize()
    tag = f"turn{nV}x{nO}"
    for (x, t0, _), d in zip(calls, dense):
        for b in range(B):
            md = MM.dense(OM.RowConstants(base, rows[b]), x[b], t0)
            for k in ("gap_veh", "gap_obs", "xtrack"):
                close(f"{tag}.{k}", d[k][b].cpu().numpy(), md[k])
    want = OM.run(base, rows, calls, B)
    check_result(res, want, tag)
    # the constructed overlap
    assert float(dense[1]["gap_obs"][0, 2, 0, 0]) == 0.0
    assert float(res["min_gap_obs"][0]) == 0.0 and int(res["first_collision_tick"][0]) >= 0
    assert int(res["first_collision_tick"][0]) <= hit and int(res["n_collision_ticks"][0]) >= 1
    assert MM.overlap((x2[0, 0, 2, 0], x2[0, 0, 2, 1], x2[0, 0, 2, 2], base.length[0], base.width[0]),
                      (px, py, ph, rows[0, 0, 4], rows[0, 0, 5]))
    # the rows are read: the constant obstacles give other gaps
    pm.reset(B)
    other = pm.accumulate(dev(x1, gpu), TICK0, 0, dense=True)
    assert not torch.equal(other["gap_obs"], dense[0]["gap_obs"])
    pm.close()


# ---------------------------------------------------------------------------
# 3. a bad row leaves its realisation untouched
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("field, value", [(3, math.nan), (5, -1.0), (6, math.inf)])
def test_a_bad_row_leaves_its_realisation_untouched(gpu, field, value):
    from scpqp.metrics import PathMetrics
    shape = SHAPES[0]
    B, nV, nO, K = shape
    sc, x, rng = case(shape, 41)
    rows = turning_rows(rng, sc, B)
    pm = PathMetrics(sc, B, gpu)
    pm.reset(B)
    good_dense = pm.accumulate(dev(x, gpu), TICK0, 0, dense=True, obstacles=dev(rows, gpu))
    good = pm.result()
    pm.reset(B)
    cleared = pm.result()
    bad = rows.copy()
    bad[1, nO - 1, field] = value
    d = pm.accumulate(dev(x, gpu), TICK0, 0, dense=True, obstacles=dev(bad, gpu))
    res = pm.result()
    for k in res:
        assert torch.equal(res[k][1], cleared[k][1]), k            # the reset values
        assert torch.equal(res[k][0], good[k][0]) and torch.equal(res[k][2], good[k][2]), k
    assert (res["n_ticks_seen"] == torch.tensor([K, 0, K], device=gpu, dtype=torch.int32)).all()
    for k in ("gap_veh", "gap_obs", "xtrack"):
        assert torch.equal(d[k][0], good_dense[k][0]) and torch.equal(d[k][2], good_dense[k][2]), k
    # the dense rows of realisation 1 are not written either: an array prefilled with a sentinel
    from scpqp import _lib as LB
    import ctypes as C
    sentinel = -7.0
    gap = torch.full((B, K, nV, nO), sentinel, dtype=torch.float64, device=gpu)
    D = LB.MetricsDense(gap_veh=None, gap_obs=gap.data_ptr(), xtrack=None)
    xd, rd = dev(x, gpu), dev(bad, gpu)
    rc = pm.lib.scpqp_metrics_accumulate_obstacles(
        pm.h, B, K - 1, TICK0, 0, C.c_void_p(xd.data_ptr()), None, C.byref(D), None,
        C.c_void_p(rd.data_ptr()), pm._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert (gap[1] == sentinel).all() and torch.equal(gap[0], good_dense["gap_obs"][0])
    assert torch.equal(gap[2], good_dense["gap_obs"][2])
    pm.close()


# ---------------------------------------------------------------------------
# 4. batch splits and variant indices
# ---------------------------------------------------------------------------
def test_split_and_variant_order_change_nothing(gpu):
    """B = 6 with rows and two variants (other footprints and dsafe tables) interleaved, two
    steps: the same in one call, in calls on the slices [0:2] and [2:6], and with the
    realisations sorted by variant; and it is what the mirror gives per variant."""
    from scpqp.metrics import PathMetrics
    shape = (6, 3, 4, 9)
    B, nV, nO, K = shape
    sc, x1, rng = case(shape, 43)
    x2 = random_path(rng, B, nV, K, 14.0)
    x2[:, :, 0] = x1[:, :, -1]
    rows = turning_rows(rng, sc, B)
    sc_b = types.SimpleNamespace(**vars(sc))
    sc_b.Length, sc_b.Width = [v * 1.5 for v in sc.Length], [w * 0.5 for w in sc.Width]
    sc_b.dsafeObstacles, sc_b.dsafeVehicles = sc.dsafeObstacles + 1.0, sc.dsafeVehicles + 0.5
    var = np.array([0, 1, 0, 1, 0, 1], np.int32)
    calls = [(x1, TICK0, 0), (x2, TICK0 + K - 1, 1)]

    def run(idx, max_batch):
        pm = PathMetrics(sc, max_batch, gpu, variants=[sc, sc_b])
        pm.reset(len(idx))
        for x, t0, kf in calls:
            pm.accumulate(dev(x[idx], gpu), t0, kf, variant=var[idx], obstacles=dev(rows[idx], gpu))
        out = pm.result()
        pm.close()
        return out

    whole = run(np.arange(6), 6)
    a, b = run(np.arange(0, 2), 2), run(np.arange(2, 6), 7)
    order = np.argsort(var, kind="stable")
    srt = run(order, 6)
    for k in INT_FIELDS + DBL_FIELDS:
        assert torch.equal(whole[k], torch.cat([a[k], b[k]])), k
        assert torch.equal(whole[k][torch.as_tensor(order, device=gpu)], srt[k]), k
    bases = [MM.Constants.of_scenario(sc), MM.Constants.of_scenario(sc_b)]
    for v in (0, 1):
        idx = np.flatnonzero(var == v)
        assert min(smallest_margin(bases[v], rows[idx], x[idx], t0) for x, t0, _ in calls) > 1e-6
        want = OM.run(bases[v], rows[idx], [(x[idx], t0, kf) for x, t0, kf in calls], len(idx))
        check_result({k: t[torch.as_tensor(idx, device=gpu)] for k, t in whole.items()}, want, f"var{v}")
    assert not torch.equal(whole["min_margin_obs"][0::2], whole["min_margin_obs"][1::2])


def test_accumulate_checks_the_rows(gpu):
    from scpqp.metrics import PathMetrics
    shape = SHAPES[0]
    B, nV, nO, K = shape
    sc, x, rng = case(shape, 47)
    rows = dev(turning_rows(rng, sc, B), gpu)
    pm = PathMetrics(sc, B, gpu)
    pm.reset(B)
    xd = dev(x, gpu)
    for bad in (rows[:2], rows[:, :2], rows[..., :6], rows.float(), rows.cpu(), rows.cpu().numpy()):
        with pytest.raises(ValueError, match="obstacles"):
            pm.accumulate(xd, TICK0, 0, obstacles=bad)
    assert (pm.result()["n_ticks_seen"] == 0).all()
    pm.close()
    rng = np.random.default_rng(1)
    free = scenario(rng, 2, 0, 3.0)
    pm = PathMetrics(free, 1, gpu)
    pm.reset(1)
    with pytest.raises(ValueError, match="no obstacles"):
        pm.accumulate(dev(random_path(rng, 1, 2, 3, 3.0), gpu), 0, 0,
                      obstacles=torch.zeros((1, 0, 7), dtype=torch.float64, device=gpu))
    pm.close()
