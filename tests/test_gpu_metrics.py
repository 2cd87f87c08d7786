"""Realised-path metrics on the GPU (csrc/metrics.hip) against the fp64 mirror
(tests/metrics_mirror.py).

Integer outputs, infinities and the exact zeros of the gaps are compared exactly.  The
double-valued outputs differ from the mirror only through sincos / hypot and FMA
contraction.  Measured on an MI355X: the largest |device - mirror| of the outputs in
metres (gaps, margins, cross-track errors) over the dense-output, ABI-limit and
strided-tail tests is 2.8e-14 m (a gap between rectangles at coordinates of 200 m, one
unit in the last place there); over every test of this file it is the same figure.  The
tolerance is ten times that, far below the 1e-9 m of the plant path's own agreement with
the exact flow.  sum_sq_xtrack is a sum of n squares e^2 in m^2: with every e within the
tolerance d its bound is n d (2 max e + d) (measured: 5.7e-14 m^2 in those three tests,
3.6e-12 m^2 in the 49-tick, 16-vehicle test).
"""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import metrics_mirror as MM
from oracle import scp_reference as R

pytestmark = pytest.mark.gpu

MEASURED_MAX_DIFF = 2.842e-14     # metres; see the module docstring
TOL = 10 * MEASURED_MAX_DIFF
assert TOL <= 1e-9
PI = math.pi
INT_FIELDS = ("argmin_gap_veh", "argmin_gap_obs", "first_collision_tick", "n_collision_ticks",
              "n_ticks_seen")
DBL_FIELDS = ("min_gap_veh", "min_gap_obs", "min_margin_veh", "min_margin_obs", "max_xtrack",
              "sum_sq_xtrack")
worst = {}


def scenario(length, width, obstacles=(), polylines=None, dsafe=2.0, tick_length=0.01):
    nV, nO = len(length), len(obstacles)
    if polylines is None:
        polylines = [[(-100.0, float(v)), (100.0, float(v))] for v in range(nV)]
    return types.SimpleNamespace(
        nVeh=nV, nObst=nO, Length=list(length), Width=list(width),
        obstacles=[np.asarray(o, float) for o in obstacles],
        dsafeVehicles=np.full((nV, nV), dsafe) + 0.01 * np.arange(nV * nV).reshape(nV, nV),
        dsafeObstacles=np.full((nV, nO), dsafe) + 0.01 * np.arange(nV * nO).reshape(nV, nO),
        referenceTrajectories=[np.asarray(p, float) for p in polylines], tick_length=tick_length)


def random_path(rng, B, nV, K, span):
    x = np.zeros((B, nV, K, 6))
    x[..., 0:2] = rng.uniform(-span, span, (B, nV, K, 2))
    x[..., 2] = rng.uniform(-PI, PI, (B, nV, K))
    x[..., 3:] = rng.normal(0, 1, (B, nV, K, 3))      # never read by the metrics
    return x


def smallest_margin(Cn, x, tick0):
    """The smallest |separation margin| over every rectangle pair and axis of the path."""
    m = math.inf
    for b in range(x.shape[0]):
        for k in range(x.shape[2]):
            rects = [MM._rect(x[b, v, k, 0], x[b, v, k, 1], x[b, v, k, 2], Cn.length[v], Cn.width[v])
                     for v in range(Cn.nV)]
            obs = [Cn.obstacle_rect(o, tick0 + k) for o in range(Cn.nO)]
            for v in range(Cn.nV):
                for other in rects[v + 1:] + obs:
                    m = min(m, min(abs(t) for t in MM.separation_margins(rects[v], other)))
    return m


def close(name, got, want, tol=None):
    """Doubles: infinities exactly, and for the gaps also the exact zeros (a collision on
    one side is a collision on the other); the rest within the tolerance."""
    tol = TOL if tol is None else tol
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, name
    special = np.isinf(want) | np.isinf(got)
    if "gap" in name:
        special |= (want == 0.0) | (got == 0.0)
    assert np.array_equal(got[special], want[special]), name
    d = float(np.abs(got[~special] - want[~special]).max()) if (~special).any() else 0.0
    worst[name] = max(worst.get(name, 0.0), d)
    print(f"max |device - mirror| {name}: {d:.3e}")
    assert d <= tol, (name, d)


def check_result(res, want, tag):
    for k in INT_FIELDS:
        assert np.array_equal(res[k].cpu().numpy(), want[k]), (tag, k)
    for k in DBL_FIELDS[:-1]:
        close(f"{tag}.{k}", res[k].cpu().numpy(), want[k])
    # n squares, each error within TOL of its mirror value
    n, e = float(want["n_ticks_seen"].max()), float(want["max_xtrack"].max())
    close(f"{tag}.sum_sq_xtrack", res["sum_sq_xtrack"].cpu().numpy(), want["sum_sq_xtrack"],
          tol=n * TOL * (2 * e + TOL))


def run_dense_case(gpu, sc, x, tick0, tag, k_first=0):
    """One call with dense outputs: dense arrays and the accumulator against the mirror."""
    from scpqp.metrics import PathMetrics
    Cn = MM.Constants.of_scenario(sc)
    B = x.shape[0]
    pm = PathMetrics(sc, B, gpu)
    pm.reset(B)
    d = pm.accumulate(torch.as_tensor(x, device=gpu), tick0, k_first, dense=True)
    res = pm.result()
    torch.cuda.synchronize()
    for b in range(B):
        md = MM.dense(Cn, x[b], tick0)
        for k in ("gap_veh", "gap_obs", "xtrack"):
            close(f"{tag}.{k}", d[k][b].cpu().numpy(), md[k])
    check_result(res, MM.run(Cn, [(x, tick0, k_first)], B), tag)
    pm.close()
    return d, res


def known_answer_path():
    """The host test's known answers packed into one path: three pairs of vehicles
    (0.98 x 0.88, unit squares, 4 x 0.2), 100 m apart in y, over 6 ticks."""
    sc = scenario([0.98, 0.98, 1, 1, 4, 4], [0.88, 0.88, 1, 1, 0.2, 0.2],
                  polylines=[[(-100, 0), (100, 0)], [(-100, 0), (100, 0)],
                             [(0, 100), (10, 100), (10, 110)], [(-100, 100), (100, 100)],
                             [(-100, 200), (100, 200)], [(-100, 200), (100, 200)]])
    K = 6
    x = np.zeros((1, 6, K, 6))
    c = 0.5 + 0.9 / math.sqrt(2)
    x[0, 1, :, 0] = 3.0                                   # k0: 3 apart, headings 0
    x[0, 1, 1, 2] = PI / 2                                # k1: second turned a quarter
    x[0, 1, 2, 1] = 4.0                                   # k2: corner to corner
    x[0, 1, 3, 0] = 0.5                                   # k3: half a metre apart
    x[0, 0, 4, 0:2] = (5.0, 0.3)                          # k4, k5: cross-track of vehicle 0
    x[0, 0, 5, 0:2] = (150.0, 0.3)
    x[0, 1, 4:, 0] = 50.0
    x[0, 2:4, :, 1] = 100.0
    x[0, 3, :, 0:3] = (3.0, 100.0, PI / 4)                # unit squares, second at 45 degrees
    x[0, 3, 1, 0:2] = (c, 100.0 + c)                      # k1: just off the corner
    x[0, 2, 4, 0:2] = (11.0, 99.0)                        # k4: nearest to the polyline's corner
    x[0, 4:6, :, 1] = 200.0
    x[0, 5, :, 2] = PI / 2                                # k0: crossed thin rectangles
    x[0, 5, 1:, 1] = 203.0                                # later: 0.9 apart
    pair = {p: i for i, p in enumerate((v, w) for v in range(6) for w in range(v + 1, 6))}
    gaps = {(0, pair[0, 1]): 3 - 0.49 - 0.49, (1, pair[0, 1]): 3 - 0.49 - 0.44,
            (2, pair[0, 1]): math.hypot(3 - 0.98, 4 - 0.88), (3, pair[0, 1]): 0.0,
            (0, pair[2, 3]): 3 - 0.5 - math.sqrt(2) / 2, (1, pair[2, 3]): 0.4,
            (0, pair[4, 5]): 0.0, (1, pair[4, 5]): 0.9}
    xtrack = {(4, 0): 0.3, (5, 0): 0.3, (4, 2): math.sqrt(2)}
    return sc, x, gaps, xtrack, pair


def test_dense_outputs_against_the_mirror(gpu):
    rng = np.random.default_rng(7)
    sc = scenario([0.98, 2.0, 1.0], [0.88, 0.5, 1.0],
                  obstacles=[(1.0, -1.0, 0.4, 2.0, 4.0, 2.0), (-2.0, 2.0, PI / 2, 0.0, 2.0, 2.0)],
                  polylines=[[(-9, 0), (9, 0)], [(0, -5), (3, 0), (5, 5)],
                             [(-4, -4), (0, -3), (2, 0), (4, 4)]])
    x = random_path(rng, 3, 3, 5, 3.0)
    assert smallest_margin(MM.Constants.of_scenario(sc), x, 17) > 1e-6
    d, res = run_dense_case(gpu, sc, x, 17, "random")
    gv = d["gap_veh"].cpu().numpy()
    assert (gv == 0).any() and (gv > 0).any()       # both kinds occur
    go = d["gap_obs"].cpu().numpy()
    assert (go == 0).any() and (go > 0).any()

    sc, x, gaps, xtrack, _ = known_answer_path()
    assert smallest_margin(MM.Constants.of_scenario(sc), x, 0) > 1e-6
    d, res = run_dense_case(gpu, sc, x, 0, "known")
    gv, xt = d["gap_veh"][0].cpu().numpy(), d["xtrack"][0].cpu().numpy()
    for (k, p), want in gaps.items():
        close(f"known.gap[{k},{p}]", gv[k, p], want)
    for (k, v), want in xtrack.items():
        close(f"known.xtrack[{k},{v}]", xt[k, v], want)
    assert int(res["first_collision_tick"][0]) == 0 and int(res["n_collision_ticks"][0]) == 2
    assert res["argmin_gap_veh"][0].tolist() == [0, 4, 5]     # the first gap of 0.0


def test_limits_of_the_abi(gpu):
    rng = np.random.default_rng(11)
    nV, nO = 16, 32
    obstacles = [(rng.uniform(-12, 12), rng.uniform(-12, 12), rng.uniform(-PI, PI),
                  rng.uniform(0, 3), rng.uniform(1, 4), rng.uniform(1, 3)) for _ in range(nO)]
    polylines = [np.cumsum(rng.uniform(0.5, 4.0, (8, 2)), 0) - 12.0 for _ in range(nV)]
    sc = scenario(rng.uniform(0.5, 2.0, nV), rng.uniform(0.4, 1.0, nV), obstacles, polylines)
    x = random_path(rng, 2, nV, 3, 12.0)
    assert smallest_margin(MM.Constants.of_scenario(sc), x, 1000) > 1e-6
    run_dense_case(gpu, sc, x, 1000, "limits")


def test_strided_tail_without_obstacles(gpu):
    """410 (tick, vehicle) entries and 246 pair items per realisation: several passes of
    the 64 lanes and no multiple of 64; no obstacles."""
    rng = np.random.default_rng(13)
    sc = scenario([0.98] * 4, [0.88] * 4)
    x = random_path(rng, 5, 4, 41, 4.0)
    assert smallest_margin(MM.Constants.of_scenario(sc), x, 0) > 1e-6
    d, res = run_dense_case(gpu, sc, x, 0, "tail")
    assert d["gap_obs"].numel() == 0
    assert torch.isinf(res["min_gap_obs"]).all() and torch.isinf(res["min_margin_obs"]).all()
    assert (res["argmin_gap_obs"] == -1).all()


def test_more_ticks_than_one_staged_chunk(gpu):
    """16 vehicles x 50 ticks = 800 entries: more than the kernel stages at once, so the
    lane state has to carry over its chunks of ticks (42 here); k_first = 1."""
    rng = np.random.default_rng(17)
    sc = scenario(rng.uniform(0.5, 2.0, 16), rng.uniform(0.4, 1.0, 16),
                  obstacles=[(0.0, -20.0, PI / 2, 2.0, 4.0, 2.0)])
    x = random_path(rng, 2, 16, 50, 14.0)
    # the closest approach lies in the second chunk of realisation 1
    x[1, 0, 47, 0:3] = x[1, 1, 47, 0:3] + (0.0, 2.5, 0.0)
    assert smallest_margin(MM.Constants.of_scenario(sc), x, 3) > 1e-6
    run_dense_case(gpu, sc, x, 3, "chunks", k_first=1)


def tie_path():
    """Two realisations of 3 vehicles over 11 ticks.  The vehicles stand on a fixed
    pattern scaled by a factor per tick: factor 1 gives the closest approach and is used
    at ticks {1, 2, 6} in realisation 0 and {3, 9} in realisation 1 (bitwise-equal poses,
    hence bitwise-equal gaps)."""
    base = np.array([[0.0, 0.0, 0.3], [2.1, 0.4, -1.0], [-0.5, 2.6, 2.0]])
    x = np.zeros((2, 3, 11, 6))
    for b, ties in enumerate(({1, 2, 6}, {3, 9})):
        for k in range(11):
            s = 1.0 if k in ties else 1.5 + 0.1 * k
            x[b, :, k, 0:2] = base[:, 0:2] * s
            x[b, :, k, 2] = base[:, 2]
    return x


def test_accumulation_over_calls_and_ties(gpu):
    from scpqp.metrics import PathMetrics
    sc = scenario([0.98, 2.0, 1.0], [0.88, 0.5, 1.0], obstacles=[(4.0, 4.0, 0.2, 1.0, 2.0, 1.0)],
                  polylines=[[(-9, 0), (9, 0)], [(0, -5), (3, 0), (5, 5)], [(-4, -4), (4, 4)]])
    Cn = MM.Constants.of_scenario(sc)
    x = tie_path()
    xt = torch.as_tensor(x, device=gpu)
    pm = PathMetrics(sc, 2, gpu)
    pm.reset(2)
    for lo, hi, kf in ((0, 5, 0), (4, 8, 1), (7, 11, 1)):
        pm.accumulate(xt[:, :, lo:hi].contiguous(), tick0=100 + lo, k_first=kf)
    res = pm.result()
    want = MM.run(Cn, [(x, 100, 0)], 2)                 # one pass over the concatenated ticks
    check_result(res, want, "calls")
    assert res["n_ticks_seen"].tolist() == [11, 11]
    # the earlier tick of a tie is kept: inside a call (1 before 2), across calls (1 before
    # 6; 3 before 9)
    assert res["argmin_gap_veh"][:, 0].tolist() == [101, 103]
    assert want["argmin_gap_veh"][:, 0].tolist() == [101, 103]
    d = pm.accumulate(xt, 100, 0, dense="only")["gap_veh"].cpu().numpy()
    assert np.array_equal(d[0, 1], d[0, 2]) and np.array_equal(d[0, 1], d[0, 6])
    assert np.array_equal(d[1, 3], d[1, 9])
    assert d[0, 1].min() == float(res["min_gap_veh"][0]) > 0.0
    assert torch.equal(pm.result()["n_ticks_seen"], res["n_ticks_seen"])   # dense="only"
    pm.close()


def test_split_invariance(gpu):
    """B = 6 in one call against calls on the slices [0:2] and [2:6], two steps each:
    every accumulator is bitwise equal, the running sums included."""
    from scpqp.metrics import PathMetrics
    rng = np.random.default_rng(19)
    sc = scenario([0.98, 2.0, 1.0], [0.88, 0.5, 1.0],
                  obstacles=[(1.0, -1.0, 0.4, 2.0, 4.0, 2.0), (-2.0, 2.0, PI / 2, 0.0, 2.0, 2.0)],
                  polylines=[[(-9, 0), (9, 0)], [(0, -5), (3, 0), (5, 5)], [(-4, -4), (4, 4)]])
    steps = [torch.as_tensor(random_path(rng, 6, 3, 9, 3.0), device=gpu) for _ in range(2)]

    def run(sl, max_batch):
        pm = PathMetrics(sc, max_batch, gpu)
        pm.reset(sl.stop - sl.start)
        for i, x in enumerate(steps):
            pm.accumulate(x[sl].contiguous(), tick0=8 * i, k_first=0 if i == 0 else 1)
        out = pm.result()
        pm.close()
        return out

    whole, a, b = run(slice(0, 6), 6), run(slice(0, 2), 2), run(slice(2, 6), 7)
    for k in INT_FIELDS + DBL_FIELDS:
        assert torch.equal(whole[k], torch.cat([a[k], b[k]])), k
    assert (whole["sum_sq_xtrack"] > 0).all() and whole["n_ticks_seen"].tolist() == [17] * 6


def test_collision_bookkeeping(gpu):
    """Realisation 0: two 4 x 0.2 vehicles on one line driven through each other, 3 m per
    tick, overlapping at entries 7..9 (|dx| <= 4).  Realisation 1: the crossed thin
    rectangles at every tick."""
    from scpqp.metrics import PathMetrics
    sc = scenario([4.0, 4.0], [0.2, 0.2])
    K = 15
    x = np.zeros((2, 2, K, 6))
    x[0, 1, :, 0] = 3.0 * (8 - np.arange(K))
    x[1, 1, :, 2] = PI / 2
    pm = PathMetrics(sc, 2, gpu)
    pm.reset(2)
    pm.accumulate(torch.as_tensor(x, device=gpu), tick0=40, k_first=0)
    res = {k: v.cpu().numpy() for k, v in pm.result().items()}
    assert res["first_collision_tick"].tolist() == [47, 40]
    assert res["n_collision_ticks"].tolist() == [3, K]
    assert res["min_gap_veh"].tolist() == [0.0, 0.0]
    assert res["argmin_gap_veh"].tolist() == [[47, 0, 1], [40, 0, 1]]
    assert res["n_ticks_seen"].tolist() == [K, K]
    check_result(pm.result(), MM.run(MM.Constants.of_scenario(sc), [(x, 40, 0)], 2), "collision")
    pm.close()


def test_moving_obstacle_uses_the_global_tick(gpu):
    """A frog-style obstacle (4 x 2, heading pi/2, speed 2) started at (7, -15): at global
    tick 400 + k it is centred at y = -7 + 0.02 k, its front at y = -5 + 0.02 k, and the
    vehicle's rear edge is at y = -3.44."""
    from scpqp.metrics import PathMetrics
    sc = scenario([0.98], [0.88], obstacles=[(7.0, -15.0, PI / 2, 2.0, 4.0, 2.0)])
    K = 5
    x = np.zeros((1, 1, K, 6))
    x[0, 0, :, 0:2] = (7.0, -3.0)
    pm = PathMetrics(sc, 1, gpu)
    pm.reset(1)
    d = pm.accumulate(torch.as_tensor(x, device=gpu), tick0=400, k_first=0, dense=True)
    got = d["gap_obs"][0, :, 0, 0].cpu().numpy()
    close("moving", got, 1.56 - 0.02 * np.arange(K), tol=max(TOL, 1e-14))
    res = pm.result()
    assert res["argmin_gap_obs"][0].tolist() == [404, 0, 0]
    check_result(res, MM.run(MM.Constants.of_scenario(sc), [(x, 400, 0)], 1), "moving")
    pm.close()


def test_size_validation_with_a_handle(gpu):
    """SCPQP_E_SIZE is returned before anything is launched."""
    from scpqp import _lib as LB
    from scpqp.metrics import PathMetrics
    pm = PathMetrics(scenario([1.0] * 4, [1.0] * 4), 1, gpu)
    rc = pm.lib.scpqp_metrics_accumulate(pm.h, 1 << 30, 40, 0, 0, None, C.byref(pm._acc), None, None)
    assert rc == -4 and b"too large" in pm.lib.scpqp_last_error()
    assert pm.lib.scpqp_metrics_accumulate(pm.h, 1, 4, 0, 0, None, None, None, None) == -1
    assert pm.lib.scpqp_metrics_accumulate(pm.h, 0, 4, 0, 0, None, C.byref(pm._acc), None, None) == 0
    assert pm.lib.scpqp_metrics_reset(pm.h, 0, None, None) == 0
    empty = LB.MetricsDense()
    assert pm.lib.scpqp_metrics_accumulate(pm.h, 1, 4, 0, 0, None, None, C.byref(empty), None) == -1
    pm.close()


def _rollout(sc, x_init, gpu, steps, metrics, seed):
    from scpqp.rollout import ClosedLoopBatch
    cl = ClosedLoopBatch(sc, x_init.shape[0], device=gpu, keep_path=True, metrics=metrics)
    cl.reset(x_init, seed=seed)
    cl.run(steps)
    return cl


def test_rollout_metrics_match_the_mirror_on_the_kept_paths(gpu):
    sigma = np.array([0.05, 0.05, 0.005, 0.02, 0.0, 0.002])
    sc = R.circle_scenario(4, Hp=10)
    rng = np.random.default_rng(23)
    x_init = np.array(sc.x0)[None] + rng.normal(0, 1, (4, 4, 6)) * sigma
    on = _rollout(sc, x_init, gpu, 3, True, 99)
    off = _rollout(sc, x_init, gpu, 3, False, 99)
    with pytest.raises(ValueError):
        off.metrics()
    for a, b in zip(on.history, off.history):
        for k in ("path", "U", "n_scp", "x0", "traj"):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(on.state, off.state)
    assert torch.equal(torch.nan_to_num(on.control), torch.nan_to_num(off.control))
    tps = sc.ticks_per_sim
    calls = [(h["path"].cpu().numpy(), i * tps, 0 if i == 0 else 1) for i, h in enumerate(on.history)]
    res = on.metrics()
    check_result(res, MM.run(MM.Constants.of_scenario(sc), calls, 4), "rollout")
    assert res["n_ticks_seen"].tolist() == [3 * tps + 1] * 4
    s = on.metrics_summary()
    assert s["n_realisations"] == 4 and s["min_gap_obs"] is None
    assert s["min_gap_veh"]["min"] == float(res["min_gap_veh"].min())
    on.reset(x_init, seed=99)
    cleared = on.metrics()
    assert torch.isinf(cleared["min_gap_veh"]).all() and (cleared["argmin_gap_veh"] == -1).all()
    assert (cleared["n_ticks_seen"] == 0).all() and (cleared["sum_sq_xtrack"] == 0).all()
    assert (cleared["first_collision_tick"] == -1).all()
    on.close()
    off.close()


def test_rollout_metrics_with_moving_obstacles(gpu):
    sc = R.frog_scenario(Hp=10)
    rng = np.random.default_rng(29)
    x_init = np.array(sc.x0)[None] + rng.normal(0, 1, (2, 1, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])
    cl = _rollout(sc, x_init, gpu, 2, True, None)
    tps = sc.ticks_per_sim
    calls = [(h["path"].cpu().numpy(), i * tps, 0 if i == 0 else 1) for i, h in enumerate(cl.history)]
    res = cl.metrics()
    check_result(res, MM.run(MM.Constants.of_scenario(sc), calls, 2), "frog")
    assert torch.isfinite(res["min_gap_obs"]).all() and torch.isinf(res["min_gap_veh"]).all()
    assert cl.metrics_summary()["min_gap_obs"]["min"] == float(res["min_gap_obs"].min())
    cl.close()
