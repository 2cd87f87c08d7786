"""The obstacle truth on the device (include/scpqp_obstacles.h): the controller's prediction
and the pose against the oracle and the CPU mirror (tests/obstacle_mirror.py), the bad-row
rule, the sampler against the mirror, and the rollout.

Shapes (B, n_obst, hp) are the smallest at which lane indexing, the workgroup boundary and
the tail guard can go wrong: (2, 3, 4), no power of two; (5, 22, 10), frog's obstacle count:
1100 lanes, five workgroups of 256 with a ragged tail; (1, 1, 1).

Bound: 1e-12 m.  The coordinates stay below 100 m, where one rounding is 1.4e-14 m; the
bound leaves about a hundred of them for sincos and the contraction of a * b + c.  Measured
on an MI355X: the largest |device - oracle| of the nominal prediction is 7.1e-15 m for frog
and 0 for parallel5 (measurement ticks 0, 40 and 1999); the largest |device - mirror| of the
prediction and of the pose of turning rows is 7.1e-15 m over the three shapes; nominal rows
against the rollout's host prediction at step 0 differ by 7.1e-15 m, and
obstaclePathFullRes of a turning realisation from the mirror by 1.4e-14 m.
"""
import math
import types

import numpy as np
import pytest
import torch

import metrics_mirror as MM
import obstacle_mirror as OM
from oracle import plant_reference as PR
from oracle import scp_reference as R
from scpqp import obstacles as OB

pytestmark = pytest.mark.gpu

BOUND = 1e-12
SHAPES = [(2, 3, 4), (5, 22, 10), (1, 1, 1)]          # (B, n_obst, hp)
T_MEAS, LEAD, DT, TICK = 1.6, 0.43, 0.4, 0.01


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _rows(B, nO, seed=5):
    """Turning rows with their own footprints inside +-60 m: headings over the circle, speeds
    0..3 m/s, turn rates +-0.5 rad/s, one in eight below the sinc switch at t = 1.6 s, one in
    eight exactly straight."""
    rng = np.random.default_rng(seed)
    r = np.zeros((B, nO, 7))
    r[..., 0:2] = rng.uniform(-60, 60, (B, nO, 2))
    r[..., 2] = rng.uniform(-math.pi, math.pi, (B, nO))
    r[..., 3] = rng.uniform(0.0, 3.0, (B, nO))
    r[..., 4] = rng.uniform(0.5, 4.0, (B, nO))
    r[..., 5] = rng.uniform(0.5, 2.0, (B, nO))
    r[..., 6] = rng.uniform(-0.5, 0.5, (B, nO))
    n = np.arange(B * nO).reshape(B, nO)
    r[..., 6] = np.where(n % 8 == 3, 1e-5, np.where(n % 8 == 6, 0.0, r[..., 6]))
    return r


def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu)


# ---------------------------------------------------------------------------
# 1. nominal rows: the oracle's prediction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["frog", "parallel5"])
def test_nominal_prediction_matches_the_oracle(gpu, name):
    sc = R.frog_scenario(Hp=10) if name == "frog" else R.parallel_scenario(5, Hp=10)
    B = 2
    rows = OB.nominal(sc, B, device=gpu)
    lead = sc.delay_x + sc.dt + sc.delay_u
    worst = 0.0
    for tick in (0, 40, 1999):
        got = OB.predict(rows, tick * sc.tick_length, lead, sc.dt, sc.Hp).cpu().numpy()
        want = PR.obstacle_prediction(sc, tick)
        assert got.shape == (B, sc.nObst, 2, sc.Hp)
        assert np.abs(want).max() < 128.0               # one rounding there: 1.4e-14 m
        worst = max(worst, float(np.abs(got - want[None]).max()))
    print(f"{name}: max |device - oracle| of the nominal prediction = {worst:.3e} m")
    assert worst <= BOUND


# ---------------------------------------------------------------------------
# 2. turning rows: the mirror; the rows are per lane
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B, nO, hp", SHAPES)
def test_turning_rows_match_the_mirror(gpu, B, nO, hp):
    rows = _rows(B, nO)
    if B * nO >= 8:
        assert (rows[..., 6] == 0.0).any() and (np.abs(0.5 * rows[..., 6] * T_MEAS) < 1e-4).any()
    d = _dev(rows, gpu)
    pred = OB.predict(d, T_MEAS, LEAD, DT, hp)
    pose = OB.pose(d, TICK, 157, hp)                      # hp + 1 ticks from tick 157
    assert tuple(pred.shape) == (B, nO, 2, hp) and tuple(pose.shape) == (B, nO, hp + 1, 3)
    want_pred, want_pose = OM.predict(rows, T_MEAS, LEAD, DT, hp), OM.poses(rows, TICK, 157, hp)
    assert np.abs(want_pred).max() < 100.0 and np.abs(want_pose).max() < 100.0
    e1 = float(np.abs(pred.cpu().numpy() - want_pred).max())
    e2 = float(np.abs(pose.cpu().numpy() - want_pose).max())
    print(f"({B}, {nO}, {hp}): max |device - mirror| predict {e1:.3e} m, pose {e2:.3e}")
    assert e1 <= BOUND and e2 <= BOUND
    # the heading is one multiply-add
    assert np.abs(pose.cpu().numpy()[..., 2] - want_pose[..., 2]).max() <= 2.0 ** -49
    # the turn rate is read: the turning rows leave the straight line
    straight = rows.copy()
    straight[..., 6] = 0.0
    moved = np.abs(OM.poses(straight, TICK, 157, hp) - want_pose)[..., 0:2].max()
    assert moved > 1e-3 or B * nO == 1
    # permuting realisations permutes the outputs, bitwise
    perm = np.roll(np.arange(B), 1)
    dp = _dev(rows[perm], gpu)
    assert _eq(OB.predict(dp, T_MEAS, LEAD, DT, hp), pred[torch.as_tensor(perm, device=gpu)])
    assert _eq(OB.pose(dp, TICK, 157, hp), pose[torch.as_tensor(perm, device=gpu)])
    # changing one row (the last: the tail of the last workgroup) changes only its block
    other = rows.copy()
    other[B - 1, nO - 1] = [1.0, 2.0, 0.3, 1.5, 2.0, 1.0, -0.2]
    p2, q2 = OB.predict(_dev(other, gpu), T_MEAS, LEAD, DT, hp), OB.pose(_dev(other, gpu), TICK, 157, hp)
    keep = torch.ones((B, nO), dtype=torch.bool, device=gpu)
    keep[B - 1, nO - 1] = False
    assert _eq(p2[keep], pred[keep]) and _eq(q2[keep], pose[keep])
    assert not _eq(p2[~keep], pred[~keep]) and not _eq(q2[~keep], pose[~keep])


# ---------------------------------------------------------------------------
# 3. bad rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("field, value", [(3, math.nan), (5, -1.0), (6, math.inf)])
def test_a_bad_row_is_nan_and_alone(gpu, field, value):
    B, nO, hp = SHAPES[1]
    rows = _rows(B, nO)
    base_pred = OB.predict(_dev(rows, gpu), T_MEAS, LEAD, DT, hp)
    base_pose = OB.pose(_dev(rows, gpu), TICK, 0, hp)
    assert not torch.isnan(base_pred).any() and not torch.isnan(base_pose).any()
    b, o = B - 1, nO - 2                                  # lanes 1080..1089: the last workgroup's tail
    rows[b, o, field] = value
    assert OM.bad_row(rows[b, o])
    pred = OB.predict(_dev(rows, gpu), T_MEAS, LEAD, DT, hp)    # returns 0: no exception
    pose = OB.pose(_dev(rows, gpu), TICK, 0, hp)
    ok = torch.ones((B, nO), dtype=torch.bool, device=gpu)
    ok[b, o] = False
    assert torch.isnan(pred[b, o]).all() and torch.isnan(pose[b, o]).all()
    assert _eq(pred[ok], base_pred[ok]) and _eq(pose[ok], base_pose[ok])
    assert np.isnan(OM.predict(rows, T_MEAS, LEAD, DT, hp)[b, o]).all()


def test_zero_footprint_and_zero_batch_are_not_bad(gpu):
    rows = _rows(2, 3)
    rows[1, 2, 4:6] = 0.0
    assert not torch.isnan(OB.predict(_dev(rows, gpu), T_MEAS, LEAD, DT, 4)).any()
    empty = torch.empty((0, 3, 7), dtype=torch.float64, device=gpu)
    assert tuple(OB.predict(empty, T_MEAS, LEAD, DT, 4).shape) == (0, 3, 2, 4)
    assert tuple(OB.pose(empty, TICK, 0, 4).shape) == (0, 3, 5, 3)


# ---------------------------------------------------------------------------
# 4. the sampler against the mirror; fill_nominal
# ---------------------------------------------------------------------------
def _dists(sc, seed, b_offset=0):
    d = OB.ObstacleDist(sc, seed, b_offset)
    d.uniform("yaw_rate", 0.3).uniform("x", 0.5, 6.8, 14.3).normal("speed", 0.5, 1.5, 2.6)
    d.normal("length", 1.0, 3.0, 5.5).fixed("width", 1.5)
    m = OM.Dist(d.mean, seed, b_offset)
    m.set(OM.YAW_RATE, OM.UNIFORM, 0.3).set(OM.X, OM.UNIFORM, 0.5, 6.8, 14.3)
    m.set(OM.SPEED, OM.NORMAL, 0.5, 1.5, 2.6).set(OM.LENGTH, OM.NORMAL, 1.0, 3.0, 5.5)
    return d, m


def test_sampler_matches_the_mirror(gpu):
    """FIXED and UNIFORM fields bitwise (the uniform is exact and mean + spread * xi is two
    roundings on both sides); NORMAL fields within the tolerance of a normal draw of
    tests/test_gpu_noise.py::test_raw_draws_match_the_mirror (64 * 2^-52 * 10) times spread."""
    sc = R.frog_scenario(Hp=10)
    seed, b_off, B = 0x123456789ABCDEF, 1000, 16
    d, m = _dists(sc, seed, b_off)
    got = d.sample(B, device=gpu).cpu().numpy()
    want = OM.sample(m, B)
    assert got.shape == want.shape == (B, 22, 7)
    for f in (OM.X, OM.Y, OM.HEADING, OM.WIDTH, OM.YAW_RATE):
        assert np.array_equal(got[..., f], want[..., f]), f
    assert np.all(got[..., OM.WIDTH] == 1.5)
    assert np.array_equal(got[..., OM.Y], np.broadcast_to(OM.nominal_rows(sc)[None, :, OM.Y], (B, 22)))
    atol = 64 * 2.0 ** -52 * 10
    for f, spread in ((OM.SPEED, 0.5), (OM.LENGTH, 1.0)):
        err = np.abs(got[..., f] - want[..., f]).max()
        print(f"field {f}: max |device - mirror| = {err:.3e} (atol {atol * spread:.3e})")
        assert err <= atol * spread
    # clamps are honoured, and reached
    assert got[..., OM.X].min() == 6.8 and got[..., OM.X].max() == 14.3
    assert got[..., OM.SPEED].min() == 1.5 and got[..., OM.SPEED].max() == 2.6
    assert got[..., OM.LENGTH].min() == 3.0 and got[..., OM.LENGTH].max() == 5.5
    assert np.all(np.abs(got[..., OM.YAW_RATE]) <= 0.3) and np.ptp(got[..., OM.YAW_RATE]) > 0.5
    OB.validate(got)


def test_sampler_does_not_depend_on_the_sharding(gpu):
    sc = R.frog_scenario(Hp=10)
    d, _ = _dists(sc, 99)
    whole = d.sample(6, device=gpu)
    parts = [d.with_offset(o).sample(3, device=gpu) for o in (0, 3)]
    assert _eq(whole, torch.cat(parts))
    assert not _eq(parts[0], parts[1])
    assert not _eq(whole, _dists(sc, 100)[0].sample(6, device=gpu))


def test_fill_nominal_equals_the_host_rows(gpu):
    for sc, B in ((R.frog_scenario(Hp=10), 13), (R.parallel_scenario(5, Hp=10), 1)):
        got = OB.nominal(sc, B, device=gpu).cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(OB.nominal_rows(sc)[None], (B, sc.nObst, 7)))
    with pytest.raises(ValueError, match="obstacles"):
        OB.nominal(R.circle_scenario(2), 2, device=gpu)


# ---------------------------------------------------------------------------
# 5. rollout: frog, Hp 10, B = 4, 3 steps, noise seed 1
# ---------------------------------------------------------------------------
STEPS = 3
KEYS = ("x0", "u0", "umax", "U", "traj", "n_scp", "status", "path", "u_tick", "obst")
YAW = 0.25


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl):
    return types.SimpleNamespace(hist=[{k: h[k].clone() for k in KEYS if k in h} for h in cl.history],
                                 metrics=cl.metrics())


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.frog_scenario(Hp=10)
    B = 4
    x_init = _x_init(sc, B)
    nominal = np.broadcast_to(OB.nominal_rows(sc)[None], (B, 22, 7)).copy()
    turning = nominal.copy()
    turning[2:, :, 6] = YAW * np.where(np.arange(22) % 2, 1.0, -1.0)   # only the turn rate differs
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, rows in (("nominal", nominal), ("turning", turning)):
        cl.reset(x_init, seed=1, obstacles=rows)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
    plot = cl.result_for_plot(3)
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, obstacles=turning[o:o + 2])
        half.run(STEPS)
        runs[f"half{o}"] = _snapshot(half)
    half.close()
    plain = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True, trace=True)
    plain.reset(x_init, seed=1)
    plain.run(STEPS)
    runs["none"] = _snapshot(plain)
    plain.close()
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, runs=runs, nominal=nominal,
                                turning=turning, plot=plot)
    cl.close()


def test_rollout_records_what_predict_gives(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    lead = sc.delay_x + sc.dt + sc.delay_u
    for name, rows in (("nominal", ro.nominal), ("turning", ro.turning)):
        for i, rec in enumerate(ro.runs[name].hist):
            tick_meas = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
            again = OB.predict(_dev(rows, gpu), tick_meas * sc.tick_length, lead, sc.dt, sc.Hp)
            assert _eq(rec["obst"], again), (name, i)
    d = (ro.runs["nominal"].hist[0]["obst"] - ro.runs["none"].hist[0]["obst"]).abs().max().item()
    print(f"step 0: nominal rows against the host prediction: {d:.3e} m")
    assert d <= BOUND
    # the turning obstacles are predicted from where they really are
    a, b = ro.runs["nominal"].hist[2]["obst"], ro.runs["turning"].hist[2]["obst"]
    assert _eq(a[:2], b[:2]) and (a[2:] - b[2:]).abs().max().item() > 1e-3


def test_rollout_controller_does_not_know_the_turn_rate(rollouts):
    ro = rollouts
    a, b = ro.runs["nominal"].hist[0], ro.runs["turning"].hist[0]
    for k in ("x0", "U", "traj"):
        assert _eq(a[k], b[k]), k                          # step 0: every obstacle at its start
    ma, mb = ro.runs["nominal"].metrics, ro.runs["turning"].metrics
    for k in ma:
        assert _eq(ma[k][:2], mb[k][:2]), k                # the nominal realisations: untouched
    moved = (ma["min_gap_obs"][2:] - mb["min_gap_obs"][2:]).abs().max().item()
    print(f"the turn rate moves the smallest obstacle gap by {moved:.3e} m over {STEPS} steps")
    assert moved > 1e-6


def test_rollout_metrics_are_the_metrics_of_the_kept_paths(rollouts, gpu):
    from scpqp.metrics import PathMetrics
    ro, sc = rollouts, rollouts.sc
    pm = PathMetrics(sc, ro.B, gpu)
    for name, rows in (("nominal", ro.nominal), ("turning", ro.turning)):
        pm.reset(ro.B)
        for i, rec in enumerate(ro.runs[name].hist):
            pm.accumulate(rec["path"], tick0=i * sc.ticks_per_sim, k_first=0 if i == 0 else 1,
                          obstacles=_dev(rows, gpu))
        res = pm.result()
        for k, v in ro.runs[name].metrics.items():
            assert _eq(v, res[k]), (name, k)
        assert res["n_ticks_seen"].tolist() == [STEPS * sc.ticks_per_sim + 1] * ro.B
    # nominal rows measure what the constant obstacles measure on the same paths
    pm.reset(ro.B)
    for i, rec in enumerate(ro.runs["nominal"].hist):
        pm.accumulate(rec["path"], tick0=i * sc.ticks_per_sim, k_first=0 if i == 0 else 1)
    for k, v in pm.result().items():
        assert _eq(v, ro.runs["nominal"].metrics[k]), k
    pm.close()


def test_rollout_with_rows_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["turning"].hist):
        for k in KEYS:
            parts = torch.cat([ro.runs["half0"].hist[i][k], ro.runs["half2"].hist[i][k]])
            assert _eq(whole[k], parts), (i, k)
    for k, v in ro.runs["turning"].metrics.items():
        assert _eq(v, torch.cat([ro.runs["half0"].metrics[k], ro.runs["half2"].metrics[k]])), k


def test_reset_refuses_bad_rows_before_anything_is_launched(rollouts, gpu):
    from scpqp.rollout import ClosedLoopBatch
    ro, cl = rollouts, rollouts.cl
    n_hist, i = len(cl.history), cl.i
    state, rows_before = cl.state.clone(), cl.obst_rows.clone()
    nan, neg = ro.turning.copy(), ro.turning.copy()
    nan[1, 4, 3] = math.nan
    neg[3, 21, 5] = -0.5
    for rows in (ro.turning[:2], ro.turning[:, :21], ro.turning[..., :6], nan, neg,
                 torch.as_tensor(neg)):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, obstacles=rows)
    with pytest.raises(ValueError, match=r"rows\[3, 21\]: width"):
        cl.reset(ro.x_init, seed=1, obstacles=neg)
    assert len(cl.history) == n_hist and cl.i == i       # the refused resets changed nothing
    assert _eq(cl.state, state) and _eq(cl.obst_rows, rows_before)
    sc = R.circle_scenario(2, Hp=10)
    free = ClosedLoopBatch(sc, 2, device=gpu)
    x0 = _x_init(sc, 2)
    free.reset(x0)
    free.run(1)
    with pytest.raises(ValueError, match="no obstacles"):
        free.reset(x0, obstacles=np.zeros((2, 0, 7)))
    with pytest.raises(ValueError, match="no obstacles"):
        free.reset(x0, obstacles=ro.turning[:2])
    assert len(free.history) == 1 and free.i == 1
    free.close()


def test_result_for_plot_draws_the_turning_obstacles(rollouts):
    ro, sc = rollouts, rollouts.sc
    T = sc.ticks_total
    got = ro.plot["obstaclePathFullRes"]
    want = OM.poses(ro.turning[3:4], sc.tick_length, 0, T)[0]           # [22, T + 1, 3]
    assert got.shape == (22, 2, T + 1) and np.abs(want[..., 0:2]).max() < 100.0
    err = float(np.abs(got - want[..., 0:2].transpose(0, 2, 1)).max())
    print(f"obstaclePathFullRes of a turning realisation: max |device - mirror| = {err:.3e} m")
    assert err <= BOUND
    straight = MM.Constants.of_scenario(sc)
    off = max(abs(got[o, 0, T] - straight.obstacle_rect(o, T)[0]) for o in range(22))
    assert off > 1.0                                      # 20 s at 0.25 rad/s: far off the line
