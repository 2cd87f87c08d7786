"""The obstacle tracker with an acceleration state on the device
(include/scpqp_tracker_accel.h) against the CPU mirror (tests/tracker_accel_mirror.py): eight
tracker steps on manoeuvre snapshots with mixed lanes, the off and bad-row rules, the
independence of the lanes, recovery after trouble, the reduction to the five-state tracker,
the statistics of the innovations, and the rollout.  The inputs are those of
tests/tracker_accel_cases.py, which the CPU tests use too.

Shapes (B, n_obst, hp): (12, 22, 10): 264 (b, o) lanes, two workgroups of 256 with a ragged
tail; (2, 3, 5), no power of two; (1, 1, 1).

Tolerance of the device against the mirror, the one relative figure of
tests/test_gpu_tracker.py for the five outputs (``tracker_accel_cases.ratio``):
|dx_i| <= TOL max(1, |x_i|), |dP_ij| <= TOL sqrt(P_ii P_jj), |dnis| <= TOL max(1, nis),
|dz_i| <= TOL max(1, |z_i|), |d obst| <= TOL max(1, |obst|), and identical NaN patterns.  TOL
is not fitted to the device: it is derived on the CPU from the reference alone, on exactly
these inputs (tests/test_tracker_accel_host.py,
test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies).  The largest figure
between the mirror in float64 and the mirror in 80-bit is 5.86e-14, at (12, 22, 10), in a
covariance entry of the first correction ((2, 3, 5): 1.70e-14; (1, 1, 1): 6.1e-15): that is the
rounding this definition amplifies.  The device contracts multiply-adds and has its own
sincos, so TOL is 16 times it, rounded up to a power of two: 16 * 5.86e-14 = 9.4e-13 <= 2^-39 =
1.82e-12, the five-state test's figure.  The conditioning limits of that test are kept:
r_heading >= 0.01 rad, p0_yaw <= 0.4 rad/s, measured positions within 16 m.  Measured on an
MI355X: see MEASURED below.

The snapshots are ``manoeuvres.state`` on the device; the mirror is given the very same rows
(the device's, copied), after they have been checked against ``manoeuvre_mirror.state`` within
the manoeuvre tests' 2^-42.

The reduction compares the device with P0_ACCEL = Q_ACCEL = 0 and the holds beyond the horizon
against ``tracker.step`` on the same inputs, within RED_TOL + TOL: what the host test derived
for the two mirrors (16 times the measured 6.74e-14, rounded up: 2^-39) plus the device
tolerance.

Consistency: 1500 lanes, 12 innovations of 0.4 s, every lane one constant-acceleration piece;
the mean NIS lies within 4 +- 5 sqrt(8 / 18000) = 0.105 and the RMS position error 2.5 s ahead
is smaller than the five-state tracker's on the same measurements (only "smaller" is
asserted).  The frog rollout asserts only that the summed prediction error from step 3 on is
smaller than the five-state tracker's.  The figures are in MEASURED below and in DESIGN §7.
"""
import math
import types

import numpy as np
import pytest
import torch

import manoeuvre_mirror as MNM
import obstacle_mirror as OM
import sensing_mirror as SM
import tracker_accel_cases as TC
import tracker_accel_mirror as AM
from oracle import scp_reference as R
from scpqp import manoeuvres as MAN
from scpqp import obstacles as OB
from scpqp import sensing as SE
from scpqp import tracker as TRK
from scpqp import tracker_accel as TRKA

pytestmark = pytest.mark.gpu

TOL = TC.TOL                      # 2^-39, derived on the CPU (see above)
MAN_TOL = 2.0 ** -42              # tests/test_gpu_manoeuvres.py
LEAD, DT = TC.LEAD, TC.DT
SEED = TC.SEED
# Measured on an MI355X (the tests print the figures):
#   device against mirror  (12, 22, 10): 6.29e-14   (2, 3, 5): 3.34e-14   (1, 1, 1): 6.4e-15
#   reduction against tracker.step, (12, 22, 10): 1.30e-14
#   consistency: mean NIS 4.004; RMS error 2.5 s ahead 0.193 m, the five-state tracker 5.525 m
#   frog rollout, braking at 3 m/s^2: 329.56 m against 1514.80 m from step 3 on, ratio 0.218
MEASURED = {(12, 22, 10): 6.29e-14, (2, 3, 5): 3.34e-14, (1, 1, 1): 6.4e-15}


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64),
                                                   b.contiguous().view(torch.int64)))


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. device against mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,nO,hp", TC.SHAPES)
def test_eight_steps_match_the_mirror(gpu, B, nO, hp):
    rows, man, osense, trk = TC.case(B, nO)
    rows_d, man_d, os_d, trk_d = (_dev(a, gpu) for a in (rows, man, osense, trk))
    x_d, cov_d = TRKA.alloc(B, nO, gpu)
    x_m, cov_m = AM.alloc(B, nO)
    on = (trk != 0).any(axis=2)
    worst, seen_update = 0.0, False
    for s, (t, since) in enumerate(TC.times()):
        snap_d = MAN.state(rows_d, man_d, t)
        snap = _np(snap_d)
        want = MNM.state(rows, man, t)
        assert np.array_equal(np.isnan(snap), np.isnan(want))
        ok = ~np.isnan(want)
        assert (np.abs(snap - want)[ok] <= MAN_TOL * np.maximum(1.0, np.abs(want[ok]))).all()
        ob_d, z_d, nis_d = TRKA.step(snap_d, os_d, SEED, s, TC.B_OFFSET, trk_d, 0.0, since, LEAD,
                                     DT, hp, x_d, cov_d)
        ob_m, z_m, nis_m = AM.step(snap, osense, SEED, s, TC.B_OFFSET, trk, 0.0, since, LEAD, DT,
                                   hp, x_m, cov_m)
        # the off lanes: untouched state
        assert np.isnan(_np(x_d)[~on]).all() and (_np(cov_d)[~on] == 0).all()
        worst = max(worst, TC.ratio([(_np(x_d), x_m), (_np(z_d), z_m), (_np(ob_d), ob_m)],
                                    _np(cov_d), cov_m, _np(nis_d), nis_m))
        seen_update |= bool(np.isfinite(nis_m).any())
        c = _np(cov_d)
        assert np.array_equal(c, c.transpose(0, 1, 3, 2), equal_nan=True)
    print(f"({B}, {nO}, {hp}): largest device - mirror ratio {worst:.3e} (TOL {TOL:.3e})")
    assert seen_update
    if B * nO > 205:
        # one bad lane of each kind, NaN in all four outputs of its own lane
        for lane in TC.BAD_LANES:
            b, o = divmod(lane, nO)
            assert torch.isnan(x_d[b, o]).all() and torch.isnan(ob_d[b, o]).all()
    assert worst <= TOL


# ---------------------------------------------------------------------------
# 2. off rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sensed", [False, True])
def test_off_rows_give_the_untracked_prediction_and_leave_the_state(gpu, sensed):
    B, nO, hp = 12, 22, 10
    rows, man, osense, trk = TC.case(B, nO)
    snap = MNM.state(rows, man, 0.8)
    rng = np.random.default_rng(5)
    x0 = _dev(rng.standard_normal((B, nO, 6)), gpu)
    cov0 = _dev(rng.standard_normal((B, nO, 6, 6)), gpu)
    x, cov = x0.clone(), cov0.clone()
    rows_d = _dev(snap, gpu)
    os_d = _dev(osense, gpu) if sensed else None
    ob, z, nis = TRKA.step(rows_d, os_d, SEED, 4, 2, TRKA.off(B, nO, gpu), 0.0, TC.T_STEP, LEAD, DT,
                           hp, x, cov)
    want = SE.predict_sensed(rows_d, os_d, SEED, 4, 2, 0.0, LEAD, DT, hp) if sensed \
        else OB.predict(rows_d, 0.0, LEAD, DT, hp)
    assert _beq(ob, want)
    assert _beq(x, x0) and _beq(cov, cov0) and torch.isnan(nis).all()
    # the off lanes among lanes with a filter: the same block, the same untouched state
    x, cov = x0.clone(), cov0.clone()
    ob, z, nis = TRKA.step(rows_d, os_d, SEED, 4, 2, _dev(trk, gpu), 0.0, TC.T_STEP, LEAD, DT, hp,
                           x, cov)
    off = torch.as_tensor(~(trk != 0).any(axis=2), device=gpu)
    assert int(off.sum()) >= 30
    assert _beq(ob[off], want[off]) and _beq(x[off], x0[off]) and _beq(cov[off], cov0[off])
    assert torch.isnan(nis[off]).all()
    if sensed:
        # an all-zero osense array is the exact sensor: bitwise what NULL gives
        x1, cov1 = x0.clone(), cov0.clone()
        a = TRKA.step(rows_d, torch.zeros_like(os_d), SEED, 4, 2, _dev(trk, gpu), 0.0, TC.T_STEP,
                      LEAD, DT, hp, x1, cov1)
        x2, cov2 = x0.clone(), cov0.clone()
        b = TRKA.step(rows_d, None, 0, 0, 0, _dev(trk, gpu), 0.0, TC.T_STEP, LEAD, DT, hp, x2, cov2)
        assert all(_beq(p, q) for p, q in zip(a, b)) and _beq(x1, x2) and _beq(cov1, cov2)


# ---------------------------------------------------------------------------
# 3. split batch, lane independence, bad rows, recovery
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snapshots():
    rows, man, _, _ = TC.case(12, 22)
    return [MNM.state(rows, man, t) for t, _ in TC.times()[:3]]


def _run(snaps, osense, trk, gpu, hp=10, lo=0, hi=None, rows_edit=None):
    B, nO = trk[lo:hi].shape[:2]
    x, cov = TRKA.alloc(B, nO, gpu)
    os_d, trk_d = _dev(osense[lo:hi], gpu), _dev(trk[lo:hi], gpu)
    out = []
    for s, ((t, since), snap) in enumerate(zip(TC.times(), snaps)):
        snap = snap if rows_edit is None else rows_edit(snap.copy())
        ob, z, nis = TRKA.step(_dev(snap[lo:hi], gpu), os_d, SEED, s, lo, trk_d, 0.0, since, LEAD,
                               DT, hp, x, cov)
        out.append((x.clone(), cov.clone(), nis, ob, z))
    return out


def test_a_split_batch_gives_what_the_whole_gives(gpu, snapshots):
    _, _, osense, trk = TC.case(12, 22)
    whole = _run(snapshots, osense, trk, gpu)
    a, b = _run(snapshots, osense, trk, gpu, lo=0, hi=5), _run(snapshots, osense, trk, gpu, lo=5, hi=12)
    for s, w in enumerate(whole):
        for k in range(5):
            assert _beq(w[k], torch.cat([a[s][k], b[s][k]])), (s, k)


BAD_TRK = [(0, math.nan), (7, math.inf), (1, -1e-3), (13, -1e-300), (11, -1.0), (2, 0.0), (0, 0.0)]


def test_changing_the_last_row_changes_only_its_lane(gpu, snapshots):
    _, _, osense, trk = TC.case(12, 22)
    trk[-1, -1] = [0.05, 0.01, 0.1, 0.01, 0.005, 0.02, 0.02, 1.0, 0.5, 3.0, 1.0, 6.0, 2.0, 1.0]
    osense[-1, -1] = [0.05, 0.01, 0.1]
    base = _run(snapshots, osense, trk, gpu)
    other = trk.copy()
    other[-1, -1, 0] = 0.08
    got = _run(snapshots, osense, other, gpu)
    for s in range(len(base)):
        for k in range(5):
            w, g = base[s][k].flatten(0, 1), got[s][k].flatten(0, 1)
            assert _beq(w[:-1], g[:-1]), (s, k)
        assert _beq(base[s][4], got[s][4])                  # the measurement does not read trk
        if s:
            assert not _beq(base[s][0][-1, -1], got[s][0][-1, -1])

    def only_the_last_lane_is_nan(got, what, z_nan):
        for s in range(len(base)):
            for k in range(5):
                w, g = base[s][k].flatten(0, 1), got[s][k].flatten(0, 1)
                assert _beq(w[:-1], g[:-1]), (what, s, k)
                if k < 4 or z_nan:
                    assert torch.isnan(g[-1]).all(), (what, s, k)
                else:
                    assert _beq(w[-1], g[-1]), (what, s, k)

    # every kind of bad tracker row: NaN in its own lane, bitwise the same everywhere else,
    # and the measurement still delivered
    for f, val in BAD_TRK:
        bad = trk.copy()
        bad[-1, -1, f] = val
        assert AM.is_bad_row(bad[-1, -1])
        only_the_last_lane_is_nan(_run(snapshots, osense, bad, gpu), ("trk", f), False)
    # a bad obstacle row and a bad osense row: the same, and no measurement
    for f, val in ((OM.LENGTH, -1.0), (OM.X, math.nan), (OM.YAW_RATE, math.inf)):
        def edit(snap, f=f, val=val):
            snap[-1, -1, f] = val
            return snap
        only_the_last_lane_is_nan(_run(snapshots, osense, trk, gpu, rows_edit=edit), ("rows", f), True)
    for f, val in ((0, -0.1), (2, math.nan)):
        bad = osense.copy()
        bad[-1, -1, f] = val
        assert SM.bad_osense_row(bad[-1, -1])
        only_the_last_lane_is_nan(_run(snapshots, bad, trk, gpu), ("osense", f), True)


def test_a_lane_turned_nan_recovers_on_the_next_call(gpu):
    B, nO, hp = 2, 3, 5
    rows, man, osense, _ = TC.case(B, nO)
    snaps = [_dev(MNM.state(rows, man, t), gpu) for t in (0.0, 0.4, 0.8)]
    os_d = _dev(osense, gpu)
    trk = TRKA.rows(B, nO, device=gpu)
    x, cov = TRKA.alloc(B, nO, gpu)
    TRKA.step(snaps[0], os_d, SEED, 0, 0, trk, 0.0, 0.0, LEAD, DT, hp, x, cov)
    good = (x.clone(), cov.clone())
    cov[1, 2] = -torch.eye(6, dtype=torch.float64, device=gpu)       # no Cholesky of S
    x[0, 1, 3] = math.inf                                              # a non-finite prediction
    ob, z, nis = TRKA.step(snaps[1], os_d, SEED, 1, 0, trk, 0.0, 0.4, LEAD, DT, hp, x, cov)
    for b, o in ((1, 2), (0, 1)):
        assert torch.isnan(x[b, o]).all() and torch.isnan(cov[b, o]).all() and math.isnan(nis[b, o])
        assert torch.isnan(ob[b, o]).all() and torch.isfinite(z[b, o]).all()
    ref = (good[0].clone(), good[1].clone())
    ob_r, z_r, nis_r = TRKA.step(snaps[1], os_d, SEED, 1, 0, trk, 0.0, 0.4, LEAD, DT, hp, *ref)
    keep = torch.ones((B, nO), dtype=torch.bool, device=gpu)
    keep[1, 2] = keep[0, 1] = False
    assert _beq(x[keep], ref[0][keep]) and _beq(cov[keep], ref[1][keep])
    assert _beq(nis[keep], nis_r[keep]) and _beq(ob[keep], ob_r[keep]) and _beq(z, z_r)
    # the next call initialises the lanes again
    ob, z, nis = TRKA.step(snaps[2], os_d, SEED, 2, 0, trk, 0.0, 0.4, LEAD, DT, hp, x, cov)
    r = np.append(AM.r_diag(_np(trk[0, 0])), [TRKA.P0_YAW ** 2, TRKA.P0_ACCEL ** 2])
    for b, o in ((1, 2), (0, 1)):
        assert _beq(x[b, o, :4], z[b, o]) and (x[b, o, 4:] == 0).all() and math.isnan(nis[b, o])
        assert (_np(cov[b, o]) == np.diag(r)).all()
        assert torch.isfinite(ob[b, o]).all()
    assert torch.isfinite(nis[keep]).all()


# ---------------------------------------------------------------------------
# 4. the reduction to the five-state tracker, on the device
# ---------------------------------------------------------------------------
def test_without_an_acceleration_the_device_is_the_five_state_tracker(gpu):
    B, nO, hp = 12, 22, 10
    rows, osense, trk5, trk6 = TC.reduction_case(B, nO)
    rows_d, os_d, t5, t6 = (_dev(a, gpu) for a in (rows, osense, trk5, trk6))
    x6, c6 = TRKA.alloc(B, nO, gpu)
    x5, c5 = TRK.alloc(B, nO, gpu)
    worst = 0.0
    for s, (t, since) in enumerate(TC.reduction_times()):
        o6, z6, n6 = TRKA.step(rows_d, os_d, SEED, s, 3, t6, t, since, LEAD, DT, hp, x6, c6)
        o5, z5, n5 = TRK.step(rows_d, os_d, SEED, s, 3, t5, t, since, LEAD, DT, hp, x5, c5)
        assert _beq(z6, z5)                                  # the same measurement, bitwise
        a = x6[..., 5]
        assert (a[~torch.isnan(a)] == 0).all()
        worst = max(worst, TC.reduction_ratio(_np(x6), _np(c6), _np(n6), _np(o6), _np(x5), _np(c5),
                                              _np(n5), _np(o5)))
    print(f"device with P0_ACCEL = Q_ACCEL = 0 against tracker.step: {worst:.3e} "
          f"(RED_TOL + TOL {TC.RED_TOL + TOL:.3e})")
    assert worst <= TC.RED_TOL + TOL


# ---------------------------------------------------------------------------
# 5. statistics: the CPU consistency inputs on the device
# ---------------------------------------------------------------------------
def test_innovations_are_consistent_and_the_prediction_beats_the_five_state_tracker(gpu):
    rows, man, osense, trk, trk5 = TC.consistency_inputs()
    assert TC.no_lane_stops(rows, man)
    B, nO = rows.shape[:2]
    rows_d, man_d, os_d, trk_d, trk5_d = (_dev(a, gpu) for a in (rows, man, osense, trk, trk5))
    x, cov = TRKA.alloc(B, nO, gpu)
    x5, cov5 = TRK.alloc(B, nO, gpu)
    every = []
    for s in range(TC.CONS_STEPS + 1):
        snap = MAN.state(rows_d, man_d, s * TC.CONS_T)
        since = 0.0 if s == 0 else TC.CONS_T
        ob, z, nis = TRKA.step(snap, os_d, TC.CONS_SEED, s, 0, trk_d, 0.0, since, TC.CONS_LEAD,
                               TC.CONS_DT, TC.CONS_HP, x, cov)
        ob5, z5, _ = TRK.step(snap, os_d, TC.CONS_SEED, s, 0, trk5_d, 0.0, since, TC.CONS_LEAD,
                              TC.CONS_DT, TC.CONS_HP, x5, cov5)
        assert _beq(z, z5)                                   # the same measurements
        if s:
            every.append(_np(nis))
    every = np.array(every)
    assert np.isfinite(every).all() and every.size == 18000
    mean, bound, rms, rms5 = TC.consistency_verdict(every, _np(ob), _np(ob5), rows, man)
    print(f"mean NIS {mean:.3f} (|mean - 4| <= {bound:.3f}); RMS position error "
          f"{TC.CONS_AHEAD:.1f} s ahead {rms:.4f} m, of the five-state tracker {rms5:.4f} m")
    assert abs(mean - 4.0) <= bound
    assert rms < rms5


# ---------------------------------------------------------------------------
# 6. rollout: frog, 1 vehicle, 22 obstacles braking at 3 m/s^2, Hp 10, B = 4, 6 steps, an
#    exact sensor
# ---------------------------------------------------------------------------
STEPS = TC.FROG_STEPS
KEYS = ("x0", "u0", "umax", "U", "traj", "n_scp", "status", "path", "u_tick", "obst", "obst_state")
TRK_KEYS = ("obst_est", "obst_nis", "obst_meas")


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl):
    return types.SimpleNamespace(
        hist=[{k: h[k].clone() for k in KEYS + TRK_KEYS if k in h} for h in cl.history],
        metrics=cl.metrics(), control=cl.control.clone())


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.frog_scenario(Hp=10)
    B, nO = 4, sc.nObst
    x_init = _x_init(sc, B)
    rows, brake = TC.frog_inputs(sc, B)
    exact = np.zeros((B, nO, 3))
    trka = TRKA.matched(exact, device="cpu").numpy()
    trk5 = TRK.matched(exact, device="cpu").numpy()
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, kw in (("plain", {}), ("none", dict(tracker_accel=None)),
                     ("off", dict(tracker_accel=np.zeros((B, nO, 14)))),
                     ("off_dev", dict(tracker_accel=TRKA.off(B, nO, gpu))),
                     ("trk5", dict(tracker=trk5)), ("trka", dict(tracker_accel=_dev(trka, gpu)))):
        cl.reset(x_init, seed=1, obstacles=rows, manoeuvres=brake, **kw)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, obstacles=rows[o:o + 2],
                   manoeuvres=brake[o:o + 2], tracker_accel=trka[o:o + 2])
        half.run(STEPS)
        runs[f"half{o}"] = _snapshot(half)
    half.close()
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, rows=rows, brake=brake,
                                trka=trka, trk5=trk5, runs=runs)
    cl.close()


@pytest.mark.parametrize("same", ["none", "off", "off_dev"])
def test_rollout_without_the_tracker_is_the_rollout_of_before(rollouts, same):
    a, b = rollouts.runs["plain"], rollouts.runs[same]
    assert len(a.hist) == len(b.hist) == STEPS
    for i in range(STEPS):
        assert a.hist[i].keys() == b.hist[i].keys()
        assert not any(k in b.hist[i] for k in TRK_KEYS) and "obst_state" in b.hist[i]
        for k in a.hist[i]:
            if a.hist[i][k].dtype == torch.float64:
                assert _beq(a.hist[i][k], b.hist[i][k]), (i, k)
            else:
                assert _eq(a.hist[i][k], b.hist[i][k]), (i, k)
    assert _beq(a.control, b.control)
    for k, v in a.metrics.items():
        assert _eq(v, b.metrics[k]), k


def test_rollout_records_what_step_gives(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    rows, man, trk = _dev(ro.rows, gpu), _dev(ro.brake, gpu), _dev(ro.trka, gpu)
    x, cov = TRKA.alloc(ro.B, sc.nObst, gpu)
    lead = sc.delay_x + sc.dt + sc.delay_u
    g0 = 0
    for i, rec in enumerate(ro.runs["trka"].hist):
        g1 = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
        snap = MAN.state(rows, man, g1 * sc.tick_length)
        ob, z, nis = TRKA.step(snap, None, 0, i, 0, trk, 0.0, (g1 - g0) * sc.tick_length, lead,
                               sc.dt, sc.Hp, x, cov)
        g0 = g1
        assert _beq(rec["obst_state"], snap), i
        assert _beq(rec["obst"], ob) and _beq(rec["obst_est"], x), i
        assert _beq(rec["obst_nis"], nis) and _beq(rec["obst_meas"], z), i
        assert tuple(rec["obst_est"].shape) == (ro.B, sc.nObst, 6)
        # the exact sensor: the measurement is the snapshot
        assert _beq(z[..., :3], snap[..., :3]) and _beq(z[..., 3], snap[..., OM.SPEED])
    last = ro.runs["trka"].hist[-1]
    assert torch.isfinite(last["obst_nis"]).all()
    assert (last["obst_est"][..., 5] < -1.0).any()           # a braking has been learnt
    assert not _beq(last["obst"], ro.runs["trk5"].hist[-1]["obst"])


def test_rollout_with_the_tracker_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["trka"].hist):
        for k in KEYS + TRK_KEYS:
            parts = torch.cat([ro.runs["half0"].hist[i][k], ro.runs["half2"].hist[i][k]])
            if whole[k].dtype == torch.float64:
                assert _beq(whole[k], parts), (i, k)
            else:
                assert _eq(whole[k], parts), (i, k)
    for k, v in ro.runs["trka"].metrics.items():
        assert _eq(v, torch.cat([ro.runs["half0"].metrics[k], ro.runs["half2"].metrics[k]])), k


def test_reset_refuses_both_trackers_and_bad_rows_before_anything_is_launched(rollouts, gpu):
    ro, cl = rollouts, rollouts.cl
    cl.reset(ro.x_init, seed=1, obstacles=ro.rows, manoeuvres=ro.brake, tracker_accel=ro.trka)
    cl.run(1)
    n_hist, i = len(cl.history), cl.i
    state, rows_before = cl.state.clone(), cl.trka_rows.clone()
    x_before, cov_before = cl.trk_x.clone(), cl.trk_cov.clone()
    good = ro.trka
    neg, zero_r, nan = good.copy(), good.copy(), good.copy()
    neg[2, 1, 7] = -0.1
    zero_r[1, 0, 1] = 0.0
    nan[0, 0, 12] = math.nan
    with pytest.raises(ValueError, match="either tracker= or tracker_accel=, not both"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker=ro.trk5, tracker_accel=good)
    for bad in (good[:2], good[:, :1], good[..., :9], neg, torch.as_tensor(neg), zero_r, nan):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker_accel=bad)
    with pytest.raises(ValueError, match=r"rows\[2, 1\]: q_accel must be >= 0"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker_accel=neg)
    with pytest.raises(ValueError, match=r"rows\[1, 0\]: r_heading must be > 0"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker_accel=zero_r)
    with pytest.raises(ValueError, match=r"tracker_accel needs obstacles= rows"):
        cl.reset(ro.x_init, seed=1, tracker_accel=good)
    assert len(cl.history) == n_hist and cl.i == i           # the refused resets changed nothing
    assert _eq(cl.state, state) and _eq(cl.trka_rows, rows_before) and cl.trk_rows is None
    assert _beq(cl.trk_x, x_before) and _beq(cl.trk_cov, cov_before)


def test_against_braking_obstacles_the_prediction_beats_the_five_state_trackers(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    rows, man = _dev(ro.rows, gpu), _dev(ro.brake, gpu)
    tps, tdx, tdu, Hp = sc.ticks_per_sim, sc.ticks_delay_x, sc.ticks_delay_u, sc.Hp
    ahead = [(k + 1) * tps + tdx + tps + tdu for k in range(Hp)]       # tau_k in ticks
    err = {}
    for name in ("trk5", "trka"):
        total = 0.0
        for i in range(3, STEPS):
            g1 = max(0, i * tps - tdx)
            true = MAN.pose(rows, man, sc.tick_length, g1, ahead[-1])[:, :, ahead, 0:2]
            d = ro.runs[name].hist[i]["obst"].transpose(2, 3) - true   # [B, nO, Hp, 2]
            total += float(d.norm(dim=-1).sum().item())
        err[name] = total
    print(f"summed prediction error from step 3 on: {err['trka']:.4f} m with the acceleration "
          f"state, {err['trk5']:.4f} m without, ratio {err['trka'] / err['trk5']:.3e}")
    assert err["trka"] < err["trk5"]
