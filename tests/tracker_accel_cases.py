"""The inputs of the tests of the tracker with an acceleration state, shared by the CPU tests
(tests/test_tracker_accel_host.py: the tolerance is derived there, from the mirror alone) and
the GPU tests (tests/test_gpu_tracker_accel.py), so that both see exactly the same numbers.
numpy only, but for ``frog_inputs``."""
import math

import numpy as np

import manoeuvre_mirror as MNM
import obstacle_mirror as OM
import tracker_accel_mirror as AM
import tracker_mirror as TM

SHAPES = [(12, 22, 10), (2, 3, 5), (1, 1, 1)]          # (B, n_obst, hp)
T_STEP, LEAD, DT = 0.4, 0.13, 0.4
N_STEPS = 8
SEED = 77
B_OFFSET = 3

# turn rates of the rows: theta = w T_STEP on both sides of the sinc switch (|theta / 2| =
# 1e-4), of the g' switch (|theta / 2| = 0.02), of the p, r switch (0.1) and of the p', r'
# switch (0.3); w = 0 exactly; large ones of both signs
W_LIST = [0.0, 1e-9, 1.8e-4 / T_STEP, 2.2e-4 / T_STEP, 0.038 / T_STEP, 0.042 / T_STEP,
          0.095 / T_STEP, 0.105 / T_STEP, 0.29 / T_STEP, 0.31 / T_STEP, -1.2, 2.0,
          -0.305 / T_STEP]


def templates():
    """Schedules (dur, accel, dyaw) of the lanes that are not off."""
    return [
        # brakes to a stop inside a step, stands, starts again at t = 1.6
        [(0.3, 0.0, 0.0), (1.3, -3.0, 0.1), (1.5, 2.0, 0.2), (0.0, 0.0, 0.0)],
        # brakes gently for the whole run: the predicted stop lies inside the horizon
        [(6.0, -0.6, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)],
        # a lane change, coasting first
        [(0.5, 0.0, 0.0), (0.8, 0.0, 0.5), (0.8, 0.0, -0.5), (0.0, 0.0, 0.0)],
        # no manoeuvre: a = 0, the row's own turn rate
        [(0.0, 0.0, 0.0)] * 4,
        # accelerates in a turn, then brakes in the other
        [(1.0, 1.5, 0.3), (1.0, -1.0, -0.3), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)],
        # a != 0 at the row's turn rate
        [(0.75, 1.5, 0.0), (1.25, -0.5, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)],
    ]


# (lane g of the (12, 22) shape, what is bad there)
BAD_LANES = {200: "trk_nan", 201: "trk_negative", 202: "trk_r_zero", 204: "row", 205: "osense"}


def case(B, nO, seed=11):
    """Obstacle rows, schedules, osense rows and tracker rows.  Lane g: every seventh is off;
    g % 5 == 1 has Q = 0; g % 4 == 2 has W_CLAMP = 0, g % 9 == 4 A_CLAMP = 0; g % 6 == 1 has
    W_HOLD = 0, g % 6 == 4 A_HOLD = 0, the other holds lie inside the horizon or beyond it;
    g % 11 == 5 has P0_YAW = 0, g % 13 == 6 P0_ACCEL = 0 (with Q = 0 the turn rate or the
    acceleration then stays exactly 0); every third lane has an exact sensor; the (12, 22)
    shape has one bad lane of each kind (BAD_LANES).  Magnitudes as in
    tests/test_gpu_tracker.py: r_heading >= 0.01, p0_yaw <= 0.4, measured positions within
    16 m (asserted by the host test on the mirror)."""
    rng = np.random.default_rng(seed + 100 * B + nO)
    g = np.arange(B * nO).reshape(B, nO)
    rows = np.zeros((B, nO, 7))
    rows[..., OM.X], rows[..., OM.Y] = (g % 22) * 0.5 - 5.5, 4.0 - (g // 22) * 0.7
    rows[..., OM.HEADING] = rng.uniform(-1.5, 1.5, (B, nO))
    rows[..., OM.SPEED] = rng.uniform(0.5, 2.5, (B, nO))
    rows[..., OM.LENGTH], rows[..., OM.WIDTH] = 4.0, 2.0
    rows[..., OM.YAW_RATE] = np.array(W_LIST)[g % len(W_LIST)]
    tpl = np.array(templates())
    man = tpl[(g // 2) % len(tpl)]
    osense = np.empty((B, nO, 3))
    osense[..., 0] = rng.uniform(0.05, 0.15, (B, nO))
    osense[..., 1] = rng.uniform(0.01, 0.03, (B, nO))
    osense[..., 2] = rng.uniform(0.05, 0.2, (B, nO))
    osense[g % 3 == 0] = 0.0
    trk = np.empty((B, nO, AM.NP))
    trk[..., AM.R_POS] = rng.uniform(0.05, 0.15, (B, nO))
    trk[..., AM.R_HEADING] = rng.uniform(0.01, 0.03, (B, nO))
    trk[..., AM.R_SPEED] = rng.uniform(0.05, 0.2, (B, nO))
    trk[..., AM.Q_POS:AM.Q_ACCEL + 1] = rng.uniform(0.0, 1.0, (B, nO, 5)) * np.array(
        [0.05, 0.02, 0.1, 0.05, 1.0])
    trk[..., AM.P0_YAW] = rng.uniform(0.1, 0.4, (B, nO))
    trk[..., AM.P0_ACCEL] = rng.uniform(0.5, 2.0, (B, nO))
    trk[..., AM.W_CLAMP] = rng.uniform(0.2, 2.0, (B, nO))
    trk[..., AM.A_CLAMP] = rng.uniform(0.5, 6.0, (B, nO))
    hold = rng.uniform(0.3, 3.0, (B, nO, 2))
    hold[g % 4 == 3] = 1e3
    trk[..., AM.W_HOLD], trk[..., AM.A_HOLD] = hold[..., 0], hold[..., 1]
    trk[g % 5 == 1, AM.Q_POS:AM.Q_ACCEL + 1] = 0.0
    trk[g % 4 == 2, AM.W_CLAMP] = 0.0
    trk[g % 9 == 4, AM.A_CLAMP] = 0.0
    trk[g % 6 == 1, AM.W_HOLD] = 0.0
    trk[g % 6 == 4, AM.A_HOLD] = 0.0
    trk[g % 11 == 5, AM.P0_YAW] = 0.0
    trk[g % 13 == 6, AM.P0_ACCEL] = 0.0
    trk[g % 7 == 3] = 0.0
    for lane, kind in BAD_LANES.items():
        if lane >= B * nO:
            continue
        b, o = divmod(lane, nO)
        assert trk[b, o].any()
        if kind == "trk_nan":
            trk[b, o, AM.Q_ACCEL] = math.nan
        elif kind == "trk_negative":
            trk[b, o, AM.A_HOLD] = -1e-3
        elif kind == "trk_r_zero":
            trk[b, o, AM.R_SPEED] = 0.0
        elif kind == "row":
            rows[b, o, OM.LENGTH] = -1.0
        elif kind == "osense":
            osense[b, o] = [0.05, -0.01, 0.1]
    return rows, man, osense, trk


def times():
    """(t, t_since) of the eight steps: step 4 measures again at the time of step 3."""
    out, t = [], 0.0
    for s in range(N_STEPS):
        since = 0.0 if s in (0, 4) else T_STEP
        t += since
        out.append((t, since))
    return out


def ratio(pairs_x, dev_P, mir_P, dev_nis, mir_nis):
    """The one relative figure of tests/test_gpu_tracker.py: |dx| / max(1, |x|) over the pairs
    (estimate, measurement, obst), |dP_ij| / sqrt(P_ii P_jj), |dnis| / max(1, nis); NaN patterns
    must be identical.  The second of each pair is the reference."""
    f = lambda a: np.asarray(a, dtype=np.longdouble)
    for d, m in list(pairs_x) + [(dev_P, mir_P), (dev_nis, mir_nis)]:
        assert (np.isnan(f(d)) == np.isnan(f(m))).all()
    worst = 0.0
    for d, m in pairs_x:
        d, m = f(d), f(m)
        ok = ~np.isnan(m)
        if ok.any():
            worst = max(worst, float((np.abs(d - m)[ok] / np.maximum(1.0, np.abs(m[ok]))).max()))
    dev_P, mir_P, dev_nis, mir_nis = f(dev_P), f(mir_P), f(dev_nis), f(mir_nis)
    dg = np.sqrt(np.abs(np.einsum("...ii->...i", mir_P)))
    scale = dg[..., :, None] * dg[..., None, :]
    ok = ~np.isnan(mir_P) & (scale > 0)
    if ok.any():
        worst = max(worst, float((np.abs(dev_P - mir_P)[ok] / scale[ok]).max()))
    ok = ~np.isnan(mir_nis)
    if ok.any():
        worst = max(worst, float((np.abs(dev_nis - mir_nis)[ok] / np.maximum(1.0, mir_nis[ok])).max()))
    return worst


# Tolerance of the device against the mirror, in the figure of ``ratio``.  It is derived on
# the CPU from the reference alone (tests/test_tracker_accel_host.py,
# test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies): the largest figure
# between the mirror in float64 and the mirror in 80-bit on the inputs of ``case`` is
# MIRROR_ROUNDING, at (12, 22, 10), in a covariance entry of the first correction ((2, 3, 5):
# 1.70e-14, (1, 1, 1): 6.1e-15).  The device contracts multiply-adds and has its own sincos:
# 16 times the figure, rounded up to a power of two.
MIRROR_ROUNDING = 5.86e-14
TOL = 2.0 ** -39                  # 16 * 5.86e-14 = 9.4e-13 <= 2^-39 = 1.82e-12
# The six-state mirror with P0_ACCEL = Q_ACCEL = 0 against the five-state mirror on
# ``reduction_case``: measured 6.74e-14 (another order of the dense products, and the
# straight-line branch of the obstacle pose at w == 0); 16 times it, rounded up.
REDUCTION_MEASURED = 6.74e-14
RED_TOL = 2.0 ** -39              # 16 * 6.74e-14 = 1.08e-12 <= 2^-39 = 1.82e-12


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def run_mirror(B, nO, hp, fm, snapshots=None):
    """The eight steps of ``case`` on the mirror in the format ``fm``.  ``snapshots``: the
    snapshot rows per step (default: ``manoeuvre_mirror.state``).  Returns a list of
    (x, cov, nis, obst, z, x_before) per step."""
    rows, man, osense, trk = case(B, nO)
    x, cov = AM.alloc(B, nO, fm)
    out = []
    for s, (t, since) in enumerate(times()):
        snap = MNM.state(rows, man, t) if snapshots is None else snapshots[s]
        before = x.copy()
        ob, z, nis = AM.step(snap, osense, SEED, s, B_OFFSET, trk, 0.0, since, LEAD, DT, hp, x,
                             cov, fm)
        out.append((x.copy(), cov.copy(), nis, ob, z, before))
    return out


# ---------------------------------------------------------------------------
# The reduction to the five-state tracker: the inputs of tests/test_gpu_tracker.py's kind
# (rows that turn at a constant rate, measured at t_meas), six steps.
# ---------------------------------------------------------------------------
RED_STEPS = 6


def reduction_case(B, nO, seed=7):
    """rows, osense, trk5 [B, nO, 9] and its widened rows [B, nO, 14]: the mixed lanes of
    tests/test_gpu_tracker.py (every seventh off, Q = 0, W_CLAMP = 0, P0_YAW = 0, every third
    sensor exact).  Speeds >= 0.5 and no acceleration, so no lane stops.  Where the estimated
    turn rate is exactly 0 (P0_YAW = 0 with Q = 0) the five-state flow takes the
    straight-line branch of the obstacle pose, with another rounding order than the piece."""
    rng = np.random.default_rng(seed + 100 * B + nO)
    g = np.arange(B * nO).reshape(B, nO)
    rows = np.zeros((B, nO, 7))
    rows[..., OM.X], rows[..., OM.Y] = (g % 22) * 0.7 - 7.5, 6.0 - (g // 22)
    rows[..., OM.HEADING] = rng.uniform(-1.5, 1.5, (B, nO))
    rows[..., OM.SPEED] = rng.uniform(0.5, 4.0, (B, nO))
    rows[..., OM.LENGTH], rows[..., OM.WIDTH] = 4.0, 2.0
    rows[..., OM.YAW_RATE] = np.array(W_LIST)[g % len(W_LIST)]
    osense = np.empty((B, nO, 3))
    osense[..., 0] = rng.uniform(0.05, 0.15, (B, nO))
    osense[..., 1] = rng.uniform(0.01, 0.03, (B, nO))
    osense[..., 2] = rng.uniform(0.05, 0.2, (B, nO))
    osense[g % 3 == 0] = 0.0
    trk5 = np.empty((B, nO, TM.NP))
    trk5[..., 0] = rng.uniform(0.05, 0.15, (B, nO))
    trk5[..., 1] = rng.uniform(0.01, 0.03, (B, nO))
    trk5[..., 2] = rng.uniform(0.05, 0.2, (B, nO))
    trk5[..., 3:7] = rng.uniform(0.0, 1.0, (B, nO, 4)) * np.array([0.05, 0.02, 0.1, 0.05])
    trk5[..., 7] = rng.uniform(0.1, 0.4, (B, nO))
    trk5[..., 8] = rng.uniform(0.2, 2.0, (B, nO))
    trk5[g % 5 == 1, 3:7] = 0.0
    trk5[g % 4 == 2, 8] = 0.0
    trk5[g % 11 == 5, 7] = 0.0
    trk5[g % 7 == 3] = 0.0
    return rows, osense, trk5, AM.widen(trk5)


def reduction_times():
    out, t = [], 0.0
    for s in range(RED_STEPS):
        since = 0.0 if s in (0, 3) else T_STEP
        t += since
        out.append((t, since))
    return out


def reduction_ratio(x6, P6, nis6, ob6, x5, P5, nis5, ob5):
    """``ratio`` of the six-state outputs, cut to the five states, against the five-state's."""
    x6, P6 = np.asarray(x6, float), np.asarray(P6, float)
    return ratio([(x6[..., :5], x5), (ob6, ob5)], P6[..., :5, :5], P5, nis6, nis5)


# ---------------------------------------------------------------------------
# Consistency: every lane is one constant-acceleration piece at a constant turn rate,
# measured once per step through a noisy sensor, tracked with R equal to the sensor's sigmas,
# Q = 0, P0_ACCEL and P0_YAW equal to the sigmas the accelerations and turn rates were drawn
# with.  The five-state tracker runs on the same measurements with the same R and P0_YAW.
# ---------------------------------------------------------------------------
CONS_B, CONS_NO = 250, 6
CONS_STEPS, CONS_T = 12, 0.4
CONS_SIGMA = np.array([0.05, 0.01, 0.1])                  # position, heading, speed
CONS_YAW_SIGMA = 0.1
CONS_ACCEL_SIGMA = 0.5
CONS_SEED = 2026
CONS_HP, CONS_DT, CONS_LEAD = 6, 0.4, 0.1                  # the horizon ends 2.5 s ahead
CONS_AHEAD = CONS_HP * CONS_DT + CONS_LEAD


def consistency_inputs(B=CONS_B, n_obst=CONS_NO, seed=2027):
    """rows [B, nO, 7], man [B, nO, 4, 3] (one piece of 100 s), osense [B, nO, 3], the
    tracker rows [B, nO, 14] and the five-state rows [B, nO, 9].  Step s = 0 .. CONS_STEPS
    measures the snapshot at t = s CONS_T with epoch s; the first step initialises.  The
    speeds (15 .. 20 m/s) are high enough that no lane stops before the last predicted time
    (``no_lane_stops``)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((B, n_obst, OM.NP))
    rows[..., OM.X] = rng.uniform(-20.0, 20.0, (B, n_obst))
    rows[..., OM.Y] = rng.uniform(-20.0, 20.0, (B, n_obst))
    rows[..., OM.HEADING] = rng.uniform(-3.0, 3.0, (B, n_obst))
    rows[..., OM.SPEED] = rng.uniform(15.0, 20.0, (B, n_obst))
    rows[..., OM.LENGTH], rows[..., OM.WIDTH] = 4.0, 2.0
    rows[..., OM.YAW_RATE] = CONS_YAW_SIGMA * rng.standard_normal((B, n_obst))
    man = np.zeros((B, n_obst, MNM.NSEG, MNM.NF))
    man[..., 0, MNM.DUR] = 100.0
    man[..., 0, MNM.ACCEL] = CONS_ACCEL_SIGMA * rng.standard_normal((B, n_obst))
    osense = np.broadcast_to(CONS_SIGMA, (B, n_obst, 3)).copy()
    trk = np.zeros((B, n_obst, AM.NP))
    trk[..., AM.R_POS], trk[..., AM.R_HEADING], trk[..., AM.R_SPEED] = CONS_SIGMA
    trk[..., AM.P0_YAW], trk[..., AM.P0_ACCEL] = CONS_YAW_SIGMA, CONS_ACCEL_SIGMA
    trk[..., AM.W_CLAMP], trk[..., AM.A_CLAMP] = 10.0, 10.0
    trk[..., AM.W_HOLD], trk[..., AM.A_HOLD] = 1e3, 1e3
    trk5 = np.zeros((B, n_obst, TM.NP))
    trk5[..., TM.R_POS], trk5[..., TM.R_HEADING], trk5[..., TM.R_SPEED] = CONS_SIGMA
    trk5[..., TM.P0_YAW] = CONS_YAW_SIGMA
    trk5[..., TM.W_CLAMP] = 10.0
    return rows, man, osense, trk, trk5


def no_lane_stops(rows, man):
    """True when every lane still moves at the last predicted time (on the mirror)."""
    t_end = CONS_STEPS * CONS_T + CONS_AHEAD
    return bool((MNM.state(rows, man, t_end)[..., OM.SPEED] > 1.0).all())


def consistency_verdict(nis, obst_final, obst5_final, rows, man):
    """(mean NIS, its bound around 4, RMS position error CONS_AHEAD s after the last
    measurement of this tracker's prediction, of the five-state tracker's).  The mean of N
    chi^2_4 variables has standard deviation sqrt(8 / N): the bound is five of them."""
    nis = np.asarray(nis, float).reshape(-1)
    bound = 5.0 * np.sqrt(8.0 / nis.size)
    true = MNM.state(rows, man, CONS_STEPS * CONS_T + CONS_AHEAD)[..., :2].reshape(-1, 2)
    rms = lambda a: float(np.sqrt(((np.asarray(a, float).reshape(len(true), 2, -1)[:, :, -1]
                                    - true) ** 2).sum(axis=1).mean()))
    return float(nis.mean()), float(bound), rms(obst_final), rms(obst5_final)


# ---------------------------------------------------------------------------
# The frog rollout: every obstacle brakes at 3 m/s^2 until it stands, from a time inside the
# first three of the six steps.
# ---------------------------------------------------------------------------
FROG_STEPS = 6


def frog_inputs(sc, B):
    """rows [B, nObst, 7] and the braking schedule [B, nObst, 4, 3] of the frog rollout."""
    from scpqp import manoeuvres as MAN
    rows = np.broadcast_to(OM.nominal_rows(sc), (B, sc.nObst, 7)).copy()
    rows[..., OM.YAW_RATE] = np.random.default_rng(21).uniform(-0.3, 0.3, (B, sc.nObst))
    t0 = np.random.default_rng(22).uniform(0.0, FROG_STEPS * sc.dt * 0.5, (B, sc.nObst))
    brake = MAN.rows(B, sc.nObst, MAN.brake(t0, 3.0, 20.0), device="cpu").numpy()
    return rows, brake
