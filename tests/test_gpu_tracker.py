"""The obstacle tracker on the device (include/scpqp_tracker.h) against the CPU mirror
(tests/tracker_mirror.py): six tracker steps with mixed rows, the off and bad-row rules, the
independence of the lanes, recovery after trouble, the statistics of the innovations, and the
rollout.

Shapes (B, n_obst, hp): (2, 3, 5), no power of two; (12, 22, 10): 264 (b, o) lanes, two
workgroups of 256 with a ragged tail; (1, 1, 1).

Tolerance of the device against the mirror, one relative figure for the five outputs:
|dx_i| <= TOL max(1, |x_i|), |dP_ij| <= TOL sqrt(P_ii P_jj), |dnis| <= TOL max(1, nis),
|dz_i| <= TOL max(1, |z_i|), |d obst| <= TOL max(1, |obst|), and identical NaN patterns.  The
device's sin, cos and log differ from libm's by a few ulp, and its sums are fused and ordered
differently from numpy's dense products; the flow is closed-form and six steps long.  Measured
on an MI355X against the mirror (the test prints the figure; DESIGN §7, "Obstacle tracker"):
the largest ratio is MEASURED_RATIO below, at (12, 22, 10), in a covariance entry of the first
correction.  TOL is 16 times that, rounded up to a power of two; it is below the state
estimator's 2^-37.

Conditioning.  Two outputs amplify one unit in the last place of their inputs, in the mirror
as on the device, and the magnitudes of ``_case`` are chosen so that neither amplification hides
a defect of the kernel.  (1) The correction P - P S^-1 P subtracts nearly equal numbers in the
turn-rate variance of the first correction: the prior is P0_YAW^2 and the posterior is
P0_YAW^2 / (1 + T^2 P0_YAW^2 / (2 R_HEADING^2)), so one rounding of the predicted P is amplified
by that denominator: at most 1 + 0.16 * 0.16 / 2e-4 = 129 with R_HEADING >= 0.01 rad and
P0_YAW <= 0.4 rad/s, the sigmas of a plausible sensor.  (2) nis = y' S^-1 y moves by 2 |y| / S
times a change of the measured position, which the device and the mirror compute to a few units
in the last place of the coordinate: the obstacles stay within 16 m of the origin and
R_POS >= 0.05 m.  A first version of the case with R_HEADING down to 0.002 rad, P0_YAW up to
1 rad/s (a denominator of 1.5e4) and positions up to 375 m measured 4.0e-12, all of it in
P[4][4], P[2][2] and nis of such lanes; x, z and obst agreed to 5e-14 there.

The frog rollout prints the ratio of the tracked prediction's summed error to the untracked
one's from step 2 on, with an exact sensor; it asserts only "smaller".  Measured on an MI355X
(DESIGN §7): 0.0725 m tracked against 2188.5 m untracked, a ratio of 3.3e-5.
"""
import math
import types

import numpy as np
import pytest
import torch

import obstacle_mirror as OM
import sensing_mirror as SM
import tracker_mirror as TM
from oracle import scp_reference as R
from scpqp import obstacles as OB
from scpqp import sensing as SE
from scpqp import tracker as TRK

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 5), (12, 22, 10), (1, 1, 1)]          # (B, n_obst, hp)
T_STEP, LEAD, DT = 0.4, 0.13, 0.4
N_STEPS = 6
SEED = 77
MEASURED_RATIO = 1.07e-13         # (2, 3, 5): 1.8e-14; (1, 1, 1): 5.0e-15
TOL = 2.0 ** -39                  # 16 * 1.07e-13 = 1.71e-12 <= 2^-39 = 1.82e-12


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _bits(t):
    return t.contiguous().view(torch.int64)


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


# turn rates on both sides of the sinc switch (|a| = 1e-4) and of the g' switch (|a| = 0.02)
# at a = 0.5 w T_STEP, w = 0 exactly, and large ones of both signs
W_LIST = [0.0, 1e-9, 1e-3, 0.9e-4 * 2 / T_STEP, 1.1e-4 * 2 / T_STEP, 0.019 * 2 / T_STEP,
          0.021 * 2 / T_STEP, 0.3, -1.2, 3.0, -0.021 * 2 / T_STEP]


def _case(B, nO, seed=7):
    """Obstacle rows, osense rows and tracker rows.  Lane g: every seventh is off, g % 5 == 1
    has Q = 0, g % 4 == 2 has W_CLAMP = 0, g % 11 == 5 has P0_YAW = 0; every third lane has
    an exact sensor.  Magnitudes: see "Conditioning" in the module's docstring."""
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
    trk = np.empty((B, nO, 9))
    trk[..., 0] = rng.uniform(0.05, 0.15, (B, nO))
    trk[..., 1] = rng.uniform(0.01, 0.03, (B, nO))
    trk[..., 2] = rng.uniform(0.05, 0.2, (B, nO))
    trk[..., 3:7] = rng.uniform(0.0, 1.0, (B, nO, 4)) * np.array([0.05, 0.02, 0.1, 0.05])
    trk[..., 7] = rng.uniform(0.1, 0.4, (B, nO))
    trk[..., 8] = rng.uniform(0.2, 2.0, (B, nO))
    trk[g % 5 == 1, 3:7] = 0.0
    trk[g % 4 == 2, 8] = 0.0
    trk[g % 11 == 5, 7] = 0.0
    trk[g % 7 == 3] = 0.0
    return rows, osense, trk


def _times():
    """(t_meas, t_since) of the six steps: step 3 measures again at the time of step 2."""
    out, t = [], 0.0
    for s in range(N_STEPS):
        since = 0.0 if s in (0, 3) else T_STEP
        t += since
        out.append((t, since))
    return out


def _ratio(pairs_x, dev_P, mir_P, dev_nis, mir_nis):
    """The largest relative difference; NaN patterns must be identical.  pairs_x: (device,
    mirror) arrays measured against max(1, |mirror|)."""
    for d, m in list(pairs_x) + [(dev_P, mir_P), (dev_nis, mir_nis)]:
        assert (np.isnan(d) == np.isnan(m)).all()
    worst = 0.0
    for d, m in pairs_x:
        ok = ~np.isnan(m)
        if ok.any():
            worst = max(worst, float((np.abs(d - m)[ok] / np.maximum(1.0, np.abs(m[ok]))).max()))
    dg = np.sqrt(np.abs(np.einsum("...ii->...i", mir_P)))
    scale = dg[..., :, None] * dg[..., None, :]
    ok = ~np.isnan(mir_P) & (scale > 0)
    if ok.any():
        worst = max(worst, float((np.abs(dev_P - mir_P)[ok] / scale[ok]).max()))
    ok = ~np.isnan(mir_nis)
    if ok.any():
        worst = max(worst, float((np.abs(dev_nis - mir_nis)[ok] / np.maximum(1.0, mir_nis[ok])).max()))
    return worst


# ---------------------------------------------------------------------------
# 1. device against mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,nO,hp", SHAPES)
def test_six_steps_match_the_mirror(gpu, B, nO, hp):
    rows, osense, trk = _case(B, nO)
    rows_d, osense_d, trk_d = _dev(rows, gpu), _dev(osense, gpu), _dev(trk, gpu)
    x_d, cov_d = TRK.alloc(B, nO, gpu)
    x_m, cov_m = np.full((B, nO, 5), np.nan), np.zeros((B, nO, 5, 5))
    on = (trk != 0).any(axis=2)
    worst = 0.0
    seen_update = False
    for s, (t_meas, since) in enumerate(_times()):
        ob_d, z_d, nis_d = TRK.step(rows_d, osense_d, SEED, s, 3, trk_d, t_meas, since, LEAD, DT,
                                    hp, x_d, cov_d)
        ob_m, z_m, nis_m = TM.step(rows, osense, SEED, s, 3, trk, t_meas, since, LEAD, DT, hp,
                                   x_m, cov_m)
        # the off lanes: untouched state
        assert np.isnan(x_d.cpu().numpy()[~on]).all() and (cov_d.cpu().numpy()[~on] == 0).all()
        worst = max(worst, _ratio([(x_d.cpu().numpy(), x_m), (z_d.cpu().numpy(), z_m),
                                   (ob_d.cpu().numpy(), ob_m)], cov_d.cpu().numpy(), cov_m,
                                  nis_d.cpu().numpy(), nis_m))
        seen_update |= bool(np.isfinite(nis_m).any())
    print(f"({B}, {nO}, {hp}): largest device - mirror ratio {worst:.3e} (TOL {TOL:.3e})")
    assert seen_update
    assert worst <= TOL


# ---------------------------------------------------------------------------
# 2. off rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sensed", [False, True])
def test_off_rows_give_the_untracked_prediction_and_leave_the_state(gpu, sensed):
    B, nO, hp = 12, 22, 10
    rows, osense, _ = _case(B, nO)
    rng = np.random.default_rng(5)
    x0 = _dev(rng.standard_normal((B, nO, 5)), gpu)
    cov0 = _dev(rng.standard_normal((B, nO, 5, 5)), gpu)
    x, cov = x0.clone(), cov0.clone()
    rows_d = _dev(rows, gpu)
    os_d = _dev(osense, gpu) if sensed else None
    ob, z, nis = TRK.step(rows_d, os_d, SEED, 4, 2, TRK.off(B, nO, gpu), 0.8, T_STEP, LEAD, DT, hp,
                          x, cov)
    want = SE.predict_sensed(rows_d, os_d, SEED, 4, 2, 0.8, LEAD, DT, hp) if sensed \
        else OB.predict(rows_d, 0.8, LEAD, DT, hp)
    assert _beq(ob, want)
    assert _beq(x, x0) and _beq(cov, cov0) and torch.isnan(nis).all()
    z_m = np.array([[TM.measurement(rows[b, o], osense[b, o] if sensed else None, SEED, 4, o,
                                    2 + b, 0.8) for o in range(nO)] for b in range(B)])
    assert (np.abs(z.cpu().numpy() - z_m) <= TOL * np.maximum(1.0, np.abs(z_m))).all()
    if sensed:
        # an all-zero osense array is the exact sensor: bitwise what NULL gives
        x1, cov1 = x0.clone(), cov0.clone()
        trk = _dev(_case(B, nO)[2], gpu)
        a = TRK.step(rows_d, torch.zeros_like(os_d), SEED, 4, 2, trk, 0.8, T_STEP, LEAD, DT, hp,
                     x1, cov1)
        x2, cov2 = x0.clone(), cov0.clone()
        b = TRK.step(rows_d, None, 0, 0, 0, trk, 0.8, T_STEP, LEAD, DT, hp, x2, cov2)
        assert all(_beq(p, q) for p, q in zip(a, b)) and _beq(x1, x2) and _beq(cov1, cov2)


# ---------------------------------------------------------------------------
# 3. split batch, lane independence, bad rows, recovery
# ---------------------------------------------------------------------------
def _run(rows, osense, trk, gpu, hp=10, lo=0, hi=None, steps=3):
    B, nO = rows[lo:hi].shape[:2]
    x, cov = TRK.alloc(B, nO, gpu)
    rows_d, os_d, trk_d = _dev(rows[lo:hi], gpu), _dev(osense[lo:hi], gpu), _dev(trk[lo:hi], gpu)
    out = []
    for s, (t_meas, since) in enumerate(_times()[:steps]):
        ob, z, nis = TRK.step(rows_d, os_d, SEED, s, lo, trk_d, t_meas, since, LEAD, DT, hp, x, cov)
        out.append((x.clone(), cov.clone(), nis, ob, z))
    return out


def test_a_split_batch_gives_what_the_whole_gives(gpu):
    B, nO = 12, 22
    case = _case(B, nO)
    whole = _run(*case, gpu)
    a, b = _run(*case, gpu, lo=0, hi=5), _run(*case, gpu, lo=5, hi=B)
    for s, w in enumerate(whole):
        for k in range(5):
            assert _beq(w[k], torch.cat([a[s][k], b[s][k]])), (s, k)


BAD_TRK = [(0, math.nan), (6, math.inf), (1, -1e-3), (8, -1e-300), (2, 0.0), (0, 0.0)]


def test_changing_the_last_row_changes_only_its_lane(gpu):
    B, nO = 12, 22
    rows, osense, trk = _case(B, nO)
    trk[-1, -1] = [0.05, 0.01, 0.1, 0.01, 0.005, 0.02, 0.02, 0.5, 1.0]
    osense[-1, -1] = [0.05, 0.01, 0.1]
    base = _run(rows, osense, trk, gpu)
    other = trk.copy()
    other[-1, -1, 0] = 0.08
    got = _run(rows, osense, other, gpu)
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
        assert TM.is_bad_row(bad[-1, -1])
        only_the_last_lane_is_nan(_run(rows, osense, bad, gpu), ("trk", f), False)
    # a bad obstacle row and a bad osense row: the same, and no measurement
    for f, val in ((OM.LENGTH, -1.0), (OM.X, math.nan), (OM.YAW_RATE, math.inf)):
        bad = rows.copy()
        bad[-1, -1, f] = val
        assert OM.bad_row(bad[-1, -1])
        only_the_last_lane_is_nan(_run(bad, osense, trk, gpu), ("rows", f), True)
    for f, val in ((0, -0.1), (2, math.nan)):
        bad = osense.copy()
        bad[-1, -1, f] = val
        assert SM.bad_osense_row(bad[-1, -1])
        only_the_last_lane_is_nan(_run(rows, bad, trk, gpu), ("osense", f), True)


def test_a_lane_turned_nan_recovers_on_the_next_call(gpu):
    B, nO, hp = 2, 3, 5
    rows, osense, _ = _case(B, nO)
    rows_d, os_d = _dev(rows, gpu), _dev(osense, gpu)
    trk = TRK.rows(B, nO, device=gpu)
    x, cov = TRK.alloc(B, nO, gpu)
    TRK.step(rows_d, os_d, SEED, 0, 0, trk, 0.0, 0.0, LEAD, DT, hp, x, cov)
    good = (x.clone(), cov.clone())
    cov[1, 2] = -torch.eye(5, dtype=torch.float64, device=gpu)       # no Cholesky of S
    x[0, 1, 3] = math.inf                                              # a non-finite prediction
    ob, z, nis = TRK.step(rows_d, os_d, SEED, 1, 0, trk, 0.4, 0.4, LEAD, DT, hp, x, cov)
    for b, o in ((1, 2), (0, 1)):
        assert torch.isnan(x[b, o]).all() and torch.isnan(cov[b, o]).all() and math.isnan(nis[b, o])
        assert torch.isnan(ob[b, o]).all() and torch.isfinite(z[b, o]).all()
    ref = (good[0].clone(), good[1].clone())
    ob_r, z_r, nis_r = TRK.step(rows_d, os_d, SEED, 1, 0, trk, 0.4, 0.4, LEAD, DT, hp, *ref)
    keep = torch.ones((B, nO), dtype=torch.bool, device=gpu)
    keep[1, 2] = keep[0, 1] = False
    assert _beq(x[keep], ref[0][keep]) and _beq(cov[keep], ref[1][keep])
    assert _beq(nis[keep], nis_r[keep]) and _beq(ob[keep], ob_r[keep]) and _beq(z, z_r)
    # the next call initialises the lanes again
    ob, z, nis = TRK.step(rows_d, os_d, SEED, 2, 0, trk, 0.8, 0.4, LEAD, DT, hp, x, cov)
    r = np.append(TM.r_diag(trk[0, 0].cpu().numpy()), TRK.P0_YAW ** 2)
    for b, o in ((1, 2), (0, 1)):
        assert _beq(x[b, o, :4], z[b, o]) and x[b, o, 4] == 0 and math.isnan(nis[b, o])
        assert (cov[b, o].cpu().numpy() == np.diag(r)).all()
        assert torch.isfinite(ob[b, o]).all()
    assert torch.isfinite(nis[keep]).all()


# ---------------------------------------------------------------------------
# 4. statistics: the CPU consistency inputs on the device
# ---------------------------------------------------------------------------
def test_innovations_are_consistent_on_the_device(gpu):
    rows, osense, trk = TM.consistency_inputs()
    B, nO = rows.shape[:2]
    rows_d, os_d, trk_d = _dev(rows, gpu), _dev(osense, gpu), _dev(trk, gpu)
    x, cov = TRK.alloc(B, nO, gpu)
    every = []
    for s in range(TM.CONS_STEPS + 1):
        ob, z, nis = TRK.step(rows_d, os_d, TM.CONS_SEED, s, 0, trk_d, s * TM.CONS_T,
                              0.0 if s == 0 else TM.CONS_T, TM.CONS_LEAD, TM.CONS_DT, TM.CONS_HP,
                              x, cov)
        if s:
            every.append(nis.cpu().numpy())
    every = np.array(every)
    assert np.isfinite(every).all() and every.size == 18000
    mean, bound, rms_trk, rms_line = TM.consistency_verdict(
        every, ob.cpu().numpy(), z.cpu().numpy(), rows, TM.CONS_STEPS * TM.CONS_T)
    print(f"mean NIS {mean:.3f} (|mean - 4| <= {bound:.3f}); RMS error 2.5 s ahead {rms_trk:.4f} m "
          f"of the tracked prediction, {rms_line:.4f} m of the straight extrapolation")
    assert abs(mean - 4.0) <= bound
    assert rms_trk < rms_line


# ---------------------------------------------------------------------------
# 5. rollout: frog, 1 vehicle, 22 obstacles, Hp 10, B = 4, 4 steps, noise seed 1
# ---------------------------------------------------------------------------
STEPS = 4
KEYS = ("x0", "u0", "umax", "U", "traj", "n_scp", "status", "path", "u_tick", "obst")
TRK_KEYS = ("obst_est", "obst_nis", "obst_meas")
SENSE_SEED = 31


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl):
    return types.SimpleNamespace(
        hist=[{k: h[k].clone() for k in KEYS + TRK_KEYS if k in h} for h in cl.history],
        metrics=cl.metrics(), control=cl.control.clone())


def _frog_rows(sc, B):
    rows = np.broadcast_to(OM.nominal_rows(sc), (B, sc.nObst, 7)).copy()
    rows[..., OM.YAW_RATE] = np.random.default_rng(21).uniform(-0.3, 0.3, (B, sc.nObst))
    return rows


def _frog_osense(sc, B):
    osense = np.zeros((B, sc.nObst, 3))
    osense[..., 0], osense[..., 1], osense[..., 2] = 0.05, 0.01, 0.1
    osense[1, 3] = 0.0                 # one exact sensor among the noisy ones
    return osense


def _frog_trk(osense):
    trk = TRK.matched(osense, device="cpu").numpy()
    trk[3, 0] = 0.0                    # one lane without a filter among lanes with one
    return trk


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.frog_scenario(Hp=10)
    B = 4
    x_init = _x_init(sc, B)
    rows = _frog_rows(sc, B)
    osense = _frog_osense(sc, B)
    trk_exact = _frog_trk(np.zeros_like(osense))
    trk_noisy = _frog_trk(osense)
    off = np.zeros((B, sc.nObst, 9))
    sense = dict(obstacle_sensing=osense, sense_seed=SENSE_SEED)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, kw in (("plain", {}), ("plain_none", dict(tracker=None)),
                     ("plain_off", dict(tracker=off)), ("plain_trk", dict(tracker=trk_exact)),
                     ("noisy", sense), ("noisy_off", dict(tracker=_dev(off, gpu), **sense)),
                     ("noisy_trk", dict(tracker=trk_noisy, **sense))):
        cl.reset(x_init, seed=1, obstacles=rows, **kw)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, obstacles=rows[o:o + 2],
                   obstacle_sensing=osense[o:o + 2], sense_seed=SENSE_SEED,
                   tracker=trk_noisy[o:o + 2])
        half.run(STEPS)
        runs[f"half{o}"] = _snapshot(half)
    half.close()
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, rows=rows, osense=osense,
                                trk_exact=trk_exact, trk_noisy=trk_noisy, runs=runs)
    cl.close()


@pytest.mark.parametrize("base,same", [("plain", "plain_none"), ("plain", "plain_off"),
                                       ("noisy", "noisy_off")])
def test_rollout_without_a_tracker_is_the_rollout_of_before(rollouts, base, same):
    a, b = rollouts.runs[base], rollouts.runs[same]
    assert len(a.hist) == len(b.hist) == STEPS
    for i in range(STEPS):
        assert not any(k in a.hist[i] for k in TRK_KEYS)
        for k in KEYS:
            if a.hist[i][k].dtype == torch.float64:
                assert _beq(a.hist[i][k], b.hist[i][k]), (i, k)
            else:
                assert _eq(a.hist[i][k], b.hist[i][k]), (i, k)
        if same.endswith("off"):
            assert torch.isnan(b.hist[i]["obst_est"]).all() and torch.isnan(b.hist[i]["obst_nis"]).all()
            assert torch.isfinite(b.hist[i]["obst_meas"]).all()
        else:
            assert not any(k in b.hist[i] for k in TRK_KEYS)
    assert _eq(a.control.view(torch.int64), b.control.view(torch.int64))
    for k, v in a.metrics.items():
        assert _eq(v, b.metrics[k]), k


@pytest.mark.parametrize("name", ["plain_trk", "noisy_trk"])
def test_rollout_records_what_step_gives(rollouts, gpu, name):
    ro, sc = rollouts, rollouts.sc
    run = ro.runs[name]
    noisy = name == "noisy_trk"
    rows = _dev(ro.rows, gpu)
    osense = _dev(ro.osense, gpu) if noisy else None
    trk = _dev(ro.trk_noisy if noisy else ro.trk_exact, gpu)
    x, cov = TRK.alloc(ro.B, sc.nObst, gpu)
    lead = sc.delay_x + sc.dt + sc.delay_u
    g0 = 0
    for i, rec in enumerate(run.hist):
        g1 = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
        ob, z, nis = TRK.step(rows, osense, SENSE_SEED, i, 0, trk, g1 * sc.tick_length,
                              (g1 - g0) * sc.tick_length, lead, sc.dt, sc.Hp, x, cov)
        g0 = g1
        assert _beq(rec["obst"], ob) and _beq(rec["obst_est"], x), i
        assert _beq(rec["obst_nis"], nis) and _beq(rec["obst_meas"], z), i
        # the measurement is the one the untracked controller extrapolates
        zh = z.cpu().numpy()
        if not noisy:
            pose = OB.pose(rows, sc.tick_length, g1, 0)[:, :, 0].cpu().numpy()
            # (the same formulas in another kernel: no rounding order is promised between them)
            assert (np.abs(zh[..., :3] - pose) <= TOL * np.maximum(1.0, np.abs(pose))).all()
            assert np.array_equal(zh[..., 3], ro.rows[..., 3])
        # the lane without a filter keeps the untracked prediction
        # (the obstacle prediction reads nothing of the vehicles, so at every step)
        assert _beq(rec["obst"][3, 0], ro.runs["noisy" if noisy else "plain"].hist[i]["obst"][3, 0])
        assert torch.isnan(rec["obst_est"][3, 0]).all()
    last = run.hist[-1]
    assert torch.isfinite(last["obst_nis"][0]).all()
    assert not _beq(last["obst_est"][0, :, :4], last["obst_meas"][0])


def test_rollout_with_a_tracker_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["noisy_trk"].hist):
        for k in KEYS + TRK_KEYS:
            parts = torch.cat([ro.runs["half0"].hist[i][k], ro.runs["half2"].hist[i][k]])
            if whole[k].dtype == torch.float64:
                assert _beq(whole[k], parts), (i, k)
            else:
                assert _eq(whole[k], parts), (i, k)
    for k, v in ro.runs["noisy_trk"].metrics.items():
        assert _eq(v, torch.cat([ro.runs["half0"].metrics[k], ro.runs["half2"].metrics[k]])), k


def test_reset_refuses_a_bad_tracker_before_anything_is_launched(rollouts, gpu):
    ro, cl = rollouts, rollouts.cl
    cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker=ro.trk_exact)
    cl.run(1)
    n_hist, i = len(cl.history), cl.i
    state, rows_before = cl.state.clone(), cl.trk_rows.clone()
    x_before, cov_before = cl.trk_x.clone(), cl.trk_cov.clone()
    good = ro.trk_exact
    neg, zero_r, nan = good.copy(), good.copy(), good.copy()
    neg[2, 1, 6] = -0.1
    zero_r[1, 0, 1] = 0.0
    nan[0, 0, 4] = math.nan
    for bad in (good[:2], good[:, :1], good[..., :8], neg, torch.as_tensor(neg), zero_r, nan):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker=bad)
    with pytest.raises(ValueError, match=r"rows\[2, 1\]: q_yaw must be >= 0"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker=neg)
    with pytest.raises(ValueError, match=r"rows\[1, 0\]: r_heading must be > 0"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker=zero_r)
    with pytest.raises(ValueError, match=r"tracker needs obstacles= rows"):
        cl.reset(ro.x_init, seed=1, tracker=good)
    assert len(cl.history) == n_hist and cl.i == i           # the refused resets changed nothing
    assert _eq(cl.state, state) and _eq(cl.trk_rows, rows_before)
    assert _beq(cl.trk_x, x_before) and _beq(cl.trk_cov, cov_before)


def test_with_an_exact_sensor_the_tracked_prediction_beats_the_straight_one(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    rows = _dev(ro.rows, gpu)
    tps, tdx, tdu, Hp = sc.ticks_per_sim, sc.ticks_delay_x, sc.ticks_delay_u, sc.Hp
    ahead = [(k + 1) * tps + tdx + tps + tdu for k in range(Hp)]       # tau_k in ticks
    on = torch.as_tensor((ro.trk_exact != 0).any(axis=2), device=gpu)
    err = {}
    for name in ("plain", "plain_trk"):
        total = 0.0
        for i in range(2, STEPS):
            g1 = max(0, i * tps - tdx)
            true = OB.pose(rows, sc.tick_length, g1, ahead[-1])[:, :, ahead, 0:2]   # [B, nO, Hp, 2]
            d = ro.runs[name].hist[i]["obst"].transpose(2, 3) - true
            total += float(d.norm(dim=-1)[on].sum().item())
        err[name] = total
    print(f"summed prediction error from step 2 on: tracked {err['plain_trk']:.4f} m, untracked "
          f"{err['plain']:.4f} m, ratio {err['plain_trk'] / err['plain']:.3e}")
    assert err["plain_trk"] < err["plain"]
