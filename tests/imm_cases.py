"""The inputs of the tests of the interacting-multiple-model tracker, shared by the CPU tests
(tests/test_imm_host.py: the tolerances are derived there, from the mirror alone) and the GPU
tests (tests/test_gpu_imm.py), so that both see exactly the same numbers.  The lanes are those
of tests/tracker_accel_cases.py, widened to banks.  numpy only, but for ``response_bank``."""
import math

import numpy as np

import imm_mirror as IM
import manoeuvre_mirror as MNM
import obstacle_mirror as OM
import tracker_accel_cases as TC
import tracker_accel_mirror as AM

SHAPES = TC.SHAPES                                     # (B, n_obst, hp)
MODES = (1, 2, 3, 4)
T_STEP, LEAD, DT = TC.T_STEP, TC.LEAD, TC.DT
N_STEPS = TC.N_STEPS
SEED = TC.SEED
B_OFFSET = TC.B_OFFSET
times = TC.times                                       # step 4 has t_since = 0
pow2_ceil = TC.pow2_ceil

# (lane g of the (12, 22) shape, what is bad there), besides TC.BAD_LANES (a bad row of mode
# 0, a bad obstacle row, a bad osense row).  "mixed" needs two modes.
BAD_LANES = {210: "sw_negative", 211: "sw_nan", 212: "sw_sum", 214: "mixed"}


def widen(trk14, M):
    """[B, nO, M, 14]: mode 0 is the row itself; mode 1 lets go of the acceleration and hardly
    expects one; mode 2 keeps both for the whole horizon and expects a strong one; mode 3 lets
    go of the turn rate and expects more of it.  An off row stays off in every mode."""
    out = np.repeat(np.asarray(trk14, float)[:, :, None, :], M, axis=2).copy()
    on = (out[:, :, 0] != 0).any(axis=-1)
    if M > 1:
        out[on, 1, AM.A_HOLD] = 0.0
        out[on, 1, AM.Q_ACCEL] *= 0.1
    if M > 2:
        out[on, 2, AM.W_HOLD] = out[on, 2, AM.A_HOLD] = 1e3
        out[on, 2, AM.Q_ACCEL] = 3.0 * out[on, 2, AM.Q_ACCEL] + 0.5
    if M > 3:
        out[on, 3, AM.W_HOLD] = 0.0
        out[on, 3, AM.Q_YAW] += 0.05
    return out


def switching(B, nO, M, seed=5):
    """sw [B, nO, M + 1, M]: random mu0 and Pi whose rows sum to 1.  Lane g: g % 8 == 1 has a
    Pi whose last column is zero (a dead mode; with g % 16 == 9 its mu0 is 0 too),
    g % 8 == 5 has Pi = I, g % 10 == 2 a mu0 whose first entry is exactly 0 (these need
    M >= 2, but Pi = I)."""
    rng = np.random.default_rng(seed + 100 * B + nO + 7 * M)
    sw = rng.uniform(0.05, 1.0, (B, nO, M + 1, M))
    g = np.arange(B * nO).reshape(B, nO)
    sw[..., 1:, :] += 3.0 * np.eye(M)
    sw[g % 8 == 5, 1:] = np.eye(M)
    if M > 1:
        sw[g % 8 == 1, 1:, M - 1] = 0.0
        sw[g % 16 == 9, 0, M - 1] = 0.0
        sw[g % 10 == 2, 0, 0] = 0.0
    sw /= sw.sum(axis=-1, keepdims=True)
    return sw


def kinds(B, nO, M):
    """How many lanes of the case are of each special kind (the host test counts them)."""
    _, _, _, trk, sw = case(B, nO, M)
    lanes = [(trk[b, o], sw[b, o]) for b in range(B) for o in range(nO)]
    off = [IM.is_off_lane(t) for t, _ in lanes]
    good = [(t, s) for (t, s), f in zip(lanes, off) if not f and not IM.is_bad_lane(t, s)]
    return dict(
        off=sum(off),
        dead=sum(bool((s[1:, M - 1] == 0).all()) for _, s in good) if M > 1 else 0,
        identity=sum(bool((s[1:] == np.eye(M)).all()) for _, s in good),
        mu0_zero=sum(bool((s[0] == 0).any()) for _, s in good),
        bad_row=sum(any(AM.is_bad_row(r) for r in t) for (t, _), f in zip(lanes, off) if not f),
        mixed=sum((not f) and any(AM.is_off_row(r) for r in t) for (t, _), f in zip(lanes, off)),
        sw_negative=sum(bool((s < 0).any()) for (_, s), f in zip(lanes, off) if not f),
        sw_nan=sum(bool(np.isnan(s).any()) for (_, s), f in zip(lanes, off) if not f),
        sw_sum=sum(bool(np.isfinite(s).all() and (s >= 0).all() and IM.bad_sw(s))
                   for (_, s), f in zip(lanes, off) if not f))


def case(B, nO, M):
    """rows, man, osense of ``tracker_accel_cases.case``, its tracker rows widened to M modes,
    and ``switching``; the (12, 22) shape has one bad lane of each kind (BAD_LANES) on top of
    those of ``tracker_accel_cases``."""
    rows, man, osense, trk14 = TC.case(B, nO)
    trk, sw = widen(trk14, M), switching(B, nO, M)
    for lane, kind in BAD_LANES.items():
        if lane >= B * nO:
            continue
        b, o = divmod(lane, nO)
        assert trk[b, o].any()
        if kind == "sw_negative":
            sw[b, o, 1, 0] = -1e-3
        elif kind == "sw_nan":
            sw[b, o, 0, M - 1] = math.nan
        elif kind == "sw_sum":
            sw[b, o, M, 0] += 1e-6
        elif kind == "mixed" and M > 1:
            trk[b, o, M - 1] = 0.0
    return rows, man, osense, trk, sw


def ratio(dev, mir):
    """The relative figure of ``tracker_accel_cases.ratio`` over (x_imm, cov, mu, x_hat, nis,
    obst, z), with mu compared absolutely; NaN patterns must be identical.  ``mir`` is the
    reference."""
    (dx, dP, dmu, dxh, dnis, dob, dz), (mx, mP, mmu, mxh, mnis, mob, mz) = dev, mir
    worst = TC.ratio([(dx, mx), (dxh, mxh), (dz, mz), (dob, mob)], dP, mP, dnis, mnis)
    f = lambda a: np.asarray(a, dtype=np.longdouble)
    assert (np.isnan(f(dmu)) == np.isnan(f(mmu))).all()
    ok = ~np.isnan(f(mmu))
    if ok.any():
        worst = max(worst, float(np.abs(f(dmu) - f(mmu))[ok].max()))
    return worst


def run_mirror(B, nO, hp, M, fm, snapshots=None):
    """The eight steps of ``case`` on the mirror in the format ``fm``.  Returns a list of
    (x_imm, cov, mu, x_hat, nis, obst, z) per step."""
    rows, man, osense, trk, sw = case(B, nO, M)
    x, cov, mu = IM.alloc(B, nO, M, fm)
    out = []
    for s, (t, since) in enumerate(times()):
        snap = MNM.state(rows, man, t) if snapshots is None else snapshots[s]
        ob, xh, z, nis = IM.step(snap, osense, SEED, s, B_OFFSET, trk, sw, 0.0, since, LEAD, DT,
                                 hp, x, cov, mu, fm)
        out.append((x.copy(), cov.copy(), mu.copy(), xh, nis, ob, z))
    return out


# Tolerance of the device against the mirror, in the figure of ``ratio``.  It is derived on the
# CPU from the reference alone (tests/test_imm_host.py,
# test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies): the largest figure
# between the mirror in float64 and the mirror in 80-bit on the inputs of ``case``, over the
# three shapes and M = 1 .. 4, is MIRROR_ROUNDING (per M in MIRROR_ROUNDING_BY_M, each at
# (12, 22, 10)).  The device contracts multiply-adds and has its own sincos, exp and log: 16
# times the figure, rounded up to a power of two.
# The largest figures sit in mu: the likelihood turns an error of nis / 2 into a relative error
# of a probability.  ((2, 3, 5): at most 3.5e-14, (1, 1, 1): at most 2.1e-14.)
MIRROR_ROUNDING_BY_M = {1: 5.87e-14, 2: 9.87e-13, 3: 9.38e-13, 4: 2.66e-13}
MIRROR_ROUNDING_SMALL = {1: 1.71e-14, 2: 3.46e-14, 3: 3.01e-14, 4: 1.73e-14}   # at (2, 3, 5)
MIRROR_ROUNDING = max(MIRROR_ROUNDING_BY_M.values())
# Two float64 runs of the mirror that differ only in the order of the modes are each about that
# far from the exact result, so they are at most twice that apart: the bound of the permutation
# test, per shape, at M = 3 (no factor 16: no device is involved).
PERM_SHAPES = {(12, 22, 10): 2 * MIRROR_ROUNDING_BY_M[3], (2, 3, 5): 2 * MIRROR_ROUNDING_SMALL[3]}
TOL = 2.0 ** -35                  # 16 * 9.87e-13 = 1.58e-11 <= 2^-35 = 2.91e-11


# ---------------------------------------------------------------------------
# The reductions to the single filter of scpqp_tracker_accel.h, on the lanes of ``case``
# (without the bad sw and mixed lanes, which the single filter does not have).
# ---------------------------------------------------------------------------
REDUCTIONS = ("one_mode", "identity", "identical")


def reduction_case(B, nO, kind):
    """rows, man, osense, trk14 of ``tracker_accel_cases.case`` and the bank (trk, sw) that
    must reproduce ``tracker_accel_mirror.step`` on trk14:
      one_mode   M = 1
      identity   M = 2, Pi = I, mu0 = (1, 0): the second mode never gets a probability
      identical  M = 3, the same row in every mode, an arbitrary Pi: the mixing runs with a
                 spread term that is zero up to rounding"""
    rows, man, osense, trk14 = TC.case(B, nO)
    M = {"one_mode": 1, "identity": 2, "identical": 3}[kind]
    if kind == "identical":
        trk = np.repeat(trk14[:, :, None, :], M, axis=2).copy()
        sw = switching(B, nO, M, seed=9)
    else:
        trk = widen(trk14, M)
        sw = np.zeros((B, nO, M + 1, M))
        sw[..., 0, 0] = 1.0
        sw[..., 1:, :] = np.eye(M)
    return rows, man, osense, trk14, trk, sw


def reduction_ratio(bank, single):
    """``tracker_accel_cases.ratio`` of (x_hat, cov of mode 0, nis of mode 0, obst) of the bank
    against (x_trk, cov, nis, obst) of the single filter."""
    (xh, cov, nis, ob), (x1, cov1, nis1, ob1) = bank, single
    return TC.ratio([(xh, x1), (ob, ob1)], np.asarray(cov)[:, :, 0], cov1,
                    np.asarray(nis)[:, :, 0], nis1)


# The float64 bank mirror against the float64 single-filter mirror on ``reduction_case`` at
# (12, 22, 10), eight steps (tests/test_imm_host.py, test_reductions_...): one_mode and
# identity reproduce the single filter bitwise; identical differs by the rounding of the
# weights and of the mixing sums.  16 times the largest, rounded up to a power of two; the
# device test compares two device results and allows RED_TOL (and 0 where the mirrors show 0).
REDUCTION_MEASURED = {"one_mode": 0.0, "identity": 0.0, "identical": 1.03e-13}
RED_TOL = 2.0 ** -39              # 16 * 1.03e-13 = 1.65e-12 <= 2^-39 = 1.82e-12


# ---------------------------------------------------------------------------
# Mode response: every lane drives straight at a constant speed for six calls and then brakes
# at 3 m/s^2 for six calls, measured through the consistency sensor, tracked with the default
# bank (straight, arc, brake).
# ---------------------------------------------------------------------------
RESP_B, RESP_NO = 16, 4
RESP_CRUISE, RESP_BRAKE = 6, 6
RESP_T = 0.4
RESP_DECEL = 3.0
RESP_SEED = 2031
RESP_HP, RESP_DT, RESP_LEAD = 6, 0.4, 0.1
# "brake" must be above "straight" within this many calls of the onset.  On the mirror with
# these 64 lanes (the host test prints the batch means per call) the mean of "straight" is
# 0.66 against 0.045 of "brake" at the last cruising call (a gap of 0.62 with a spread of 0.05
# between the lanes), and at the first braking call "brake" is at 0.9999 against less than
# 1e-4: the measured speed has dropped by 1.2 m/s against a sigma of 0.1 m/s.  Both gaps are
# many orders of magnitude above the device tolerance, so k = 1 and 64 lanes suffice.
RESP_K = 1


def response_inputs(B=RESP_B, n_obst=RESP_NO, seed=2032):
    """rows [B, nO, 7], man [B, nO, 4, 3], osense [B, nO, 3].  Call s = 0 .. 11 measures the
    snapshot at t = s RESP_T with epoch s; the braking sets in right after call 5.  Speeds of
    15 .. 20 m/s: no lane stops."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((B, n_obst, OM.NP))
    rows[..., OM.X] = rng.uniform(-20.0, 20.0, (B, n_obst))
    rows[..., OM.Y] = rng.uniform(-20.0, 20.0, (B, n_obst))
    rows[..., OM.HEADING] = rng.uniform(-3.0, 3.0, (B, n_obst))
    rows[..., OM.SPEED] = rng.uniform(15.0, 20.0, (B, n_obst))
    rows[..., OM.LENGTH], rows[..., OM.WIDTH] = 4.0, 2.0
    man = np.zeros((B, n_obst, MNM.NSEG, MNM.NF))
    man[..., 0, MNM.DUR] = (RESP_CRUISE - 1) * RESP_T
    man[..., 1, MNM.DUR] = 100.0
    man[..., 1, MNM.ACCEL] = -RESP_DECEL
    osense = np.broadcast_to(TC.CONS_SIGMA, (B, n_obst, 3)).copy()
    return rows, man, osense


def response_bank(osense):
    """The default bank of scpqp/imm.py for the sensing rows, as host arrays, and its names."""
    from scpqp import imm as IMM
    trk, sw = IMM.bank(osense, device="cpu")
    return trk.numpy(), sw.numpy(), IMM.MODES


def response_verdict(mu_mean, names):
    """mu_mean [calls, M], the batch mean of mu per call.  Returns (straight above brake at the
    last cruising call, the first braking call 1.. at which brake is above straight or None)."""
    s, b = names.index("straight"), names.index("brake")
    last = RESP_CRUISE - 1
    first = next((k for k in range(1, RESP_BRAKE + 1) if mu_mean[last + k, b] > mu_mean[last + k, s]),
                 None)
    return bool(mu_mean[last, s] > mu_mean[last, b]), first


# ---------------------------------------------------------------------------
# Consistency: ``tracker_accel_cases.consistency_inputs`` with the matched row in mode 0 alone
# alive (Pi = I, mu0 = (1, 0)); mode 1 is a mismatched row that never gets a probability.
# ---------------------------------------------------------------------------
def consistency_bank(trk14):
    trk = widen(trk14, 2)
    trk[:, :, 1, AM.Q_ACCEL] = 1.0
    B, nO = trk.shape[:2]
    sw = np.zeros((B, nO, 3, 2))
    sw[..., 0, 0] = 1.0
    sw[..., 1:, :] = np.eye(2)
    return trk, sw
