"""CPU mirror of the obstacle tracker (include/scpqp_tracker.h), for the tracker tests: one
tracker step of every lane in plain fp64 numpy with dense 5 x 5 algebra and
``numpy.linalg.cholesky``.  The flow and the horizon are ``obstacle_mirror.pose``, the
measurement is ``sensing_mirror``'s draw on that pose; nothing of them is restated here.
Written from the header's description, not from the device code."""
import math

import numpy as np

import obstacle_mirror as OM
import sensing_mirror as SM

NS = 5
NZ = 4
NP = 9
R_POS, R_HEADING, R_SPEED, Q_POS, Q_HEADING, Q_SPEED, Q_YAW, P0_YAW, W_CLAMP = range(NP)
DSINC_SWITCH = 0.02


def r_diag(row):
    return np.array([row[R_POS], row[R_POS], row[R_HEADING], row[R_SPEED]]) ** 2


def q_diag(row):
    return np.array([row[Q_POS], row[Q_POS], row[Q_HEADING], row[Q_SPEED], row[Q_YAW]]) ** 2


def is_off_row(row):
    return bool((np.asarray(row, float) == 0.0).all())


def is_bad_row(row):
    row = np.asarray(row, float)
    if (~np.isfinite(row)).any() or (row < 0.0).any():
        return True
    return not is_off_row(row) and bool((row[R_POS:R_SPEED + 1] == 0.0).any())


def dsinc_series(a):
    return -a / 3 + a ** 3 / 30 - a ** 5 / 840


def dsinc_closed(a):
    return (a * math.cos(a) - math.sin(a)) / (a * a)


def dsinc(a):
    """g'(a), the derivative of sin(a) / a, with the header's switch."""
    return dsinc_series(a) if abs(a) < DSINC_SWITCH else dsinc_closed(a)


def flow(x, T):
    """The estimate (x, y, h, s, w) after T on the obstacle truth's own flow."""
    px, py, ph = OM.pose((x[0], x[1], x[2], x[3], 0.0, 0.0, x[4]), T)
    return np.array([px, py, ph, x[3], x[4]])


def transition(x, T):
    """F of the header's step 1 at the estimate x."""
    h, s, w = float(x[2]), float(x[3]), float(x[4])
    a, c = 0.5 * w * T, s * T
    g, gp = OM.sinc(a), dsinc(a)
    sa, ca = math.sin(h + a), math.cos(h + a)
    F = np.eye(NS)
    F[0, 2], F[0, 3] = -c * g * sa, T * g * ca
    F[0, 4] = c * (T / 2) * (gp * ca - g * sa)
    F[1, 2], F[1, 3] = c * g * ca, T * g * sa
    F[1, 4] = c * (T / 2) * (gp * sa + g * ca)
    F[2, 4] = T
    return F


def predict(x, P, T, q):
    F = transition(x, T)
    P = F @ P @ F.T + T * np.diag(q)
    return flow(x, T), 0.5 * (P + P.T)


def update(x, P, z, r):
    """The measurement update with H = [I4 | 0]; (x, P, nis) or None on a bad pivot."""
    S = P[:NZ, :NZ] + np.diag(r)
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(L).all() or (np.diag(L) <= 0.0).any():
        return None
    y = z - x[:NZ]
    v = np.linalg.solve(L, y)
    nis = float(v @ v)
    w = np.linalg.solve(L.T, v)
    x = x + P[:, :NZ] @ w
    W = np.linalg.solve(L, P[:NZ, :])
    P = P - W.T @ W
    return x, 0.5 * (P + P.T), nis


def measurement(row, osense, seed, epoch, o, b_global, t_meas):
    """z [4] of one lane, or NaN when the obstacle row or the osense row is bad."""
    if OM.bad_row(row) or (osense is not None and SM.bad_osense_row(osense)):
        return np.full(NZ, np.nan)
    x, y, h = OM.pose(row, t_meas)
    s = float(row[OM.SPEED])
    if osense is None or not np.asarray(osense).any():
        return np.array([x, y, h, s])
    sp, sh, ss = (float(v) for v in osense)
    z0, z1, _ = SM.call(seed, 0, epoch, SM.SITE_SENSE_OBST, o, b_global)
    w0, w1, _ = SM.call(seed, 1, epoch, SM.SITE_SENSE_OBST, o, b_global)
    return np.array([x + sp * z0, y + sp * z1, h + sh * w0, s + ss * w1])


def horizon(x, w_clamp, lead, dt, hp):
    """[2, hp]: x, y of the estimate's flow with w clamped, at (k + 1) dt + lead."""
    wc = min(max(float(x[4]), -w_clamp), w_clamp)
    out = np.empty((2, hp))
    for k in range(hp):
        px, py, _ = OM.pose((x[0], x[1], x[2], x[3], 0.0, 0.0, wc), (k + 1) * dt + lead)
        out[0, k], out[1, k] = px, py
    return out


def straight(z, lead, dt, hp):
    """[2, hp]: the straight extrapolation of one measurement (scpqp_sensing.h)."""
    out = np.empty((2, hp))
    for k in range(hp):
        step = ((k + 1) * dt + lead) * z[3]
        out[0, k] = step * math.cos(z[2]) + z[0]
        out[1, k] = step * math.sin(z[2]) + z[1]
    return out


def lane_step(trk, z, T, lead, dt, hp, x_trk, cov, untracked):
    """One lane: returns (x_trk [5], cov [5, 5], nis, obst [2, hp]).  ``untracked``: the
    [2, hp] block of the untracked prediction, an off lane's output."""
    nan5, nan55, nanb = np.full(NS, np.nan), np.full((NS, NS), np.nan), np.full((2, hp), np.nan)
    if is_bad_row(trk):
        return nan5, nan55, np.nan, nanb
    if is_off_row(trk):
        return np.array(x_trk, float), np.array(cov, float), np.nan, np.array(untracked, float)
    if np.isnan(z).any():
        return nan5, nan55, np.nan, nanb
    x, P = np.array(x_trk, float), np.array(cov, float)
    nis = np.nan
    if np.isnan(x[0]):
        x = np.append(z, 0.0)
        P = np.diag(np.append(r_diag(trk), trk[P0_YAW] ** 2))
    else:
        P = np.triu(P) + np.triu(P, 1).T                    # only the upper triangle is read
        x, P = predict(x, P, T, q_diag(trk))
        res = update(x, P, z, r_diag(trk))
        if res is None or not np.isfinite(res[2]):
            return nan5, nan55, np.nan, nanb
        x, P, nis = res
    if not (np.isfinite(x).all() and np.isfinite(P).all()):
        return nan5, nan55, np.nan, nanb
    return x, P, nis, horizon(x, float(trk[W_CLAMP]), lead, dt, hp)


def step(rows, osense, seed, epoch, b_offset, trk, t_meas, t_since, lead, dt, hp, x_trk, cov):
    """The mirror of scpqp_obstacles_track: rows [B, nO, 7], osense [B, nO, 3] or None, trk
    [B, nO, 9]; x_trk [B, nO, 5] and cov [B, nO, 5, 5] are updated in place.  Returns
    (obst [B, nO, 2, hp], z [B, nO, 4], nis [B, nO])."""
    rows, trk = np.asarray(rows, float), np.asarray(trk, float)
    B, nO = rows.shape[:2]
    # the untracked prediction: only an off lane shows it
    if not any(is_off_row(r) for r in trk.reshape(-1, NP)):
        base = np.full((B, nO, 2, hp), np.nan)
    elif osense is None:
        base = OM.predict(rows, t_meas, lead, dt, hp)
    else:
        base = SM.predict_sensed(rows, osense, seed, epoch, b_offset, t_meas, lead, dt, hp)
    obst = np.empty((B, nO, 2, hp))
    z = np.empty((B, nO, NZ))
    nis = np.full((B, nO), np.nan)
    for b in range(B):
        for o in range(nO):
            z[b, o] = measurement(rows[b, o], None if osense is None else osense[b, o], seed,
                                  epoch, o, b_offset + b, t_meas)
            x_trk[b, o], cov[b, o], nis[b, o], obst[b, o] = lane_step(
                trk[b, o], z[b, o], t_since, lead, dt, hp, x_trk[b, o], cov[b, o], base[b, o])
    return obst, z, nis


# ---------------------------------------------------------------------------
# The inputs of the consistency test, shared by the CPU and the GPU version: turning
# obstacles, measured once per step through a noisy obstacle sensor, tracked with R equal to
# the sensor's sigmas, Q = 0 and P0_YAW equal to the sigma the turn rates were drawn with.
# ---------------------------------------------------------------------------
CONS_B, CONS_NO = 250, 6
CONS_STEPS, CONS_T = 12, 0.4
CONS_SIGMA = np.array([0.05, 0.01, 0.1])                  # position, heading, speed
CONS_YAW_SIGMA = 0.3
CONS_SEED = 2025
CONS_HP, CONS_DT, CONS_LEAD = 6, 0.4, 0.1                  # the horizon ends 2.5 s ahead


def consistency_inputs(B=CONS_B, n_obst=CONS_NO, seed=2024):
    """rows [B, nO, 7] (turn rates N(0, CONS_YAW_SIGMA^2)), osense [B, nO, 3] (CONS_SIGMA)
    and the tracker rows [B, nO, 9].  Step s = 0 .. CONS_STEPS measures at t = s CONS_T with
    epoch s and the sensing seed CONS_SEED; the first step initialises."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((B, n_obst, OM.NP))
    rows[..., OM.X] = rng.uniform(-20.0, 20.0, (B, n_obst))
    rows[..., OM.Y] = rng.uniform(-20.0, 20.0, (B, n_obst))
    rows[..., OM.HEADING] = rng.uniform(-3.0, 3.0, (B, n_obst))
    rows[..., OM.SPEED] = rng.uniform(1.0, 4.0, (B, n_obst))
    rows[..., OM.LENGTH], rows[..., OM.WIDTH] = 4.0, 2.0
    rows[..., OM.YAW_RATE] = CONS_YAW_SIGMA * rng.standard_normal((B, n_obst))
    osense = np.broadcast_to(CONS_SIGMA, (B, n_obst, 3)).copy()
    trk = np.zeros((B, n_obst, NP))
    trk[..., R_POS], trk[..., R_HEADING], trk[..., R_SPEED] = CONS_SIGMA
    trk[..., P0_YAW] = CONS_YAW_SIGMA
    trk[..., W_CLAMP] = 10.0
    return rows, osense, trk


def consistency_verdict(nis, obst_final, z_final, rows, t_final):
    """(mean NIS, its bound around 4, RMS error at the end of the horizon of the tracked
    prediction, of the straight extrapolation of the last measurement).  nis: every
    innovation of the run (CONS_STEPS per lane).  The mean of N chi^2_4 variables has
    standard deviation sqrt(8 / N): the bound is five of them."""
    nis = np.asarray(nis, float).reshape(-1)
    bound = 5.0 * np.sqrt(8.0 / nis.size)
    rows = np.asarray(rows, float).reshape(-1, OM.NP)
    ob = np.asarray(obst_final, float).reshape(len(rows), 2, -1)
    zf = np.asarray(z_final, float).reshape(len(rows), NZ)
    hp = ob.shape[2]
    tau = hp * CONS_DT + CONS_LEAD
    true = np.array([OM.pose(r, t_final + tau)[:2] for r in rows])
    line = np.array([straight(z, CONS_LEAD, CONS_DT, hp)[:, -1] for z in zf])
    rms = lambda a: float(np.sqrt(((a - true) ** 2).sum(axis=1).mean()))
    return float(nis.mean()), float(bound), rms(ob[:, :, -1]), rms(line)
