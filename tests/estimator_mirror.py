"""CPU mirror of the state estimator (include/scpqp_estimator.h), for the estimator tests:
one filter step of every lane in plain fp64 numpy with dense 5 x 5 algebra and
``numpy.linalg.cholesky``.  The Jacobian, the right-hand side and the RK4 flow are the
oracle's own (``oracle.scp_reference.bicycle_jacobian`` / ``bicycle_rhs`` through
``oracle.plant_reference._rk4_flow`` / ``_rk4_steps``); nothing of them is restated here.
Written from the header's description, not from the device code."""
import numpy as np

from oracle import plant_reference as PR
from oracle.scp_reference import bicycle_jacobian, bicycle_rhs

NS = 5
NP = 8
R_POS, R_HEADING, R_SPEED, R_STEER, Q_POS, Q_HEADING, Q_SPEED, Q_STEER = range(NP)
IDX = np.array([0, 1, 2, 3, 5])          # the filtered states of the model's six
H_MAX = PR.H_MAX


def r_diag(row):
    return np.array([row[R_POS], row[R_POS], row[R_HEADING], row[R_SPEED], row[R_STEER]]) ** 2


def q_diag(row):
    return np.array([row[Q_POS], row[Q_POS], row[Q_HEADING], row[Q_SPEED], row[Q_STEER]]) ** 2


def is_off_row(row):
    return bool((np.asarray(row, float) == 0.0).all())


def is_bad_row(row):
    row = np.asarray(row, float)
    if (~np.isfinite(row)).any() or (row < 0.0).any():
        return True
    return not is_off_row(row) and bool((row[R_POS:R_STEER + 1] == 0.0).any())


def jacobian5(x, lf, lr):
    """A: Model.py:46-52 at x, restricted to the five filtered states."""
    Ac = bicycle_jacobian(np.asarray(x, float), 0.0, lf, lr)[0]
    return Ac[np.ix_(IDX, IDX)]


def rhs5(x, u, lf, lr):
    """The right-hand side of the five filtered states (the flow's own, for checks of A)."""
    return bicycle_rhs(np.asarray(x, float), float(u), lf, lr)[IDX]


def transition(x, lf, lr, T):
    """F = I + T A + T^2/2 A A."""
    A = jacobian5(x, lf, lr)
    return np.eye(NS) + T * A + (0.5 * T * T) * (A @ A)


def predict(x, P, u_span, lf, lr, tick, q, h_max=H_MAX):
    """The ticks of u_span from (x [6], P [5, 5]); returns the new pair."""
    x, P = np.array(x, float), np.array(P, float)
    n = PR._rk4_steps(tick, h_max)
    for u in u_span:
        F = transition(x, lf, lr, tick)
        x = PR._rk4_flow(x, tick, float(u), lf, lr, n)
        P = F @ P @ F.T + tick * np.diag(q)
        P = 0.5 * (P + P.T)
    return x, P


def update(x, P, m, r):
    """The measurement update with H = I; returns (x, P, nis) or None on a bad pivot."""
    S = P + np.diag(r)
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(L).all() or (np.diag(L) <= 0.0).any():
        return None
    y = m[IDX] - x[IDX]
    z = np.linalg.solve(L, y)
    nis = float(z @ z)
    w = np.linalg.solve(L.T, z)
    x = x.copy()
    x[IDX] = x[IDX] + P @ w
    W = np.linalg.solve(L, P)
    P = P - W.T @ W
    P = 0.5 * (P + P.T)
    x[4] = m[4]
    return x, P, nis


def lane_step(row, lf, lr, tick, u_span, m, delivered, x_est, cov, h_max=H_MAX):
    """One lane: returns (x_est [6], cov [5, 5], nis)."""
    nan6, nan55 = np.full(6, np.nan), np.full((NS, NS), np.nan)
    m = np.asarray(m, float)
    if is_bad_row(row):
        return nan6, nan55, np.nan
    if is_off_row(row):
        return m.copy(), np.array(cov, float), np.nan
    x, P = np.array(x_est, float), np.array(cov, float)
    init = not np.isnan(x[0])
    if init:
        x, P = predict(x, P, u_span, lf, lr, tick, q_diag(row), h_max)
    counts = bool(delivered) and bool(np.isfinite(m).all())
    nis = np.nan
    if counts and not init:
        x, P = m.copy(), np.diag(r_diag(row))
    elif counts:
        res = update(x, P, m, r_diag(row))
        if res is None:
            return nan6, nan55, np.nan
        x, P, nis = res
        if not np.isfinite(nis):
            return nan6, nan55, np.nan
    elif not init:
        return nan6, np.array(cov, float), np.nan
    if not (np.isfinite(x).all() and np.isfinite(P).all()):
        return nan6, nan55, np.nan
    return x, P, nis


def step(lf, lr, tick, u_span, x_meas, delivered, rows, x_est, cov, h_max=H_MAX):
    """The mirror of scpqp_est_step: u_span [B, V, n_span] or None, x_meas [B, V, 6],
    delivered [B, V] or None, rows [B, V, 8]; x_est [B, V, 6] and cov [B, V, 5, 5] are
    updated in place.  Returns nis [B, V]."""
    B, V = rows.shape[:2]
    nis = np.full((B, V), np.nan)
    for b in range(B):
        for v in range(V):
            us = () if u_span is None else u_span[b, v]
            d = 1 if delivered is None else int(delivered[b, v]) == 1
            x_est[b, v], cov[b, v], nis[b, v] = lane_step(
                rows[b, v], lf[v], lr[v], tick, us, x_meas[b, v], d, x_est[b, v], cov[b, v], h_max)
    return nis


# ---------------------------------------------------------------------------
# The inputs of the consistency test, shared by the CPU and the GPU version: one gently
# turning truth path, measured once per step by every lane with its own seeded noise.
# ---------------------------------------------------------------------------
CONS_TICK = 0.01
CONS_STEPS, CONS_SPAN = 6, 8
CONS_SIGMA = np.array([0.05, 0.05, 0.01, 0.1, 0.002])     # x, y, heading, speed, steering
CONS_LF = CONS_LR = 0.34
CONS_X0 = np.array([1.0, -2.0, 0.3, 4.0, 0.0, 0.02])


def consistency_inputs(n_lanes, seed=2024):
    """truth [STEPS + 1, 6] (the state at the measured ticks 0, 8, .., 48), u [STEPS, SPAN]
    (the command of every tick, u = 0.03 sin(0.2 j) at global tick j = 1..48), meas
    [STEPS + 1, n_lanes, 6] (truth plus N(0, CONS_SIGMA^2) on the five filtered states) and
    the rows [n_lanes, 8]: R equal to the sigmas, Q = 0."""
    n = PR._rk4_steps(CONS_TICK)
    u = np.array([[0.03 * np.sin(0.2 * (s * CONS_SPAN + k + 1)) for k in range(CONS_SPAN)]
                  for s in range(CONS_STEPS)])
    truth = [CONS_X0.copy()]
    for s in range(CONS_STEPS):
        x = truth[-1]
        for k in range(CONS_SPAN):
            x = PR._rk4_flow(x, CONS_TICK, float(u[s, k]), CONS_LF, CONS_LR, n)
        truth.append(x)
    truth = np.array(truth)
    rng = np.random.default_rng(seed)
    meas = np.repeat(truth[:, None, :], n_lanes, axis=1)
    meas[:, :, IDX] += rng.standard_normal((CONS_STEPS + 1, n_lanes, NS)) * CONS_SIGMA
    rows = np.zeros((n_lanes, NP))
    rows[:, R_POS], rows[:, R_HEADING] = CONS_SIGMA[0], CONS_SIGMA[2]
    rows[:, R_SPEED], rows[:, R_STEER] = CONS_SIGMA[3], CONS_SIGMA[4]
    return truth, u, meas, rows


def consistency_verdict(nis, x_final, truth_final, meas_final):
    """(mean NIS, its bound around 5, RMS position error of the estimate, of the measurement).
    nis: every innovation of the run (CONS_STEPS per lane).  The mean of N chi^2_5 variables
    has standard deviation sqrt(10 / N): the bound is five of them."""
    nis = np.asarray(nis, float).reshape(-1)
    bound = 5.0 * np.sqrt(10.0 / nis.size)
    rms = lambda a: float(np.sqrt(((a[:, 0:2] - truth_final[0:2]) ** 2).sum(axis=1).mean()))
    return float(nis.mean()), float(bound), rms(np.asarray(x_final)), rms(np.asarray(meas_final))
