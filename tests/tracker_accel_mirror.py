"""CPU mirror of the obstacle tracker with an acceleration state
(include/scpqp_tracker_accel.h), for its tests: one tracker step of every lane in numpy with
dense 6 x 6 algebra and a hand-written 4 x 4 Cholesky.  The code is generic in the number
format: ``F64`` runs it in float64 (libm's sin and cos, as ``manoeuvre_mirror`` does, whose
``piece`` it then equals bitwise) and ``F80`` in ``numpy.longdouble``, so the difference of
the two measures the rounding the definition amplifies.  The measurement is
``tracker_mirror.measurement`` (``sensing_mirror``'s draw on ``obstacle_mirror``'s pose), the
off lanes are the untracked predictions of those mirrors.  Written from the header's
description, not from the device code."""
import math

import numpy as np

import manoeuvre_mirror as MNM
import obstacle_mirror as OM
import sensing_mirror as SM
import tracker_mirror as TM

NS = 6
NZ = 4
NP = 14
(R_POS, R_HEADING, R_SPEED, Q_POS, Q_HEADING, Q_SPEED, Q_YAW, Q_ACCEL, P0_YAW, P0_ACCEL, W_CLAMP,
 A_CLAMP, W_HOLD, A_HOLD) = range(NP)
DPR_SWITCH = 0.3
DSINC_SWITCH = TM.DSINC_SWITCH
PR_SWITCH = MNM.PR_SWITCH
SINC_SWITCH = OM.SINC_SWITCH

# the denominators of the series: p, r (scpqp_manoeuvres.h), p', r' (scpqp_tracker_accel.h)
P_DEN = (2, 8, 144, 5760, 403200, 43545600)
R_DEN = (3, 30, 840, 45360, 3991680, 518918400)
DP_DEN = (4, 36, 960, 50400, 4354560, 558835200)
DR_DEN = (3, 10, 168, 6480, 443520, 47174400)


class Format:
    """A number format: its scalar type and its sin, cos and sqrt."""

    def __init__(self, dtype, sin, cos, sqrt):
        self.dtype, self.sin, self.cos, self.sqrt = dtype, sin, cos, sqrt
        self.inf = dtype(math.inf)

    def num(self, v):
        return self.dtype(v)

    def array(self, a):
        return np.array(a, dtype=self.dtype)


F64 = Format(np.float64, lambda v: np.float64(math.sin(v)), lambda v: np.float64(math.cos(v)),
             lambda v: np.float64(math.sqrt(v)) if v >= 0 else np.float64(np.nan))
F80 = Format(np.longdouble, np.sin, np.cos, np.sqrt)


def _horner(den, t2, fm):
    one = fm.num(1)
    acc = one / fm.num(den[-1])
    for d in den[-2::-1]:
        acc = one / fm.num(d) - t2 * acc
    return acc


def p_of(th, fm=F64):
    if abs(th) < PR_SWITCH:
        return _horner(P_DEN, th * th, fm)
    return (fm.cos(th) + th * fm.sin(th) - fm.num(1)) / (th * th)


def r_of(th, fm=F64):
    if abs(th) < PR_SWITCH:
        return th * _horner(R_DEN, th * th, fm)
    return (fm.sin(th) - th * fm.cos(th)) / (th * th)


def dp_series(th, fm=F64):
    return -th * _horner(DP_DEN, th * th, fm)


def dr_series(th, fm=F64):
    return _horner(DR_DEN, th * th, fm)


def dp_closed(th, fm=F64):
    t2, two = th * th, fm.num(2)
    return (t2 * fm.cos(th) - two * th * fm.sin(th) - two * fm.cos(th) + two) / (t2 * th)


def dr_closed(th, fm=F64):
    t2, two = th * th, fm.num(2)
    return ((t2 - two) * fm.sin(th) + two * th * fm.cos(th)) / (t2 * th)


def dp_of(th, fm=F64):
    return dp_series(th, fm) if abs(th) < DPR_SWITCH else dp_closed(th, fm)


def dr_of(th, fm=F64):
    return dr_series(th, fm) if abs(th) < DPR_SWITCH else dr_closed(th, fm)


def sinc(A, fm=F64):
    return fm.num(1) - A * A / fm.num(6) if abs(A) < SINC_SWITCH else fm.sin(A) / A


def dsinc(A, fm=F64):
    """g' of scpqp_tracker.h with its switch."""
    if abs(A) < DSINC_SWITCH:
        return -A / fm.num(3) + A ** 3 / fm.num(30) - A ** 5 / fm.num(840)
    return (A * fm.cos(A) - fm.sin(A)) / (A * A)


def stop_time(s0, a, fm=F64):
    if a < 0:
        return s0 / -a
    return fm.num(0) if (a == 0 and s0 == 0) else fm.inf


def piece(q, a, w, tau, fm=F64):
    """``manoeuvre_mirror.piece`` in the format ``fm``: (x, y, h, s) after a piece of
    acceleration a and turn rate w over tau; returns (x, y, h, s)."""
    x, y, h, s = q
    stop = stop_time(s, a, fm)
    stops = tau >= stop
    T = stop if stops else tau
    th = w * T
    A = fm.num(0.5) * th
    chord = (s * T) * sinc(A, fm)
    dx, dy = chord * fm.cos(h + A), chord * fm.sin(h + A)
    if a != 0:
        p, r, aT2 = p_of(th, fm), r_of(th, fm), a * (T * T)
        dx = dx + aT2 * (p * fm.cos(h) - r * fm.sin(h))
        dy = dy + aT2 * (p * fm.sin(h) + r * fm.cos(h))
    s1 = fm.num(0) if stops else max(s + a * T, fm.num(0))
    return (x + dx, y + dy, h + th, s1)


def flow(x, T, fm=F64):
    """The estimate (x, y, h, s, w, a) after T: one piece from s0 = max(s, 0)."""
    s0 = max(x[3], fm.num(0))
    q = piece((x[0], x[1], x[2], s0), x[5], x[4], T, fm)
    return fm.array([q[0], q[1], q[2], q[3], x[4], x[5]])


def transition(x, T, fm=F64):
    """F of the header's step 1 at the estimate x, with T_e held fixed."""
    h, w, a = x[2], x[4], x[5]
    s0 = max(x[3], fm.num(0))
    stop = stop_time(s0, a, fm)
    Te = stop if T >= stop else T
    th = w * Te
    A, c = fm.num(0.5) * th, s0 * Te
    g, gp = sinc(A, fm), dsinc(A, fm)
    sa, ca, sh, ch = fm.sin(h + A), fm.cos(h + A), fm.sin(h), fm.cos(h)
    p, r, dp, dr = p_of(th, fm), r_of(th, fm), dp_of(th, fm), dr_of(th, fm)
    hT, Te2 = fm.num(0.5) * Te, Te * Te
    aT3 = a * (Te2 * Te)
    F = np.eye(NS, dtype=fm.dtype)
    F[0, 3], F[1, 3] = Te * g * ca, Te * g * sa
    F[0, 5], F[1, 5] = Te2 * (p * ch - r * sh), Te2 * (p * sh + r * ch)
    F[0, 2] = -(c * g * sa + a * F[1, 5])
    F[1, 2] = c * g * ca + a * F[0, 5]
    F[0, 4] = c * hT * (gp * ca - g * sa) + aT3 * (dp * ch - dr * sh)
    F[1, 4] = c * hT * (gp * sa + g * ca) + aT3 * (dp * sh + dr * ch)
    F[2, 4] = Te
    F[3, 5] = Te
    return F


def r_diag(row, fm=F64):
    row = fm.array(row)
    return fm.array([row[R_POS], row[R_POS], row[R_HEADING], row[R_SPEED]]) ** 2


def q_diag(row, fm=F64):
    row = fm.array(row)
    return fm.array([row[Q_POS], row[Q_POS], row[Q_HEADING], row[Q_SPEED], row[Q_YAW],
                     row[Q_ACCEL]]) ** 2


def is_off_row(row):
    return bool((np.asarray(row, float) == 0.0).all())


def is_bad_row(row):
    row = np.asarray(row, float)
    if (~np.isfinite(row)).any() or (row < 0.0).any():
        return True
    return not is_off_row(row) and bool((row[R_POS:R_SPEED + 1] == 0.0).any())


def predict(x, P, T, q, fm=F64):
    F = transition(x, T, fm)
    P = F @ P @ F.T + fm.num(T) * np.diag(q)
    return flow(x, T, fm), fm.num(0.5) * (P + P.T)


def cholesky(S, fm=F64):
    """L of S = L L' (4 x 4, any format), or None on a pivot <= 0 or not finite."""
    n = S.shape[0]
    L = np.zeros((n, n), dtype=fm.dtype)
    for j in range(n):
        d = S[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not (np.isfinite(d) and d > 0):
            return None
        L[j, j] = fm.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (S[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def _forward(L, B):
    """L^-1 B by forward substitution (B a vector or a matrix)."""
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - (L[i, :i, None] * X[:i] if B.ndim == 2 else L[i, :i] * X[:i]).sum(axis=0)) \
            / L[i, i]
    return X


def _backward(L, v):
    """L'^-1 v by back substitution."""
    n = L.shape[0]
    w = np.zeros_like(v)
    for i in range(n - 1, -1, -1):
        w[i] = (v[i] - (L[i + 1:, i] * w[i + 1:]).sum()) / L[i, i]
    return w


def update(x, P, z, r, fm=F64):
    """The measurement update with H = [I4 | 0]; (x, P, nis) or None on a bad pivot."""
    L = cholesky(P[:NZ, :NZ] + np.diag(r), fm)
    if L is None:
        return None
    y = z - x[:NZ]
    v = _forward(L, y)
    nis = (v * v).sum()
    w = _backward(L, v)
    x = x + P[:, :NZ] @ w
    W = _forward(L, P[:NZ, :])
    P = P - W.T @ W
    return x, fm.num(0.5) * (P + P.T), nis


def horizon(x, row, lead, dt, hp, fm=F64):
    """[2, hp]: the three-piece walk of the header's step 4 from the estimate x."""
    row = fm.array(row)
    zero = fm.num(0)
    wc = min(max(x[4], -row[W_CLAMP]), row[W_CLAMP])
    ac = min(max(x[5], -row[A_CLAMP]), row[A_CLAMP])
    wh, ah = row[W_HOLD], row[A_HOLD]
    t1, t2 = min(wh, ah), max(wh, ah)
    a2, w2 = (ac, zero) if ah > wh else (zero, wc)
    q0 = (x[0], x[1], x[2], max(x[3], zero))
    q1 = q2 = None                         # the boundary states, formed once, when needed
    out = np.empty((2, hp), dtype=fm.dtype)
    for k in range(hp):
        tau = fm.num((k + 1) * dt + lead)
        if tau < t1:
            q = piece(q0, ac, wc, tau, fm)
        else:
            if q1 is None:
                q1 = piece(q0, ac, wc, t1, fm)
            if tau < t2:
                q = piece(q1, a2, w2, tau - t1, fm)
            else:
                if q2 is None:
                    q2 = piece(q1, a2, w2, t2 - t1, fm)
                q = piece(q2, zero, zero, tau - t2, fm)
        out[0, k], out[1, k] = q[0], q[1]
    return out


def lane_step(trk, z, T, lead, dt, hp, x_trk, cov, untracked, fm=F64):
    """One lane: returns (x_trk [6], cov [6, 6], nis, obst [2, hp]).  ``untracked``: the
    [2, hp] block of the untracked prediction, an off lane's output."""
    nan = fm.num(np.nan)
    nan6, nan66 = np.full(NS, nan), np.full((NS, NS), nan)
    nanb = np.full((2, hp), nan)
    if is_bad_row(trk):
        return nan6, nan66, nan, nanb
    if is_off_row(trk):
        return fm.array(x_trk), fm.array(cov), nan, fm.array(untracked)
    if np.isnan(np.asarray(z, float)).any():
        return nan6, nan66, nan, nanb
    x, P, z = fm.array(x_trk), fm.array(cov), fm.array(z)
    trk = fm.array(trk)
    nis = nan
    if np.isnan(x[0]):
        x = np.concatenate([z, fm.array([0, 0])])
        P = np.diag(np.concatenate([r_diag(trk, fm), fm.array([trk[P0_YAW], trk[P0_ACCEL]]) ** 2]))
    else:
        P = np.triu(P) + np.triu(P, 1).T                    # only the upper triangle is read
        with np.errstate(all="ignore"):
            x, P = predict(x, P, T, q_diag(trk, fm), fm)
            res = update(x, P, z, r_diag(trk, fm), fm)
        if res is None or not np.isfinite(res[2]):
            return nan6, nan66, nan, nanb
        x, P, nis = res
    if not (np.isfinite(x).all() and np.isfinite(P).all()):
        return nan6, nan66, nan, nanb
    return x, P, nis, horizon(x, trk, lead, dt, hp, fm)


def step(rows, osense, seed, epoch, b_offset, trk, t_meas, t_since, lead, dt, hp, x_trk, cov,
         fm=F64):
    """The mirror of scpqp_obstacles_track_accel: rows [B, nO, 7], osense [B, nO, 3] or None,
    trk [B, nO, 14]; x_trk [B, nO, 6] and cov [B, nO, 6, 6] (arrays of ``fm.dtype``) are
    updated in place.  Returns (obst [B, nO, 2, hp], z [B, nO, 4], nis [B, nO]); z is the
    float64 measurement in every format."""
    rows, trk = np.asarray(rows, float), np.asarray(trk, float)
    B, nO = rows.shape[:2]
    # the untracked prediction: only an off lane shows it
    if not any(is_off_row(r) for r in trk.reshape(-1, NP)):
        base = np.full((B, nO, 2, hp), np.nan)
    elif osense is None:
        base = OM.predict(rows, t_meas, lead, dt, hp)
    else:
        base = SM.predict_sensed(rows, osense, seed, epoch, b_offset, t_meas, lead, dt, hp)
    obst = np.empty((B, nO, 2, hp), dtype=fm.dtype)
    z = np.empty((B, nO, NZ))
    nis = np.full((B, nO), np.nan, dtype=fm.dtype)
    for b in range(B):
        for o in range(nO):
            z[b, o] = TM.measurement(rows[b, o], None if osense is None else osense[b, o], seed,
                                     epoch, o, b_offset + b, t_meas)
            x_trk[b, o], cov[b, o], nis[b, o], obst[b, o] = lane_step(
                trk[b, o], z[b, o], fm.num(t_since), lead, dt, hp, x_trk[b, o], cov[b, o],
                base[b, o], fm)
    return obst, z, nis


def alloc(B, nO, fm=F64):
    return np.full((B, nO, NS), np.nan, dtype=fm.dtype), np.zeros((B, nO, NS, NS), dtype=fm.dtype)


def widen(trk5, w_hold=1e3, a_hold=1e3, a_clamp=6.0):
    """Rows of scpqp_tracker.h [..., 9] as rows of this tracker with P0_ACCEL = Q_ACCEL = 0
    and the holds beyond any horizon: the reduction to the five-state tracker."""
    trk5 = np.asarray(trk5, float)
    out = np.zeros(trk5.shape[:-1] + (NP,))
    out[..., :Q_ACCEL] = trk5[..., :TM.P0_YAW]
    out[..., P0_YAW] = trk5[..., TM.P0_YAW]
    out[..., W_CLAMP] = trk5[..., TM.W_CLAMP]
    on = (trk5 != 0).any(axis=-1)
    out[on, A_CLAMP], out[on, W_HOLD], out[on, A_HOLD] = a_clamp, w_hold, a_hold
    return out
