"""CPU mirror of the interacting-multiple-model obstacle tracker (include/scpqp_imm.h), for its
tests: one step of every lane's bank in dense numpy, generic in the number format (``F64``,
``F80`` of ``tracker_accel_mirror``).  Every mode is ``tracker_accel_mirror``'s ``predict``,
``update`` and ``horizon`` with its ``cholesky`` for the likelihood and its bad and off rules
for the rows; the mixing, the probabilities and the weighted outputs are written here from the
header's description, not from the device code."""
import math

import numpy as np

import obstacle_mirror as OM
import sensing_mirror as SM
import tracker_accel_mirror as AM
import tracker_mirror as TM

NS, NZ, NP = AM.NS, AM.NZ, AM.NP
MAX_MODES = 4
SUM_TOL = 1e-12
F64, F80 = AM.F64, AM.F80


def _exp(v, fm):
    return np.exp(v) if fm.dtype is np.longdouble else np.float64(math.exp(v))


def _log(v, fm):
    return np.log(v) if fm.dtype is np.longdouble else np.float64(math.log(v))


def is_off_lane(trk):
    return all(AM.is_off_row(r) for r in trk)


def ordered_sum(v):
    s = 0.0
    for a in v:
        s = s + a
    return s


def bad_sw(sw):
    sw = np.asarray(sw, float)
    if (~np.isfinite(sw)).any() or (sw < 0.0).any():
        return True
    return any(not abs(ordered_sum(row) - 1.0) <= SUM_TOL for row in sw)


def is_bad_lane(trk, sw):
    """The bad rule of the header, of a lane that is not off."""
    if any(AM.is_bad_row(r) for r in trk):
        return True
    if any(AM.is_off_row(r) for r in trk):
        return True                                  # off and non-off rows mixed
    return bad_sw(sw)


def mix(x, P, mu, Pi, fm=F64):
    """Step 2: (c [M], x0 [M, 6], P0 [M, 6, 6]) from the modes' states and probabilities."""
    M = len(mu)
    zero, one = fm.num(0), fm.num(1)
    c = np.zeros(M, dtype=fm.dtype)
    x0 = np.zeros((M, NS), dtype=fm.dtype)
    P0 = np.zeros((M, NS, NS), dtype=fm.dtype)
    for j in range(M):
        t = [Pi[i, j] * mu[i] for i in range(M)]
        for i in range(M):
            c[j] = c[j] + t[i]
        w = [(one if i == j else zero) if c[j] == 0 else t[i] / c[j] for i in range(M)]
        for i in range(M):
            if w[i] != 0:
                x0[j] = x0[j] + w[i] * x[i]
        for i in range(M):
            if w[i] != 0:
                d = x[i] - x0[j]
                P0[j] = P0[j] + w[i] * (P[i] + np.outer(d, d))
        P0[j] = fm.num(0.5) * (P0[j] + P0[j].T)
    return c, x0, P0


def log_likelihood(nis, L, fm=F64):
    """l = -nis / 2 - sum_k log L_kk."""
    s = fm.num(0)
    for k in range(L.shape[0]):
        s = s + _log(L[k, k], fm)
    return -fm.num(0.5) * nis - s


def probabilities(c, l, fm=F64):
    """Step 4: mu_j = c_j exp(l_j - max l) / sum over the modes with c_j > 0; the others 0."""
    M = len(c)
    alive = [j for j in range(M) if c[j] > 0]
    mu = np.zeros(M, dtype=fm.dtype)
    if not alive:
        return np.full(M, fm.num(np.nan))
    mx = max(l[j] for j in alive)
    e = {j: c[j] * _exp(l[j] - mx, fm) for j in alive}
    s = fm.num(0)
    for j in alive:
        s = s + e[j]
    for j in alive:
        mu[j] = e[j] / s
    return mu


def weighted(mu, vals, fm=F64):
    """sum_j mu_j vals[j] in mode order from 0, the modes with mu_j == 0 skipped."""
    acc = np.zeros(np.shape(vals[0]), dtype=fm.dtype)
    for j in range(len(mu)):
        if mu[j] != 0:
            acc = acc + mu[j] * vals[j]
    return acc


def lane_step(trk, sw, z, T, lead, dt, hp, x_imm, cov, mu, untracked, fm=F64):
    """One lane: returns (x_imm [M, 6], cov [M, 6, 6], mu [M], x_hat [6], nis [M],
    obst [2, hp])."""
    M = trk.shape[0]
    nan = fm.num(np.nan)
    lost = (np.full((M, NS), nan), np.full((M, NS, NS), nan), np.full(M, nan), np.full(NS, nan),
            np.full(M, nan), np.full((2, hp), nan))
    if is_off_lane(trk):
        return (fm.array(x_imm), fm.array(cov), fm.array(mu), np.full(NS, nan), np.full(M, nan),
                fm.array(untracked))
    if is_bad_lane(trk, sw) or np.isnan(np.asarray(z, float)).any():
        return lost
    x, P, mu, z = fm.array(x_imm), fm.array(cov), fm.array(mu), fm.array(z)
    trk, sw = fm.array(trk), fm.array(sw)
    nis = np.full(M, nan)
    if np.isnan(x[0, 0]):
        for j in range(M):
            x[j] = np.concatenate([z, fm.array([0, 0])])
            P[j] = np.diag(np.concatenate([AM.r_diag(trk[j], fm),
                                           fm.array([trk[j, AM.P0_YAW], trk[j, AM.P0_ACCEL]]) ** 2]))
        mu = sw[0].copy()
    else:
        for j in range(M):
            P[j] = np.triu(P[j]) + np.triu(P[j], 1).T       # only the upper triangles are read
        with np.errstate(all="ignore"):
            if T > 0:
                c, x, P = mix(x, P, mu, sw[1:], fm)
            else:
                c = mu.copy()
            l = np.zeros(M, dtype=fm.dtype)
            for j in range(M):
                xj, Pj = AM.predict(x[j], P[j], T, AM.q_diag(trk[j], fm), fm)
                r = AM.r_diag(trk[j], fm)
                L = AM.cholesky(Pj[:NZ, :NZ] + np.diag(r), fm)
                res = AM.update(xj, Pj, z, r, fm)
                if L is None or res is None or not np.isfinite(res[2]):
                    return lost
                x[j], P[j], nis[j] = res
                l[j] = log_likelihood(nis[j], L, fm)
            mu = probabilities(c, l, fm)
    if not (np.isfinite(x).all() and np.isfinite(P).all() and np.isfinite(mu).all()):
        return lost
    pts = [AM.horizon(x[j], trk[j], lead, dt, hp, fm) for j in range(M)]
    return x, P, mu, weighted(mu, x, fm), nis, weighted(mu, pts, fm)


def step(rows, osense, seed, epoch, b_offset, trk, sw, t_meas, t_since, lead, dt, hp, x_imm, cov,
         mu, fm=F64):
    """The mirror of scpqp_obstacles_track_imm: rows [B, nO, 7], osense [B, nO, 3] or None, trk
    [B, nO, M, 14], sw [B, nO, M + 1, M]; x_imm [B, nO, M, 6], cov [B, nO, M, 6, 6] and mu
    [B, nO, M] (arrays of ``fm.dtype``) are updated in place.  Returns (obst [B, nO, 2, hp],
    x_hat [B, nO, 6], z [B, nO, 4], nis [B, nO, M]); z is the float64 measurement."""
    rows, trk, sw = np.asarray(rows, float), np.asarray(trk, float), np.asarray(sw, float)
    B, nO, M = trk.shape[:3]
    if not any(is_off_lane(t) for t in trk.reshape(-1, M, NP)):
        base = np.full((B, nO, 2, hp), np.nan)
    elif osense is None:
        base = OM.predict(rows, t_meas, lead, dt, hp)
    else:
        base = SM.predict_sensed(rows, osense, seed, epoch, b_offset, t_meas, lead, dt, hp)
    obst = np.empty((B, nO, 2, hp), dtype=fm.dtype)
    x_hat = np.empty((B, nO, NS), dtype=fm.dtype)
    z = np.empty((B, nO, NZ))
    nis = np.empty((B, nO, M), dtype=fm.dtype)
    for b in range(B):
        for o in range(nO):
            z[b, o] = TM.measurement(rows[b, o], None if osense is None else osense[b, o], seed,
                                     epoch, o, b_offset + b, t_meas)
            (x_imm[b, o], cov[b, o], mu[b, o], x_hat[b, o], nis[b, o], obst[b, o]) = lane_step(
                trk[b, o], sw[b, o], z[b, o], fm.num(t_since), lead, dt, hp, x_imm[b, o],
                cov[b, o], mu[b, o], base[b, o], fm)
    return obst, x_hat, z, nis


def alloc(B, nO, M, fm=F64):
    return (np.full((B, nO, M, NS), np.nan, dtype=fm.dtype),
            np.zeros((B, nO, M, NS, NS), dtype=fm.dtype), np.zeros((B, nO, M), dtype=fm.dtype))
