"""CPU mirror of the obstacle margin step (include/scpqp_margin.h), for its tests: numpy,
generic in the number format (``F64``, ``F80`` of ``tracker_accel_mirror``), built on
``tracker_accel_mirror.horizon`` and ``cholesky`` and ``imm_mirror.weighted``.  Written from the
header's description, not from the device code."""
import math

import numpy as np

import imm_mirror as IM
import tracker_accel_mirror as AM

NS, NP = AM.NS, AM.NP
F64, F80 = AM.F64, AM.F80


def kappa_for(p_miss):
    return math.sqrt(-2.0 * math.log(p_miss))


def mode_moment(x, P, row, lead, dt, hp, fm=F64):
    """(c [2, hp], S [hp, 3]) of one mode, or None on a bad Cholesky pivot: the nominal points
    and the second moment (Sxx, Sxy, Syy) of the twelve sigma points about them, plus
    tau Q_POS^2 on the diagonal."""
    L = AM.cholesky(P, fm)
    if L is None:
        return None
    root6 = fm.sqrt(fm.num(6))
    c = AM.horizon(x, row, lead, dt, hp, fm)
    acc = np.zeros((hp, 3), dtype=fm.dtype)
    for i in range(NS):
        for sign in (1, -1):
            e = AM.horizon(x + fm.num(sign) * root6 * L[:, i], row, lead, dt, hp, fm) - c
            acc[:, 0] += e[0] * e[0]
            acc[:, 1] += e[0] * e[1]
            acc[:, 2] += e[1] * e[1]
    S = acc / fm.num(12)
    q2 = fm.num(row[AM.Q_POS]) * fm.num(row[AM.Q_POS])
    for k in range(hp):
        tau = fm.num((k + 1) * dt + lead)
        S[k, 0] += tau * q2
        S[k, 2] += tau * q2
    return c, S


def largest_eigenvalue(S, fm=F64):
    """lam [hp] of S [hp, 3] = Sxx, Sxy, Syy."""
    half = fm.num(0.5)
    return half * (S[:, 0] + S[:, 2]) + np.hypot(half * (S[:, 0] - S[:, 2]), S[:, 1])


def lane(trk, x, P, mu, lead, dt, hp, kappa, m_max, fm=F64):
    """One lane: trk [M, 14], x [M, 6], P [M, 6, 6], mu [M] or None (M = 1: 1).  Returns
    (margin [hp], Sigma [hp, 3])."""
    trk = np.asarray(trk, float)
    M = trk.shape[0]
    zero = (np.zeros(hp, dtype=fm.dtype), np.zeros((hp, 3), dtype=fm.dtype))
    nan = (np.full(hp, fm.num(np.nan)), np.full((hp, 3), fm.num(np.nan)))
    if IM.is_off_lane(trk):
        return zero
    if any(AM.is_bad_row(r) or AM.is_off_row(r) for r in trk):
        return nan
    x, P = fm.array(x), fm.array(P)
    mu = np.ones(1, dtype=fm.dtype) if mu is None else fm.array(mu)
    P = np.stack([np.triu(p) + np.triu(p, 1).T for p in P])     # the upper triangles are read
    if np.isnan(x[0, 0]) or not (np.isfinite(x).all() and np.isfinite(P).all()
                                 and np.isfinite(mu).all()):
        return nan
    if (mu < 0).any() or not (mu > 0).any():
        return nan
    cs, Ss = [], []
    with np.errstate(all="ignore"):
        for j in range(M):
            if mu[j] > 0:
                res = mode_moment(x[j], P[j], fm.array(trk[j]), lead, dt, hp, fm)
                if res is None:
                    return nan
            else:
                res = (np.zeros((2, hp), dtype=fm.dtype), np.zeros((hp, 3), dtype=fm.dtype))
            cs.append(res[0])
            Ss.append(res[1])
        cbar = IM.weighted(mu, cs, fm)
        full = []
        for j in range(M):
            d = cs[j] - cbar
            full.append(Ss[j] + np.stack([d[0] * d[0], d[0] * d[1], d[1] * d[1]], axis=1))
        Sigma = IM.weighted(mu, full, fm)
        lam = largest_eigenvalue(Sigma, fm)
        if not np.isfinite(lam).all():
            bad = ~np.isfinite(lam)
            margin = np.minimum(fm.num(kappa) * np.sqrt(np.where(bad, 0, lam)), fm.num(m_max))
            margin[bad] = np.nan
            Sigma = Sigma.copy()
            Sigma[bad] = np.nan
            return margin, Sigma
        margin = np.minimum(fm.num(kappa) * np.sqrt(lam), fm.num(m_max))
    return margin, Sigma


def step(trk, x, cov, mu, lead, dt, hp, kappa, m_max, fm=F64):
    """The mirror of scpqp_obstacles_margin: trk [B, nO, M, 14] (or [B, nO, 14]: M = 1), x, cov,
    mu likewise.  Returns (margin [B, nO, hp], Sigma [B, nO, hp, 3])."""
    trk = np.asarray(trk, float)
    if trk.ndim == 3:
        trk, x, cov = trk[:, :, None], np.asarray(x)[:, :, None], np.asarray(cov)[:, :, None]
    B, nO = trk.shape[:2]
    margin = np.empty((B, nO, hp), dtype=fm.dtype)
    Sigma = np.empty((B, nO, hp, 3), dtype=fm.dtype)
    for b in range(B):
        for o in range(nO):
            margin[b, o], Sigma[b, o] = lane(trk[b, o], x[b, o], cov[b, o],
                                             None if mu is None else mu[b, o], lead, dt, hp,
                                             kappa, m_max, fm)
    return margin, Sigma
