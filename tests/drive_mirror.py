"""CPU mirror of the drive truth (include/scpqp_drive.h), for the drive tests: numpy, generic
in the number format (``F64``, ``F80``), on top of the plant truth's right-hand side
(tests/truth_mirror.py): a_eff in its two roundings, the gate, the lag, the projection after
every RK4 step, the device's step count, the bad rule, the closed form at HOLD = 0 and the
sampler on the mirror's Philox (tests/noise_mirror.py).  Written from the header's
description, not from the device code."""
import math

import numpy as np

import noise_mirror as NM
import truth_mirror as TM
from governor_mirror import F64, F80  # noqa: F401  (the number formats)
from noise_mirror import steps_for  # noqa: F401

NP = 6
TAU_A, GAIN_A, BIAS_A, A_MAX, B_MAX, HOLD = range(NP)
FIELDS = ("tau_a", "gain_a", "bias_a", "a_max", "b_max", "hold")
FIXED, UNIFORM, NORMAL = 0, 1, 2
SITE_DRIVE = 9
IDEAL_ROW = np.array([0.0, 1.0, 0.0, np.inf, np.inf, 0.0])


def ideal_row():
    return IDEAL_ROW.copy()


def is_bad(drow, a_cmd):
    """The header's bad rule (the drive row's part and the command's)."""
    t, g, b, am, bm, h = (float(v) for v in drow)
    return (not t >= 0.0 or not math.isfinite(g) or not math.isfinite(b) or not am >= 0.0
            or not bm >= 0.0 or h not in (0.0, 1.0) or not math.isfinite(float(a_cmd)))


def is_bad_truth(trow):
    return not (trow[TM.LF] + trow[TM.LR] > 0.0) or not (trow[TM.TAU] > 0.0)


def raw_command(drow, a_cmd, fm=F64):
    """gain * a_cmd + bias in two roundings (numpy scalars never fuse): the clamp's argument."""
    return fm.num(drow[GAIN_A]) * fm.num(a_cmd) + fm.num(drow[BIAS_A])


def a_eff(drow, a_cmd, fm=F64):
    """fmin(fmax(gain * a_cmd + bias, -B_MAX), A_MAX)."""
    r = raw_command(drow, a_cmd, fm)
    return min(max(r, fm.num(-drow[B_MAX])), fm.num(drow[A_MAX]))


def _base_rhs(x, ue, trow, noise, fm):
    """The truth row's right-hand side: tests/truth_mirror.py's own in float64, the same
    expressions on numpy scalars in any other format."""
    if fm.dtype is np.float64:
        return TM.rhs(x, ue, trow, noise)
    n = fm.num
    L = n(trow[TM.LF]) + n(trow[TM.LR])
    rho = n(trow[TM.LR]) / L
    t = np.tan(x[5])
    beta = np.arctan(rho * t)
    vc = x[3] * np.sqrt(1 + (rho * t) ** 2)
    dx = np.empty(6, dtype=fm.dtype)
    dx[0] = vc * np.cos(x[2] + beta) + n(noise[0])
    dx[1] = vc * np.sin(x[2] + beta) + n(noise[1])
    dx[2] = vc * t * np.cos(beta) / L
    dx[3] = x[4]
    dx[4] = 0.0
    dx[5] = (ue - x[5]) / n(trow[TM.TAU])
    return dx


def rhs(x, ue, ae, trow, drow, noise=(0.0, 0.0), fm=F64):
    """The right-hand side of a drive lane: the truth row's, then dx[4] of the lag and the
    gate on dx[3]."""
    dx = _base_rhs(x, ue, trow, noise, fm)
    if drow[TAU_A] > 0.0:
        dx[4] = (ae - x[4]) / fm.num(drow[TAU_A])
    if drow[HOLD] == 1.0 and not (x[3] > 0.0) and x[4] < 0.0:
        dx[3] = 0.0
    return dx


def rk4_flow(x, u_ref, a_cmd, trow, drow, T, n, z=None, sigma=0.0, pair=(0.0, 0.0), fm=F64,
             watch=None):
    """The lane of the header over T in n RK4 steps, in the device's evaluation order;
    z [4 n, 2]: the lane's draws; ``pair``: the constant noise terms.  ``watch``: a dict that
    collects 'speeds' (every stage's and every step's speed, HOLD lanes), 'accels' (the
    acceleration wherever the gate's speed test held) and 'projected' (the count)."""
    x = fm.array(x).copy()
    ue = fm.num(trow[TM.GAIN]) * fm.num(u_ref) + fm.num(trow[TM.BIAS])
    ae = a_eff(drow, a_cmd, fm)
    hold = drow[HOLD] == 1.0
    if not drow[TAU_A] > 0.0:
        x[4] = ae
    if n == 0:
        return x
    h = fm.num(T) / fm.num(n)
    half, two, six = fm.num(0.5), fm.num(2.0), fm.num(6.0)
    for s in range(n):
        def f(y, j):
            nz = pair if z is None else sigma * z[4 * s + j]
            if watch is not None and hold:
                watch["speeds"].append(float(y[3]))
                if not (y[3] > 0.0):
                    watch["accels"].append(float(y[4]))
            return rhs(y, ue, ae, trow, drow, nz, fm)
        s0 = x[3]
        k1 = f(x, 0)
        k2 = f(x + half * h * k1, 1)
        k3 = f(x + half * h * k2, 2)
        k4 = f(x + h * k3, 3)
        x = x + h / six * (k1 + two * k2 + two * k3 + k4)
        if hold and s0 >= 0.0 and x[3] < 0.0:
            x[3] = 0.0
            if watch is not None:
                watch["projected"] += 1
    return x


def plant_step(x_start, u_tick, truth, a_cmd, drive, tick, h_max, pair=None, seeded=None, fm=F64,
               watch=None):
    """x_start [B, V, 6], u_tick [B, V, K], truth [B, V, 5], a_cmd [B, V], drive [B, V, 6] ->
    [B, V, K, 6] in ``fm``: scpqp_plant_step_drive.  ``pair`` [B, V, 2]: the constant noise;
    ``seeded`` = (seed, sigma, epoch, b_offset): the per-evaluation noise of site 1.
    ``watch``: a dict (b, v, k) -> the watch of rk4_flow."""
    B, V, K = u_tick.shape
    out = np.zeros((B, V, K, 6), dtype=fm.dtype)
    for b in range(B):
        for v in range(V):
            if is_bad(drive[b, v], a_cmd[b, v]) or is_bad_truth(truth[b, v]):
                out[b, v] = np.nan
                continue
            for k in range(K):
                T = k * tick
                n = steps_for(T, h_max) if k else 0
                z, sigma = None, 0.0
                if seeded is not None and k:
                    seed, sigma, epoch, b_off = seeded
                    z = NM.draws(seed, epoch, NM.SITE_PLANT, k, v, b_off + b, 4 * n)
                w = None
                if watch is not None:
                    w = watch[(b, v, k)] = dict(speeds=[], accels=[], projected=0)
                out[b, v, k] = rk4_flow(x_start[b, v], u_tick[b, v, k], a_cmd[b, v], truth[b, v],
                                        drive[b, v], T, n, z, sigma,
                                        (0.0, 0.0) if pair is None else pair[b, v], fm, w)
    return out


def closed_form(s0, a0, ae, tau, t):
    """(a(t), s(t)) of the lag at HOLD = 0, in 80-bit."""
    L = np.longdouble
    s0, a0, ae, tau, t = L(s0), L(a0), L(ae), L(tau), L(t)
    e = np.exp(-t / tau)
    return ae + (a0 - ae) * e, s0 + ae * t + (a0 - ae) * tau * (-np.expm1(-t / tau))


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
class Dist:
    """The fields of scpqp_drive_dist; every field starts FIXED at its ideal value."""

    def __init__(self, n_veh, seed, b_offset=0):
        self.n_veh = n_veh
        self.mean = np.broadcast_to(IDEAL_ROW[:, None], (NP, n_veh)).copy()   # [6, nVeh]
        self.seed, self.b_offset = seed, b_offset
        self.kind = [FIXED] * NP
        self.spread = [0.0] * NP
        self.lo = [-np.inf] * NP
        self.hi = [np.inf] * NP

    def fixed(self, f, value):
        self.mean[f, :] = value
        self.kind[f] = FIXED
        return self

    def set(self, f, kind, spread, lo=-np.inf, hi=np.inf):
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = kind, spread, lo, hi
        return self


def counters(dist, B):
    """The four counter words of every (b, v, f): arrays [B, V, 6]."""
    b, v, f = np.meshgrid(np.arange(B), np.arange(dist.n_veh), np.arange(NP), indexing="ij")
    return f, np.zeros_like(f), (SITE_DRIVE << 24) | v, (dist.b_offset + b) & NM.MASK


def xi(dist, B):
    """[B, V, 6] the unit draws (0 for a FIXED field) of realisations b_offset .. + B."""
    seed = dist.seed
    w = NM.philox4x32_10(counters(dist, B), (seed & NM.MASK, (seed >> 32) & NM.MASK))
    u1, u2 = NM.uniforms(w)
    uni = 2.0 * u2 - 1.0
    nor = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    kind = np.array(dist.kind)[None, None, :]
    return np.where(kind == UNIFORM, uni, np.where(kind == NORMAL, nor, 0.0))


def sample(dist, B):
    """[B, V, 6]: fmin(fmax(mean + spread * xi, lo), hi); a FIXED field is its mean."""
    x = xi(dist, B)
    mean = dist.mean.T[None]                                # [1, V, 6]
    fixed = (np.array(dist.kind) == FIXED)[None, None, :]
    with np.errstate(invalid="ignore"):
        val = np.where(fixed, 0.0, mean) + np.array(dist.spread)[None, None, :] * x
    val = np.minimum(np.maximum(val, np.array(dist.lo)[None, None, :]),
                     np.array(dist.hi)[None, None, :])
    return np.where(fixed, np.broadcast_to(mean, val.shape), val)
