"""CPU mirror of the plant truth (include/scpqp_truth.h), for the truth tests: the
generalised right-hand side, its exact flow (DOP853 at 1e-13), the device's fixed-step
RK4 over it, and the sampler on the mirror's Philox (tests/noise_mirror.py).  Written
from the header's description, not from the device code."""
import math

import numpy as np
import scipy.integrate

import noise_mirror as NM
from noise_mirror import rk4_noise_shift, steps_for  # noqa: F401  (reused by the tests)

NP = 5
LF, LR, TAU, GAIN, BIAS = range(NP)
FIXED, UNIFORM, NORMAL = 0, 1, 2
SITE_TRUTH = 3
TAU_NOMINAL = 0.1


def nominal_row(Lf, Lr):
    return np.array([Lf, Lr, TAU_NOMINAL, 1.0, 0.0])


def u_eff(row, u_ref):
    """gain * u_ref + bias, two roundings (numpy float64 never fuses)."""
    return np.float64(row[GAIN]) * np.float64(u_ref) + np.float64(row[BIAS])


def rhs(x, ue, row, noise=(0.0, 0.0)):
    """Model.py:61-87 with the row's geometry and lag; ``ue`` is the lane's u_eff."""
    L = row[LF] + row[LR]
    rho = row[LR] / L
    t = math.tan(x[5])
    beta = math.atan(rho * t)
    vc = x[3] * math.sqrt(1 + (rho * t) ** 2)
    dx = np.empty(6)
    dx[0] = vc * math.cos(x[2] + beta) + noise[0]
    dx[1] = vc * math.sin(x[2] + beta) + noise[1]
    dx[2] = vc * t * math.cos(beta) / L
    dx[3] = x[4]
    dx[4] = 0.0
    dx[5] = (ue - x[5]) / row[TAU]
    return dx


def exact_flow(x, u_ref, row, T):
    """The exact flow over [0, T]: DOP853 at rtol = atol = 1e-13."""
    if T == 0.0:
        return np.array(x, float)
    ue = u_eff(row, u_ref)
    sol = scipy.integrate.solve_ivp(lambda t, y: rhs(y, ue, row), (0.0, T), np.asarray(x, float),
                                    method="DOP853", rtol=1e-13, atol=1e-13)
    return sol.y[:, -1]


def rk4_flow(x, u_ref, row, T, n, z=None, sigma=0.0):
    """n RK4 steps over T in the device's evaluation order; z [4 n, 2]: the lane's draws."""
    x = np.array(x, float)
    ue = u_eff(row, u_ref)
    h = T / n
    for s in range(n):
        def f(y, j):
            nz = (0.0, 0.0) if z is None else sigma * z[4 * s + j]
            return rhs(y, ue, row, nz)
        k1 = f(x, 0)
        k2 = f(x + 0.5 * h * k1, 1)
        k3 = f(x + 0.5 * h * k2, 2)
        k4 = f(x + h * k3, 3)
        x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


def plant_step_exact(x_start, u_tick, truth, tick):
    """x_start [B, V, 6], u_tick [B, V, K], truth [B, V, 5] -> [B, V, K, 6], output k the
    exact flow over k ticks with the command of tick k."""
    B, V, K = u_tick.shape
    out = np.zeros((B, V, K, 6))
    for b in range(B):
        for v in range(V):
            for k in range(K):
                out[b, v, k] = exact_flow(x_start[b, v], u_tick[b, v, k], truth[b, v], k * tick)
    return out


class Dist:
    """The fields of scpqp_truth_dist."""

    def __init__(self, mean, seed, b_offset=0):
        self.mean = np.array(mean, float)                   # [5, nVeh]
        self.n_veh = self.mean.shape[1]
        self.seed, self.b_offset = seed, b_offset
        self.kind = [FIXED] * NP
        self.spread = [0.0] * NP
        self.lo = [-np.inf] * NP
        self.hi = [np.inf] * NP

    def set(self, f, kind, spread, lo=-np.inf, hi=np.inf):
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = kind, spread, lo, hi
        return self


def xi(dist, B):
    """[B, V, 5] the unit draws (0 for a FIXED field) of realisations b_offset .. + B."""
    b, v, f = np.meshgrid(np.arange(B), np.arange(dist.n_veh), np.arange(NP), indexing="ij")
    seed = dist.seed
    w = NM.philox4x32_10((f, 0, (SITE_TRUTH << 24) | v, (dist.b_offset + b) & NM.MASK),
                         (seed & NM.MASK, (seed >> 32) & NM.MASK))
    u1, u2 = NM.uniforms(w)
    uni = 2.0 * u2 - 1.0
    nor = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    kind = np.array(dist.kind)[None, None, :]
    return np.where(kind == UNIFORM, uni, np.where(kind == NORMAL, nor, 0.0))


def sample(dist, B):
    """[B, V, 5]: fmin(fmax(mean + spread * xi, lo), hi); a FIXED field is its mean."""
    x = xi(dist, B)
    mean = dist.mean.T[None]                                # [1, V, 5]
    val = mean + np.array(dist.spread)[None, None, :] * x
    val = np.minimum(np.maximum(val, np.array(dist.lo)[None, None, :]),
                     np.array(dist.hi)[None, None, :])
    fixed = (np.array(dist.kind) == FIXED)[None, None, :]
    return np.where(fixed, np.broadcast_to(mean, val.shape), val)
