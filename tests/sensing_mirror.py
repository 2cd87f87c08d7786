"""CPU mirror of the sensing truth (include/scpqp_sensing.h), for the sensing tests: the
measurement of one MPC step with its drop-and-hold logic, the controller's obstacle prediction
from a noisy pose (on ``obstacle_mirror``'s pose), and the row sampler, all on the mirror's
Philox (tests/noise_mirror.py).  Plain fp64, one rounding per operation (numpy never fuses);
written from the header's description, not from the device code."""
import math

import numpy as np

import noise_mirror as NM
import obstacle_mirror as OM

NP = 8
SIG_POS, SIG_HEADING, SIG_SPEED, SIG_STEER, BIAS_HEADING, SCALE_SPEED, P_DROP, LAG = range(NP)
ONP = 3
FIXED, UNIFORM, NORMAL = 0, 1, 2
SITE_SENSE, SITE_SENSE_DRAW, SITE_SENSE_OBST = 5, 6, 7
NOMINAL = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0])


def nominal_rows(B, n_veh):
    return np.broadcast_to(NOMINAL, (B, n_veh, NP)).copy()


def bad_row(row):
    row = np.asarray(row, float)
    if (~np.isfinite(row)).any() or (row[SIG_POS:SIG_STEER + 1] < 0.0).any():
        return True
    return bool(row[P_DROP] < 0.0 or row[P_DROP] > 1.0 or row[LAG] < 0.0
                or row[LAG] != np.rint(row[LAG]))


def bad_osense_row(row):
    row = np.asarray(row, float)
    return bool((~np.isfinite(row)).any() or (row < 0.0).any())


def calls(seed, c0, epoch, site, idx, b_global):
    """(z0, z1, u2) of the Philox calls at counter (c0, epoch, (site << 24) | idx, b_global);
    the counter fields broadcast.  The mapping is ``noise_mirror.normals``' own."""
    c2 = (site << 24) | np.asarray(idx, dtype=np.uint64)
    c3 = np.asarray(b_global, dtype=np.uint64) & np.uint64(NM.MASK)
    w = NM.philox4x32_10((c0, epoch, c2, c3), (seed & NM.MASK, (seed >> 32) & NM.MASK))
    u1, u2 = NM.uniforms(w)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2), u2


def call(seed, c0, epoch, site, idx, b_global):
    """``calls`` for one counter, as Python floats."""
    z0, z1, u2 = calls(seed, c0, epoch, site, idx, b_global)
    return float(z0), float(z1), float(u2)


def measure(x_path, k_meas, rows, seed, epoch, b_offset, x_held):
    """x_path [B, V, K, 6], rows [B, V, 8], x_held [B, V, 6] (updated in place) ->
    (x_meas [B, V, 6], delivered [B, V] of 0 / 1)."""
    x_path, rows = np.asarray(x_path, float), np.asarray(rows, float)
    B, V = rows.shape[:2]
    out = np.empty((B, V, 6))
    delivered = np.zeros((B, V), np.int32)
    for b in range(B):
        for v in range(V):
            r = rows[b, v]
            if bad_row(r):
                out[b, v] = np.nan
                x_held[b, v] = np.nan
                continue
            if np.array_equal(r, NOMINAL):
                out[b, v] = x_path[b, v, k_meas]
                x_held[b, v] = out[b, v]
                delivered[b, v] = 1
                continue
            g = b_offset + b
            if not np.isnan(x_held[b, v, 0]) and call(seed, 3, epoch, SITE_SENSE_DRAW, v, g)[2] < r[P_DROP]:
                out[b, v] = x_held[b, v]
                continue
            x = x_path[b, v, max(0, k_meas - int(r[LAG]))]
            a0, a1, _ = call(seed, 0, epoch, SITE_SENSE_DRAW, v, g)
            b0, b1, _ = call(seed, 1, epoch, SITE_SENSE_DRAW, v, g)
            c0, _, _ = call(seed, 2, epoch, SITE_SENSE_DRAW, v, g)
            m = np.array([x[0] + r[SIG_POS] * a0,
                          x[1] + r[SIG_POS] * a1,
                          (x[2] + r[BIAS_HEADING]) + r[SIG_HEADING] * b0,
                          r[SCALE_SPEED] * x[3] + r[SIG_SPEED] * b1,
                          x[4],
                          x[5] + r[SIG_STEER] * c0])
            out[b, v] = m
            x_held[b, v] = m
            delivered[b, v] = 1
    return out, delivered


def predict_sensed(rows, osense, seed, epoch, b_offset, t_meas, lead, dt, hp):
    """rows [B, nO, 7], osense [B, nO, 3] -> [B, nO, 2, hp]: the straight line of
    ``obstacle_mirror.predict`` from the measured pose and speed; an all-zero osense row is
    that function's own output."""
    rows, osense = np.asarray(rows, float), np.asarray(osense, float)
    B, nO = rows.shape[:2]
    out = np.full((B, nO, 2, hp), np.nan)
    for b in range(B):
        for o in range(nO):
            if OM.bad_row(rows[b, o]) or bad_osense_row(osense[b, o]):
                continue
            if not osense[b, o].any():
                out[b, o] = OM.predict(rows[b:b + 1, o:o + 1], t_meas, lead, dt, hp)[0, 0]
                continue
            x, y, h = OM.pose(rows[b, o], t_meas)
            s = float(rows[b, o, OM.SPEED])
            sp, sh, ss = (float(q) for q in osense[b, o])
            z0, z1, _ = call(seed, 0, epoch, SITE_SENSE_OBST, o, b_offset + b)
            w0, w1, _ = call(seed, 1, epoch, SITE_SENSE_OBST, o, b_offset + b)
            x, y, h, s = x + sp * z0, y + sp * z1, h + sh * w0, s + ss * w1
            for k in range(hp):
                step = ((k + 1) * dt + lead) * s
                out[b, o, 0, k] = step * math.cos(h) + x
                out[b, o, 1, k] = step * math.sin(h) + y
    return out


class Dist:
    """The fields of scpqp_sense_dist."""

    def __init__(self, n_veh, seed, b_offset=0):
        self.mean = np.tile(NOMINAL[:, None], (1, n_veh))    # [8, nVeh]
        self.n_veh = n_veh
        self.seed, self.b_offset = seed, b_offset
        self.kind = [FIXED] * NP
        self.spread = [0.0] * NP
        self.lo = [-np.inf] * NP
        self.hi = [np.inf] * NP

    def set(self, f, kind, spread, lo=-np.inf, hi=np.inf, mean=None):
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = kind, spread, lo, hi
        if mean is not None:
            self.mean[f, :] = mean
        return self


def xi(dist, B):
    """[B, V, 8] the unit draws (0 for a FIXED field) of realisations b_offset .. + B."""
    b, v, f = np.meshgrid(np.arange(B), np.arange(dist.n_veh), np.arange(NP), indexing="ij")
    seed = dist.seed
    w = NM.philox4x32_10((f, 0, (SITE_SENSE << 24) | v, (dist.b_offset + b) & NM.MASK),
                         (seed & NM.MASK, (seed >> 32) & NM.MASK))
    u1, u2 = NM.uniforms(w)
    uni = 2.0 * u2 - 1.0
    nor = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    kind = np.array(dist.kind)[None, None, :]
    return np.where(kind == UNIFORM, uni, np.where(kind == NORMAL, nor, 0.0))


def sample(dist, B):
    """[B, V, 8]: fmin(fmax(mean + spread * xi, lo), hi), a FIXED field its mean; LAG rounded
    to the nearest whole number."""
    x = xi(dist, B)
    mean = dist.mean.T[None]                                # [1, V, 8]
    val = mean + np.array(dist.spread)[None, None, :] * x
    val = np.minimum(np.maximum(val, np.array(dist.lo)[None, None, :]),
                     np.array(dist.hi)[None, None, :])
    fixed = (np.array(dist.kind) == FIXED)[None, None, :]
    val = np.where(fixed, np.broadcast_to(mean, val.shape), val)
    val[..., LAG] = np.rint(val[..., LAG])
    return val
