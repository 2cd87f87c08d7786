"""CPU mirror of the device's model-noise generator (include/scpqp_noise.h), for the
noise tests: Philox4x32-10 in numpy, the uniform / Box-Muller mapping, the counter
layout, and an RK4 flow over ``oracle.scp_reference.bicycle_rhs`` that consumes the
draws in the device's evaluation order.  Written from the header's description (the
generator from Salmon et al., SC'11), not from the device code."""
import math

import numpy as np

from oracle import scp_reference as R

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
SITE_DELAY, SITE_PLANT, SITE_LINEARIZE = 0, 1, 2


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: two -> four uint64 arrays holding
    the 32-bit output words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    mask, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask,
             (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c


def uniforms(w):
    """u1 in (0, 1], u2 in [0, 1) from the four words."""
    a = ((w[0] << np.uint64(32)) | w[1]) >> np.uint64(11)
    b = ((w[2] << np.uint64(32)) | w[3]) >> np.uint64(11)
    return (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53


def normals(seed, c0, c1, c2, c3):
    """The standard-normal pair (z0, z1) of counter (c0, c1, c2, c3) under ``seed``."""
    w = philox4x32_10((c0, c1, c2, c3), (seed & MASK, (seed >> 32) & MASK))
    u1, u2 = uniforms(w)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def counter2(site, k, v):
    return (site << 24) | (k << 8) | v


def draws(seed, epoch, site, k, v, b_global, n_eval):
    """[n_eval, 2]: (z0, z1) of evaluations c0 = 0..n_eval-1 of one lane's stream."""
    z0, z1 = normals(seed, np.arange(n_eval), epoch, counter2(site, k, v), b_global & MASK)
    return np.stack([z0, z1], axis=-1)


def steps_for(T, h_max):
    """RK4 steps of a span of length T (steps of at most h_max, scpqp.h)."""
    return max(1, int(math.ceil(abs(T) / h_max - 1e-9)))


def rk4_noise_shift(z, h, sigma):
    """What the draws z [4 * n_steps, 2] add to (x, y) over n_steps RK4 steps of size h:
    the right-hand side does not read x or y, so the noise enters linearly as
    sum_steps h/6 * sigma * (z_k1 + 2 z_k2 + 2 z_k3 + z_k4)."""
    q = z.reshape(-1, 4, 2)
    return (h / 6.0 * sigma * (q[:, 0] + 2.0 * q[:, 1] + 2.0 * q[:, 2] + q[:, 3])).sum(axis=0)


def flow(x, u_ref, Lf, Lr, T, n, z, sigma):
    """n RK4 steps over a span T from state x with the draws z [4 n, 2], in the device's
    order: evaluation 4 s + j is stage k_(j+1) of step s."""
    x = np.array(x, float)
    h = T / n
    for s in range(n):
        def f(y, j):
            return R.bicycle_rhs(y, u_ref, Lf, Lr, noise=sigma * z[4 * s + j])
        k1 = f(x, 0)
        k2 = f(x + 0.5 * h * k1, 1)
        k3 = f(x + 0.5 * h * k2, 2)
        k4 = f(x + h * k3, 3)
        x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x
