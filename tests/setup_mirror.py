"""Plain reference of the problem setup of csrc/scpqp_kernel.h (``setup_problem``: the bicycle
Jacobian and its affine residual, the 8x8 matrix exponential, the prediction recursions, the
cost gradient and the reference sampler), generic in the number format (float64 and the 80-bit
``numpy.longdouble``), like tests/qp_phase_mirror.py.

The mirror restates the reference's definitions (``oracle.scp_reference.bicycle_jacobian``,
``bicycle_rhs``, ``discretize``, ``prediction_matrices``, ``cost_matrices``,
``sample_reference``), not the device's algorithm: its matrix exponential is a scaled Taylor
series, the device's is Pade-13.

Yardsticks.  Beside every value the mirror returns its yardstick, the same expression with
every term replaced by its absolute value:

    Mh     dt |M| for the 8x8 argument M = [[Ac Bc Ec]; 0], the Ec column replaced by
           dt (|f| + |Ac| |x| + |Bc| |u|), |f| termwise (|vc cos| + |noise| on rows 0 and 1)
    S      expm(Mh): its blocks are the yardsticks of Ad, Bd and Ed
    Yp0, Yg  the recursions of p0 and g on |Ad|, |Bd|, |Ed| and |x0| (the values' own
           magnitudes, not S: S has e^(+10 dt) where Ad has the steering lag's e^(-10 dt),
           and its powers would make every later step's yardstick meaningless)
    Ypsi   2 sum_k q_k Yg_{k-l} . (|ref_k| + Yp0_k)

A float64 evaluation of a value errs by a modest multiple of u times its yardstick, u = 2^-53,
whatever the cancellation in the value itself; where a yardstick is exactly zero no term
contributes, the entry is structurally zero, and the device must return exactly 0.0
(``structural_zero``).  tests/setup_cases.py holds the multiples measured on a float64
restatement of the device's algorithm, which lives here too (``expm_pade13`` and
``expm="pade"``): reference-side code, with the seeded mistakes of tests/test_setup_host.py.

The sampler (``sample``) follows the oracle's, returns what the reference would raise on
instead of raising (``raises``: "xor" the float ``^`` of SampleReferTraj.py:70, "index" the
index past the end, "assert" the segment-length assert) and lists every branch decision with
its distance from the threshold (``decisions``)."""
import math

import numpy as np

F64 = np.float64
F80 = np.longdouble
U = 2.0 ** -53
THETA13 = 5.371920351148152
MAX_SQUARINGS = 1100
ED_THRESHOLD = 1e-30        # MPC_Iter.py:87

SEEDS = ("a05_sign", "a15_rho", "squaring", "ec5_u", "g_shift", "qf_hpmax", "sampler_index1")


def mm(A, B):
    """A B with every entry summed over k in ascending order, products and sums rounded one by
    one: the same on every machine (``@`` in float64 goes through the BLAS, whose order and
    fused operations depend on the processor)."""
    acc = A[:, 0:1] * B[0:1, :]
    for k in range(1, A.shape[1]):
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
    return acc


def mv(A, x):
    return mm(A, x.reshape(-1, 1))[:, 0]


def vec(x, ft):
    return np.array([ft(v) for v in np.asarray(x).reshape(-1)], dtype=ft)


# ---------------------------------------------------------------------------------------
# vehicle model (Model.py:45-87)
# ---------------------------------------------------------------------------------------
def model(x, u, Lf, Lr, noise, ft, seed=None):
    """(M, Mh): the continuous 8x8 argument [[Ac Bc Ec]; 0] and its yardstick (both without
    the factor dt)."""
    x = vec(x, ft)
    u, Lf, Lr = ft(u), ft(Lf), ft(Lr)
    n0, n1 = ft(noise[0]), ft(noise[1])
    L = Lf + Lr
    rho = Lr / L
    v, psi, d = x[3], x[2], x[5]
    t = np.tan(d)
    sec2 = t * t + 1
    kap = np.sqrt(rho * rho * t * t + 1)
    beta = np.arctan(rho * t)
    th = psi + beta
    cth, sth = np.cos(th), np.sin(th)
    Ac = np.zeros((6, 6), dtype=ft)
    Ac[0, 2] = -v * sth * kap
    Ac[0, 3] = cth * kap
    a05 = (rho * rho * v * cth * t * sec2 / kap, rho * v * sth * sec2 / kap)
    Ac[0, 5] = a05[0] + a05[1] if seed == "a05_sign" else a05[0] - a05[1]
    Ac[1, 2] = v * cth * kap
    Ac[1, 3] = sth * kap
    a15 = (rho * v * cth * sec2 / kap, (rho if seed == "a15_rho" else rho * rho) * v * sth * t * sec2 / kap)
    Ac[1, 5] = a15[0] + a15[1]
    Ac[2, 3] = t / L
    Ac[2, 5] = v * sec2 / L
    Ac[3, 4] = 1
    Ac[5, 5] = -10
    Bc = np.zeros(6, dtype=ft)
    Bc[5] = 10
    # bicycle_rhs
    vc = v * np.sqrt(1 + (rho * t) ** 2)
    f = np.zeros(6, dtype=ft)
    fa = np.zeros(6, dtype=ft)
    f[0] = vc * np.cos(psi + beta) + n0
    fa[0] = abs(vc * np.cos(psi + beta)) + abs(n0)
    f[1] = vc * np.sin(psi + beta) + n1
    fa[1] = abs(vc * np.sin(psi + beta)) + abs(n1)
    f[2] = vc * t * np.cos(beta) / L
    fa[2] = abs(f[2])
    f[3] = x[4]
    fa[3] = abs(x[4])
    f[5] = (u - x[5]) / ft(0.1)
    fa[5] = (abs(u) + abs(x[5])) / ft(0.1)
    Ec = f - mv(Ac, x) - (0 if seed == "ec5_u" else Bc * u)
    Aa = np.abs(Ac)
    # a05 and a15 are sums of two terms themselves
    Aa[0, 5] = abs(a05[0]) + abs(a05[1])
    Aa[1, 5] = abs(a15[0]) + abs(a15[1])
    Eh = fa + mv(Aa, np.abs(x)) + Bc * abs(u)
    M = np.zeros((8, 8), dtype=ft)
    Mh = np.zeros((8, 8), dtype=ft)
    M[:6, :6], M[:6, 6], M[:6, 7] = Ac, Bc, Ec
    Mh[:6, :6], Mh[:6, 6], Mh[:6, 7] = Aa, Bc, Eh
    return M, Mh


# ---------------------------------------------------------------------------------------
# matrix exponential
# ---------------------------------------------------------------------------------------
def norm1(A):
    return float(np.max(np.sum(np.abs(A), axis=0)))


def squarings(nrm):
    """expm_squarings of csrc/scpqp_kernel.h, restated."""
    if not (nrm > THETA13) or not (nrm <= 1.7976931348623157e308):
        return 0
    return min(int(math.ceil(math.log2(nrm / THETA13))), MAX_SQUARINGS)


def expm_taylor(A, ft, terms=26):
    """Scaled Taylor series: A / 2^s of 1-norm <= 1/4, ``terms`` terms (the remainder is below
    (1/4)^27 / 27! = 5e-45 of the sum), s squarings."""
    A = np.asarray(A, dtype=ft)
    n = A.shape[0]
    nrm = norm1(A)
    s = 0 if nrm <= 0.25 else max(0, int(math.ceil(math.log2(nrm / 0.25))))
    B = A / ft(2.0 ** s)
    X = np.eye(n, dtype=ft)
    T = np.eye(n, dtype=ft)
    for k in range(1, terms + 1):
        T = mm(T, B) / ft(k)
        X = X + T
    for _ in range(s):
        X = mm(X, X)
    return X


PADE13 = (64764752532480000.0, 32382376266240000.0, 7771770303897600.0, 1187353796428800.0,
          129060195264000.0, 10559470521600.0, 670442572800.0, 33522128640.0, 1323241920.0,
          40840800.0, 960960.0, 16380.0, 182.0, 1.0)


def gauss_jordan(P, Q):
    """Solve P X = Q by Gauss-Jordan with partial pivoting, the first maximal row of the pivot
    column taken (LAPACK's idamax).  Returns (X, row swaps, pivot columns whose maximum two
    rows share)."""
    n = P.shape[0]
    aug = np.concatenate([P, Q], axis=1).copy()
    swaps = ties = 0
    for k in range(n):
        col = np.abs(aug[k:, k])
        p = k + int(np.argmax(col))          # argmax: the first maximal entry
        ties += int(np.sum(col == col.max()) > 1)
        if p != k:
            aug[[k, p]] = aug[[p, k]]
            swaps += 1
        piv = aug[k, k]
        rowk = aug[k] / piv
        for i in range(n):
            if i != k:
                aug[i] = aug[i] - aug[i, k] * rowk
        aug[k] = rowk
    return aug[:, n:], swaps, ties


def expm_pade13(A, ft=F64, drop_squarings=0, info=None):
    """Pade-13 with scaling and squaring as expm8 of csrc/scpqp_kernel.h forms it (Higham
    2005): the float64 restatement of the device's algorithm.  ``drop_squarings``: a seeded
    mistake.  ``info``: a dict that receives the squaring count, the row swaps and the tied pivot columns."""
    A = np.asarray(A, dtype=ft)
    n = A.shape[0]
    b = [ft(c) for c in PADE13]
    s = squarings(norm1(A))
    A = A * ft(2.0 ** -s)
    I = np.eye(n, dtype=ft)
    A2 = mm(A, A)
    A4 = mm(A2, A2)
    A6 = mm(A4, A2)
    U2 = mm(A6, b[13] * A6 + b[11] * A4 + b[9] * A2) + b[7] * A6 + b[5] * A4 + b[3] * A2 + b[1] * I
    V = mm(A6, b[12] * A6 + b[10] * A4 + b[8] * A2) + b[6] * A6 + b[4] * A4 + b[2] * A2 + b[0] * I
    Um = mm(A, U2)
    X, swaps, ties = gauss_jordan(V - Um, V + Um)
    for _ in range(max(0, s - drop_squarings)):
        X = mm(X, X)
    if info is not None:
        info["s"], info["swaps"], info["ties"] = s, swaps, ties
    return X


# ---------------------------------------------------------------------------------------
# one vehicle: discretisation, prediction recursions, cost gradient
# ---------------------------------------------------------------------------------------
class Vehicle:
    """Values and yardsticks of one vehicle's linearisation at horizon Hb:
    Ad [6, 6], Bd [6], Ed [6], p0 [Hb, 2] (const_term), g [Hb, 2] and Y* their yardsticks;
    s the device's squaring count, nrm the 1-norm of its argument."""


def vehicle(x, u, Lf, Lr, noise, dt, Hb, ft, expm="taylor", seed=None):
    M, Mh = model(x, u, Lf, Lr, noise, ft, seed)
    dtf = ft(dt)
    r = Vehicle()
    r.M, r.Mh = M * dtf, Mh * dtf
    r.nrm = norm1(np.asarray(r.M, dtype=F64))
    r.s = squarings(r.nrm)
    if expm == "taylor":
        X = expm_taylor(r.M, ft)
    else:
        X = expm_pade13(r.M, ft, drop_squarings=1 if seed == "squaring" else 0)
    S = expm_taylor(r.Mh, ft)
    r.X, r.S = X, S
    r.Ad, r.Bd, r.Ed = X[:6, :6].copy(), X[:6, 6].copy(), X[:6, 7].copy()
    r.Ed[np.abs(r.Ed) <= ED_THRESHOLD] = 0
    r.YAd, r.YBd, r.YEd = S[:6, :6].copy(), S[:6, 6].copy(), S[:6, 7].copy()
    # p0_k = C (Ad^(k+1) x0 + sum_{i<=k} Ad^i Ed),  g_m = C Ad^m Bd
    # (their yardsticks: the same recursions on |Ad|, |Bd|, |Ed| and |x0|)
    xs, ys = vec(x, ft), np.abs(vec(x, ft))
    bs, cs = r.Bd.copy(), np.abs(r.Bd)
    absA, absE = np.abs(r.Ad), np.abs(r.Ed)
    if seed == "g_shift":
        bs = mv(r.Ad, bs)
    r.p0 = np.zeros((Hb, 2), dtype=ft)
    r.g = np.zeros((Hb, 2), dtype=ft)
    r.Yp0 = np.zeros((Hb, 2), dtype=ft)
    r.Yg = np.zeros((Hb, 2), dtype=ft)
    for k in range(Hb):
        xs = mv(r.Ad, xs) + r.Ed
        ys = mv(absA, ys) + absE
        r.p0[k], r.Yp0[k] = xs[:2], ys[:2]
        r.g[k], r.Yg[k] = bs[:2], cs[:2]
        bs = mv(r.Ad, bs)
        cs = mv(absA, cs)
    return r


def psi0(r, ref, Q, Qf, ft, last=None):
    """(Psi0 [Hb], its yardstick) of a vehicle: Psi0_l = -2 sum_{k>=l} q_k g_{k-l} . (ref_k - p0_k),
    q_k = Qf on step ``last`` (the last step of the vehicle's own horizon), else Q.
    ref [Hb, 2] in float64 (data)."""
    Hb = r.p0.shape[0]
    last = Hb - 1 if last is None else last
    ref = np.asarray(ref, dtype=ft).reshape(Hb, 2)
    q = np.array([ft(Qf) if k == last else ft(Q) for k in range(Hb)], dtype=ft)
    err = ref - r.p0
    ea = np.abs(ref) + r.Yp0
    out = np.zeros(Hb, dtype=ft)
    ya = np.zeros(Hb, dtype=ft)
    for l in range(Hb):
        acc, aa = ft(0), ft(0)
        for k in range(l, Hb):
            acc = acc + q[k] * (r.g[k - l, 0] * err[k, 0] + r.g[k - l, 1] * err[k, 1])
            aa = aa + q[k] * (r.Yg[k - l, 0] * ea[k, 0] + r.Yg[k - l, 1] * ea[k, 1])
        out[l], ya[l] = -2 * acc, 2 * aa
    return out, ya


OUTPUTS = ("Ad", "Bd", "Ed", "g", "const_term", "psi0")


def outputs(r, ref, Q, Qf, ft, last=None):
    """{output name: (value, yardstick)} of a vehicle, the names of ``ScpQpSolver.linearize``."""
    ps, yps = psi0(r, ref, Q, Qf, ft, last)
    return {"Ad": (r.Ad, r.YAd), "Bd": (r.Bd, r.YBd), "Ed": (r.Ed, r.YEd), "g": (r.g, r.Yg),
            "const_term": (r.p0, r.Yp0), "psi0": (ps, yps)}


def ratio(x, ref, yard):
    """max |x - ref| / (u yardstick) over the entries with a yardstick; ``x`` in float64."""
    x = np.asarray(x, dtype=F80)
    ref = np.asarray(ref, dtype=F80)
    yard = np.asarray(yard, dtype=F80)
    m = yard > 0
    if not m.any():
        return 0.0
    return float(np.max(np.abs(x - ref)[m] / (F80(U) * yard[m])))


def ratio_of(diff, yard):
    """max |diff| / (u yardstick); infinite if diff is not zero where the yardstick is."""
    diff, yard = np.abs(np.asarray(diff, dtype=F80)), np.asarray(yard, dtype=F80)
    m = yard > 0
    if (diff[~m] != 0).any():
        return math.inf
    return float(np.max(diff[m] / (F80(U) * yard[m]))) if m.any() else 0.0


def structural_zero(yard):
    return np.asarray(yard) == 0


# ---------------------------------------------------------------------------------------
# reference sampler (SampleReferTraj.py:8-122)
# ---------------------------------------------------------------------------------------
class Sample:
    """points [n, 2]; raises: the set of reasons the reference would raise for; decisions:
    [(kind, distance from the threshold)] of every branch decision taken (kinds: "lam" in
    units of lambda, "sd", "assert", "rem" in metres, "seed" the distance to point 1 against
    the seed, which is that distance: equal by construction); index: the walk's start index."""


def _project(x1, y1, x2, y2, x3, y3, ft):
    b = np.sqrt((x2 - x1) ** 2 + (y2 - y1) ** 2)
    if b != 0:
        xn, yn = (x2 - x1) / b, (y2 - y1) / b
        x31, y31 = x3 - x1, y3 - y1
        dot = xn * x31 + yn * y31
        dist = xn * y31 - yn * x31
        return x1 + dot * xn, y1 + dot * yn, dist, dot / b, b
    return x1, y1, np.sqrt((x3 - x1) ** 2 + (y3 - y1) ** 2), ft(0), b


def sample(n_samples, poly, vx, vy, step, ft=F64, seed=None):
    poly = np.asarray(poly, dtype=np.float64)
    cx, cy = vec(poly[:, 0], ft), vec(poly[:, 1], ft)
    x, y, step = ft(vx), ft(vy), ft(step)
    n = len(cx)
    r = Sample()
    r.raises, r.decisions = set(), []
    dec = r.decisions
    xm, ym = cx[1], cy[1]
    dmin = np.sqrt((x - cx[1]) ** 2 + (y - cy[1]) ** 2)
    imin = seed_index = 1 if seed == "sampler_index1" else 2
    for j in range(1, n):
        xp, yp, sd, lam, plen = _project(cx[j - 1], cy[j - 1], cx[j], cy[j], x, y, ft)
        if plen != 0:
            if j != 1:
                dec.append(("lam", abs(float(lam))))
            if j != n - 1:
                dec.append(("lam", abs(float(1 - lam))))
        if (0 < lam or j == 1) and (lam < 1 or j == n - 1):
            dec.append(("sd", abs(float(abs(sd) - abs(dmin)))))
            if abs(sd) < abs(dmin):
                xm, ym, dmin, imin = xp, yp, sd, j
        else:
            r.raises.add("xor")
            d_end = np.sqrt((x - cx[j]) ** 2 + (y - cy[j]) ** 2)
            # on segment 1 against the untouched seed both sides are the same expression
            dec.append(("seed" if j == 1 and imin == seed_index else "sd", abs(float(d_end - abs(dmin)))))
            if d_end < abs(dmin):
                xm, ym = cx[j], cy[j]
                dmin = (d_end if sd > 0 else -d_end) if sd != 0 else ft(0)
                imin = j
    for i in range(n - 1):
        ln = np.sqrt((cx[i + 1] - cx[i]) ** 2 + (cy[i + 1] - cy[i]) ** 2)
        dec.append(("assert", abs(float(ln - step))))
        if not ln > step:
            r.raises.add("assert")
    idx = imin
    r.index = imin
    if idx > n - 1:
        # the reference raises IndexError at its first step; the device goes on from the
        # last point (include/scpqp.h, SCPQP_FL_SAMPLER)
        r.raises.add("index")
        idx = n - 1
    cur = np.array([xm, ym], dtype=ft)
    ref = np.stack([cx, cy], axis=1)
    r.points = np.zeros((n_samples, 2), dtype=ft)
    for i in range(n_samples):
        rem = np.sqrt((cur[0] - ref[idx, 0]) ** 2 + (cur[1] - ref[idx, 1]) ** 2)
        dec.append(("rem", abs(float(rem - step))))
        if rem > step:
            d = ref[idx] - ref[idx - 1]
            cur = cur + step * d / np.sqrt(d[0] ** 2 + d[1] ** 2)
        else:
            cur = ref[idx].copy()
            d = ref[idx] - ref[idx - 1]
            cur = cur + (step - rem) * d / np.sqrt(d[0] ** 2 + d[1] ** 2)
        r.points[i] = cur
    return r


def separation(r, exact=()):
    """The smallest distance of a branch decision from its threshold, the kinds in ``exact``
    left out (decisions that are exact in float64 by the case's construction)."""
    vals = [v for k, v in r.decisions if k not in exact and k != "seed"]
    return min(vals) if vals else math.inf
