"""Plain reference of the KKT assembly and the IPM's vector phases of csrc/scpqp_kernel.h, as
dense algebra in numpy, generic in the number format (float64 and the 80-bit
``numpy.longdouble``), like tests/linalg_mirror.py.

A state is the structured data the kernel keeps: the Toeplitz generators ``g`` [V, Hb, 2], the
factored scaled rows ``rowE`` [m, 2], ``rowW``, ``rowH`` (row order of
``scp_reference.row_list``, scaling of the comment above ``linearise_rows``:
a_r = -(e_r . g_i,k-l) on vehicle i, +(e_r . g_j,k-l) on vehicle j, w_r on omega), ``qs``, the
iterate and the constraint-space vectors; the parameters are ``Q, Qf, R, uLim, slackW``.
``Dense`` builds from them

    G   [mc, n]  rows: collision (m), u <= 1 (N), -u <= 1 (N), -omega <= 0
    h   [mc]     rowH, ones, ones, 0
    P   [n, n]   2 uLim^2 (calB' diag(Q .. Q Qf) calB + R I) per vehicle, 0 on omega
    q   [n]      qs, slackW

and beside each the matrix of absolute values of the terms (``Ga``, ``Pa``), so that every site
below returns, with each value, a bound on the error of a float64 evaluation of it,

    c gamma(p) abs   (+ the first-order image of the bounds of the values it is formed from),

abs being the sum of the absolute values of the terms, p the number of operations on the
longest chain of the kernel's code for that value and c = 2 where the chain has a quotient
formed with ``recip`` (two roundings per operation at most), else 1.  The counts are derived
in the docstring of tests/test_gpu_qp_phases.py.

Values that hang on an extremum (a step length, omega of the starting point, a largest
residual) come with a separation flag: the binding entry must lead the runner-up by more than
the two bounds together, and the value's bound is then the binding entry's."""
import numpy as np

F64 = np.float64
F80 = np.longdouble
U = 2.0 ** -53
NT = 256


def gamma(k):
    return k * U / (1.0 - k * U)


def pair_index(i, j, V):
    return i * (2 * V - i - 1) // 2 + (j - i - 1)


def row_list(V, Hb, O):
    """scp_reference.row_list, restated here so that the mirror stands alone."""
    rows = [(i, j, -1, k) for i in range(V - 1) for j in range(i + 1, V) for k in range(Hb)]
    rows += [(i, -1, o, k) for i in range(V) for o in range(O) for k in range(Hb)]
    return rows


# ---------------------------------------------------------------------------------------
# operation counts (derived in tests/test_gpu_qp_phases.py)
# ---------------------------------------------------------------------------------------
class Counts:
    def __init__(self, V, O, Hb):
        N = V * Hb
        m = V * (V - 1) // 2 * Hb + V * O * Hb
        mc = m + 2 * N + 1
        L3 = -(-Hb // 3)
        self.toe = L3 + 3                 # calB x: product, <= L3 adds, two combining adds
        self.toeT = L3 + 5                # calB' y: two products and an add per term
        self.gx = self.toe + 4            # (G x)_r from ya
        self.inc = V + O                  # incident_sum of a stored coefficient
        self.sum_rows = lambda k: -(-k // NT) + 9      # per-thread chain, wave (6), block (3)
        self.sum_outs = lambda k: -(-k // 84) + 9      # the same over split3's owner lanes
        self.gt_u = self.inc + self.toeT + 2
        self.gt_w = self.sum_rows(m) + 2
        self.K_uu = 2 * Hb + V + O + 8
        self.K_wu = self.inc + 1 + self.toeT
        self.K_ww = self.sum_rows(m) + 4
        self.rp = self.gx + 2
        self.rd_u = max(self.toe + 4, self.inc + 1) + self.toeT + 4
        self.rd_w = self.sum_rows(m) + 3
        self.gap = self.sum_rows(mc) + 1
        self.pobj = 2 * self.toe + 5 + self.sum_outs(N) + 4
        self.mc, self.m, self.N = mc, m, N


# ---------------------------------------------------------------------------------------
# the dense problem
# ---------------------------------------------------------------------------------------
class Dense:
    def __init__(self, st, par, T=F80, mutate=None):
        """mutate (tests only): 'q_for_qf', 'obst_sign', 'toeplitz_limit'."""
        V, O, Hb = st["V"], st["O"], st["Hb"]
        N, n = V * Hb, V * Hb + 1
        mp = V * (V - 1) // 2 * Hb
        m = mp + V * O * Hb
        mc = m + 2 * N + 1
        g = np.asarray(st["g"], dtype=T).reshape(V, Hb, 2)
        E = np.asarray(st["rowE"], dtype=T).reshape(m, 2)
        W = np.asarray(st["rowW"], dtype=T)
        G = np.zeros((mc, n), dtype=T)
        Ga = np.zeros((mc, n), dtype=T)
        ag, aE = np.abs(g), np.abs(E)
        for r, (i, j, o, k) in enumerate(row_list(V, Hb, O)):
            k0 = 1 if mutate == "toeplitz_limit" else 0      # the l = k term left out
            for v, sgn in ((i, -1), (j, 1)):
                if v < 0:
                    continue
                if mutate == "obst_sign" and j < 0:
                    sgn = -sgn
                gk = g[v, k::-1][:k + 1 - k0]                 # g_{k-l}, l = 0..k
                ak = ag[v, k::-1][:k + 1 - k0]
                G[r, v * Hb:v * Hb + k + 1 - k0] = sgn * (E[r, 0] * gk[:, 0] + E[r, 1] * gk[:, 1])
                Ga[r, v * Hb:v * Hb + k + 1 - k0] = aE[r, 0] * ak[:, 0] + aE[r, 1] * ak[:, 1]
        G[:m, N] = W
        Ga[:m, N] = np.abs(W)
        idx = np.arange(N)
        G[m + idx, idx] = 1
        G[m + N + idx, idx] = -1
        Ga[m + idx, idx] = 1
        Ga[m + N + idx, idx] = 1
        G[mc - 1, N] = -1
        Ga[mc - 1, N] = 1
        h = np.concatenate([np.asarray(st["rowH"], dtype=T), np.ones(2 * N, dtype=T), np.zeros(1, dtype=T)])
        uL = T(par["uLim"])
        u2 = uL * uL
        P = np.zeros((n, n), dtype=T)
        Pa = np.zeros((n, n), dtype=T)
        for v in range(V):
            cB = np.zeros((2 * Hb, Hb), dtype=T)
            for k in range(Hb):
                cB[2 * k:2 * k + 2, :k + 1] = g[v, k::-1].T
            Qf = par["Q"][v] if mutate == "q_for_qf" else par["Qf"][v]
            qd = np.full(2 * Hb, T(par["Q"][v]), dtype=T)
            qd[-2:] = T(Qf)
            sl = slice(v * Hb, (v + 1) * Hb)
            I = np.eye(Hb, dtype=T)
            P[sl, sl] = 2 * u2 * (cB.T @ (qd[:, None] * cB) + T(par["R"][v]) * I)
            Pa[sl, sl] = 2 * u2 * (np.abs(cB).T @ (qd[:, None] * np.abs(cB)) + T(par["R"][v]) * I)
        q = np.concatenate([np.asarray(st["qs"], dtype=T), np.array([par["slackW"]], dtype=T)])
        self.V, self.O, self.Hb, self.N, self.n, self.m, self.mp, self.mc = V, O, Hb, N, n, m, mp, mc
        self.G, self.Ga, self.h, self.P, self.Pa, self.q, self.T = G, Ga, h, P, Pa, q, T
        self.cnt = Counts(V, O, Hb)
        self.slackW = T(par["slackW"])


def _v(st, k, T):
    return np.asarray(st[k], dtype=T).reshape(-1)


def _gam(T, p, c=1):
    return T(c * gamma(p))


def _dot(a, b):
    """A long inner product by numpy's pairwise summation.  The kernel reduces its sums over
    the rows as a tree (a thread's short chain, then the wave and the workgroup), and the
    bounds count that tree; a float64 evaluation in BLAS's order, one long chain, would not be
    covered by them."""
    return np.sum(a * b)


def _colsum(M):
    """Column sums of M, each by pairwise summation."""
    return np.ascontiguousarray(M.T).sum(axis=1)


# ---------------------------------------------------------------------------------------
# extrema with a separation condition
# ---------------------------------------------------------------------------------------
def sep_max(val, bnd, floor=None):
    """(max, its bound, separated): the largest entry and its own bound; separated when it
    leads every other entry (and the floor, an exact candidate, if given) by more than the two
    bounds together."""
    T = val.dtype.type
    if val.size == 0:
        return (T(floor) if floor is not None else T(0)), T(0), True
    i = int(np.argmax(val))
    lo = val[i] - bnd[i]
    others = np.delete(val + bnd, i)
    ok = bool(others.size == 0 or lo > others.max())
    if floor is not None:
        if val[i] + bnd[i] < floor:
            return T(floor), T(0), bool(np.all(val + bnd < floor))
        ok = ok and lo > floor
    return val[i], bnd[i], ok


def min_ratio(num, den, eden, T, nops=2):
    """min over den < 0 of -num / den, capped at 1, for den known to within eden and num
    exactly (num > 0): (value, bound, separated).  A row's quotient lies in
    [num / (-den + eden), num / (-den - eden)] (1 -+ 2 gamma(nops)): the binding row's upper end
    must lie below every other row's lower end, and below the cap."""
    gq = _gam(T, nops, 2)
    one = T(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(den < 0, -num / den, T(np.inf))
        lo = np.where(-den + eden > 0, num / (-den + eden) * (one - gq), T(np.inf))
        hi = np.where(-den - eden > 0, num / (-den - eden) * (one + gq), T(np.inf))
    if val.size == 0 or val.min() >= 1:
        return one, T(0), bool(val.size == 0 or lo.min() > 1)
    b = int(np.argmin(val))
    rest = np.delete(lo, b)
    ok = bool(hi[b] < 1 and (rest.size == 0 or hi[b] < rest.min()))
    return val[b], max(hi[b] - val[b], val[b] - lo[b]), ok


# ---------------------------------------------------------------------------------------
# the sites: each returns {name: (value, bound)} (and "sep": {name: bool})
# ---------------------------------------------------------------------------------------
def site_assemble(D, st, rho, drop=None, no_rho=False):
    """K = P + rho I + G' diag(d) G (lower triangle, rows 0..N), and the W~ blocks.
    drop (tests only): (r, a): row r's term left out of block (a, a) of W~."""
    T, c = D.T, D.cnt
    d = _v(st, "dd", T)
    rho = T(rho)
    I = np.eye(D.n, dtype=T)
    key = id(st["dd"])          # the two products, kept for the same d at another rho
    if getattr(D, "_gdg", (None,))[0] != key:
        D._gdg = (key, D.G.T @ (d[:, None] * D.G), D.Ga.T @ (np.abs(d)[:, None] * D.Ga), st["dd"])
    K = D.P + (0 if no_rho else rho) * I + D._gdg[1]
    kw = _colsum((D.G[:, D.N] * d)[:, None] * D.G)       # the omega row: sums over every row
    K[D.N, :] = D.P[D.N, :] + kw
    K[:, D.N] = D.P[:, D.N] + kw
    if not no_rho:
        K[D.N, D.N] += rho
    Ka = D.Pa + rho * I + D._gdg[2]
    if drop is not None:
        r, a = drop
        sl = slice(a * D.Hb, (a + 1) * D.Hb)
        K[sl, sl] -= d[r] * np.outer(D.G[r, sl], D.G[r, sl])
    p = np.full((D.n, D.n), c.K_uu)
    p[D.N, :] = c.K_wu
    p[D.N, D.N] = c.K_ww
    bnd = np.vectorize(gamma)(p).astype(T) * Ka
    return {"K": (np.tril(K), np.tril(bnd))}


def wt_blocks(D, st, par):
    """W~ [Hb, nb, 4] as assemble's phase 1 defines it, with its bound (p = V + O + 1)."""
    T, V, O, Hb = D.T, D.V, D.O, D.Hb
    d = _v(st, "dd", T)
    E = np.asarray(st["rowE"], dtype=T).reshape(D.m, 2)
    nb = V * (V + 1) // 2
    u2 = T(par["uLim"]) * T(par["uLim"])
    W = np.zeros((Hb, nb, 4), dtype=T)
    Wa = np.zeros((Hb, nb, 4), dtype=T)

    def add(k, ab, r, sgn):
        o = (d[r] * np.outer(E[r], E[r])).reshape(4)
        W[k, ab] += sgn * o
        Wa[k, ab] += np.abs(o)
    for k in range(Hb):
        for a in range(V):
            aa = a * (a + 1) // 2 + a
            qk = 2 * u2 * T(par["Qf"][a] if k == Hb - 1 else par["Q"][a])
            W[k, aa, 0] += qk
            W[k, aa, 3] += qk
            Wa[k, aa, 0] += qk
            Wa[k, aa, 3] += qk
            for w in range(V):
                if w != a:
                    add(k, aa, pair_index(min(a, w), max(a, w), V) * Hb + k, 1)
            for o in range(O):
                add(k, aa, D.mp + (a * O + o) * Hb + k, 1)
            for b in range(a):
                add(k, a * (a + 1) // 2 + b, pair_index(b, a, V) * Hb + k, -1)
    return W, _gam(T, V + O + 1) * Wa


def site_gapply(D, st, minus_h, x=None):
    T, c = D.T, D.cnt
    x = _v(st, "z", T) if x is None else x
    v = D.G @ x
    a = D.Ga @ np.abs(x)
    p = c.gx
    if minus_h:
        v = v - D.h
        a = a + np.abs(D.h)
        p += 1
    return {"rp": (v, _gam(T, p) * a)}


def gt(D, t):
    """(G't, its bound) for a given t."""
    T, c = D.T, D.cnt
    v = D.G.T @ t
    v[D.N] = _dot(D.G[:, D.N], t)
    a = D.Ga.T @ np.abs(t)
    g = np.full(D.n, gamma(c.gt_u))
    g[D.N] = gamma(c.gt_w)
    return v, g.astype(T) * a, a


def site_rhs_from_tv(D, st, rho, skip=None):
    """rhs = G' tv - q + rho dz.  skip (tests only): output e is formed as zero."""
    T, c = D.T, D.cnt
    t, dz = _v(st, "tv", T), _v(st, "dz", T)
    v, _, a = gt(D, t)
    if skip is not None:
        v = v.copy()
        v[skip] = 0
    rho = T(rho)
    g = np.full(D.n, gamma(c.gt_u + 3))
    g[D.N] = gamma(c.gt_w + 3)
    return {"rhs": (v - D.q + rho * dz, g.astype(T) * (a + np.abs(D.q) + rho * np.abs(dz)))}


def site_residuals(D, st, z=None, s=None, lam=None):
    """rp dd tv rd and {max|rp|, max|rd|, gap, pobj} at (z, s, lam)."""
    T, c = D.T, D.cnt
    z = _v(st, "z", T) if z is None else np.asarray(z, dtype=T)
    s = _v(st, "s", T) if s is None else np.asarray(s, dtype=T)
    lam = _v(st, "lam", T) if lam is None else np.asarray(lam, dtype=T)
    az, al = np.abs(z), np.abs(lam)
    rp = D.G @ z + s - D.h
    rp_b = _gam(T, c.rp) * (D.Ga @ az + np.abs(s) + np.abs(D.h))
    dd = lam / s
    dd_b = _gam(T, 2, 2) * np.abs(dd)
    tv = dd * rp - lam
    tv_b = np.abs(dd) * rp_b + _gam(T, 5, 2) * (np.abs(dd * rp) + al)
    rd = D.P @ z + D.q + D.G.T @ lam
    rd[D.N] = D.P[D.N] @ z + D.q[D.N] + _dot(D.G[:, D.N], lam)
    gr = np.full(D.n, gamma(c.rd_u))
    gr[D.N] = gamma(c.rd_w)
    rd_b = gr.astype(T) * (D.Pa @ az + np.abs(D.q) + D.Ga.T @ al)
    mrp, mrp_b, ok0 = sep_max(np.abs(rp), rp_b)
    mrd, mrd_b, ok1 = sep_max(np.abs(rd), rd_b)
    gap = _dot(s, lam)
    gap_b = _gam(T, c.gap) * (np.abs(s) @ al)
    pobj = T(0.5) * (z @ (D.P @ z)) + D.q @ z
    pobj_b = _gam(T, c.pobj) * (T(0.5) * (az @ (D.Pa @ az)) + np.abs(D.q) @ az)
    return {"rp": (rp, rp_b), "dd": (dd, dd_b), "tv": (tv, tv_b), "rd": (rd, rd_b),
            "ret": (np.array([mrp, mrd, gap, pobj], dtype=T), np.array([mrp_b, mrd_b, gap_b, pobj_b], dtype=T)),
            "sep": {"max|rp|": ok0, "max|rd|": ok1}}


def site_init_b(D, st):
    """ph_init_b from a given z_u: omega, s, lam (ipm_start_omega's point)."""
    T, c, m, N, mc = D.T, D.cnt, D.m, D.N, D.mc
    z = _v(st, "z", T)[:N]
    az = np.abs(z)
    Gu, Gau = D.G[:, :N], D.Ga[:, :N]
    W, h = D.G[:m, N], D.h
    gu = Gu @ z
    gu_a = Gau @ az
    gu_b = _gam(T, c.gx) * gu_a
    cand = (gu[:m] - h[:m]) / -W
    cand_b = _gam(T, c.gx + 2) * (gu_a[:m] + np.abs(h[:m])) / np.abs(W)
    vmax, vmax_b, ok_om = sep_max(cand, cand_b, floor=0.0)
    om = vmax + 1
    om_b = vmax_b + _gam(T, 1) * abs(om)
    s0 = h - gu - D.G[:, N] * om
    s0_b = gu_b + D.Ga[:, N] * om_b + _gam(T, 3) * (gu_a + D.Ga[:, N] * abs(om) + np.abs(h))
    ns, ns_b, ok_min = sep_max(-s0, s0_b)
    xs, xs_b, ok_max = sep_max(s0, s0_b)
    ok_sign = bool(abs(ns) > ns_b)
    ts = max(T(1.5) * ns, T(0))
    ts_b = (T(1.5) * ns_b + _gam(T, 1) * ts) if ts > 0 else T(0)
    big = xs + ts
    ok_fl = bool(abs(big - 1) > xs_b + ts_b + _gam(T, 1) * abs(big))
    fl = T(0.1) * max(T(1), big)
    fl_b = (T(0.1) * (xs_b + ts_b + _gam(T, 1) * abs(big)) if big > 1 else T(0)) + _gam(T, 1) * fl
    sh = s0 + ts
    sh_b = s0_b + ts_b + _gam(T, 1) * np.abs(sh)
    s = np.maximum(sh, fl)
    s_b = np.maximum(sh_b, fl_b)
    lam0 = T(0.3) * D.slackW / mc
    lam = np.full(mc, lam0, dtype=T)
    lam[mc - 1] = D.slackW
    lam_b = np.full(mc, _gam(T, 2) * lam0, dtype=T)
    lam_b[mc - 1] = 0
    return {"s": (s, s_b), "lam": (lam, lam_b), "om": (om, om_b),
            "sep": {"omega": ok_om, "s min": ok_min and ok_sign, "s max": ok_max and ok_fl}}


def direction(D, st, corr, smu, ds=None):
    """The Newton back-substitution: ds = -rp - G dz and dl = -(rc + lam ds) / s with
    rc = s lam (+ sa la - smu if corr).  With ds given (a device's), dl is formed from it and
    its bound holds no image of ds's."""
    T, c = D.T, D.cnt
    s, lam, rp, dz = (_v(st, k, T) for k in ("s", "lam", "rp", "dz"))
    rc = s * lam
    rc_a = np.abs(rc)
    if corr:
        rc = rc + _v(st, "sa", T) * _v(st, "la", T) - T(smu)
        rc_a = rc_a + np.abs(_v(st, "sa", T) * _v(st, "la", T)) + abs(T(smu))
    ds0 = -rp - D.G @ dz
    ds_b = _gam(T, c.gx + 1) * (np.abs(rp) + D.Ga @ np.abs(dz))
    given = ds is not None
    ds = ds0 if not given else np.asarray(ds, dtype=T)
    dl = -(rc + lam * ds) / s
    dl_b = _gam(T, 8, 2) * (rc_a + np.abs(lam * ds)) / np.abs(s)
    if not given:
        dl_b = dl_b + np.abs(lam / s) * ds_b
    return {"ds": (ds0, ds_b), "dl": (dl, dl_b)}


def centring(D, st, mu, ds, dl):
    """sigma mu of Mehrotra's predictor from a given affine direction (a device's (ds, dl),
    taken as exact): a = min(1, the two ratio tests), mua = sum (s + a ds)(lam + a dl),
    sigma mu = (mua / mc / mu)^3 mu."""
    T, c = D.T, D.cnt
    s, lam = _v(st, "s", T), _v(st, "lam", T)
    ds, dl = np.asarray(ds, dtype=T), np.asarray(dl, dtype=T)
    zero = np.zeros_like(ds)
    num = np.concatenate([s, lam])
    a, a_b, ok = min_ratio(num, np.concatenate([ds, dl]), np.concatenate([zero, zero]), T)
    sn, ln = s + a * ds, lam + a * dl
    mua = _dot(sn, ln)
    mua_b = a_b * (np.abs(ds) @ np.abs(ln) + np.abs(dl) @ np.abs(sn)) + \
        _gam(T, 5 + c.sum_rows(D.mc)) * ((np.abs(s) + a * np.abs(ds)) @ (np.abs(lam) + a * np.abs(dl)))
    sr = mua / D.mc / T(mu)
    smu = sr * sr * sr * T(mu)
    smu_b = abs(smu) * (3 * mua_b / abs(mua) + _gam(T, 9))
    return {"smu": (smu, smu_b), "a": (a, a_b), "sep": {"affine step": ok}}


def corrector_tv(D, st, smu, ds, dl):
    """tv = dd rp - (s lam + ds dl - smu) / s from a given (ds, dl, smu)."""
    T = D.T
    s, lam, rp, dd = (_v(st, k, T) for k in ("s", "lam", "rp", "dd"))
    ds, dl = np.asarray(ds, dtype=T), np.asarray(dl, dtype=T)
    rc = s * lam + ds * dl - T(smu)
    tv = dd * rp - rc / s
    tv_b = _gam(T, 7, 2) * (np.abs(dd * rp) + (np.abs(s * lam) + np.abs(ds * dl) + abs(T(smu))) / np.abs(s))
    return {"tv": (tv, tv_b)}


def newton_rhs(D, st, tv):
    """rhs = -rd - G' tv from a given tv."""
    T, c = D.T, D.cnt
    rd = _v(st, "rd", T)
    v, _, a = gt(D, np.asarray(tv, dtype=T))
    g = np.full(D.n, gamma(c.gt_u + 2))
    g[D.N] = gamma(c.gt_w + 2)
    return {"rhs": (-rd - v, g.astype(T) * (np.abs(rd) + a))}


def site_update(D, st, smu, eta, leave_out_binding=False):
    """The corrector's direction, the two damped ratio tests and the new (z, s, lam), the
    bounds of ds and dl carried to first order.  leave_out_binding (tests only): the primal
    ratio test without its binding row."""
    T = D.T
    s, lam, z, dz = (_v(st, k, T) for k in ("s", "lam", "z", "dz"))
    dr = direction(D, st, 1, smu)
    (ds, ds_b), (dl, dl_b) = dr["ds"], dr["dl"]
    rp_, rp_b, okp = min_ratio(s, ds, ds_b, T, 4)
    rd_, rd_b, okd = min_ratio(lam, dl, dl_b, T, 4)
    if leave_out_binding and rp_ < 1:
        keep = np.ones(ds.size, dtype=bool)
        keep[int(np.argmin(np.where(ds < 0, -s / ds, T(np.inf))))] = False
        rp_ = min_ratio(s[keep], ds[keep], ds_b[keep], T, 4)[0]
    eta = T(eta)
    ap, ad = min(T(1), eta * rp_), min(T(1), eta * rd_)
    ap_b = (eta * rp_b + _gam(T, 1) * ap) if ap < 1 else T(0)
    ad_b = (eta * rd_b + _gam(T, 1) * ad) if ad < 1 else T(0)
    g2 = _gam(T, 2)
    zn = z + ap * dz
    zn_b = ap_b * np.abs(dz) + g2 * (np.abs(z) + np.abs(ap * dz))
    sn = s + ap * ds
    sn_b = ap_b * np.abs(ds) + ap * ds_b + g2 * (np.abs(s) + np.abs(ap * ds))
    ln = lam + ad * dl
    ln_b = ad_b * np.abs(dl) + ad * dl_b + g2 * (np.abs(lam) + np.abs(ad * dl))
    cap_ok = bool(abs(eta * rp_ - 1) > eta * rp_b + 2 * U and abs(eta * rd_ - 1) > eta * rd_b + 2 * U)
    return {"z": (zn, zn_b), "s": (sn, sn_b), "lam": (ln, ln_b), "ds": (ds, ds_b), "dl": (dl, dl_b),
            "ap": (ap, ap_b), "ad": (ad, ad_b), "ratio_p": (rp_, rp_b), "ratio_d": (rd_, rd_b),
            "sep": {"primal step": okp and cap_ok, "dual step": okd and cap_ok}}


def ratio(dev, ref, bnd):
    """max |dev - ref| / bnd; where the bound is zero an exact match counts 0, anything else inf."""
    dev = np.asarray(dev, dtype=F80).reshape(-1)
    ref = np.asarray(ref, dtype=F80).reshape(-1)
    bnd = np.asarray(bnd, dtype=F80).reshape(-1)
    err = np.abs(dev - ref)
    out = np.where(err == 0, F80(0), F80(np.inf))
    np.divide(err, bnd, out=out, where=bnd > 0)
    return float(out.max()) if out.size else 0.0
