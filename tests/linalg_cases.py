"""The case table of the linear-algebra tests (tests/test_linalg_host.py on the CPU,
tests/test_gpu_linalg.py on the GPU): matrices, orders and right-hand sides, all generated on
the host from a fixed seed.

Families
  (a) random SPD: A A' + n I, A standard normal.
  (b) the real KKT systems of the first QP of a dispatch_cases row (problem 0), captured by
      re-running the oracle's ``qp_ipm(init="omega")`` loop the way tools/polish_reuse_study.py
      does: P + G' diag(lam / s) G of the first, a middle and the last IPM iteration (the last
      is the ill-conditioned one), and the polish system P + rho I + G_A' G_A / delta at the
      oracle's POLISH_DELTA and POLISH_RHO.  For an order other than the row's own the leading
      n x n principal block is used: it stays positive definite.
  (c) indefinite and non-finite matrices for the failure path: an SPD matrix with one
      diagonal entry lowered so that exactly pivot k is non-positive, and one with a NaN.

Orders, per (HG, RM) pair of the product's kernels: the sweep (lead 0, family (a)) runs every
n from 2 to the largest order at which ``scpqp_plan_query`` returns that pair (a kernel with
RM row slots also runs the smaller problems of a mixed-horizon batch); the boundary set runs
with leads 0 to 3 on families (a) and (b)."""
import ctypes as C
import functools

import numpy as np

import dispatch_cases as DC
import linalg_mirror as M
from linalg_harness import CT_ORDERS, PAIRS

SEED = 20240611
BOUNDARY = (2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73, 127, 128, 129, 191, 192, 193, 249, 255, 256)
STAGES = ("ipm first", "ipm middle", "ipm last", "polish")
CB = 8
C_BOUND = 4.0      # the constant of both backward-error bounds (test_gpu_linalg docstring)


@functools.lru_cache(maxsize=None)
def max_orders():
    """{(HG, RM): largest n = V Hp + 1 over every shape the plan query accepts on that pair}."""
    from scpqp import _lib as LB
    lib = LB.load()
    info = LB.PlanInfo()
    best = {}
    for V in range(1, LB.MAX_VEH + 1):
        for O in range(0, LB.MAX_OBST + 1):
            for H in range(1, LB.MAX_HP + 1):
                D = LB.Dims(n_veh=V, hp_max=H, n_obst=O, max_batch=0)
                if lib.scpqp_plan_query(C.byref(D), 0, C.byref(info)) == 0:
                    key = (int(info.hg), int(info.rm))
                    best[key] = max(best.get(key, 0), V * H + 1)
    return best


def case_orders(pair):
    """Every order a dispatch_cases row runs on the pair (its mixed-horizon problems too)."""
    out = set()
    for c in DC.CASES:
        if (c.kernel[0], c.kernel[2]) != pair:
            continue
        out.add(c.n_veh * c.hp_max + 1)
        for h in c.hps or ():
            out.add(c.n_veh * h + 1)
        if c.mixed is not None:
            out.update(c.mixed[0] * h + 1 for h in c.mixed[2])
    return out


def boundary_orders(pair):
    nmax = max_orders()[pair]
    s = set(BOUNDARY) | case_orders(pair) | set(CT_ORDERS)
    return sorted(n for n in s if 2 <= n <= nmax)


def sweep_orders(pair):
    """Every n from 2 to the pair's largest order.  (The 80-bit products of the 255 matrices of
    the largest pair take about 10 s of CPU time, so no order is left out.)"""
    return list(range(2, max_orders()[pair] + 1))


def _rng(*key):
    return np.random.default_rng([SEED, *key])


@functools.lru_cache(maxsize=None)
def spd(n):
    """Family (a)."""
    A = _rng(1, n).standard_normal((n, n))
    K = A @ A.T + n * np.eye(n)
    return M.full_lower(K)


def rhs(K, tag):
    """Two right-hand sides of a system: standard normal, and K times the vector of ones."""
    n = K.shape[0]
    return np.stack([_rng(2, n, tag).standard_normal(n), K @ np.ones(n)])


# ---------------------------------------------------------------------------------------
# family (b)
# ---------------------------------------------------------------------------------------
def ipm_systems(P, q, G, h, tol=None, maxit=60, iterates=None):
    """qp_ipm(init='omega') of the oracle, restated as tools/polish_reuse_study.py does, that
    also returns the normal matrix of every iteration: (x, s, lam, iterations, status, [K]).
    ``iterates``: a list that receives, per iteration that factors, a dict of the iterate
    (x s lam rd rp mu), the affine direction (dx_aff ds_aff dl_aff), sigma mu (smu), the
    corrected direction (dx ds dl) and the damped steps (eta ap ad); tests/qp_phase_cases.py."""
    from oracle import scp_reference as R
    import scipy.linalg
    tol = R.IPM_TOL if tol is None else tol
    mc = len(h)
    x, s, lam = R.ipm_start_omega(P, q, G, h)
    qn = max(1.0, np.abs(q).max())
    hn = max(1.0, np.abs(h).max())
    Ks = []
    for it in range(maxit):
        rd = P @ x + q + G.T @ lam
        rp = G @ x + s - h
        gap = s @ lam
        pobj = 0.5 * x @ P @ x + q @ x
        if (np.abs(rp).max() <= tol * hn and np.abs(rd).max() <= tol * qn
                and gap <= tol * max(1.0, abs(pobj))):
            return x, s, lam, it, 1, Ks
        mu = gap / mc
        d = lam / s
        K = P + G.T @ (d[:, None] * G)
        try:
            Lc = np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            return x, s, lam, it, 2, Ks
        Ks.append(K)

        def solve(rc):
            dx = scipy.linalg.cho_solve((Lc, True), -rd - G.T @ (d * rp - rc / s))
            ds = -rp - G @ dx
            return dx, ds, -(rc + lam * ds) / s
        dx, ds, dl = solve(s * lam)
        a = R._max_step(s, ds, lam, dl)
        sigma = ((s + a * ds) @ (lam + a * dl) / mc / mu) ** 3
        aff = (dx, ds, dl)
        dx, ds, dl = solve(s * lam + ds * dl - sigma * mu)
        eta = max(0.99, 1.0 - mu)
        ap = min(1.0, eta * R._max_step(s, ds, np.ones_like(lam), np.zeros_like(dl)))
        ad = min(1.0, eta * R._max_step(np.ones_like(s), np.zeros_like(ds), lam, dl))
        if iterates is not None:
            iterates.append(dict(x=x, s=s, lam=lam, rd=rd, rp=rp, mu=mu, dx_aff=aff[0], ds_aff=aff[1],
                                 dl_aff=aff[2], smu=sigma * mu, dx=dx, ds=ds, dl=dl, eta=eta, ap=ap, ad=ad))
        x = x + ap * dx
        s = s + ap * ds
        lam = lam + ad * dl
    return x, s, lam, maxit, 0, Ks


def first_qp(src, b=0):
    """The scaled first QP (P, q, G, h) of problem b of a source (scenario, n_veh, hp_max, s),
    inputs as dispatch_cases makes them."""
    sc, bt = DC.make_inputs(*src)
    return DC.first_qp_job(DC.oracle_jobs(src[0], src[1], sc, bt)[b])


# What family (b) is captured from: dispatch_cases rows, one per order, the orders spread over
# the row slots, and, because no row reaches past n = 241, the circle of 5 vehicles at Hp 51
# (n = 256) for the orders above.
KKT_ROWS = ("k00130_frog1x10", "k01230_circle8x8", "k01231_circle4x20", "k01320_circle12x12",
            "k11320_circle6x22", "k11430_circle7x28", "k11423_circle8x30")
KKT_SOURCES = tuple((DC.by_id(c).scenario, DC.by_id(c).n_veh, DC.by_id(c).hp_max, DC.by_id(c).s)
                    for c in KKT_ROWS) + (("circle", 5, 51, 1.0),)


@functools.lru_cache(maxsize=None)
def kkt_systems(src):
    """({stage: K} of a source's first QP (STAGES), the restated IPM's iteration count and
    status)."""
    from oracle import scp_reference as R
    P, q, G, h = first_qp(src)
    x, s, lam, it, st, Ks = ipm_systems(P, q, G, h)
    assert len(Ks) >= 3, (src, len(Ks))
    act = lam > s
    Ga = G[act]
    Kp = P + R.POLISH_RHO * np.eye(len(q)) + Ga.T @ Ga / R.POLISH_DELTA
    last = max(i for i, K in enumerate(Ks) if pivot_margin(M.full_lower(K)) >= 2 * C_BOUND)
    assert last >= len(Ks) - 3 and last > len(Ks) // 2, (src, last, len(Ks))
    out = {"ipm first": Ks[0], "ipm middle": Ks[len(Ks) // 2], "ipm last": Ks[last], "polish": Kp}
    return {k: M.full_lower(v) for k, v in out.items()}, it, st


def pivot_margin(K):
    """min_k D_k / (gamma(n + 1) (|L||D||L'|)_kk) of the fp64 mirror, 0 if a pivot is not
    positive: how far every pivot is from zero in units of the componentwise backward-error
    bound on its diagonal entry.  The IPM's last systems are singular to working precision
    (the oracle's own Cholesky breaks down on the next one on half the rows, status 2, and
    the mirror's smallest pivot of the very last one is 0.1 to 1 of these units, negative on
    8 vehicles at Hp 30): whether such a factorisation succeeds is decided by the rounding,
    and the solver treats a failure there as the end of the central path.  "ipm last" is
    therefore the last iteration whose margin is at least 2 C_BOUND, twice what the asserted
    bound lets a correct factorisation move a pivot: always one of the last three, with
    condition numbers of 1e13 and more."""
    L, D, fail = M.ldl(K)
    if fail is not None:
        return 0.0
    Pa = (np.abs(L) * D) @ np.abs(L).T
    return float(np.min(D / np.diag(Pa)) / M.gamma(K.shape[0] + 1))


def kkt_source_for(n):
    """The source whose own order is the smallest one >= n."""
    for m, src in sorted((s[1] * s[2] + 1, s) for s in KKT_SOURCES):
        if m >= n:
            return src
    raise ValueError(n)


def kkt(n, stage):
    """Family (b) at order n: the leading principal block of the nearest source's system."""
    return kkt_systems(kkt_source_for(n))[0][stage][:n, :n]


# ---------------------------------------------------------------------------------------
# family (c)
# ---------------------------------------------------------------------------------------
def indefinite(n, k):
    """spd(n) with entry (k, k) lowered by 1.5 times pivot k of the fp64 mirror: the pivots
    before k are unchanged and pivot k becomes about -0.5 times its old value."""
    K = spd(n).copy()
    _, D, fail = M.ldl(K)
    assert fail is None
    K[k, k] -= 1.5 * D[k]
    return K


def with_nan(n):
    """spd(n) with a NaN at (n // 2, n // 3): the first pivot it reaches is n // 2."""
    K = spd(n).copy()
    K[n // 2, n // 3] = K[n // 3, n // 2] = np.nan
    return K, n // 2


def failure_cases(pair):
    """[(label, K, k)]: pivot k must be the first non-positive one.  Per pair a matrix whose
    last panel is short (jb = 5) and one whose last panel is the lone pivot (jb == 1), at the
    small end and near the pair's largest order; k at the first and the second column of a
    pivot pair in the first panel, a middle panel and the last panel."""
    nmax = max_orders()[pair]
    big = (nmax - 1) // CB * CB       # n = big + 1: jb == 1; n = big - 3: jb = 5
    out = []
    for n5, n1 in ((29, 25), (big - 3, big + 1)):
        r0 = n5 // CB * CB
        mid = (r0 // CB // 2) * CB
        for k in (0, 1, mid + 2, mid + 3, r0 + 2, r0 + 3):
            out.append((f"n {n5} pivot {k}", indefinite(n5, k), k))
        out.append((f"n {n1} lone pivot {n1 - 1}", indefinite(n1, n1 - 1), n1 - 1))
        Kn, kn = with_nan(n5)
        out.append((f"n {n5} NaN", Kn, kn))
    return out
