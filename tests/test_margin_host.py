"""Obstacle margins without a GPU (include/scpqp_margin.h):

1. the boundary: the header's three functions, their exports, ``scpqp_batch_in`` left as it was
   (a gcc probe of the header), argument validation before any HIP call;
2. the solver mirror (tests/margin_solver_mirror.py): at zero margin the oracle bitwise, a
   per-obstacle constant margin the oracle with ``dsafe_obs + m_o`` bitwise, and the input
   conditions of tests/margin_cases.py on the mirror alone;
3. the margin mirror (tests/margin_mirror.py): its limits and invariances, the derivation of
   the GPU tolerance, and the calibration of ``kappa_for(0.05)``.
"""
import copy
import ctypes as C
import math
import multiprocessing as mp
import os
import re
import subprocess

import numpy as np
import pytest

import imm_mirror as IM
import manoeuvre_mirror as MNM
import margin_cases as MC
import margin_mirror as MM
import margin_solver_mirror as MS
import tracker_accel_cases as TC
import tracker_accel_mirror as AM
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import margin as MG
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "scpqp_margin.h")
E_ARG, E_SIZE = -1, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(8) as p:
        yield p


# ---------------------------------------------------------------------------
# 1. boundary
# ---------------------------------------------------------------------------
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_margin.h"
/* the prototypes, restated: a mismatch with the header's is a compile error */
int scpqp_solve_margin(scpqp_handle* h, int32_t B, const scpqp_batch_in* in,
                       const double* obst_margin, const scpqp_batch_out* out, void* stream);
int scpqp_evaluate_margin(scpqp_handle* h, int32_t B, const scpqp_batch_in* in,
                          const double* obst_margin, const double* u, const scpqp_eval_out* out,
                          void* stream);
int main(void) {
  printf("%zu %zu\n", sizeof(scpqp_batch_in), offsetof(scpqp_batch_in, variant));
  return 0;
}
"""


def test_the_margin_entry_points_leave_batch_in_alone(tmp_path, lib):
    """The margins reach the solve through scpqp_solve_margin / scpqp_evaluate_margin of
    scpqp_margin.h; scpqp_batch_in is what it was (it still ends with the variant pointer), so
    a caller built against scpqp.h alone passes a struct of the size the library reads."""
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{INCLUDE}", str(src), "-o", str(exe)],
                   check=True)
    size, off_var = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                            check=True).stdout.split())
    assert LB.BatchIn._fields_[-1][0] == "variant" and not hasattr(LB.BatchIn, "obst_margin")
    assert size == C.sizeof(LB.BatchIn) == off_var + 8 and off_var == LB.BatchIn.variant.offset
    V = C.c_void_p
    assert lib.scpqp_solve_margin.argtypes == [V, C.c_int32, C.POINTER(LB.BatchIn), V,
                                               C.POINTER(LB.BatchOut), V]
    assert lib.scpqp_evaluate_margin.argtypes == [V, C.c_int32, C.POINTER(LB.BatchIn), V, V,
                                                  C.POINTER(LB.EvalOut), V]
    # the argument checks of scpqp_solve and scpqp_evaluate, before any device is touched
    bi, bo, eo = LB.BatchIn(), LB.BatchOut(), LB.EvalOut()
    assert lib.scpqp_solve_margin(None, 1, C.byref(bi), None, C.byref(bo), None) == E_ARG
    assert b"null handle" in lib.scpqp_last_error()
    assert lib.scpqp_evaluate_margin(None, 1, C.byref(bi), None, None, C.byref(eo), None) == E_ARG


def test_header_declares_the_boundary_and_the_definition():
    txt = open(HEADER).read()
    assert sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M))) == sorted(LB.MARGIN_EXPORTS) \
        == ["scpqp_evaluate_margin", "scpqp_obstacles_margin", "scpqp_solve_margin"]
    for word in ("sqrt(6)", "1 / 12", "tau_k Q_POS", "cbar", "hypot", "min(kappa * sqrt(lam), m_max)",
                 "Off lane", "Trouble", "not initialised", "What the margin does not know",
                 "Non-Gaussian", "footprint", "exp(-kappa^2 / 2)", "sqrt(-2 ln p_miss)",
                 "upper triangles", "dsafe_extra + obst_margin[b][o][k]", "all-zero array",
                 "SCPQP_ST_INVALID with zero counters", "past the prefix are never read",
                 "scpqp_batch_in itself is unchanged"):
        assert word in txt, word


def test_library_exports_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert set(LB.MARGIN_EXPORTS) <= set(re.findall(r"\sT\s(scpqp_\w+)", out))
    for name in LB.MARGIN_EXPORTS:
        assert getattr(lib, name).argtypes is not None


def test_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    D = C.cast(buf, C.c_void_p)

    def err():
        return lib.scpqp_last_error()

    def call(B=0, n_obst=2, hp=5, M=2, trk=None, x=None, cov=None, mu=None, lead=0.1, dt=0.4,
             kappa=2.0, m_max=1.0, margin=None, sigma=None):
        return lib.scpqp_obstacles_margin(B, n_obst, hp, M, trk, x, cov, mu, lead, dt, kappa,
                                          m_max, margin, sigma, None)

    assert call() == 0                                       # B = 0: a no-op, NULL arrays
    assert call(kappa=0.0, m_max=0.0) == 0
    assert call(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_OBST + 1):
        assert call(n_obst=n) == E_ARG and b"n_obst" in err()
    for h in (0, -1, LB.MAX_HP + 1):
        assert call(hp=h) == E_ARG and b"hp" in err()
    for m in (0, -1, 5):
        assert call(M=m) == E_ARG and b"n_modes" in err()
    for kw in (dict(lead=math.inf), dict(dt=math.nan)):
        assert call(**kw) == E_ARG and b"finite" in err()
    for v in (-1e-9, math.nan, math.inf):
        assert call(kappa=v) == E_ARG and b"kappa" in err()
        assert call(m_max=v) == E_ARG and b"m_max" in err()
    full = dict(trk=D, x=D, cov=D, mu=D, margin=D)
    for missing, word in (("trk", b"trk"), ("x", b"null x"), ("cov", b"cov"), ("mu", b"mu"),
                          ("margin", b"margin")):
        kw = dict(full)
        kw[missing] = None
        assert call(B=3, **kw) == E_ARG and word in err(), missing
    # sizes before the pointers: nothing is launched for a size error
    assert call(B=1 << 24, n_obst=1, M=4, **full) == E_SIZE and b"36" in err()
    assert call(B=1 << 24, n_obst=1, M=4) == E_SIZE
    assert call(B=1 << 22, n_obst=4, hp=64, M=1, **full) == E_SIZE and b"hp" in err()


def test_python_side_validates():
    assert MG.kappa_for(0.05) == math.sqrt(-2.0 * math.log(0.05)) == MM.kappa_for(0.05)
    assert MG.kappa_for(1.0) == 0.0
    for p in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            MG.kappa_for(p)
    assert MG.validate(2, 1) == (2.0, 1.0)
    for bad in ((-1.0, 1.0), (math.nan, 1.0), (1.0, -1e-9), (1.0, math.inf)):
        with pytest.raises(ValueError):
            MG.validate(*bad)


# ---------------------------------------------------------------------------
# 2. the solver mirror
# ---------------------------------------------------------------------------
def _zero_job(args):
    MC._paths()
    cid, b = args
    sc, bt, _ = MC.inputs(MC.by_id(cid))
    p = MC.problem(sc, bt, b)
    return bool(np.array_equal(MS.scp_solve(p, None).u, R.scp_solve(p, mode="structured").u))


def test_mirror_at_zero_margin_is_the_oracle_bitwise(pool):
    jobs = [(cid, b) for cid in MC.IDS for b in range(MC.N_PROBLEMS)]
    assert len(jobs) == 48 and all(pool.map(_zero_job, jobs, chunksize=2))


def exact_scenario(sc, add=None):
    """``sc`` with its obstacle safety distances rounded to multiples of 2^-20 (plus ``add``
    [nObst], multiples of 2^-20 too): every sum dsafe + dsafe_extra + m is then exact in either
    order, and a constant margin and a larger dsafe_obs are one problem bitwise."""
    out = copy.deepcopy(sc)
    d = np.round(np.asarray(sc.dsafeObstacles, float).reshape(sc.nVeh, sc.nObst) * 2.0 ** 20) / 2.0 ** 20
    out.dsafeObstacles = d if add is None else d + np.asarray(add)[None, :]
    out.dsafeExtra = round(float(sc.dsafeExtra) * 2.0 ** 20) / 2.0 ** 20
    return out


CONST_MARGIN = lambda nO: 0.25 * (np.arange(nO) % 3)


def _const_job(args):
    MC._paths()
    cid, b = args
    sc, bt, _ = MC.inputs(MC.by_id(cid))
    m = CONST_MARGIN(sc.nObst)
    p = MC.problem(exact_scenario(sc), bt, b)
    q = MC.problem(exact_scenario(sc, m), bt, b)
    assert np.array_equal(q.dsafe_obs, p.dsafe_obs + m[None, :])
    a = MS.scp_solve(p, np.repeat(m[:, None], p.Hp, axis=1))
    o = R.scp_solve(q, mode="structured")
    moved = float(np.max(np.abs(a.u - MS.scp_solve(p, None).u)))
    return bool(np.array_equal(a.u, o.u)) and a.n_scp == o.n_scp, moved


def test_constant_margin_is_a_larger_safety_distance(pool):
    for cid in ("frog1x20", "parallel5x10"):
        res = pool.map(_const_job, [(cid, b) for b in range(MC.N_PROBLEMS)], chunksize=1)
        assert all(ok for ok, _ in res), cid
        # the comparison says something: the constant moves every frog problem's u (in the
        # parallel shape the rows that bind are pair rows, and u stays)
        if cid == "frog1x20":
            assert min(mv for _, mv in res) > MC.MOVE_MIN, cid


@pytest.mark.parametrize("cid", MC.IDS)
def test_solver_case_conditions(pool, cid):
    c = MC.by_id(cid)
    with_m = pool.map(MC.mirror_job, MC.mirror_jobs(cid, True), chunksize=1)
    assert all(h["certified"] for r in with_m for h in r.history)
    assert all(r.converged and r.n_scp < R.MAX_SCP_ITER for r in with_m)
    print(f"margin_cases {cid}: n_scp {[r.n_scp for r in with_m]}, active rows "
          f"{[r.active for r in with_m]}")
    if c.frog and c.hps is None:
        without = pool.map(MC.mirror_job, MC.mirror_jobs(cid, False), chunksize=1)
        moved = [float(np.max(np.abs(a.u - b.u))) for a, b in zip(with_m, without)]
        print(f"margin_cases {cid}: max |du| against zero margin {['%.1e' % v for v in moved]}")
        assert min(r.n_scp for r in with_m) >= 4
        assert min(r.active for r in with_m) >= 2
        assert min(moved) > MC.MOVE_MIN


# ---------------------------------------------------------------------------
# 3. the margin mirror
# ---------------------------------------------------------------------------
LEAD, DT = MC.lead_dt()
KAPPA = MM.kappa_for(MC.P_MISS)


def good_lane(M=2, g=0):
    """(trk [M, 14], x [M, 6], P [M, 6, 6], mu [M]) of a good lane of the (2, 3, 5) case."""
    trk, x, cov, mu = MC.states(2, 3, 5, M)
    b, o = divmod(g, 3)
    assert not IM.is_off_lane(trk[b, o]) and np.isfinite(x[b, o]).all()
    return trk[b, o].copy(), x[b, o].copy(), cov[b, o].copy(), mu[b, o].copy()


def test_small_covariance_leaves_the_position_process_noise():
    trk, x, P, _ = good_lane(1)
    trk[0, AM.Q_POS] = 0.05
    _, S = MM.lane(trk, x, P * 1e-30, None, LEAD, DT, 5, KAPPA, MC.M_MAX)
    tau = (np.arange(5) + 1) * DT + LEAD
    assert np.allclose(S[:, 0], tau * 0.05 ** 2, rtol=1e-12, atol=0)
    assert np.allclose(S[:, 2], tau * 0.05 ** 2, rtol=1e-12, atol=0)
    assert np.abs(S[:, 1]).max() < 1e-25


def test_two_identical_modes_equal_one():
    trk, x, P, _ = good_lane(1)
    m1, S1 = MM.lane(trk, x, P, None, LEAD, DT, 5, KAPPA, MC.M_MAX)
    two = lambda a: np.repeat(a, 2, axis=0)
    m2, S2 = MM.lane(two(trk), two(x), two(P), np.array([0.25, 0.75]), LEAD, DT, 5, KAPPA, MC.M_MAX)
    assert np.allclose(S2, S1, rtol=1e-13, atol=1e-18) and np.allclose(m2, m1, rtol=1e-13)
    # a mode with mu exactly 0 is skipped, whatever its state
    x0 = two(x)
    x0[1, :2] += 50.0
    m3, S3 = MM.lane(two(trk), x0, two(P), np.array([1.0, 0.0]), LEAD, DT, 5, KAPPA, MC.M_MAX)
    assert np.array_equal(S3, S1) and np.array_equal(m3, m1)


def test_zero_covariance_gives_the_spread_between_the_modes():
    trk, x, P, _ = good_lane(2)
    trk[:, AM.Q_POS] = 0.0
    x[1, :2] += (0.3, -0.4)
    mu = np.array([0.3, 0.7])
    c = [AM.horizon(x[j], trk[j], LEAD, DT, 5) for j in range(2)]
    d = c[0] - c[1]
    w = mu[0] * mu[1]                                      # sum_j mu_j (c_j - cbar)^2
    _, S = MM.lane(trk, x, P * 1e-30, mu, LEAD, DT, 5, KAPPA, MC.M_MAX)
    want = np.stack([w * d[0] * d[0], w * d[0] * d[1], w * d[1] * d[1]], axis=1)
    assert np.allclose(S, want, rtol=1e-12, atol=1e-20)


def test_sigma_is_psd_and_lam_is_its_largest_eigenvalue():
    worst = 0.0
    for M in MC.MODES:
        trk, x, cov, mu = MC.states(2, 3, 5, M)
        m, S = MM.step(trk, x, cov, mu, LEAD, DT, 5, 1.0, MC.M_MAX)
        for s, mk in zip(S.reshape(-1, 3), m.reshape(-1)):
            ev = np.linalg.eigvalsh(np.array([[s[0], s[1]], [s[1], s[2]]]))
            assert ev[0] >= -1e-15 * ev[1]
            worst = max(worst, abs(mk - math.sqrt(ev[1])) / max(1.0, mk)) if ev[1] > 0 else worst
    assert worst <= 1e-14


def test_mode_permutation_invariance():
    trk, x, cov, mu = MC.states(2, 3, 5, 3)
    perm = [2, 0, 1]
    a = MM.step(trk, x, cov, mu, LEAD, DT, 5, KAPPA, MC.M_MAX)
    b = MM.step(trk[:, :, perm], x[:, :, perm], cov[:, :, perm], mu[:, :, perm], LEAD, DT, 5, KAPPA,
                MC.M_MAX)
    # two float64 runs that differ only in the order of the mode sums: each within the
    # measured rounding of the exact result (MC.MIRROR_ROUNDING), so at most twice that apart
    assert MC.ratio(a, b) <= 2 * MC.MIRROR_ROUNDING


def test_off_and_trouble_lanes():
    trk, x, P, mu = good_lane(2)
    hp = 5
    run = lambda t=trk, xx=x, pp=P, m=mu: MM.lane(t, xx, pp, m, LEAD, DT, hp, KAPPA, MC.M_MAX)
    m, S = run()
    assert np.isfinite(m).all() and (m > 0).all()
    m, S = run(t=np.zeros_like(trk), xx=np.full_like(x, np.nan))
    assert (m == 0).all() and (S == 0).all()
    for kind, (t, xx, pp, mm) in trouble_lanes(trk, x, P, mu).items():
        m, S = MM.lane(t, xx, pp, mm, LEAD, DT, hp, KAPPA, MC.M_MAX)
        assert np.isnan(m).all() and np.isnan(S).all(), kind


def trouble_lanes(trk, x, P, mu):
    """Every kind of trouble of the header on copies of a good two-mode lane."""
    out = {}

    def put(kind, t=None, xx=None, pp=None, mm=None):
        out[kind] = tuple(a.copy() for a in (trk if t is None else t, x if xx is None else xx,
                                             P if pp is None else pp, mu if mm is None else mm))

    a = x.copy(); a[0, 0] = np.nan; put("not_initialised", xx=a)
    a = trk.copy(); a[1, AM.A_HOLD] = -1e-3; put("bad_row", t=a)
    a = trk.copy(); a[1] = 0.0; put("mixed", t=a)
    a = x.copy(); a[1, 4] = np.inf; put("x_inf", xx=a)
    a = P.copy(); a[0, 1, 3] = np.nan; put("p_nan", pp=a)
    a = mu.copy(); a[1] = np.nan; put("mu_nan", mm=a)
    a = mu.copy(); a[0] = -0.1; put("mu_negative", mm=a)
    put("mu_none_positive", mm=np.zeros_like(mu))
    a = P.copy(); a[1, 2, 2] = -1.0; put("pivot", pp=a, mm=np.array([0.5, 0.5]))
    return out


def test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies():
    worst = {}
    for (B, nO, hp) in MC.SHAPES:
        for M in MC.MODES:
            trk, x, cov, mu = MC.states(B, nO, hp, M)
            a = MM.step(trk, x, cov, mu, LEAD, DT, hp, KAPPA, MC.M_MAX, MM.F64)
            b = MM.step(trk, x, cov, mu, LEAD, DT, hp, KAPPA, MC.M_MAX, MM.F80)
            worst[(B, nO, hp, M)] = MC.ratio(a, b)
            m = np.asarray(a[0], float)
            assert np.nanmax(m) < MC.M_MAX                 # nothing is capped
            if (B, nO, hp) == (12, 22, 10):
                # the case holds good, off and trouble lanes
                assert np.isnan(m[..., 0]).sum() >= 10 and (m == 0).all(-1).sum() == 38
                assert (m[..., 0] > 0).sum() >= 200
    big = max(worst.values())
    print("margin mirror float64 against 80-bit:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert 0.5 * MC.MIRROR_ROUNDING <= big <= MC.MIRROR_ROUNDING
    assert MC.TOL == MC.pow2_ceil(16 * MC.MIRROR_ROUNDING)


def test_calibration_of_kappa_for_five_percent():
    """The share of 20 000 states drawn from N(x, P) of filtered lanes whose predicted point lies
    farther than the margin from the told point, per horizon step, with Q_POS = 0 in the rows
    and nothing capped.  Measured: 0.0394, 0.0386, 0.0381, 0.0380, 0.0378, 0.0375 (below 0.05:
    the bound exp(-kappa^2 / 2) is attained by a circular Sigma only, and these are longer along
    the track than across it); the covariances are used as filtered (CAL_P_SCALE = 1)."""
    rows, man, osense, trk, _ = TC.consistency_inputs(MC.CAL_B, MC.CAL_NO)
    assert (trk[..., AM.Q_POS] == 0).all() and MC.CAL_P_SCALE == 1.0
    x, cov = AM.alloc(MC.CAL_B, MC.CAL_NO)
    for s in range(TC.CONS_STEPS + 1):
        AM.step(MNM.state(rows, man, s * TC.CONS_T), osense, TC.CONS_SEED, s, 0, trk, 0.0,
                0.0 if s == 0 else TC.CONS_T, TC.CONS_LEAD, TC.CONS_DT, TC.CONS_HP, x, cov)
    hp = TC.CONS_HP
    mg, _ = MM.step(trk, x, cov, None, TC.CONS_LEAD, TC.CONS_DT, hp, MM.kappa_for(0.05), 1e6)
    rng = np.random.default_rng(MC.CAL_SEED)
    out, n = np.zeros(hp), 0
    for b in range(MC.CAL_B):
        for o in range(MC.CAL_NO):
            L = np.linalg.cholesky(cov[b, o])
            c = AM.horizon(x[b, o], trk[b, o], TC.CONS_LEAD, TC.CONS_DT, hp)
            for _ in range(MC.CAL_DRAWS):
                p = AM.horizon(x[b, o] + L @ rng.standard_normal(6), trk[b, o], TC.CONS_LEAD,
                               TC.CONS_DT, hp)
                out += np.hypot(p[0] - c[0], p[1] - c[1]) > mg[b, o]
                n += 1
    share = out / n
    print("calibration: share beyond the margin per horizon step", share)
    assert n == 20000 and abs(MC.CAL_BOUND - 0.0546) < 5e-5
    assert share.max() <= MC.CAL_BOUND
    assert share.min() > 0.005                             # the margin is not vacuous either
