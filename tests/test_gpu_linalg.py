"""The L D L' factorisation (``cholesky``: panel_factor, trailing_update, trailing_update_mfma)
and the lead wave's triangular solves (``chol_solve`` / ``Solver``) of csrc/scpqp_kernel.h,
called outside the solver by tests/linalg/linalg_harness.hip and held to an 80-bit reference
at every order n and every lead wave (tests/linalg_cases.py has the case table,
tests/linalg_mirror.py the reference).

Bounds.  With u = 2^-53 and gamma(k) = k u / (1 - k u):

  factor   |K - L D L'| <= c gamma(n + 1) |L||D||L'|   componentwise, D = 1 / dinv in 80-bit
  solve    |b - L D L' x| <= c gamma(3 n + 1) |L||D||L'||x|   with the device's own factor

Higham's bound for a factorisation without pivoting holds for any order of the sums, so it
covers the panel, the 2 x 2 register tiles and the MFMA tiles alike.  c = 4 because the
device forms every quotient as ``recip(x) * y``.  ``recip`` is v_rcp_f64 (relative error up to
2^-50 or so: it only seeds the iteration) and two Newton steps r += r (1 - x r) with the
residual in one FMA; each step squares the error, so after two the result is the rounding of
a value within 2^-100 of 1 / x: relative error at most u (1 + 2^-46), not always the
correctly rounded reciprocal.  A quotient therefore takes two roundings, (1 + d1)(1 + d2),
and the second pivot of a pair three, d1 = det * recip(d0) with det = fma(d0, e, -(b b)),
where a division takes one; gamma counts one rounding per operation.

Bitwise equalities: the lead wave only decides which wave runs the serial parts and which
tiles a trailing wave takes (every tile is computed by one thread or wave with the same
operations whoever takes it), so leads 0 to 3 give the same bits; the compile-time Solver
performs "the same operations in the same order" as the run-time one; two workgroups of a
launch that run the same case agree.

Every test prints ``linalg_gpu`` lines with its figures; profiles/linalg_gpu_tests.txt is one
run's output."""
import numpy as np
import pytest

import linalg_cases as LC
import linalg_harness as LH
import linalg_mirror as M

pytestmark = pytest.mark.gpu

PAIR_IDS = ["hg%d_rm%d" % p for p in LH.PAIRS]
LEADS = (0, 1, 2, 3)
FAMILIES = ("a",) + LC.STAGES


def matrix(fam, n):
    return LC.spd(n) if fam == "a" else LC.kkt(n, fam)


_runs = {}


def device_run(pair):
    """One launch per pair with every case of every test below: {key: (K, rhs, Result)}."""
    if pair in _runs:
        return _runs[pair]
    keys, cases = [], []

    def add(key, K, lead, form, b):
        keys.append(key)
        cases.append((K, lead, form, b))
    rhs = {}

    def system(fam, n):
        if (fam, n) not in rhs:
            K = matrix(fam, n)
            rhs[(fam, n)] = (K, LC.rhs(K, FAMILIES.index(fam)))
        return rhs[(fam, n)]
    for n in LC.sweep_orders(pair):
        K, b = system("a", n)
        add(("sweep", n), K, 0, 0, b)
    for n in LC.boundary_orders(pair):
        for fam in FAMILIES:
            K, b = system(fam, n)
            for lead in LEADS:
                add(("bnd", fam, n, lead), K, lead, 0, b)
        K, b = system("a", n)
        add(("dup", n), K, 0, 0, b)
        if n in LH.CT_ORDERS:
            for fam in ("a", "ipm last"):
                K, b = system(fam, n)
                for lead in LEADS:
                    add(("ct", fam, n, lead), K, lead, n, b)
    for i, (label, K, k) in enumerate(LC.failure_cases(pair)):
        for lead in (0, 3):
            add(("fail", i, lead), K, lead, 0, np.zeros((1, K.shape[0])))
    res = LH.run(pair[0], pair[1], cases)
    _runs[pair] = {key: (c[0], c[3], r) for key, c, r in zip(keys, cases, res)}
    return _runs[pair]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(r0, r1):
    return (np.array_equal(bits(r0.L), bits(r1.L)) and np.array_equal(bits(r0.dinv), bits(r1.dinv))
            and np.array_equal(bits(r0.x), bits(r1.x)))


def ratios(K, b, r):
    """(factor ratio, solve ratio) of one result, in units of gamma (not yet divided by c)."""
    prods = M.products(r.L, M.F80(1) / r.dinv.astype(M.F80))
    fr = M.factor_ratio(K, r.L, r.dinv, prods)
    sr = max(M.solve_ratio(r.L, r.dinv, b[i], r.x[i], prods) for i in range(b.shape[0]))
    return fr, sr


@pytest.mark.parametrize("pair", LH.PAIRS, ids=PAIR_IDS)
def test_return_value_and_canaries(gpu, pair):
    """cholesky returns true on every matrix of families (a) and (b) and false on every one of
    (c); nothing after the factor's plan allocation, after entry n - 1 of dinv or of x is
    written, for any case."""
    run = device_run(pair)
    assert len(run) > 100
    for key, (K, b, r) in run.items():
        assert r.bad == (0, 0, 0, 0), (pair, key, r.bad)
        assert r.ok == (key[0] != "fail"), (pair, key)
    print(f"linalg_gpu {pair} {len(run)} cases in one launch: return values as expected, "
          f"every canary intact")


@pytest.mark.parametrize("pair", LH.PAIRS, ids=PAIR_IDS)
def test_sweep_backward_error(gpu, pair):
    """Family (a) at every order of the sweep, lead 0: both componentwise bounds."""
    run = device_run(pair)
    worst_f = worst_s = (0.0, None)
    for n in LC.sweep_orders(pair):
        K, b, r = run[("sweep", n)]
        assert np.all(np.isfinite(r.x)) and np.all(r.dinv > 0), (pair, n)
        fr, sr = ratios(K, b, r)
        worst_f = max(worst_f, (fr, n))
        worst_s = max(worst_s, (sr, n))
    print(f"linalg_gpu {pair} sweep n 2..{LC.max_orders()[pair]} ({len(LC.sweep_orders(pair))} orders): "
          f"factor |K - LDL'| / (gamma(n+1) |L||D||L'|) max {worst_f[0]:.3f} at n {worst_f[1]}, "
          f"solve |b - LDL'x| / (gamma(3n+1) |L||D||L'||x|) max {worst_s[0]:.3f} at n {worst_s[1]}; "
          f"bound c = {LC.C_BOUND}")
    assert worst_f[0] <= LC.C_BOUND, (pair, worst_f)
    assert worst_s[0] <= LC.C_BOUND, (pair, worst_s)


@pytest.mark.parametrize("pair", LH.PAIRS, ids=PAIR_IDS)
def test_boundary_backward_error(gpu, pair):
    """Families (a) and (b) at the boundary orders, lead 0: both bounds; the forward error of
    the family-(b) systems per stage is printed, not asserted (the matrix's conditioning
    governs it)."""
    run = device_run(pair)
    worst = {f: [0.0, 0.0, 0.0] for f in FAMILIES}
    over = []
    for n in LC.boundary_orders(pair):
        for fam in FAMILIES:
            K, b, r = run[("bnd", fam, n, 0)]
            assert np.all(np.isfinite(r.x)), (pair, fam, n)
            fr, sr = ratios(K, b, r)
            w = worst[fam]
            w[0], w[1] = max(w[0], fr), max(w[1], sr)
            if fam != "a":
                L8, D8, fail = M.ldl(K, M.F80)
                assert fail is None
                for i in range(b.shape[0]):
                    x8 = M.solve(L8, D8, b[i], M.F80)
                    w[2] = max(w[2], float(np.max(np.abs(r.x[i] - x8)) / np.max(np.abs(x8))))
            if not (fr <= LC.C_BOUND and sr <= LC.C_BOUND):
                over.append((fam, n, fr, sr))
    for fam in FAMILIES:
        w = worst[fam]
        print(f"linalg_gpu {pair} boundary orders, family {fam}: factor ratio max {w[0]:.3f}, "
              f"solve ratio max {w[1]:.3f}" +
              (f", forward error |x - x_80bit| / |x| max {w[2]:.2e}" if fam != "a" else ""))
    assert not over, (pair, over)


@pytest.mark.parametrize("pair", LH.PAIRS, ids=PAIR_IDS)
def test_leads_bitwise(gpu, pair):
    """Leads 0, 1, 2 and 3 give identical factor, dinv and x: boundary orders, families (a)
    and (b), and the compile-time solves."""
    run = device_run(pair)
    n_cmp = 0
    for key, (K, b, r) in run.items():
        if key[0] in ("bnd", "ct") and key[-1] != 0:
            r0 = run[key[:-1] + (0,)][2]
            assert same_bits(r0, r), (pair, key)
            n_cmp += 1
    assert n_cmp >= 3 * len(FAMILIES) * len(LC.boundary_orders(pair))
    print(f"linalg_gpu {pair} leads 1..3 against lead 0: {n_cmp} cases bitwise equal")


@pytest.mark.parametrize("pair", LH.PAIRS, ids=PAIR_IDS)
def test_same_case_twice_in_one_launch(gpu, pair):
    run = device_run(pair)
    for n in LC.boundary_orders(pair):
        assert same_bits(run[("dup", n)][2], run[("bnd", "a", n, 0)][2]), (pair, n)


@pytest.mark.parametrize("pair", LH.PAIRS, ids=PAIR_IDS)
def test_compile_time_solver(gpu, pair):
    """The Solver with n compiled in (immediate-lane capture) against the run-time one (select
    capture) at n = 41, 81, 121 and 241 where the pair's row slots hold them.

    n = 41 (one row slot): bitwise equal.  With two or more row slots the two differ in the last
    place, legitimately: Solver::run forms z = D^-1 y as ``r[t] = xf[t] * dinv[ic[t]]`` and the
    first backward step subtracts ``cur[t][q] * xj`` from it.  The owner slot's r is broadcast,
    so it is rounded there; for every other slot t the compiler is free to contract
    xf dinv - cur xj either as fma(-cur, xj, round(xf dinv)) or as fma(xf, dinv, -round(cur xj)),
    and it chooses differently in the unrolled compile-time sweep and in the rolled run-time
    loop, where that subtraction is the loop body's and the product is outside it.  Both are one
    rounding of the same expression.  (With the product kept from contraction, an empty asm
    on r[t] after it in a scratch copy of the header, all 34 comparisons of these orders are
    bitwise equal; the shipped header is left as it is, since pinning the product changes the
    solver's bits.)  For these orders the
    compile-time solve is held to the solve bound on its own, with the same factor bits, and its
    distance to the run-time solve is printed."""
    run = device_run(pair)
    orders = [n for n in LH.CT_ORDERS if n in LC.boundary_orders(pair)]
    assert orders and orders[0] == 41
    worst_s = worst_d = 0.0
    for n in orders:
        for fam in ("a", "ipm last"):
            for lead in LEADS:
                K, b, ct = run[("ct", fam, n, lead)]
                rt = run[("bnd", fam, n, lead)][2]
                assert np.all(np.isfinite(ct.x))
                assert np.array_equal(bits(ct.L), bits(rt.L)) and np.array_equal(bits(ct.dinv), bits(rt.dinv))
                if n <= 64:
                    assert same_bits(ct, rt), (pair, n, fam, lead, float(np.max(np.abs(ct.x - rt.x))))
                    continue
                if lead == 0:
                    worst_s = max(worst_s, ratios(K, b, ct)[1])
                    worst_d = max(worst_d, float(np.max(np.abs(ct.x - rt.x)) / np.max(np.abs(rt.x))))
                else:
                    assert same_bits(ct, run[("ct", fam, n, 0)][2]), (pair, n, fam, lead)
    print(f"linalg_gpu {pair} compile-time Solver: n 41 bitwise equal to the run-time Solver; "
          f"n {orders[1:]} solve ratio max {worst_s:.3f} (bound c = {LC.C_BOUND}), "
          f"|x_ct - x_rt| / |x| max {worst_d:.2e}")
    assert worst_s <= LC.C_BOUND, (pair, worst_s)


@pytest.mark.parametrize("pair", LH.PAIRS, ids=PAIR_IDS)
def test_failure_path(gpu, pair):
    """Every matrix of family (c) makes cholesky return false (what it leaves is unspecified
    and not compared); the same matrices before the pivot was lowered pass (the sweep)."""
    run = device_run(pair)
    labels = [c[0] for c in LC.failure_cases(pair)]
    for i, label in enumerate(labels):
        for lead in (0, 3):
            assert not run[("fail", i, lead)][2].ok, (pair, label, lead)
    print(f"linalg_gpu {pair} failure path: {len(labels)} matrices x 2 leads return false: {labels}")
