"""The references of the problem-setup tests, on the CPU alone: the 80-bit mirror
(tests/setup_mirror.py) against mpmath at 40 digits and the float64 mirror against scipy and
the oracle; the conditions the case table (tests/setup_cases.py) must meet for the GPU tests
to mean something; the bounds, measured on a float64 restatement of the device's algorithm;
seeded mistakes, each of which must break its output's bound; and the squaring count of
csrc/scpqp_kernel.h through the test harness (tests/setup_harness.py)."""
import math
import sys

import mpmath
import numpy as np
import pytest

import setup_cases as SC
import setup_harness as SH
import setup_mirror as SM
from oracle import scp_reference as R
from scpqp.solver import plan_query

U80 = 2.0 ** -64
# the mirror's argument and exponential may err by this multiple of u yardstick: a hundredth of
# the smallest bound on the exponential's blocks
MIRROR_SHARE = 0.01 * min(SC.BOUND[k] for k in ("Ad", "Bd", "Ed"))
DBL_MAX = sys.float_info.max


def slots(c):
    return [(b, v) for b in range(c.B) for v in range(c.V)]


# ---------------------------------------------------------------------------------------
# the mirror against mpmath
# ---------------------------------------------------------------------------------------
def mp_model(x, u, Lf, Lr, noise):
    """Model.py:45-87 in mpmath: the 8x8 argument [[Ac Bc Ec]; 0] (without dt)."""
    mp = mpmath.mp
    x = [mp.mpf(float(v)) for v in x]
    u, Lf, Lr = mp.mpf(float(u)), mp.mpf(float(Lf)), mp.mpf(float(Lr))
    L = Lf + Lr
    rho = Lr / L
    v, psi, d = x[3], x[2], x[5]
    t = mp.tan(d)
    sec2 = t * t + 1
    kap = mp.sqrt(rho * rho * t * t + 1)
    beta = mp.atan(rho * t)
    th = psi + beta
    cth, sth = mp.cos(th), mp.sin(th)
    M = mp.zeros(8, 8)
    M[0, 2] = -v * sth * kap
    M[0, 3] = cth * kap
    M[0, 5] = rho * rho * v * cth * t * sec2 / kap - rho * v * sth * sec2 / kap
    M[1, 2] = v * cth * kap
    M[1, 3] = sth * kap
    M[1, 5] = rho * v * cth * sec2 / kap + rho * rho * v * sth * t * sec2 / kap
    M[2, 3] = t / L
    M[2, 5] = v * sec2 / L
    M[3, 4] = 1
    M[5, 5] = -10
    M[5, 6] = 10
    vc = v * mp.sqrt(1 + (rho * t) ** 2)
    f = [vc * mp.cos(psi + beta) + mp.mpf(float(noise[0])), vc * mp.sin(psi + beta) + mp.mpf(float(noise[1])),
         vc * t * mp.cos(beta) / L, x[4], mp.mpf(0), (u - x[5]) / mp.mpf(0.1)]
    for i in range(6):
        M[i, 7] = f[i] - sum(M[i, j] * x[j] for j in range(6)) - M[i, 6] * u
    return M


def mp_to_f80(M):
    """An mpmath matrix as 80-bit numbers: head and tail, each a float64."""
    out = np.zeros((M.rows, M.cols), dtype=SM.F80)
    for i in range(M.rows):
        for j in range(M.cols):
            hi = float(M[i, j])
            out[i, j] = SM.F80(hi) + SM.F80(float(M[i, j] - mpmath.mpf(hi)))
    return out


def f80_to_mp(A):
    M = mpmath.zeros(*A.shape)
    for i in range(A.shape[0]):
        for j in range(A.shape[1]):
            hi = float(A[i, j])
            M[i, j] = mpmath.mpf(hi) + mpmath.mpf(float(A[i, j] - SM.F80(hi)))
    return M


@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_mirror_80bit_against_mpmath(sid):
    """Jacobian, Ec and the exponential of every case: the 80-bit mirror lies within
    MIRROR_SHARE u yardstick of the 40-digit values, so it can stand for the exact value in
    every ratio below."""
    c = SC.case(sid)
    ref = SC.reference(sid)
    worst = {"M": 0.0, "X": 0.0, "S": 0.0}
    with mpmath.workdps(40):
        for b, v in slots(c):
            r = ref[(b, v)]["_vehicle"]
            M = mp_model(c.x0[b, v], c.u0[b, v], c.Lf[b, v], c.Lr[b, v], c.ec[b, v]) * mpmath.mpf(SC.DT)
            X = mpmath.expm(M)
            worst["M"] = max(worst["M"], SM.ratio_of(r.M - mp_to_f80(M), r.Mh))
            worst["X"] = max(worst["X"], SM.ratio_of(r.X - mp_to_f80(X), r.S))
            # the yardstick's exponential too (a non-negative matrix: itself its yardstick)
            S = mpmath.expm(f80_to_mp(r.Mh))
            worst["S"] = max(worst["S"], SM.ratio_of(r.S - mp_to_f80(S), r.S))
    print(f"setup_mirror {sid}: 80-bit mirror against mpmath, in u yardstick: argument "
          f"{worst['M']:.2e}, exponential {worst['X']:.2e}, the yardstick's {worst['S']:.2e} "
          f"(allowed {MIRROR_SHARE:.2e}; the yardstick's own: 1e3)")
    assert worst["M"] <= MIRROR_SHARE and worst["X"] <= MIRROR_SHARE
    # a yardstick needs its leading digits only (the squarings of a non-negative matrix of
    # norm 100 and more cost the Taylor series some 2^s u80 here)
    assert worst["S"] <= 1e3


def test_float64_mirror_against_scipy_and_the_oracle():
    """At the nominal start of c2 (4 vehicles, Hp 20): the float64 mirror, scipy's expm behind
    ``R.discretize`` and the oracle's faithful linearisation all lie within the bounds of the
    80-bit mirror."""
    sc = R.circle_scenario(4, Hp=20)
    x0 = np.array(sc.x0)
    p = R.make_problem(sc, x0, Hp=20)
    lin = R.linearise(p, "faithful")
    for v in range(4):
        ref = p.ref_points[:, :, v]
        r80 = SM.vehicle(x0[v], 0.0, sc.Lf[v], sc.Lr[v], (0.0, 0.0), sc.dt, 20, SM.F80)
        o80 = SM.outputs(r80, ref, sc.Q[v], sc.Q_final[v], SM.F80)
        r64 = SM.vehicle(x0[v], 0.0, sc.Lf[v], sc.Lr[v], (0.0, 0.0), sc.dt, 20, SM.F64)
        o64 = SM.outputs(r64, ref, sc.Q[v], sc.Q_final[v], SM.F64)
        Ad, Bd, _, Ed = R.discretize(x0[v], 0.0, sc.Lf[v], sc.Lr[v], sc.dt)
        theirs = {"Ad": Ad, "Bd": Bd[:, 0], "Ed": Ed[:, 0], "g": lin.g[v],
                  "const_term": lin.const[v].reshape(20, 2), "psi0": lin.Psi0[v]}
        for k in SM.OUTPUTS:
            val, yard = o80[k]
            assert SM.ratio(o64[k][0], val, yard) <= SC.BOUND[k], k
            assert SM.ratio(theirs[k], val, yard) <= SC.BOUND[k], k


# ---------------------------------------------------------------------------------------
# conditions on the inputs, on the reference alone
# ---------------------------------------------------------------------------------------
def test_shapes_run_the_kernels_they_stand_for():
    kernels = set()
    for sid in SC.SHAPE_IDS:
        c = SC.case(sid)
        q = plan_query(c.V, 22 if c.scenario == "frog" else 0, c.hp_max, c.hp_arg is not None)
        assert q["kernel"] == SC.KERNELS[sid], sid
        kernels.add(q["kernel"])
        assert c.B <= 16
    assert len(kernels) == len(SC.SHAPE_IDS)


def test_squaring_counts_of_the_table():
    """Every count 0 .. 5 occurs; no norm lies within 1e-6 relative of a threshold
    theta13 2^k; one problem has four different counts in one round of four waves and one has
    a larger count in a later round than in the first."""
    seen, four, later = set(), False, False
    for sid in SC.SHAPE_IDS:
        c = SC.case(sid)
        ref = SC.reference(sid)
        for b in range(c.B):
            s = []
            for v in range(c.V):
                r = ref[(b, v)]["_vehicle"]
                k = round(math.log2(r.nrm / SM.THETA13)) if r.nrm > 0 else 0
                assert abs(r.nrm / (SM.THETA13 * 2.0 ** k) - 1) > 1e-6, (sid, b, v)
                assert r.s == SH.squarings(r.nrm)
                s.append(r.s)
            seen |= set(s)
            rounds = [s[i:i + 4] for i in range(0, c.V, 4)]
            four |= any(len(set(r)) == 4 for r in rounds)
            later |= any(max(r) > max(rounds[0]) for r in rounds[1:])
    assert set(range(6)) <= seen
    assert four and later


def test_table_covers_the_states_the_issue_lists():
    xs = np.concatenate([SC.case(sid).x0.reshape(-1, 6) for sid in SC.SHAPE_IDS])
    us = np.concatenate([SC.case(sid).u0.reshape(-1) for sid in SC.SHAPE_IDS])
    for s in (0.0, 0.01, -0.01, 1.0, -1.0, 4.0, 8.0, 16.0, 32.0, 64.0):
        assert (xs[:, 3] == s).any(), s
    for d in (0.0, 0.05, -0.05, 0.3, -0.3, 0.6, -0.6):
        assert (xs[:, 5] == d).any(), d
    psi = np.mod(xs[:, 2], 2 * math.pi)
    assert all(((psi >= q * math.pi / 2) & (psi < (q + 1) * math.pi / 2)).any() for q in range(4))
    assert (xs[:, 2] > math.pi).any() and (xs[:, 2] < -math.pi).any()
    assert (xs[:, 4] == 2.0).any() and (xs[:, 4] == -2.0).any()
    assert (np.abs(us) > SC.U_LIM).any() and (np.abs(us) == SC.U_LIM).any() and (us == 0).any()
    ec = np.concatenate([SC.case(sid).ec.reshape(-1, 2) for sid in SC.SHAPE_IDS])
    assert np.abs(ec).max() == 1e-3
    assert any((SC.case(sid).Lf != SC.case(sid).Lr).any() for sid in SC.SHAPE_IDS)
    npts = {len(p) for sid in SC.SHAPE_IDS for row in SC.case(sid).poly for p in row}
    assert set(range(3, 9)) <= npts


def test_sampler_cases_are_separated_or_exact():
    """Every vehicle's sampler decisions keep 1e-9 from their thresholds, but for the listed
    exact kinds; every placement kind and every reason to raise occurs, alone where it can;
    every shape with more than two problems has problems with and without the flag."""
    kinds, reasons = set(), set()
    for sid in SC.SHAPE_IDS:
        c = SC.case(sid)
        for b, v in slots(c):
            r = SC.samples(c, b, v)
            assert SM.separation(r, SC.exact_kinds(c, b, v)) >= SC.SEPARATION, (sid, b, v, c.kind[b][v])
            assert np.isfinite(np.asarray(r.points, dtype=np.float64)).all(), (sid, b, v)
            kinds.add(c.kind[b][v])
            reasons.add(frozenset(r.raises))
            step = c.x0[b, v, 3] * SC.DT
            kinds |= {"step0"} if step == 0 else ({"stepneg"} if step < 0 else set())
        flags = {SC.would_raise(c, b) for b in range(c.B)}
        assert flags == {False, True}, sid
    assert kinds >= set(SC.KINDS) | {"wedge", "endpoint2", "short2", "step0", "stepneg"}
    assert {frozenset(), frozenset({"xor"}), frozenset({"index"}), frozenset({"assert"}),
            frozenset({"xor", "assert"})} <= reasons


def test_would_raise_is_the_strict_oracle_and_points_are_the_lenient_one():
    """The predicate equals "the strict oracle raises" on every vehicle, by the exception's
    type; where the lenient oracle returns, the mirror's points are its points."""
    names = {"xor": TypeError, "assert": AssertionError, "index": IndexError}
    worst = 0.0
    for sid in SC.SHAPE_IDS:
        c = SC.case(sid)
        for b, v in slots(c):
            r = SC.samples(c, b, v)
            x = c.x0[b, v]
            args = (int(c.hp[b]), c.poly[b][v], x[0], x[1], x[3] * SC.DT)
            raised = None
            try:
                R.sample_reference(*args, strict_xor_quirk=True)
            except (TypeError, AssertionError, IndexError) as e:
                raised = type(e)
            assert (raised is not None) == bool(r.raises), (sid, b, v)
            if raised is not None:
                # the oracle meets them in this order
                first = next(k for k in ("xor", "assert", "index") if k in r.raises)
                assert raised is names[first], (sid, b, v)
            if r.raises <= {"xor"}:
                pts = R.sample_reference(*args, strict_xor_quirk=False)
                worst = max(worst, float(np.abs(pts - np.asarray(r.points, dtype=np.float64)).max()))
            else:
                with pytest.raises((AssertionError, IndexError)):
                    R.sample_reference(*args, strict_xor_quirk=False)
    assert worst <= 1e-13


# ---------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------
def measure(seed=None):
    """{output: (worst ratio, where)} of the float64 restatement over the table, and whether
    it returns exact zeros at every structural zero."""
    worst = {k: (0.0, None) for k in SM.OUTPUTS}
    zeros_ok = True
    for sid in SC.SHAPE_IDS:
        c = SC.case(sid)
        ref = SC.reference(sid)
        got = SC.evaluate(c, SM.F64, "pade", seed)
        for b, v in slots(c):
            for k in SM.OUTPUTS:
                val, yard = ref[(b, v)][k]
                x = np.asarray(got[(b, v)][k][0], dtype=np.float64)
                zeros_ok &= bool((x[SM.structural_zero(yard)] == 0).all())
                r = SM.ratio(x, val, yard)
                if r > worst[k][0]:
                    worst[k] = (r, (sid, b, v))
    return worst, zeros_ok


def test_bound_of_the_float64_restatement():
    """The worst ratio |x_f64 - x_80| / (u yardstick) per output over the whole table is what
    setup_cases.MEASURED records (rounded up; a table that has changed needs them measured
    again), and the GPU bound is four times it."""
    worst, zeros_ok = measure()
    for k in SM.OUTPUTS:
        print(f"setup_bound {k}: float64 restatement {worst[k][0]:.4g} u yardstick at {worst[k][1]}, "
              f"recorded {SC.MEASURED[k]}, GPU bound {SC.BOUND[k]:.4g}")
    assert zeros_ok
    for k in SM.OUTPUTS:
        assert 0.9 * SC.MEASURED[k] <= worst[k][0] <= SC.MEASURED[k], k
        assert SC.BOUND[k] == 4.0 * SC.MEASURED[k]


def test_far_state_is_in_the_table_only_if_the_restatement_keeps_the_bound():
    x = np.array([1.0, 2.0, 0.4, SC.FAR["v"], 0.0, SC.FAR["delta"]])
    a = SM.vehicle(x, 0.01, 0.34, 0.3, (1e-3, 0.0), SC.DT, 10, SM.F80)
    f = SM.vehicle(x, 0.01, 0.34, 0.3, (1e-3, 0.0), SC.DT, 10, SM.F64, "pade")
    assert 12 <= a.s <= 14
    within = all(SM.ratio(getattr(f, k), getattr(a, k), getattr(a, "Y" + k)) <= SC.BOUND[k]
                 for k in ("Ad", "Bd", "Ed"))
    assert within == SC.FAR_KEPT


SEEDED = {"a05_sign": "Ad", "a15_rho": "Ad", "squaring": "Ad", "ec5_u": "Ed", "g_shift": "g",
          "qf_hpmax": "psi0"}


@pytest.mark.parametrize("seed", sorted(SEEDED))
def test_seeded_mistake_breaks_its_bound(seed):
    worst, _ = measure(seed)
    k = SEEDED[seed]
    print(f"setup_seeded {seed}: {k} {worst[k][0]:.3g} u yardstick at {worst[k][1]} (bound {SC.BOUND[k]:.4g})")
    assert worst[k][0] > SC.BOUND[k]


def test_seeded_sampler_index_breaks_the_reference_points():
    """The walk started from index 1 instead of the seed's 2 moves the points of the
    vehicles exactly on a vertex and outside a corner by more than the tolerance, and on the
    end point of a line of two points it loses the index past the end (the points there are
    those of the device's clamp either way)."""
    moved, lost = set(), set()
    for sid in SC.SHAPE_IDS:
        c = SC.case(sid)
        for b, v in slots(c):
            good = np.asarray(SC.samples(c, b, v).points, dtype=np.float64)
            seeded = SC.samples(c, b, v, seed="sampler_index1")
            bad = np.asarray(seeded.points, dtype=np.float64)
            if np.abs(good - bad).max() > SC.REF_TOL:
                moved.add(c.kind[b][v])
            if seeded.raises != SC.samples(c, b, v).raises:
                lost.add(c.kind[b][v])
    assert {"vertex", "corner"} <= moved and lost == {"endpoint2"}


# ---------------------------------------------------------------------------------------
# the squaring count (expm_squarings of csrc/scpqp_kernel.h, through the harness)
# ---------------------------------------------------------------------------------------
def test_squaring_count():
    th = SM.THETA13
    for nrm in (0.0, 1.0, th, math.nan, math.inf, -math.inf, -1.0):
        assert SH.squarings(nrm) == 0, nrm
    for k in range(0, 11):
        assert SH.squarings(th * 2.0 ** k * (1 + 2.0 ** -50)) == k + 1, k
        assert SH.squarings(th * 2.0 ** k * (1 - 2.0 ** -50)) == k, k
    cap = SH.load().sh_max_squarings()
    assert cap == SM.MAX_SQUARINGS == 1100
    assert SH.squarings(DBL_MAX) == 1022 <= cap      # ceil(log2(DBL_MAX / theta13)): below the cap
    for nrm in (3.9, 5.3, 5.4, 7.4, 20.0, 100.0, 1e4, 1e100, 1e308):
        assert SH.squarings(nrm) == SM.squarings(nrm)


def test_expm_matrices_of_the_harness_test():
    """The matrices of the expm8 GPU test do what they are there for (on the float64
    restatement): row swaps, a tie in a pivot column, norms on both sides of theta13, and the
    bound measured on them."""
    info = {k: {} for k in SC.EXPM_MATRICES}
    worst = 0.0
    for k, A in SC.EXPM_MATRICES.items():
        X = SM.expm_pade13(A, info=info[k])
        val, yard = SM.expm_taylor(A, SM.F80), SM.expm_taylor(np.abs(A), SM.F80)
        assert (X[SM.structural_zero(yard)] == 0).all(), k
        worst = max(worst, SM.ratio(X, val, yard))
    print(f"setup_bound expm8 alone: float64 restatement {worst:.4g} u expm(|A|), recorded "
          f"{SC.EXPM_MEASURED}, GPU bound {SC.EXPM_BOUND:.4g}")
    assert info["dense"]["swaps"] >= 1 and info["tie"]["swaps"] >= 1 and info["tie"]["ties"] >= 1
    assert info["below"]["s"] == 0 and info["above"]["s"] == 1 and info["big"]["s"] == 3
    assert (SM.expm_pade13(SC.EXPM_MATRICES["zero"]) == np.eye(8)).all()
    assert 0.9 * SC.EXPM_MEASURED <= worst <= SC.EXPM_MEASURED
    assert SC.EXPM_BOUND == 4.0 * SC.EXPM_MEASURED
    used = {n for names, _ in SC.EXPM_LAUNCHES for n in names}
    assert used == set(SC.EXPM_MATRICES)
    assert any(mask != 15 for _, mask in SC.EXPM_LAUNCHES)
