"""The CPU side of the QP-phase tests (tests/test_gpu_qp_phases.py runs the kernels): the dense
mirror (tests/qp_phase_mirror.py) is tied to the oracle, its bounds are shown to hold for a
float64 evaluation and to catch seeded errors, and the case table (tests/qp_phase_cases.py)
is checked against the header's own helpers.

  * the dense (P, q, G, h) the mirror builds from the oracle's structured state is
    dispatch_cases.first_qp_job's scaled QP to a few ulps, and the factored rows give the
    oracle's through scpqp.trace.dense_rows;
  * the float64 mirror stays within every bound of its 80-bit self at every case (the
    largest ratio per site is printed), and every separation condition holds;
  * seven seeded errors each break their site's bound at every shape that has the feature;
  * the tile-size switch and the row table's encoding are restated and compared with the
    helpers the harness exports; the units' shapes fit what scpqp_plan_query runs on them."""
import numpy as np
import pytest

import dispatch_cases as DC
import linalg_cases as LC
import qp_phase_cases as QC
import qp_phase_mirror as QM
import qp_phases_harness as QH

UNITS = tuple(QC.SHAPES)
SOURCES = sorted({s for u in UNITS for s in QC.ORACLE[u]}, key=str)
EPS = 2.0 ** -52


# ---------------------------------------------------------------------------------------
# the mirror against the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: "%s%dx%d_hb%d" % (s[0], s[1], s[2], s[6]))
def test_mirror_is_the_oracles_scaled_qp(src):
    from oracle import scp_reference as R
    from scpqp import trace as TR
    base, par, (P, q, G, h), rows = QC.oracle_problem(src)
    V, O, Hb = base["V"], base["O"], base["Hb"]
    N, n, m, mc = QH.dims(V, O, Hb)
    assert QM.row_list(V, Hb, O) == R.row_list(V, Hb, O) == TR.row_list(V, Hb, O)
    D = QM.Dense(base, par, QM.F64)
    assert D.G.shape == G.shape == (mc, n) and D.P.shape == P.shape
    # a float64 entry of either side is a sum of at most Hb + 3 rounded terms
    tol = 2 * QM.gamma(Hb + 4)
    assert np.all(np.abs(D.P - P) <= tol * D.Pa), float(np.max(np.abs(D.P - P)))
    assert np.all(np.abs(D.G - G) <= 8 * EPS * D.Ga), float(np.max(np.abs(D.G - G)))
    assert np.all((D.Ga == 0) == (G == 0))
    assert np.all(np.abs(D.h - h) <= 4 * EPS * np.abs(h))
    assert np.array_equal(D.q, q)
    # the factored rows are the oracle's dense rows (scpqp.trace.dense_rows), scaled as qp_scale does
    A, b = TR.dense_rows(rows, base["g"], V, O, Hb, par["uLim"])
    As = A * np.concatenate([np.full(N, par["uLim"]), [1.0]])
    rn = np.sqrt((As ** 2).sum(1))
    # (norm-wise: dense_rows goes back through d = e nrm / (2 uLim), and 2 d . g cancels)
    assert np.allclose(rn, -1.0 / rows[:, 2], rtol=1e-12, atol=0)
    assert np.max(np.abs(As / rn[:, None] - G[:m])) <= 1e-12      # rows of unit norm
    assert np.allclose(b / rn, h[:m], rtol=1e-11, atol=1e-14)


# ---------------------------------------------------------------------------------------
# the float64 mirror within every bound; separation
# ---------------------------------------------------------------------------------------
_checks = {}


def unit_checks(unit):
    """[(case, {value: ratio}, {condition: separated})] with the float64 mirror as the device."""
    if unit not in _checks:
        out = []
        for c in QC.unit_cases(unit):
            key, V, O, HM, Hb, site, st, par, args = c
            out.append((c,) + QC.check(st, par, site, args, QC.outputs_f64(st, par, site, args)))
        _checks[unit] = out
    return _checks[unit]


@pytest.mark.parametrize("unit", UNITS)
def test_float64_mirror_within_every_bound(unit):
    worst = {}
    for c, out, sep in unit_checks(unit):
        for k, v in out.items():
            assert v <= 1.0, (c[0], k, v)
            w = worst.setdefault(c[5], {})
            w[k] = max(w.get(k, 0.0), v)
    assert sorted(worst) == list(QC.ALL_SITES)
    for site, w in sorted(worst.items()):
        print(f"qp_phases_host unit {unit} site {QH.SITES[site]}: float64 against 80-bit, largest "
              "|f64 - f80| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))


@pytest.mark.parametrize("unit", UNITS)
def test_separation_conditions_hold(unit):
    n = 0
    for c, out, sep in unit_checks(unit):
        for k, ok in sep.items():
            assert ok, (c[0], k)
            n += 1
    assert n >= 8


def test_the_last_oracle_iterate_is_late():
    """'last' is the last iterate at which every separation condition holds: past the middle,
    with d = lam / s over at least eight decades."""
    for src in SOURCES:
        its = QC.oracle_iterates(src)
        i = QC.last_separated(src)
        d = its[i]["lam"] / its[i]["s"]
        assert len(its) // 2 < i < len(its)
        assert d.max() / d.min() > 1e8, (src, i, len(its), float(d.max() / d.min()))


# ---------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------
RANDOM_SHAPES = sorted({(V, O, Hb) for u in UNITS for V, O, HM, Hb, _ in QC.SHAPES[u]})


def _ref(V, O, Hb):
    st, par = QC.random_state(V, O, Hb), QC._params("random", V)
    return st, par, QC.dense(st, par, QM.F80), QC.dense(st, par, QM.F64)


def _k_ratio(D80, st, rho, K):
    ref = QM.site_assemble(D80, st, rho)["K"]
    return QM.ratio(np.tril(K), ref[0], ref[1])


def mut_q_for_qf(V, O, Hb):
    st, par, D80, _ = _ref(V, O, Hb)
    Dm = QM.Dense(st, par, QM.F64, mutate="q_for_qf")
    return _k_ratio(D80, st, 0.0, QM.site_assemble(Dm, st, 0.0)["K"][0])


def mut_dropped_pair_row(V, O, Hb):
    if V < 2:
        return None
    st, par, D80, D64 = _ref(V, O, Hb)
    worst = np.inf
    for a in (0, 1):             # the row of pair (0, 1) at the middle step, from either vehicle's block
        r = QM.pair_index(0, 1, V) * Hb + Hb // 2
        worst = min(worst, _k_ratio(D80, st, 0.0, QM.site_assemble(D64, st, 0.0, drop=(r, a))["K"][0]))
    return worst


def mut_obstacle_sign(V, O, Hb):
    if O == 0:
        return None
    st, par, D80, _ = _ref(V, O, Hb)
    Dm = QM.Dense(st, par, QM.F64, mutate="obst_sign")
    ref = QM.site_gapply(D80, st, True)["rp"]
    return QM.ratio(QM.site_gapply(Dm, st, True)["rp"][0], ref[0], ref[1])


def mut_toeplitz_limit(V, O, Hb):
    if QH.dims(V, O, Hb)[2] == 0:
        return None
    st, par, D80, _ = _ref(V, O, Hb)
    Dm = QM.Dense(st, par, QM.F64, mutate="toeplitz_limit")
    ref = QM.site_gapply(D80, st, False)["rp"]
    rt = QM.site_rhs_from_tv(D80, st, 0.0)["rhs"]
    return min(QM.ratio(QM.site_gapply(Dm, st, False)["rp"][0], ref[0], ref[1]),
               QM.ratio(QM.site_rhs_from_tv(Dm, st, 0.0)["rhs"][0], rt[0], rt[1]))


def mut_last_output_of_a_pass(V, O, Hb):
    st, par, D80, D64 = _ref(V, O, Hb)
    ref = QM.site_rhs_from_tv(D80, st, par["polRho"])["rhs"]
    skip = min(84, V * Hb) - 1
    return QM.ratio(QM.site_rhs_from_tv(D64, st, par["polRho"], skip=skip)["rhs"][0], ref[0], ref[1])


def mut_row_left_out_of_ratio_test(V, O, Hb):
    st, par, D80, D64 = _ref(V, O, Hb)
    a = st["args"]
    ref = QM.site_update(D80, st, a["smu"], a["eta"])
    if not ref["ratio_p"][0] < 1:
        return None              # no row binds: the step is the damped full step
    z = QM.site_update(D64, st, a["smu"], a["eta"], leave_out_binding=True)["z"][0]
    return QM.ratio(z, ref["z"][0], ref["z"][1])


def mut_rho_missing(V, O, Hb):
    st, par, D80, D64 = _ref(V, O, Hb)
    return _k_ratio(D80, st, par["polRho"], QM.site_assemble(D64, st, par["polRho"], no_rho=True)["K"][0])


MUTATIONS = {"q_for_qf_at_the_terminal_step": (mut_q_for_qf, len(RANDOM_SHAPES)),
             "dropped_pair_row_in_a_wt_block": (mut_dropped_pair_row, 10),
             "flipped_sign_on_obstacle_rows": (mut_obstacle_sign, 5),
             "toeplitz_upper_limit_off_by_one": (mut_toeplitz_limit, len(RANDOM_SHAPES) - 1),
             "last_output_of_a_pass_skipped": (mut_last_output_of_a_pass, len(RANDOM_SHAPES)),
             "row_left_out_of_the_ratio_test": (mut_row_left_out_of_ratio_test, len(RANDOM_SHAPES) - 3),
             "rho_missing_from_the_diagonal": (mut_rho_missing, len(RANDOM_SHAPES))}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_breaks_its_bound(name):
    fn, at_least = MUTATIONS[name]
    hit = []
    for V, O, Hb in RANDOM_SHAPES:
        r = fn(V, O, Hb)
        if r is None:
            continue
        assert r > 1.0, (name, (V, O, Hb), r)
        hit.append(r)
    assert len(hit) >= at_least, (name, len(hit), at_least)
    print(f"qp_phases_host mutation {name}: breaks the bound at {len(hit)} shapes, by a factor of "
          f"{min(hit):.3g} at the least")


# ---------------------------------------------------------------------------------------
# the table against the header
# ---------------------------------------------------------------------------------------
def test_tile_size_switch():
    lib = QH.load()
    seen = {u: set() for u in UNITS}
    for u in UNITS:
        hg = QH.KERNELS[u][0]
        for V, O, HM, Hb, _ in QC.SHAPES[u]:
            T4, PV = (Hb + 3) // 4, V * (V - 1) // 2
            ntile4 = V * T4 * (T4 + 1) // 2 + PV * T4 * T4
            want = 4 if (not hg or ntile4 >= 512) else 2
            assert QH.tile_size(hg, V, Hb) == lib.qp_tile_size(u, V, Hb) == want, (u, V, Hb)
            assert QH.Plan(u, V, O, HM, Hb).tile == want
            if hg:
                assert QC.TILES[(u, V, Hb)] == want, (u, V, Hb, ntile4)
            seen[u].add(want)
    assert seen[4] == {2, 4} and seen[5] == {2, 4}
    # either side of the switch on unit 5
    assert QC.TILES[(5, 8, 15)] == 4 and QC.TILES[(5, 8, 12)] == 2


def test_row_table_encoding():
    from oracle import scp_reference as R
    lib = QH.load()
    for V, O, Hb in RANDOM_SHAPES + [(1, 22, 10)]:
        rows = R.row_list(V, Hb, O)
        assert len(rows) == QH.dims(V, O, Hb)[2]
        for r, (i, j, o, k) in enumerate(rows):
            info = lib.qp_rinfo_host(r, V, O, Hb)
            assert info == QH.rinfo(r, V, O, Hb, rows), (V, O, Hb, r)
            # row_decode of the header
            assert (info & 0xff, ((info >> 8) & 0xff) - 1, ((info >> 16) & 0xff) - 1, (info >> 24) & 0xff) == (i, j, o, k)


def test_plan_helpers():
    lib = QH.load()
    for i in range(0, 260):
        assert lib.qp_roff(i) == QH.roff(i)
    for u in UNITS:
        for V, O, HM, Hb, _ in QC.SHAPES[u]:
            p = QH.Plan(u, V, O, HM, Hb)
            assert (p.hg, p.vg) == QH.KERNELS[u][:2]
            assert lib.qp_in_size(V, O, Hb) == 2 * p.N + 4 * p.m + 3 * p.n + QH.KVECS * p.mc + p.N
            assert p.lds * 8 <= 163840
    # the row slots kept in registers: c2's two, c5's classes, none elsewhere
    assert QH.Plan(2, 4, 0, 20).slots == 2
    assert [QH.Plan(3, 4, 0, 30, h).slots for h in (30, 20, 10, 21, 1)] == [2, 2, 1, 0, 0]
    assert QH.Plan(6, 8, 0, 30).slots == 0


def test_boundary_shapes_sit_where_they_should():
    """The edges the table is there for, restated from the header's constants."""
    per_wave, per_pass = 21, 84
    vh = {(V, O, Hb): V * Hb for V, O, Hb in RANDOM_SHAPES}
    assert {per_wave, per_wave + 1, 3 * per_wave, per_pass, per_pass + 1} <= set(vh.values())
    mcs = {QH.dims(*s)[3] for s in RANDOM_SHAPES}
    assert {256, 257} <= mcs
    assert QH.dims(1, 0, 3)[2] == 0


def test_units_fit_what_the_plan_runs():
    """Every unit's instantiation is one scpqp_plan_query returns for some shape (a
    dispatch_cases row), and every shape's order is within what its (HG, RM) pair runs."""
    kernels = {c.kernel for c in DC.CASES}
    best = LC.max_orders()
    for u in UNITS:
        k = QH.KERNELS[u]
        assert k in kernels, (u, k)
        for V, O, HM, Hb, _ in QC.SHAPES[u]:
            assert V * HM + 1 <= min(64 * k[2], best[(k[0], k[2])]), (u, V, HM)
