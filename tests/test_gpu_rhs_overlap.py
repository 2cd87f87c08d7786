"""The right-hand sides formed beside the factorisation (cholesky's side job, GtSide) against
the same right-hand sides formed in front of it, at the three sites of csrc/scpqp_kernel.h
that do so: the IPM iteration (ph_scale_assemble_rhs_factor), the polish round that refactors
(ph_assemble_factor) and the cold start (ph_init_assemble_factor).
tests/rhs_overlap/rhs_overlap_harness.hip runs a site in either order on the same problem
state and copies the workgroup's whole LDS and workspace slice out before and after.

There is no tolerance: the side job keeps every row, output and lane where gt_apply_fin has
it and sums the partials in block_reduce4's order, so

  * the two orders leave the same bits everywhere (rhs, yb, the factor, dinv, the pivots, the
    failure flag and everything they must not touch) except in block_reduce4's partial-sum
    buffers and the side job's own four slots, and return the same value;
  * either order changes nothing outside what the site owns (Plan.owned): the canaries after
    entry n - 1 of rhs and dinv and after entry 2 N - 1 of yb, the vectors beside them (dz, rd,
    ya, qs), the slots red[65] and red[70..71] around the side job's partials, and the rest of
    the LDS and the workspace;
  * every lead wave gives the same bits.

Shapes: the smallest at which a path differs.  n = 6: one panel step, no room for two stages
(the order in front inside the same call).  n = 9: the second step is the lone omega pivot;
two stages fit exactly.  n = 11 with obstacle rows in the incident sums.  n = 17: three steps.
13 vehicles at Hp 5: m = 390 > 256, the omega sum strides twice.  c2's own kernel (n = 81, two
row slots) and c5's with horizons 10, 20 and 30 in one launch.  Indefinite matrices
(linalg_cases.indefinite) whose first bad pivot lies in the first panel (the second stage
never runs) and in the second."""
import numpy as np
import pytest

import linalg_cases as LC
import rhs_overlap_harness as RO

pytestmark = pytest.mark.gpu

LEADS = (0, 1, 2, 3)
# id -> (unit, V, O, HM, horizons)
SHAPES = {
    "n6_frog1x5": (1, 1, 2, 5, (5,)),
    "n9_2x4": (1, 2, 0, 4, (4,)),
    "n11_frog1x10": (1, 1, 2, 10, (10,)),
    "n17_2x8": (1, 2, 0, 8, (8,)),
    "n66_circle13x5": (2, 13, 0, 5, (5,)),
    "c2_kernel_n81": (3, 4, 0, 20, (20,)),
    "c5_kernel_hp10_20_30": (4, 4, 0, 30, (10, 20, 30)),
}
_runs = {}


def device_run(sid):
    """One launch per shape: {(Hb, site, order, lead): Result}, plus the plan."""
    if sid in _runs:
        return _runs[sid]
    unit, V, O, HM, hps = SHAPES[sid]
    plan = RO.Plan(unit, V, O, HM)
    rng = np.random.default_rng([20250117, unit, V, O, HM])
    keys, cases = [], []
    for Hb in hps:
        state = RO.make_state(rng, V, O, Hb)
        for site in (0, 1, 2):
            for order in (0, 1):
                for lead in LEADS:
                    keys.append((Hb, site, order, lead))
                    cases.append((Hb, lead, site, order, state, None))
    _runs[sid] = (plan, dict(zip(keys, RO.run(plan, cases))))
    return _runs[sid]


def differing(a, b, mask):
    return np.flatnonzero((a != b) & mask)


@pytest.mark.parametrize("site", (0, 1, 2), ids=RO.SITES[:3])
@pytest.mark.parametrize("sid", list(SHAPES))
def test_overlap_is_bitwise_the_order_in_front(sid, site):
    plan, res = device_run(sid)
    same = ~plan.scratch()
    for Hb in SHAPES[sid][4]:
        N, n, m, mc = plan.dims(Hb)
        owned = plan.owned(site, Hb)
        ref = res[(Hb, site, 0, 0)]
        assert ref.ret == 1, (sid, site, Hb)
        # the site did its work: rhs and dinv hold no canary any more
        assert np.all(ref.after[plan.rhs:plan.rhs + n] != ref.before[plan.rhs:plan.rhs + n])
        assert np.all(ref.after[plan.dinv:plan.dinv + n] != ref.before[plan.dinv:plan.dinv + n])
        for order in (0, 1):
            for lead in LEADS:
                r = res[(Hb, site, order, lead)]
                assert r.ret == 1
                d = differing(r.after, ref.after, same)
                print(f"rhs_overlap {sid} {RO.SITES[site]} Hb {Hb} order {order} lead {lead}: "
                      f"{d.size} words differ from the order in front at lead 0")
                assert d.size == 0, (sid, site, Hb, order, lead, d[:8])
                w = differing(r.after, r.before, ~owned)
                assert w.size == 0, ("written outside the site's own", sid, site, Hb, order, lead, w[:8])
                # named canaries: around rhs, yb and the side job's partials
                for at in (plan.red + 65, plan.red + plan.side + 4, plan.red + plan.side + 5):
                    assert r.after[at] == r.before[at]
                if RO.pad2(n) > n:
                    assert r.after[plan.rhs + n] == r.before[plan.rhs + n]
                if site != 2:      # the cold start zeroes dz, which ends right before rhs
                    assert r.after[plan.rhs - 1] == r.before[plan.rhs - 1]
                assert r.after[plan.yb - 1] == r.before[plan.yb - 1]
                assert r.after[plan.yb + RO.pad2(2 * plan.V * plan.HM)] == r.before[plan.yb + RO.pad2(2 * plan.V * plan.HM)]


@pytest.mark.parametrize("k", (1, 9), ids=("first_panel", "second_panel"))
def test_failed_factorisation_writes_nothing_it_does_not_own(k):
    """n = 17 with pivot k not positive: the factorisation returns false in either order and
    from every lead, at the same step, and neither order writes outside what the site owns.  rhs
    may be unfinished beside the factorisation (the callers abandon the solve), so it is not
    compared."""
    unit, V, O, HM = 1, 2, 0, 8
    plan = RO.Plan(unit, V, O, HM)
    N, n, m, mc = plan.dims(HM)
    K = LC.indefinite(n, k)
    Kp = np.ascontiguousarray(K[np.tril_indices(n)])
    state = RO.make_state(np.random.default_rng([20250117, 99, k]), V, O, HM)
    cases = [(HM, lead, 3, order, state, Kp) for order in (0, 1) for lead in LEADS]
    out = RO.run(plan, cases)
    owned = plan.owned(3, HM)
    same = ~plan.scratch()
    same[plan.rhs:plan.rhs + n] = False
    same[plan.yb:plan.yb + 2 * N] = False
    for (Hb, lead, site, order, _, _), r in zip(cases, out):
        assert r.ret == 0, (k, order, lead)
        w = differing(r.after, r.before, ~owned)
        print(f"rhs_overlap indefinite pivot {k} order {order} lead {lead}: ret {r.ret}, "
              f"{w.size} words written outside the site's own")
        assert w.size == 0, (k, order, lead, w[:8])
        d = differing(r.after, out[0].after, same)
        assert d.size == 0, (k, order, lead, d[:8])


def test_given_matrix_factors_the_same_in_both_orders():
    """The given-K site on a positive definite matrix (the control of the failure test)."""
    unit, V, O, HM = 1, 2, 0, 8
    plan = RO.Plan(unit, V, O, HM)
    n = plan.dims(HM)[1]
    Kp = np.ascontiguousarray(LC.spd(n)[np.tril_indices(n)])
    state = RO.make_state(np.random.default_rng([20250117, 98]), V, O, HM)
    cases = [(HM, lead, 3, order, state, Kp) for order in (0, 1) for lead in LEADS]
    out = RO.run(plan, cases)
    same = ~plan.scratch()
    for c, r in zip(cases, out):
        assert r.ret == 1
        assert differing(r.after, out[0].after, same).size == 0, c[:4]
        assert differing(r.after, r.before, ~plan.owned(3, HM)).size == 0, c[:4]
