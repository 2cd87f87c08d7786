"""The first solve's forward sweep hidden under the factorisation (FwdSide of
csrc/scpqp_kernel.h: a helper wave runs it behind the panels, the lead finishes with
ph_solve_back) against the same factor phase followed by ph_solve, at the three sites that
factor and then solve: the IPM iteration, the polish round that refactors and the cold start.
tests/fwd_overlap/fwd_overlap_harness.hip runs a site in either order on the same problem state
and copies the workgroup's whole LDS and workspace slice out before and after.

There is no tolerance.  The helper's sweep is the lead's fold over a column range, the same
operations in the same order, and ph_solve_back is the second half of ph_solve's code (the
listings of the two contract z = D^{-1} y into the first backward step in the same way, for
n > 64 too), so

  * the two orders leave the same bits everywhere: x, rhs, the factor, dinv, the pivots, the
    failure flag and every other vector (y is parked in x's own storage, which the solve then
    overwrites), except block_reduce4's partial sums and the side job's four slots, which no
    later phase reads;
  * either order changes nothing outside what the site owns (Plan.owned): the canaries around
    every array, the rest of the LDS and the workspace;
  * every lead wave gives the same bits.

Shapes: those at which the paths differ, one problem each.  c2's kernel (n = 81: two row
slots, 11 panel steps, the last panel the omega row alone); c5's kernel with horizons 10, 20
and 30 in one launch (n = 41 keeps the whole solve on the lead: 6 steps leave no room; n = 81;
n = 121: 16 steps); a run-time shape (n = 17) and c3's kernel (n = 241, factor in the
workspace), which keep the old path: there the kernel's own call is the same in both orders,
and the test asserts that the harness took it.  Indefinite matrices (linalg_cases.indefinite,
n = 81) whose first bad pivot lies in the first panel, in a panel before the sweep starts, in
the panel of the right-hand side's last stage, and inside the sweep's window."""
import numpy as np
import pytest

import fwd_overlap_harness as FO
import linalg_cases as LC

pytestmark = pytest.mark.gpu

LEADS = (0, 1, 2, 3)
# id -> (unit, V, O, HM, {horizon: whether the kernel hides the sweep})
SHAPES = {
    "c2_kernel_n81": (2, 4, 0, 20, {20: True}),
    "c5_kernel_n41_n81_n121": (3, 4, 0, 30, {10: False, 20: True, 30: True}),
    "runtime_n17_2x8": (1, 2, 0, 8, {8: False}),
    "c3_kernel_n241": (4, 8, 0, 30, {30: False}),
}
_runs = {}


def scratch(plan):
    """block_reduce4's partial sums and the side job's partials: written, never read later."""
    w = np.zeros(plan.size, dtype=bool)
    w[plan.red:plan.red + 48] = True
    w[plan.red + plan.side:plan.red + plan.side + FO.NWAVE] = True
    return w


def device_run(sid):
    """One launch per shape: {(Hb, site, order, lead): Result}, plus the plan."""
    if sid in _runs:
        return _runs[sid]
    unit, V, O, HM, hps = SHAPES[sid]
    plan = FO.Plan(unit, V, O, HM)
    rng = np.random.default_rng([20250301, unit, V, O, HM])
    keys, cases = [], []
    for Hb in hps:
        state = FO.make_state(rng, V, O, Hb)
        for site in (0, 1, 2):
            for order in (0, 1):
                for lead in LEADS:
                    keys.append((Hb, site, order, lead))
                    cases.append((Hb, lead, site, order, state, None))
    _runs[sid] = (plan, dict(zip(keys, FO.run(plan, cases))))
    return _runs[sid]


def differing(a, b, mask):
    return np.flatnonzero((a != b) & mask)


@pytest.mark.parametrize("sid", list(SHAPES))
def test_the_harness_takes_the_path_the_kernel_takes(sid):
    unit, V, O, HM, hps = SHAPES[sid]
    for Hb, hidden in hps.items():
        assert FO.load().fo_fits(unit, Hb) == int(hidden), (sid, Hb)


@pytest.mark.parametrize("site", (0, 1, 2), ids=FO.SITES[:3])
@pytest.mark.parametrize("sid", list(SHAPES))
def test_hidden_sweep_is_bitwise_the_whole_solve(sid, site):
    plan, res = device_run(sid)
    same = ~scratch(plan)
    for Hb in SHAPES[sid][4]:
        N, n, m, mc = plan.dims(Hb)
        owned = plan.owned(site, Hb)
        x = plan.x_at(site)
        ref = res[(Hb, site, 0, 0)]
        assert ref.ret == 1, (sid, site, Hb)
        # the site did its work: the solution is there, finite, where a canary or the input was
        xv = ref.after[x:x + n].view(np.float64)
        assert np.all(np.isfinite(xv)) and np.all(ref.after[x:x + n] != ref.before[x:x + n])
        assert np.all(ref.after[plan.dinv:plan.dinv + n] != ref.before[plan.dinv:plan.dinv + n])
        for order in (0, 1):
            for lead in LEADS:
                r = res[(Hb, site, order, lead)]
                assert r.ret == 1
                d = differing(r.after, ref.after, same)
                dx = differing(r.after[x:x + n], ref.after[x:x + n], np.ones(n, dtype=bool))
                print(f"fwd_overlap {sid} {FO.SITES[site]} Hb {Hb} order {order} lead {lead}: "
                      f"{d.size} words ({dx.size} of x) differ from the whole solve at lead 0")
                assert d.size == 0, (sid, site, Hb, order, lead, d[:8])
                w = differing(r.after, r.before, ~owned)
                assert w.size == 0, ("written outside the site's own", sid, site, Hb, order, lead, w[:8])
                # named canaries: behind x, rhs and dinv, around the side job's partials
                for at in (plan.red + 65, plan.red + plan.side + 4, plan.red + plan.side + 5):
                    assert r.after[at] == r.before[at]
                if FO.pad2(n) > n:
                    for v in (x, plan.rhs, plan.dinv):
                        assert r.after[v + n] == r.before[v + n]


def given(n, K):
    return np.ascontiguousarray(K[np.tril_indices(n)])


@pytest.mark.parametrize("k", (1, 34, 50, 75),
                         ids=("first_panel", "before_the_sweep", "rhs_stage_panel", "inside_the_window"))
def test_failed_factorisation_is_not_factored_in_both_orders(k):
    """c2's kernel (n = 81) with pivot k not positive: the factorisation returns false in either
    order and from every lead, at the same step, no solve runs, and neither order writes
    outside what the site owns.  rhs and y (in dz) may be unfinished (the callers abandon the
    solve), so they are not compared."""
    unit, V, O, HM = 2, 4, 0, 20
    plan = FO.Plan(unit, V, O, HM)
    N, n, m, mc = plan.dims(HM)
    assert FO.load().fo_fits(unit, HM) == 1
    Kp = given(n, LC.indefinite(n, k))
    state = FO.make_state(np.random.default_rng([20250301, 99, k]), V, O, HM)
    cases = [(HM, lead, 3, order, state, Kp) for order in (0, 1) for lead in LEADS]
    out = FO.run(plan, cases)
    owned = plan.owned(3, HM)
    same = ~scratch(plan)
    same[plan.rhs:plan.rhs + n] = False
    same[plan.yb:plan.yb + 2 * N] = False
    same[plan.dz:plan.dz + n] = False
    for (Hb, lead, site, order, _, _), r in zip(cases, out):
        assert r.ret == 0, (k, order, lead)
        w = differing(r.after, r.before, ~owned)
        print(f"fwd_overlap indefinite pivot {k} order {order} lead {lead}: ret {r.ret}, "
              f"{w.size} words written outside the site's own")
        assert w.size == 0, (k, order, lead, w[:8])
        d = differing(r.after, out[0].after, same)
        assert d.size == 0, (k, order, lead, d[:8])


def test_given_matrix_solves_the_same_in_both_orders():
    """The given-K site on a positive definite matrix (the control of the failure test), and
    the solution against numpy's at the accuracy of a backward-stable solve."""
    unit, V, O, HM = 2, 4, 0, 20
    plan = FO.Plan(unit, V, O, HM)
    n = plan.dims(HM)[1]
    K = LC.spd(n)
    state = FO.make_state(np.random.default_rng([20250301, 98]), V, O, HM)
    cases = [(HM, lead, 3, order, state, given(n, K)) for order in (0, 1) for lead in LEADS]
    out = FO.run(plan, cases)
    same = ~scratch(plan)
    for c, r in zip(cases, out):
        assert r.ret == 1
        assert differing(r.after, out[0].after, same).size == 0, c[:4]
        assert differing(r.after, r.before, ~plan.owned(3, HM)).size == 0, c[:4]
    x = out[4].after[plan.dz:plan.dz + n].view(np.float64)
    b = out[4].after[plan.rhs:plan.rhs + n].view(np.float64)
    Kf = np.tril(K) + np.tril(K, -1).T
    # |K x - b| <= c n u (|K| |x| + |b|) componentwise-in-norm for a backward-stable solve
    bound = 8 * n * np.finfo(np.float64).eps * (np.abs(Kf) @ np.abs(x) + np.abs(b)).max()
    print(f"fwd_overlap given K: residual {np.abs(Kf @ x - b).max():.3e}, bound {bound:.3e}")
    assert np.abs(Kf @ x - b).max() <= bound
