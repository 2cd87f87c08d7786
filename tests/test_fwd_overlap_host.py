"""The schedule of the hidden forward sweep (fwd_sched, fwd_sched_fits of csrc/scpqp_kernel.h),
restated in tests/fwd_overlap_harness.py and read from the header through the harness library:
for every number of panel steps 1 .. 31, every order n that has that many steps and every
step the right-hand side's last stage can fall on,

  * nothing runs before the step after the one whose barrier publishes the right-hand side;
  * the range of step s stays below column 8 s (only the panels < s are final then);
  * the ranges are disjoint, ascending, whole chunks of the solve, and cover [0, n - 1) exactly;
  * where they cannot, or fewer than the minimum number of steps is left, the predicate says
    "does not fit";

and the shapes the kernel compiles: n = 81 (c2, c4, c5's Hp 20) and n = 121 (c5's Hp 30) fit,
n = 41 (c5's Hp 10), the run-time shapes and c3's workspace factor do not."""
import pytest

import fwd_overlap_harness as FO

CB = FO.CB


def ranges(nsteps, n, s1, sched):
    return [(s, sched(s - 1, nsteps, n, s1), sched(s, nsteps, n, s1)) for s in range(nsteps)]


def check(nsteps, n, s1, sched, fits, chunk, min_steps):
    rs = ranges(nsteps, n, s1, sched)
    # ascending and contiguous by construction of the ranges: the ends never go back
    assert all(j0 <= j1 for _, j0, j1 in rs)
    assert all(a[2] == b[1] for a, b in zip(rs, rs[1:]))
    assert rs[0][1] == 0
    for s, j0, j1 in rs:
        if j1 > j0:
            assert s > s1                     # after the barrier that publishes rhs
            assert j1 <= CB * s               # only final columns
            assert j0 % chunk == 0 and (j1 % chunk == 0 or j1 == n - 1)
        assert j1 <= n - 1                    # row n - 1 has no step of its own
    covers = rs[-1][2] == n - 1
    whole = (n - 1) % chunk == 0
    room = nsteps - 1 - s1 >= min_steps
    assert fits == (n > 1 and covers and whole and room), (nsteps, n, s1)


@pytest.mark.parametrize("nsteps", range(1, 32))
def test_schedule_covers_the_sweep_or_does_not_fit(nsteps):
    lib = FO.load()
    chunk, min_steps = lib.fo_chunk(), lib.fo_min_steps()
    assert (chunk, min_steps) == (4, 2)
    nfit = 0
    for n in range(CB * (nsteps - 1) + 1, CB * nsteps + 1):
        for s1 in range(0, nsteps):
            hs = lambda s, ns, nn, ss: lib.fo_fwd_sched(s, ns, nn, ss)
            fits = bool(lib.fo_fwd_sched_fits(nsteps, n, s1))
            check(nsteps, n, s1, hs, fits, chunk, min_steps)
            # the restatement is the header's
            assert fits == FO.fwd_sched_fits(nsteps, n, s1)
            assert ranges(nsteps, n, s1, hs) == ranges(nsteps, n, s1, FO.fwd_sched)
            nfit += fits
        # the right-hand side's own stage (side_step) is one of the steps tried
        assert 0 <= lib.fo_side_step(1, nsteps) < max(nsteps, 1) or nsteps == 1
        # a wrong step count never fits
        assert not lib.fo_fwd_sched_fits(nsteps + 1, n, 0)
    # n = 8 j + 1 (the omega row alone in the last panel) fits once there is room for two steps
    assert (nfit > 0) == (nsteps >= 3)


def test_no_step_outlasts_an_even_share():
    """At the kernel's own stage step the late steps share the columns evenly: no step takes
    more than an even share rounded up to a chunk, unless the 8 s limit held an earlier one
    back."""
    lib = FO.load()
    for n in (81, 121):
        nsteps = -(-n // CB)
        s1 = lib.fo_side_step(1, nsteps)
        assert lib.fo_fwd_sched_fits(nsteps, n, s1)
        rs = [(s, a, b) for s, a, b in ranges(nsteps, n, s1, FO.fwd_sched) if b > a]
        assert [s for s, _, _ in rs] == list(range(s1 + 1, nsteps))
        even = -(-(n - 1) // len(rs))
        assert max(b - a for _, a, b in rs) <= -(-even // 4) * 4


def test_which_shapes_the_kernel_hides_the_sweep_for():
    lib = FO.load()
    assert lib.fo_fits(2, 20) == 1                       # c2 / c4: n = 81
    assert lib.fo_fits(3, 20) == 1 and lib.fo_fits(3, 30) == 1   # c5's n = 81 and n = 121
    assert lib.fo_fits(3, 10) == 0                       # n = 41: 6 steps, one after the stage
    assert lib.fo_fits(3, 15) == 0                       # a horizon without a class: run-time n
    assert lib.fo_fits(1, 8) == 0                        # run-time shapes
    assert lib.fo_fits(4, 30) == 0                       # c3: factor in the workspace
    # n = 41 by the schedule alone
    s1 = lib.fo_side_step(1, 6)
    assert s1 == 4 and not lib.fo_fwd_sched_fits(6, 41, s1)
