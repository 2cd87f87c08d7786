"""The side job's division of labour (GtSide of csrc/scpqp_kernel.h), restated in
tests/rhs_overlap_harness.py: however many helper waves there are (1 to 3) and whichever wave
leads, every output of the incident sums, every row of the omega sum and every output of the
Toeplitz product is formed exactly once, by the lane that forms it when all four waves run
gt_apply_fin themselves; and the stages fall on distinct panel steps that exist."""
import pytest

import rhs_overlap_harness as RO

# (V, O, Hb): one output pass and several, m below and above the 256 threads
SHAPES = ((1, 2, 5), (2, 0, 4), (1, 2, 10), (4, 0, 20), (13, 0, 5), (4, 0, 30), (8, 0, 30))


def reference(nout, m):
    """What thread tid of the full workgroup takes in gt_apply_fin."""
    inc, rows, toe = {}, {}, {}
    for tid in range(RO.NT):
        es, rs = RO.stage0_items(tid // 64, tid % 64, nout, m)
        for e in es:
            inc[e] = tid
        for r in rs:
            rows[r] = tid
        for e in RO.stage1_outputs(tid // 64, tid % 64, nout):
            toe[e] = tid
    return inc, rows, toe


@pytest.mark.parametrize("nh", (1, 2, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_helpers_cover_every_item_once(shape, nh):
    V, O, Hb = shape
    nout = V * Hb
    m = V * (V - 1) // 2 * Hb + V * O * Hb
    inc0, rows0, toe0 = reference(nout, m)
    assert sorted(inc0) == list(range(nout)) and sorted(toe0) == list(range(nout))
    assert sorted(rows0) == list(range(m))
    for lead in range(RO.NWAVE):
        # the first nh non-lead waves help (the product has three; fewer only restate the rule)
        helpers = [w for w in range(RO.NWAVE) if w != lead and RO.tw_of(w, lead) < nh]
        assert sorted(RO.tw_of(w, lead) for w in helpers) == list(range(nh))
        inc, rows, toe, waves = {}, {}, {}, []
        for w in helpers:
            for vw in RO.virtual_waves(RO.tw_of(w, lead), nh):
                waves.append(vw)
                for lane in range(64):
                    es, rs = RO.stage0_items(vw, lane, nout, m)
                    for e in es:
                        assert e not in inc
                        inc[e] = 64 * vw + lane
                    for r in rs:
                        assert r not in rows
                        rows[r] = 64 * vw + lane
                    for e in RO.stage1_outputs(vw, lane, nout):
                        assert e not in toe
                        toe[e] = 64 * vw + lane
        assert sorted(waves) == list(range(RO.NWAVE))      # each wave's share taken once
        assert inc == inc0 and rows == rows0 and toe == toe0


def test_stage_steps():
    for nsteps in range(2, 40):
        s0, s1 = RO.side_step(0, nsteps), RO.side_step(1, nsteps)
        assert s0 == 0 < s1 < nsteps
        # not the last step (the lone omega pivot of n = 8 j + 1) where another is free
        assert s1 < nsteps - 1 or nsteps == 2


def test_stage_steps_are_the_headers():
    lib = RO.load()
    for nsteps in range(2, 40):
        for k in (0, 1):
            assert lib.ro_side_step(k, nsteps) == RO.side_step(k, nsteps)
