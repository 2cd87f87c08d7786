"""``assemble`` of csrc/scpqp_kernel.h alone (tests/asm_overlap/asm_overlap_harness.hip), in the
order of -DSCPQP_DIAG_ASM_FRONT and in the shipped one: yb beside the diagonal W~ blocks, the
omega row on the last two waves beside a single-round tile pass.

  * H (rows 0..N of the packed factor storage) and W~ are bit for bit the same in both orders;
  * yb is the same too, in every case: both orders leave it defined everywhere (the cold
    start's assembly is a full one, with row N overwritten by e_N behind it);
  * nothing outside H's rows 0..N, W~, yb and block_reduce4's partial sums red[0, 48) is
    written: the launch's whole LDS and workspace slice start as canaries, and the rest of the
    two orders' images is bitwise equal;
  * both orders lie within the bounds of tests/test_gpu_qp_phases.py for the assembly
    (K_uu 2 Hb + V + O + 8, K_Nu V + O + L3 + 6, K_NN ceil(m / 256) + 13, W~ V + O + 1
    operations, times the sum of the terms' absolute values) of the float64 mirror
    (tests/qp_phase_mirror.py), so a defect common to both orders is still caught.  The cold
    start's row N is e_N exactly.  The mirror is consulted for lead 0 only (the assembly does
    not read the lead, and the bitwise comparison covers leads 0 to 3) and for H and W~: yb
    reaches it through row N of H, which is calB' yb, and the order in front forms yb with the
    code of before (incident_sum).

Shapes (unit of tests/qp_phases_harness.py, V, O, HM, Hb):
  2  4 0 20 20   the shipped c2 path (210 tiles: the omega row beside them)
  3  4 0 30 10   78 tiles: waves 1-3 have few or no tiles
  3  4 0 30 30   528 tiles, three rounds: the omega row behind them, yb fused
  1  2 2  7  7   run-time shape, obstacle rows, Hb no multiple of 4, nW + V Hb < 64
  1  1 1  5  5   no vehicle pairs
  6  8 0 30 30   workspace plan, nW = 1080 > 256: the fusion only
Weights: a seeded positive d = 10^U(-6, 6); the polish's d in {0, 1 / delta} with rho, with no,
one and every collision row active; the cold start's d = 1.  Every case with leads 0 to 3.
One launch of 20 workgroups per shape and order."""
import numpy as np
import pytest

import asm_overlap_harness as AH
import qp_phase_cases as QC
import qp_phase_mirror as QM
import qp_phases_harness as QH

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 0, 20, 20), (3, 4, 0, 30, 10), (3, 4, 0, 30, 30), (1, 2, 2, 7, 7), (1, 1, 1, 5, 5),
          (6, 8, 0, 30, 30)]
IDS = ["unit%d_V%d_O%d_Hp%d" % (u, V, O, Hb) for u, V, O, HM, Hb in SHAPES]
_runs = {}


def weight_sets(V, O, Hb, par):
    """[(name, site, rho, state)] of a shape: the states share everything but dd."""
    base = QC.random_state(V, O, Hb)
    N, n, m, mc = QH.dims(V, O, Hb)
    rng = np.random.default_rng([20250607, V, O, Hb])
    idl = 1.0 / par["polDelta"]

    def with_dd(dd):
        st = dict(base)
        st["dd"] = np.ascontiguousarray(dd, dtype=np.float64)
        return st
    out = [("ipm", AH.S_IPM, 0.0, with_dd(10.0 ** rng.uniform(-6.0, 6.0, mc)))]
    box = (rng.uniform(size=mc - m) < 0.3) * idl
    for name, act in (("polish none", np.zeros(m)), ("polish one", np.eye(1, m, m // 2)[0]),
                      ("polish all", np.ones(m))):
        out.append((name, AH.S_POL, par["polRho"], with_dd(np.concatenate([act * idl, box]))))
    out.append(("cold", AH.S_COLD, 0.0, with_dd(np.ones(mc))))
    return out


def device_run(shape):
    if shape not in _runs:
        unit, V, O, HM, Hb = shape
        par = QC.random_params(V)
        sets = weight_sets(V, O, Hb, par)
        cases = [(V, O, HM, Hb, site, lead, st, par, rho) for _, site, rho, st in sets for lead in range(4)]
        res = {}
        for order in (AH.FRONT, AH.SHIPPED):
            lds_img, r = AH.run(unit, order, cases)
            res[order] = r
        _runs[shape] = (QH.Plan(unit, V, O, HM, Hb), lds_img, par,
                        [(name, site, rho, st, lead) for name, site, rho, st in sets for lead in range(4)], res)
    return _runs[shape]


def regions(plan, lds_img, size):
    """Index arrays of the packed rows 0..N of H, of W~ and of yb, and the mask of block_reduce4's
    partial sums."""
    h = plan.packed_index(lds_img)[2]
    wt = plan.at("Wt", lds_img) + np.arange(4 * plan.Hb * plan.nb)
    yb = plan.at("yb", lds_img) + np.arange(2 * plan.N)
    red = np.zeros(size, dtype=bool)
    red[plan.red:plan.red + 48] = True
    return h, wt, yb, red


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_both_orders_leave_the_same_bits(gpu, shape):
    plan, lds_img, par, cases, res = device_run(shape)
    size = res[AH.FRONT][0][0].size
    h, wt, yb, red = regions(plan, lds_img, size)
    for i, (name, site, rho, st, lead) in enumerate(cases):
        (b0, a0), (b1, a1) = res[AH.FRONT][i], res[AH.SHIPPED][i]
        what = (shape, name, lead)
        assert np.array_equal(b0, b1), what
        assert np.array_equal(a0[h], a1[h]), ("H differs", what, np.flatnonzero(a0[h] != a1[h])[:8])
        assert np.array_equal(a0[wt], a1[wt]), ("W~ differs", what, np.flatnonzero(a0[wt] != a1[wt])[:8])
        assert not np.array_equal(a1[h], b1[h]) and not np.array_equal(a1[wt], b1[wt]), ("nothing ran", what)
        rest = ~red
        assert np.array_equal(a0[yb], a1[yb]), ("yb differs", what, np.flatnonzero(a0[yb] != a1[yb])[:8])
        assert not np.array_equal(a1[yb], b1[yb]), what
        assert np.array_equal(a0[rest], a1[rest]), ("images differ", what, np.flatnonzero((a0 != a1) & rest)[:8])
    print(f"asm_overlap_gpu {shape}: {len(cases)} cases, H, W~ and yb bitwise equal in both orders")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_nothing_else_is_written(gpu, shape):
    plan, lds_img, par, cases, res = device_run(shape)
    size = res[AH.FRONT][0][0].size
    own = plan.owned(QH.S_A, lds_img, size)
    for order in (AH.FRONT, AH.SHIPPED):
        for i, (name, site, rho, st, lead) in enumerate(cases):
            b, a = res[order][i]
            w = np.flatnonzero((b != a) & ~own)
            assert w.size == 0, ("written outside the assembly's own", shape, order, name, lead, w[:8], lds_img)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_both_orders_within_the_assembly_bounds_of_the_mirror(gpu, shape):
    plan, lds_img, par, cases, res = device_run(shape)
    unit, V, O, HM, Hb = shape
    size = res[AH.FRONT][0][0].size
    h, wt, yb, red = regions(plan, lds_img, size)
    i_, j_, _ = plan.packed_index(lds_img)
    T = QM.F64
    worst = {}
    D = None
    for i, (name, site, rho, st, lead) in enumerate(cases):
        if lead != 0:
            continue
        if D is None:
            D = QM.Dense(st, par, T)        # g, the rows and the cost: the same in every state
        K, Kb = QM.site_assemble(D, st, rho)["K"]
        if site == AH.S_COLD:
            K, Kb = K.copy(), Kb.copy()
            K[plan.N, :] = 0.0
            K[plan.N, plan.N] = 1.0
            Kb[plan.N, :] = 0.0
        W, Wb = QM.wt_blocks(D, st, par)
        for order in (AH.FRONT, AH.SHIPPED):
            a = res[order][i][1].view(np.float64)
            Kd = np.zeros((plan.n, plan.n))
            Kd[i_, j_] = a[h]
            rk = QM.ratio(Kd, K, Kb)
            rw = QM.ratio(a[wt].reshape(Hb, plan.nb, 4), W, Wb)
            print(f"asm_overlap_gpu {shape} {name} order {order}: |dev - ref| / bound K {rk:.3f} W~ {rw:.3f}")
            worst[(name, order)] = (rk, rw)
    bad = {k: v for k, v in worst.items() if not (v[0] <= 1.0 and v[1] <= 1.0)}
    assert not bad, bad
