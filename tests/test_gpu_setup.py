"""``setup_problem`` of csrc/scpqp_kernel.h on the GPU against the 80-bit mirror
(tests/setup_mirror.py) on the case table of tests/setup_cases.py: states off the nominal
start (speeds 0 to 64 m/s, steering to 0.6 rad, every heading, squaring counts 0 to 6 mixed
within a round of four waves), per-problem polylines of 3 to 8 points with every placement
the sampler distinguishes, on the seven shapes that run each layout of the setup scratch.

Every entry of Ad, Bd, Ed, g, const_term and psi0 lies within BOUND u yardstick of the mirror
(the yardstick: the value's expression with every term replaced by its absolute value;
BOUND: four times what a float64 restatement of the device's algorithm needs on the same
table, tests/test_setup_host.py) and is exactly zero where the yardstick is.  psi0 is held to
the mirror's value on the device's own reference points, which are held to the oracle's
sampler within 1e-12 m beside it, so that each stage answers for itself.

Bitwise: a vehicle's Ad, Bd, Ed do not depend on its neighbours' squaring counts or on its
wave and round; a problem's outputs do not depend on what its workgroup ran before.

The status flag SCPQP_FL_SAMPLER is set exactly where the reference would raise.

``expm8`` alone (tests/setup_harness.py): matrices that need row swaps and a tied pivot
column, the zero matrix, a nilpotent one, norms on both sides of theta13, idle waves, with
guards around each wave's 576 doubles of scratch.

Every input is finite."""
import numpy as np
import pytest
import torch

import setup_cases as SC
import setup_harness as SH
import setup_mirror as SM
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp.solver import ScpQpSolver, plan_query

pytestmark = pytest.mark.gpu


def solver_for(c, gpu, max_batch=None):
    scs = SC.scenarios(c)
    return ScpQpSolver(scs[0], max_batch=max_batch or c.B, device=gpu, hp_max=c.hp_max, variants=scs)


def unpack(lin, c, b):
    """Problem b's outputs in the mirror's shapes, at its own horizon."""
    V, Hb = c.V, int(c.hp[b])
    flat = {k: lin[k][b].reshape(-1).cpu().numpy() for k in ("g", "const_term", "psi0", "ref_points")}
    return {"Ad": lin["Ad"][b].cpu().numpy(), "Bd": lin["Bd"][b].cpu().numpy(),
            "Ed": lin["Ed"][b].cpu().numpy(),
            "g": flat["g"][:V * Hb * 2].reshape(V, Hb, 2),
            "const_term": flat["const_term"][:V * Hb * 2].reshape(V, Hb, 2),
            "psi0": flat["psi0"][:V * Hb].reshape(V, Hb),
            "ref_points": flat["ref_points"][:Hb * 2 * V].reshape(Hb, 2, V)}


def linearize(S, c, idx=None):
    idx = np.arange(c.B) if idx is None else idx
    hp = None if c.hp_arg is None else c.hp[idx]
    return S.linearize(c.x0[idx], c.u0[idx], c.ec[idx], hp=hp, variant=idx.astype(np.int32))


@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_linearize_within_bounds(gpu, sid):
    c = SC.case(sid)
    assert np.isfinite(c.x0).all() and np.isfinite(c.u0).all() and np.isfinite(c.ec).all()
    S = solver_for(c, gpu)
    lin = linearize(S, c)
    S.close()
    ref = SC.reference(sid)
    want_pts = SC.reference_points(sid)
    worst = {k: (0.0, None) for k in SM.OUTPUTS}
    ref_err, bad_zero = 0.0, []
    for b in range(c.B):
        got = unpack(lin, c, b)
        assert np.isfinite(got["ref_points"]).all()
        ref_err = max(ref_err, float(np.abs(got["ref_points"] - want_pts[b]).max()))
        for v in range(c.V):
            r = ref[(b, v)]["_vehicle"]
            # psi0 on the device's own reference points
            want = SM.outputs(r, got["ref_points"][:, :, v], c.Q[b, v], c.Qf[b, v], SM.F80)
            for k in SM.OUTPUTS:
                val, yard = want[k]
                x = got[k][v]
                if (x[SM.structural_zero(yard)] != 0).any():
                    bad_zero.append((k, b, v))
                q = SM.ratio(x, val, yard)
                if not q <= worst[k][0]:
                    worst[k] = (q, (b, v))
    print(f"setup_gpu {sid}: " + ", ".join(f"{k} {worst[k][0]:.4g}" for k in SM.OUTPUTS)
          + f" u yardstick; ref_points {ref_err:.2e} m")
    assert ref_err <= SC.REF_TOL
    assert not bad_zero, bad_zero
    for k in SM.OUTPUTS:
        assert worst[k][0] <= SC.BOUND[k], (k, worst[k], SC.BOUND[k])


def test_vehicle_does_not_depend_on_its_neighbours(gpu):
    """One state as vehicle 0 of a problem (round 0, wave 0), as vehicle 4 of another (round 1,
    beside one live and two idle waves) and as vehicle 3 of a third, each time beside vehicles
    of other squaring counts: Ad, Bd and Ed are the same bits."""
    sc = R.circle_scenario(6, Hp=10)
    nom = np.array(sc.x0)
    X = np.array([3.0, -2.0, 2.0, 16.0, 2.0, 0.3])

    def problem(speeds, at):
        x = nom.copy()
        x[:, 3] = speeds
        x[:, 5] = np.array([0.05, -0.3, 0.6, 0.0, -0.05, 0.3])
        x[at] = X
        return x
    x0 = np.stack([problem((16, 1, 64, 4, 0.01, 32), 0), problem((64, 0, 8, 1, 16, 4), 4),
                   problem((0.01, 64, 1, 16, 8, 0), 3)])
    u0 = np.full((3, 6), 0.02)
    ec = np.full((3, 6, 2), 5e-4)
    counts = [[SM.vehicle(x0[b, v], 0.02, 0.34, 0.34, (5e-4, 5e-4), sc.dt, 1, SM.F64).s for v in range(6)]
              for b in range(3)]
    assert len(set(counts[0][:4])) == 4 and len({counts[1][4], counts[1][5]}) == 2
    assert len(set(counts[2][:4])) >= 3
    S = ScpQpSolver(sc, max_batch=3, device=gpu)
    lin = S.linearize(x0, u0, ec)
    S.close()
    for k in ("Ad", "Bd", "Ed"):
        assert torch.equal(lin[k][0, 0], lin[k][1, 4]), k
        assert torch.equal(lin[k][0, 0], lin[k][2, 3]), k
    assert torch.isfinite(lin["Ad"]).all()


@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_problem_does_not_depend_on_its_predecessor(gpu, sid):
    """One launch of 2 grid + B problems, the case's problems tiled in a shuffled order: every
    workgroup takes further problems with the previous one's LDS contents in place, behind
    varying predecessors (other squaring counts, other horizons).  Every copy equals, bitwise,
    the same problem of the B-problem launch."""
    c = SC.case(sid)
    q = plan_query(c.V, 22 if c.scenario == "frog" else 0, c.hp_max, c.hp_arg is not None)
    grid = q["per_cu"] * torch.cuda.get_device_properties(gpu).multi_processor_count
    n = 2 * grid + c.B
    idx = np.random.default_rng(0).permutation(np.arange(n) % c.B)
    S = solver_for(c, gpu, max_batch=n)
    assert S.resources()["grid"] == grid
    small = linearize(S, c)
    big = linearize(S, c, idx)
    S.close()
    sel = torch.as_tensor(idx, device=gpu)
    for k in small:
        assert torch.equal(big[k], small[k][sel]), k


@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_sampler_flag_is_set_where_the_reference_would_raise(gpu, sid):
    """SCPQP_FL_SAMPLER in the status of a one-iteration solve, on exactly the problems with
    a vehicle the reference would raise on; the sampled points of ``sample_reference`` are
    the lenient oracle's there too (the mirror's, which equals it wherever it returns)."""
    c = SC.case(sid)
    scs = SC.scenarios(c)
    S = solver_for(c, gpu)
    var = np.arange(c.B, dtype=np.int32)
    obst = None
    if scs[0].nObst:
        st = np.array([[o[0], o[1]] for o in scs[0].obstacles])
        obst = np.repeat(R.obstacle_future(scs[0], st, c.hp_max)[None], c.B, axis=0)
    out = S.solve(c.x0, c.u0, c.ec, hp=c.hp_arg, obst=obst, variant=var, max_scp_iter=1)
    torch.cuda.synchronize()
    pts = S.sample_reference(c.x0, hp=c.hp_arg, variant=var)
    S.close()
    flag = (out.status.cpu().numpy() & LB.FL_SAMPLER) != 0
    want = np.array([SC.would_raise(c, b) for b in range(c.B)])
    assert (flag == want).all(), (flag, want)
    want_pts = SC.reference_points(sid)
    for b in range(c.B):
        Hb = int(c.hp[b])
        got = pts[b].reshape(-1)[:Hb * 2 * c.V].reshape(Hb, 2, c.V).cpu().numpy()
        assert np.abs(got - want_pts[b]).max() <= SC.REF_TOL, b


@pytest.mark.parametrize("launch", range(len(SC.EXPM_LAUNCHES)))
def test_expm8_alone(gpu, launch):
    names, mask = SC.EXPM_LAUNCHES[launch]
    mats = np.stack([SC.EXPM_MATRICES[n] for n in names])
    X, guards, idle = SH.expm(mats, mask)
    assert guards == 0 and idle == 0
    worst = 0.0
    for w, name in enumerate(names):
        if not (mask >> w) & 1:
            assert (X[w] == 0).all()
            continue
        A = SC.EXPM_MATRICES[name]
        val, yard = SM.expm_taylor(A, SM.F80), SM.expm_taylor(np.abs(A), SM.F80)
        assert (X[w][SM.structural_zero(yard)] == 0).all(), name
        if name == "zero":
            assert (X[w] == np.eye(8)).all()
        worst = max(worst, SM.ratio(X[w], val, yard))
        assert SM.ratio(X[w], val, yard) <= SC.EXPM_BOUND, (name, SM.ratio(X[w], val, yard))
    print(f"setup_gpu expm8 launch {launch} {names} mask {mask:04b}: {worst:.4g} u expm(|A|)")
