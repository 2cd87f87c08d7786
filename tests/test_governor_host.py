"""The speed governor without a GPU (include/scpqp_governor.h):

1. the boundary: the header's constants and its one function (a gcc probe of the header), the
   export, the ctypes binding, argument validation before any HIP call;
2. the mirror (tests/governor_mirror.py): against its 80-bit self, known answers, the off row and
   every kind of bad lane;
3. the case table (tests/governor_cases.py): its conditions with none left out, what it covers,
   and the derivation of the GPU tolerance;
4. the Python side: ``validate`` and ``required``.
"""
import copy
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import governor_cases as GC
import governor_mirror as GM
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import governor as GOV
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "scpqp_governor.h")
E_ARG, E_SIZE = -1, -4
INF = math.inf


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


# ---------------------------------------------------------------------------
# 1. boundary
# ---------------------------------------------------------------------------
PROBE = r"""
#include <stdio.h>
#include "scpqp_governor.h"
/* the prototype, restated: a mismatch with the header's is a compile error */
int scpqp_governor_step(int32_t n_veh, int32_t n_obst, int32_t hp_max, int32_t B, double t_hold,
                        double t_back, const double* x0, const double* traj, const double* obst,
                        const double* obst_margin, const int32_t* hp, const double* dreq_obs,
                        const double* dreq_veh, const double* gov, double* a_cmd,
                        int32_t* k_conf, double* clear, void* stream);
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d\n", SCPQP_GOV_NP, SCPQP_GOV_V_REF, SCPQP_GOV_A_ACC,
         SCPQP_GOV_A_BRAKE, SCPQP_GOV_K_V, SCPQP_GOV_J_MAX, SCPQP_GOV_LOOK, SCPQP_GOV_BAND,
         SCPQP_MAX_HP);
  return 0;
}
"""


def test_header_constants_and_ctypes_layout(tmp_path, lib):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{INCLUDE}", str(src), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == [LB.GOV_NP, LB.GOV_V_REF, LB.GOV_A_ACC, LB.GOV_A_BRAKE, LB.GOV_K_V, LB.GOV_J_MAX,
                   LB.GOV_LOOK, LB.GOV_BAND, LB.MAX_HP] == [7, 0, 1, 2, 3, 4, 5, 6, 64]
    assert (GM.NP, GM.V_REF, GM.A_ACC, GM.A_BRAKE, GM.K_V, GM.J_MAX, GM.LOOK, GM.BAND,
            GM.MAX_HP) == tuple(got)
    assert len(LB.GOV_FIELDS) == GOV.NP == 7
    I, D, V = C.c_int32, C.c_double, C.c_void_p
    assert lib.scpqp_governor_step.argtypes == [I] * 4 + [D] * 2 + [V] * 12
    assert lib.scpqp_governor_step.restype is C.c_int


def test_header_declares_the_boundary_and_the_definition():
    txt = open(HEADER).read()
    assert sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M))) == sorted(LB.GOV_EXPORTS) \
        == ["scpqp_governor_step"]
    for word in ("V_REF", "A_ACC", "A_BRAKE", "K_V", "J_MAX", "LOOK", "BAND", "min(LOOK, hp_b)",
                 "+inf when nothing was", "c = -inf", "a_des = -A_BRAKE",
                 "min(max(K_V (V_REF - s), -A_BRAKE), A_ACC)", "a_now - J_MAX t_hold",
                 "s_app = max(s - a_now t_back, 0)", "-s_app / t_hold", "never told to reverse",
                 "Off row", "bit for bit", "Bad lane", "k_conf = -2",
                 "What the governor does not know", "footprints", "no right of way",
                 "stop-before-the-conflict", "hysteresis", "neither a lag nor a truth row",
                 "spaced by the current speed", "no rows per variant", "SCPQP_E_SIZE",
                 "validated on the", "B = 0 is a no-op"):
        assert word in txt, word


def test_library_exports_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert set(LB.GOV_EXPORTS) <= set(re.findall(r"\sT\s(scpqp_\w+)", out))


def test_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    P = C.cast(buf, C.c_void_p)

    def err():
        return lib.scpqp_last_error()

    def call(n_veh=2, n_obst=1, hp_max=10, B=0, t_hold=0.4, t_back=0.03, x0=None, traj=None,
             obst=None, margin=None, hp=None, dreq_obs=None, dreq_veh=None, gov=None, a_cmd=None,
             k_conf=None, clear=None):
        return lib.scpqp_governor_step(n_veh, n_obst, hp_max, B, t_hold, t_back, x0, traj, obst,
                                       margin, hp, dreq_obs, dreq_veh, gov, a_cmd, k_conf, clear,
                                       None)

    assert call() == 0                                       # B = 0: a no-op, NULL arrays
    assert call(n_obst=0, t_back=0.0) == 0
    assert call(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_VEH + 1):
        assert call(n_veh=n) == E_ARG and b"n_veh" in err()
    for n in (-1, LB.MAX_OBST + 1):
        assert call(n_obst=n) == E_ARG and b"n_obst" in err()
    for h in (0, -1, LB.MAX_HP + 1):
        assert call(hp_max=h) == E_ARG and b"hp_max" in err()
    for v in (0.0, -0.4, math.nan, INF):
        assert call(t_hold=v) == E_ARG and b"t_hold" in err()
    for v in (-1e-9, math.nan, INF):
        assert call(t_back=v) == E_ARG and b"t_back" in err()
    full = dict(x0=P, traj=P, obst=P, dreq_obs=P, dreq_veh=P, gov=P, a_cmd=P)
    for missing, word in (("x0", b"x0"), ("traj", b"traj"), ("obst", b"null obst"),
                          ("dreq_obs", b"dreq_obs"), ("dreq_veh", b"dreq_veh"), ("gov", b"gov"),
                          ("a_cmd", b"a_cmd")):
        kw = dict(full)
        kw[missing] = None
        assert call(B=3, **kw) == E_ARG and word in err(), missing
    # sizes before the pointers: nothing is launched for a size error
    assert call(n_veh=16, hp_max=64, B=1 << 21, **full) == E_SIZE and b"n_veh * 2 * hp_max" in err()
    assert call(n_veh=1, n_obst=32, hp_max=64, B=1 << 20) == E_SIZE and b"n_obst" in err()
    assert call(n_veh=16, n_obst=0, hp_max=1, B=1 << 24, **full) == E_SIZE and b"row width" in err()


# ---------------------------------------------------------------------------
# 2. the mirror
# ---------------------------------------------------------------------------
TH, TB = GC.T_HOLD, GC.T_BACK


def row(v_ref=4.0, a_acc=1.5, a_brake=3.0, k_v=0.8, j_max=INF, look=5, band=0.25):
    return np.array([v_ref, a_acc, a_brake, k_v, j_max, look, band], float)


def road(hb=6, gap=20.0):
    """One vehicle on y = 0 (1.6 m a step from x = 1.6) and one obstacle point standing ``gap``
    metres ahead of the plan's first point; the required distance is 2 m."""
    traj = np.zeros((hb, 2, 1))
    traj[:, 0, 0] = 1.6 * (np.arange(hb) + 1)
    obst = np.zeros((1, 2, hb))
    obst[0, 0] = 1.6 + gap
    return traj, obst, np.array([2.0]), np.zeros(1)


def run(r, s, a_now, traj, obst, dreq_obs, dreq_veh, fm=GM.F64, margin=None, hb=None):
    x0 = np.array([0.0, 0.0, 0.0, s, a_now, 0.0])
    return GM.lane(r, x0, 0, traj.shape[0] if hb is None else hb, traj, obst, margin, dreq_obs,
                   dreq_veh, TH, TB, fm)


@pytest.mark.parametrize("cid", GC.IDS)
def test_mirror_against_its_eighty_bit_self(cid):
    a, b = GC.mirror(cid, GM.F64), GC.mirror(cid, GM.F80)
    assert b[0].dtype == np.longdouble and np.finfo(np.longdouble).eps < 2e-19
    assert np.array_equal(a[1], b[1])                       # k_conf: the same branches
    assert GC.ratio(a, b, cid) <= GC.MIRROR_ROUNDING


def test_known_answers_clear_road_conflict_and_stop_rule():
    traj, obst, do, dv = road()
    # a clear road at the cruise speed: nothing to do
    a, k, c = run(row(), 4.0, 0.0, traj, obst, do, dv)
    assert a == 0.0 and k == -1
    assert abs(c - ((20.0 - 1.6 * 4) - 2.25)) < 1e-14       # step 4 is the nearest examined
    # below and above the cruise speed: the speed loop, clamped
    assert run(row(), 3.0, 0.0, traj, obst, do, dv)[0] == 0.8
    assert run(row(), 1.0, 0.0, traj, obst, do, dv)[0] == 1.5
    assert run(row(), 9.0, 0.0, traj, obst, do, dv)[0] == -3.0
    # a conflict: the obstacle 2.2 m ahead of the first point, inside 2 m + band at step 0
    traj, obst, do, dv = road(gap=2.2)
    a, k, c = run(row(), 4.0, 0.0, traj, obst, do, dv)
    assert (a, k) == (-3.0, 0) and abs(c - (0.6 - 2.25)) < 1e-15   # nearest at step 1: 0.6 m
    # ... which a band of zero and LOOK = 1 do not see (2.2 > 2)
    a, k, c = run(row(look=1, band=0.0), 4.0, 0.0, traj, obst, do, dv)
    assert (a, k) == (0.0, -1) and abs(c - 0.2) < 1e-15
    # a margin of 0.3 m on top of the 2 m does
    a, k, c = run(row(look=1, band=0.0), 4.0, 0.0, traj, obst, do, dv, margin=np.full((1, 6), 0.3))
    assert (a, k) == (-3.0, 0) and abs(c + 0.1) < 1e-15
    # the stop rule: exactly -s_app / t_hold, and the held command ends at a speed >= 0
    for s, a_now in ((0.5, -1.0), (0.3, 0.0), (1.0, 2.0), (0.0, -1.0), (0.01, 1.0)):
        for fm in (GM.F64, GM.F80):
            a, k, _ = run(row(), s, a_now, traj, obst, do, dv, fm)
            s_app = max(fm.num(s) - fm.num(a_now) * fm.num(TB), fm.num(0))
            assert k == 0 and a == -s_app / fm.num(TH) and a > -3.0
            # up to rounding: the quotient and the product round once each
            assert s_app + a * fm.num(TH) >= -2 * np.finfo(fm.dtype).eps * s_app
    # s below a_now t_back: s_app clamps at 0 and the command is not negative
    a, _, _ = run(row(), 0.01, 1.0, traj, obst, do, dv)
    assert a == 0.0 and math.copysign(1.0, a) == -1.0       # -0 / t_hold: never positive either


def test_known_answers_slew_then_stop_in_that_order():
    traj, obst, do, dv = road(gap=2.2)                      # a conflict: a_des = -3
    # the slew limit holds the command at a_now - J_MAX t_hold
    a, _, _ = run(row(j_max=2.0), 4.0, 0.5, traj, obst, do, dv)
    assert a == 0.5 - 2.0 * TH
    # ... and upwards on a clear road: a_des = 1.5 from a_now = -2
    clear_road = road()
    assert run(row(j_max=2.0), 1.0, -2.0, *clear_road)[0] == -2.0 + 2.0 * TH
    # J_MAX = 0 is finite: the command does not change
    assert run(row(j_max=0.0), 4.0, 0.5, traj, obst, do, dv)[0] == 0.5
    # the stop rule comes last and may break the slew limit: from a_now = -3 at s = 0.2 the
    # slew allows [-3.8, -2.2], the stop rule asks for -(0.2 + 0.09) / 0.4
    a, _, _ = run(row(j_max=2.0), 0.2, -3.0, traj, obst, do, dv)
    assert a == -(0.2 + 3.0 * TB) / TH and a > -3.0 + 2.0 * TH
    # were the order the other way round the slew would have the last word
    det = {}
    GM.command(row(j_max=2.0), 0.2, -3.0, True, TH, TB, detail=det)
    assert det["a_slew"] == -3.0 and det["floor"] > det["hi"]


def test_known_answers_nothing_examined_and_non_finite_plans():
    traj, obst, do, dv = road(gap=2.2)
    for kw in (dict(look=0),):
        a, k, c = run(row(**kw), 4.0, 0.0, traj, obst, do, dv)
        assert (a, k, c) == (0.0, -1, INF)
    a, k, c = run(row(), 4.0, 0.0, traj, None, None, dv)    # one vehicle, no obstacle
    assert (k, c) == (-1, INF)
    # LOOK above the horizon examines the horizon
    far = road(hb=3)
    assert run(row(look=64), 4.0, 0.0, *far)[1:] == run(row(look=3), 4.0, 0.0, *far)[1:]
    # a NaN in an examined entry brakes at that step and does not NaN the lane
    traj, obst, do, dv = road()
    for where in ("traj", "obst", "margin", "dreq"):
        t, o, d, m = traj.copy(), obst.copy(), do.copy(), np.zeros((1, 6))
        if where == "traj":
            t[2, 1, 0] = np.nan
        elif where == "obst":
            o[0, 0, 2] = INF
        elif where == "margin":
            m[0, 2] = np.nan
        else:
            d[0] = np.nan
        a, k, c = run(row(), 4.0, 0.0, t, o, d, dv, margin=m)
        assert (a, k, c) == (-3.0, 0 if where == "dreq" else 2, -INF), where
        # the same entry past LOOK is ignored
        a, k, c = run(row(look=2), 4.0, 0.0, t, o, d, dv, margin=m)
        assert ((a, k) == (0.0, -1) and c > 0) or where == "dreq", where


def test_off_row_and_every_kind_of_bad_lane():
    traj, obst, do, dv = road(gap=2.2)
    off = np.zeros(7)
    off[3] = -0.0
    for a_now in (1.25, -0.0, math.nan):
        a, k, c = run(off, math.nan, a_now, traj * np.nan, obst, do, dv)
        assert np.array(a).tobytes() == np.array(a_now).tobytes() and k == -1 and math.isnan(c)
    bad = {f"{GM.NP}_{f}_{v}": (f, v) for f in range(7) for v in (-1e-300, math.nan, -INF)}
    bad.update({f"inf_{f}": (f, INF) for f in range(7) if f != GM.J_MAX})
    bad.update(look_fraction=(GM.LOOK, 2.5), look_above=(GM.LOOK, 65.0))
    assert len(bad) == 29
    for kind, (f, v) in bad.items():
        r = row()
        r[f] = v
        assert GM.is_bad_row(r), kind
        a, k, c = run(r, 4.0, 0.0, traj, obst, do, dv)
        assert math.isnan(a) and k == -2 and math.isnan(c), kind
        with pytest.raises(ValueError, match=LB.GOV_FIELDS[f]):
            GOV.validate(r[None, None])
    for s, a_now in ((math.nan, 0.0), (INF, 0.0), (4.0, math.nan), (4.0, -INF)):
        a, k, c = run(row(), s, a_now, traj, obst, do, dv)
        assert math.isnan(a) and k == -2 and math.isnan(c)
    a, k, c = GM.lane(row(), np.array([0, 0, 0, 4.0, 0, 0]), 0, None, None, None, None, do, dv, TH, TB)
    assert math.isnan(a) and k == -2                        # a horizon outside its slot
    # what is not bad: J_MAX = +inf, LOOK = 0 and 64, a -0.0, zeros next to a non-zero field
    for r in (row(j_max=INF), row(look=0), row(look=64), row(band=-0.0), row(v_ref=0.0, a_acc=0.0)):
        assert not GM.is_bad_row(r)
        GOV.validate(r[None, None])


# ---------------------------------------------------------------------------
# 3. the case table
# ---------------------------------------------------------------------------
def test_the_table_holds_the_shapes_the_governor_must_meet():
    shapes = {(c.n_veh, c.n_obst, c.hp_max) for c in GC.CASES if c.hps is None}
    assert shapes == {(1, 0, 3), (1, 1, 1), (1, 3, 10), (4, 0, 20), (5, 2, 10), (16, 32, 64)}
    mixed = [c for c in GC.CASES if c.hps]
    assert len(mixed) == 1 and mixed[0].hps == (10, 20, 30) and mixed[0].hp_max == 30
    assert all(c.B <= 64 for c in GC.CASES)
    assert {c.margin for c in GC.CASES if c.n_obst} == {True, False}


@pytest.mark.parametrize("cid", GC.IDS)
def test_case_conditions(cid):
    """Every examined clearance and every clamp argument that decides a branch keeps SEP from
    its bound, in float64 and in 80-bit: none is left out."""
    c, d = GC.by_id(cid), GC.inputs(cid)
    for fm in (GM.F64, GM.F80):
        det = GC.mirror(cid, fm, details=True)
        assert len(det) == c.B * c.n_veh
        for (b, v), e in det.items():
            r = d["rows"][b, v]
            assert not GM.is_off_row(r) and not GM.is_bad_row(r)
            for k, cc, which, _ in e["clearances"]:
                assert abs(cc) >= GC.SEP, (b, v, k, which)
            if not e["conflict"]:
                assert abs(e["wish"] + r[GM.A_BRAKE]) >= GC.SEP and abs(e["wish"] - r[GM.A_ACC]) >= GC.SEP
            if e["lo"] is not None:
                assert abs(e["a_des"] - e["lo"]) >= GC.SEP and abs(e["a_des"] - e["hi"]) >= GC.SEP
            assert abs(e["s_raw"]) >= GC.SEP
            assert abs(e["a_slew"] - e["floor"]) >= GC.SEP
            assert r[GM.A_ACC] > 0 and r[GM.A_BRAKE] > 0


def test_what_the_table_covers():
    seen = set()
    for cid in GC.IDS:
        c, d = GC.by_id(cid), GC.inputs(cid)
        a, kc, cl = GC.mirror(cid)
        det = GC.mirror(cid, details=True)
        for (b, v), e in det.items():
            r = d["rows"][b, v]
            hb = c.hp_max if d["hp"] is None else int(d["hp"][b])
            look, K = int(r[GM.LOOK]), min(int(r[GM.LOOK]), hb)
            seen.add(("look", "0" if look == 0 else "1" if look == 1 else "hp" if look == hb
                      else "above" if look > hb else "other"))
            seen.add(("j", math.isfinite(r[GM.J_MAX])))
            if not e["clearances"]:
                assert cl[b, v] == INF and kc[b, v] == -1
                seen.add("nothing_examined")
            if kc[b, v] == 0:
                seen.add("first_at_0")
            if K > 1 and kc[b, v] == K - 1:
                seen.add("first_at_last_examined")
            if kc[b, v] >= 0 and all(w[0] == "v" for k, cc, w, _ in e["clearances"] if cc < 0):
                seen.add("vehicle_only")
            if v == 0 and d["kind"][b] == "at_look" and look < hb and (c.n_obst or c.n_veh > 1):
                # not seen; one more step of LOOK would see it, at step LOOK exactly
                assert kc[b, v] == -1
                r2 = d["rows"][b].copy()
                r2[0, GM.LOOK] = look + 1
                t, o, m = GM.unpack(b, c.n_veh, c.n_obst, c.hp_max, hb, d["traj"], d["obst"], d["margin"])
                k2 = GM.lane(r2[0], d["x0"][b, 0], 0, hb, t, o, m,
                             None if not c.n_obst else d["dreq_obs"][b, 0], d["dreq_veh"][b, 0],
                             GC.T_HOLD, GC.T_BACK)[1]
                assert k2 == look
                seen.add("conflict_at_look_not_seen")
            if d["kind"][b] == "pair" and c.n_veh > 1 and v in (0, 1):
                if kc[b, 0] == 1 and kc[b, 1] == 1:
                    seen.add("pair_both_brake")
            if d["x0"][b, v, 3] == 0.0:
                seen.add("s_zero")
            if e["s_raw"] < 0:
                seen.add("s_app_clamps")
            if e["floor"] > e["a_slew"]:
                seen.add("stop_rule_binds")
            if e["lo"] is not None and e["a_slew"] != e["a_des"]:
                seen.add("slew_binds")
        if d["hp"] is not None:
            assert sorted(set(d["hp"].tolist())) == [10, 20, 30]
    want = {("look", k) for k in ("0", "1", "hp", "above")} | {("j", True), ("j", False)} | {
        "nothing_examined", "first_at_0", "first_at_last_examined", "vehicle_only",
        "conflict_at_look_not_seen", "pair_both_brake", "s_zero", "s_app_clamps",
        "stop_rule_binds", "slew_binds"}
    assert want <= seen, want - seen


def test_tolerance_is_sixteen_times_the_rounding_of_the_definition():
    worst = {cid: GC.ratio(GC.mirror(cid, GM.F64), GC.mirror(cid, GM.F80), cid) for cid in GC.IDS}
    print("governor mirror float64 against 80-bit:", {k: f"{v:.3g}" for k, v in worst.items()})
    big = max(worst.values())
    assert 0.5 * GC.MIRROR_ROUNDING <= big <= GC.MIRROR_ROUNDING
    assert GC.TOL == GC.pow2_ceil(16 * GC.MIRROR_ROUNDING)


def test_stop_scene_geometry():
    """The two distances of the rollout scene, as governor_cases.py states them."""
    sc, x_init, kw = GC.stop_scene()
    assert sc.nVeh == 1 and sc.nObst == 1 and x_init.shape == (GC.STOP_B, 1, 6)
    radius = (sc.Lf[0] + sc.Lr[0]) / math.tan(sc.mechanicalSteeringLimit)
    reach = GC.STOP_AHEAD - GC.STOP_WIDTH / 2 - sc.Length[0] / 2           # 8.51 m
    assert reach < radius
    sideways = radius * (1.0 - math.cos(math.asin(reach / radius)))
    assert sideways < GC.STOP_LENGTH / 2                    # the centre is still in front of it
    v = 4.0
    need = v * sc.dt + v * v / (2 * kw["a_brake"]) + v * sc.dt / 2
    assert need < 0.6 * reach
    assert reach / v < (GC.STOP_STEPS - 2) * sc.dt          # ungoverned, the nose gets there
    dreq = float(np.asarray(sc.dsafeObstacles)[0, 0])
    first_point = v * (sc.dt + sc.delay_u) + v * sc.dt
    assert GC.STOP_AHEAD - first_point < dreq and kw["look"] >= 1


# ---------------------------------------------------------------------------
# 4. the Python side
# ---------------------------------------------------------------------------
def test_rows_off_from_table_and_validate():
    g = GOV.rows(3, 2, v_ref=[4.0, 3.0], a_acc=1.0, a_brake=3.0, k_v=0.5, look=5, device="cpu")
    assert tuple(g.shape) == (3, 2, 7) and g[1, 1].tolist() == [3.0, 1.0, 3.0, 0.5, INF, 5.0, 0.0]
    assert GOV.is_off(GOV.off(3, 2, device="cpu")) and not GOV.is_off(g)
    t = GOV.from_table(torch_stack([GOV.off(1, 2, device="cpu")[0], g[0]]), [1, 0, 1], device="cpu")
    assert tuple(t.shape) == (3, 2, 7) and GOV.is_off(t[1:2]) and (t[2] == g[0]).all()
    with pytest.raises(ValueError, match="index"):
        GOV.from_table(g, [3], device="cpu")
    with pytest.raises(ValueError, match="a_brake"):
        GOV.rows(3, 2, v_ref=4.0, a_acc=1.0, a_brake=-3.0, k_v=0.5, look=5, device="cpu")
    with pytest.raises(ValueError, match="look"):
        GOV.rows(3, 2, v_ref=4.0, a_acc=1.0, a_brake=3.0, k_v=0.5, look=2.5, device="cpu")
    with pytest.raises(ValueError, match="j_max"):
        GOV.rows(3, 2, v_ref=4.0, a_acc=1.0, a_brake=3.0, k_v=0.5, look=5, j_max=math.nan,
                 device="cpu")
    with pytest.raises(ValueError, match="broadcast"):
        GOV.rows(3, 2, v_ref=[1.0, 2.0, 3.0], a_acc=1.0, a_brake=3.0, k_v=0.5, look=5, device="cpu")
    with pytest.raises(ValueError, match=r"\[B, nVeh, 7\]"):
        GOV.validate(np.zeros((3, 2, 8)))
    with pytest.raises(ValueError, match=r"rows\[1, 0\]: band"):
        bad = g.numpy().copy()
        bad[1, 0, GM.BAND] = -0.1
        GOV.validate(bad)


def torch_stack(ts):
    import torch
    return torch.stack(ts)


def test_required_is_the_scenarios_tables():
    sc = R.parallel_scenario(5, Hp=10)
    do, dv = GOV.required(sc, device="cpu")
    assert tuple(do.shape) == (1, 5, 4) and tuple(dv.shape) == (1, 5, 5)
    assert np.array_equal(do[0].numpy(), np.asarray(sc.dsafeObstacles, float))
    assert np.array_equal(dv[0].numpy(), np.asarray(sc.dsafeVehicles, float))
    assert (do.numpy() < np.asarray(sc.dsafeObstacles) + sc.dsafeExtra).all()   # without dsafeExtra
    wide = copy.deepcopy(sc)
    wide.dsafeObstacles = np.asarray(sc.dsafeObstacles) + 0.5
    wide.dsafeVehicles = np.asarray(sc.dsafeVehicles) * 2.0
    vo = [1, 0, 0, 1]
    do, dv = GOV.required(sc, [sc, wide], vo, device="cpu")
    assert tuple(do.shape) == (4, 5, 4) and tuple(dv.shape) == (4, 5, 5)
    for b, k in enumerate(vo):
        src = (sc, wide)[k]
        assert np.array_equal(do[b].numpy(), np.asarray(src.dsafeObstacles, float))
        assert np.array_equal(dv[b].numpy(), np.asarray(src.dsafeVehicles, float))
    one = R.circle_scenario(4, Hp=20)
    do, dv = GOV.required(one, device="cpu")
    assert tuple(do.shape) == (1, 4, 0) and tuple(dv.shape) == (1, 4, 4)
    with pytest.raises(ValueError):
        GOV.required(sc, [sc, wide], None, device="cpu")
    with pytest.raises(ValueError):
        GOV.required(sc, [sc, wide], [0, 2], device="cpu")
