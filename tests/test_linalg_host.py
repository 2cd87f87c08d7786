"""The reference and the case table of the linear-algebra tests, on the CPU alone: the
conditions under which tests/test_gpu_linalg.py's inputs exercise what they claim, and the
fp64 mirror's own distance to the bounds the device is held to.  (The harness library is built
here as well: its host side exports the header's roff and pad2.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import dispatch_cases as DC
import linalg_cases as LC
import linalg_harness as LH
import linalg_mirror as M


@functools.lru_cache(maxsize=None)
def all_boundary():
    """The union of the pairs' boundary orders (needs the built library: not at import)."""
    return sorted(set().union(*(LC.boundary_orders(p) for p in LH.PAIRS)))


def test_longdouble_is_the_80_bit_format():
    assert np.finfo(np.longdouble).nmant == 63


def test_fp64_mirror_agrees_with_numpy_and_the_80_bit_mirror():
    """L_chol = L sqrt(D) of numpy.linalg.cholesky, and the 80-bit mirror, on family (a): these
    matrices have condition numbers below 10, so the factors agree to a few hundred u."""
    worst = 0.0
    for n in all_boundary():
        K = LC.spd(n)
        L, D, fail = M.ldl(K)
        assert fail is None
        L8, D8, fail8 = M.ldl(K, M.F80)
        assert fail8 is None and L8.dtype == np.longdouble
        Lc = np.linalg.cholesky(K)
        e1 = float(np.max(np.abs(L * np.sqrt(D) - Lc)) / np.max(np.abs(Lc)))
        e2 = float(max(np.max(np.abs(L - L8)), np.max(np.abs(D - D8) / D8)))
        worst = max(worst, e1, e2)
        assert e1 <= 1e-13 and e2 <= 1e-13, (n, e1, e2)
        b = LC.rhs(K, 0)[0]
        x = M.solve(L, D, b)
        assert np.max(np.abs(x - np.linalg.solve(K, b))) <= 1e-13 * np.max(np.abs(x)), n
    print(f"linalg_host fp64 mirror against numpy and the 80-bit mirror: worst {worst:.2e}")


def test_families_a_and_b_have_positive_pivots():
    for n in range(2, 257):
        assert M.ldl(LC.spd(n))[2] is None, n
    for n in all_boundary():
        for stage in LC.STAGES:
            K = LC.kkt(n, stage)
            assert K.shape == (n, n) and np.array_equal(K, K.T)
            assert M.ldl(K)[2] is None, (n, stage)


def test_family_b_is_the_oracles_ipm():
    """The restated loop takes the oracle's own iterations to the oracle's own status, the last
    system is ill-conditioned, and the stages are distinct."""
    from oracle import scp_reference as R
    for src in LC.KKT_SOURCES:
        Ks, it, st = LC.kkt_systems(src)
        x, s, lam, it_ref, st_ref = R.qp_ipm(*LC.first_qp(src), init="omega")
        assert (it, st) == (it_ref, st_ref), src
        assert np.linalg.cond(Ks["ipm last"]) >= 1e9 > 1e4 >= np.linalg.cond(Ks["ipm first"]), src
        assert not np.array_equal(Ks["ipm middle"], Ks["ipm last"])
        assert LC.pivot_margin(Ks["ipm last"]) >= 2 * LC.C_BOUND
    assert {DC.by_id(c).id for c in LC.KKT_ROWS} <= {c.id for c in DC.CASES}
    assert max(s[1] * s[2] + 1 for s in LC.KKT_SOURCES) == 256


@pytest.mark.parametrize("pair", LH.PAIRS, ids=["hg%d_rm%d" % p for p in LH.PAIRS])
def test_family_c_fails_at_exactly_its_intended_pivot(pair):
    cases = LC.failure_cases(pair)
    nmax = LC.max_orders()[pair]
    assert len(cases) == 16
    kinds = set()
    for label, K, k in cases:
        n = K.shape[0]
        assert 2 <= n <= nmax
        L, D, fail = M.ldl(K)
        assert fail == k, (label, fail)
        if "NaN" in label:
            assert np.isnan(K).sum() == 2
            continue
        assert np.all(D[:k] > 0)
        r0 = k // LC.CB * LC.CB
        jb = min(LC.CB, n - r0)
        where = "first" if r0 == 0 else ("last" if r0 + jb == n else "middle")
        kinds.add((where, "lone" if jb == 1 else ("short" if jb < LC.CB else "full"), (k - r0) % 2))
    assert kinds >= {("first", "full", 0), ("first", "full", 1), ("middle", "full", 0),
                     ("middle", "full", 1), ("last", "short", 0), ("last", "short", 1),
                     ("last", "lone", 0)}, kinds


def test_packing_helpers_equal_the_headers():
    lib = LH.load()
    for i in range(0, 300):
        assert LH.roff(i) == lib.lh_roff(i)
        assert LH.pad2(i) == lib.lh_pad2(i)
        assert LH.factor_doubles(i) == lib.lh_factor_doubles(i)
    # rows do not overlap and start 16-byte aligned
    for i in range(0, 299):
        assert LH.roff(i + 1) - LH.roff(i) >= i + 1 and LH.roff(i) % 2 == 0
    K = np.arange(25.0).reshape(5, 5)
    assert np.array_equal(LH.unpack_lower(LH.pack_lower(K), 5), np.tril(K))
    assert LH.is_current()


def test_orders_table_equals_the_plan_query():
    """The largest order per (HG, RM) pair, by the scan test_dispatch_host.py makes (here with a
    horizon array, which never changes the plan), against the table the sweeps use."""
    from scpqp import _lib as LB
    lib = LB.load()
    info = LB.PlanInfo()
    best = {}
    for V in range(1, LB.MAX_VEH + 1):
        for O in range(0, LB.MAX_OBST + 1):
            for H in range(1, LB.MAX_HP + 1):
                D = LB.Dims(n_veh=V, hp_max=H, n_obst=O, max_batch=0)
                if lib.scpqp_plan_query(C.byref(D), 1, C.byref(info)) == 0:
                    key = (int(info.hg), int(info.rm))
                    best[key] = max(best.get(key, 0), V * H + 1)
    table = LC.max_orders()
    assert table == best
    assert set(table) == set(LH.PAIRS)
    for (hg, rm), nmax in table.items():
        assert 64 * (rm - 1) < nmax <= 64 * rm
        sweep = LC.sweep_orders((hg, rm))
        assert sweep[0] == 2 and sweep[-1] == nmax and set(LC.boundary_orders((hg, rm))) <= set(range(2, nmax + 1))
        assert sweep == list(range(2, nmax + 1))
    for c in DC.CASES:
        assert c.n_veh * c.hp_max + 1 in LC.boundary_orders((c.kernel[0], c.kernel[2])), c.id
    assert table[(1, 4)] == 256


def test_fp64_mirror_meets_the_bounds_with_margin():
    """The mirror divides where the device multiplies by a reciprocal, so it must meet both
    bounds with c = 1 (Higham's own statement), a quarter of what the device is allowed."""
    worst = {}
    for fam in ("a",) + LC.STAGES:
        wf = ws = 0.0
        for n in all_boundary():
            K = LC.spd(n) if fam == "a" else LC.kkt(n, fam)
            L, D, fail = M.ldl(K)
            assert fail is None
            dinv = 1.0 / D
            fr = M.factor_ratio(K, L, dinv)
            b = LC.rhs(K, 0)
            sr = max(M.solve_ratio(L, dinv, b[i], M.solve(L, D, b[i])) for i in range(2))
            wf, ws = max(wf, fr), max(ws, sr)
        worst[fam] = (wf, ws)
        print(f"linalg_host fp64 mirror, family {fam}: factor ratio max {wf:.3f}, solve ratio max "
              f"{ws:.3f} of gamma; device bound c = {LC.C_BOUND}")
    for fam, (wf, ws) in worst.items():
        assert wf <= 1.0 and ws <= 1.0, (fam, wf, ws)
