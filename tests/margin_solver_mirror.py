"""The oracle's SCP loop with obstacle margins (scpqp_solve_margin of include/scpqp_margin.h),
for the margin tests: ``oracle.scp_reference.scp_solve`` in structured mode, restated on the
oracle's own building blocks (``linearise``, ``positions``, ``row_list``, ``qp_matrices``,
``qp_solve``, ``forward_u``) with rows and an evaluation that use

    D = dsafe_obs[i, o] + dsafe_extra + m[o, k]

for an obstacle row and are the oracle's otherwise (pair rows, the obstacle quirk and its
repetitions, the stopping rule).  With m = 0 it returns the oracle's u bitwise."""
import numpy as np

from oracle import scp_reference as R


def rows(p, lin, u, m):
    """``linearised_rows_structured`` with the margin m [nObst, Hp]."""
    nV, Hp, nO = p.nVeh, p.Hp, p.nObst
    N = nV * Hp
    pos = R.positions(lin, u, nV, Hp)
    rl = R.row_list(nV, Hp, nO)
    A = np.zeros((len(rl), N + 1)); b = np.zeros(len(rl))
    uu = np.asarray(u, float).reshape(nV, Hp)
    for r, (i, j, o, k) in enumerate(rl):
        if j >= 0:
            d = pos[i, k] - pos[j, k]
            D = p.dsafe_veh[i, j] + p.dsafe_extra
        else:
            d = pos[i, k] - p.obst[o, :, k]
            D = p.dsafe_obs[i, o] + p.dsafe_extra + m[o, k]
        Bi = lin.calB[i][2 * k:2 * k + 2]
        A[r, Hp * i:Hp * (i + 1)] = -2 * d @ Bi
        if j >= 0:
            Bj = lin.calB[j][2 * k:2 * k + 2]
            A[r, Hp * j:Hp * (j + 1)] = 2 * d @ Bj
        c = D * D - d @ d
        b[r] = -c + A[r, :N] @ uu.reshape(-1)
    A[:, N] = -1.0
    return A, b


def evaluate(p, lin, u, m, tol=R.CONSTRAINT_TOL, obst_quirk=True):
    """``evaluate_structured`` with the margin m [nObst, Hp]."""
    nV, Hp, nO = p.nVeh, p.Hp, p.nObst
    uu = np.asarray(u, float).reshape(nV, Hp)
    pos = R.positions(lin, u, nV, Hp)
    obj = 0.0
    for v in range(nV):
        e = pos[v] - p.ref_points[:, :, v]
        w = np.full(Hp, p.Q[v]); w[-1] = p.Q_final[v]
        obj += float(np.sum(w[:, None] * e * e) + p.R[v] * uu[v] @ uu[v])
    feasible, sv, mv = True, 0.0, 0.0
    cv = np.full((nV, nV, Hp), -np.inf)
    co = np.full((nV, nO, Hp), -np.inf)
    for v in range(nV):
        for k in range(Hp):
            for w in range(v + 1, nV):
                d = pos[v, k] - pos[w, k]
                ci = (p.dsafe_veh[v, w] + p.dsafe_extra) ** 2 - d @ d
                cv[v, w, k] = cv[w, v, k] = ci
                if ci > tol:
                    feasible = False; sv += ci; mv = max(mv, ci)
            reps = (nV - 1 - v) if obst_quirk else 1
            for _ in range(reps):
                for o in range(nO):
                    d = pos[v, k] - p.obst[o, :, k]
                    ci = (p.dsafe_obs[v, o] + p.dsafe_extra + m[o, k]) ** 2 - d @ d
                    co[v, o, k] = ci
                    if ci > tol:
                        feasible = False; sv += ci; mv = max(mv, ci)
    return R.Evaluation(feasible, obj, mv, sv, cv, co)


def scp_solve(p, m=None, max_scp=R.MAX_SCP_ITER, keep_history=True, polish="exact"):
    """``scp_solve(p, mode="structured")`` with the margin m [nObst, Hp] (None: zeros)."""
    nV, Hp, nO = p.nVeh, p.Hp, p.nObst
    N = nV * Hp
    m = np.zeros((nO, Hp)) if m is None else np.asarray(m, float).reshape(nO, Hp)
    lin = R.linearise(p, "structured")
    Phi0 = np.zeros((N, N)); Psi0 = np.zeros(N)
    for v in range(nV):
        Phi0[Hp * v:Hp * (v + 1), Hp * v:Hp * (v + 1)] = lin.Phi0[v]
        Psi0[Hp * v:Hp * (v + 1)] = lin.Psi0[v]
    u = np.zeros(N)
    if abs(u[0]) < R.EPS:
        u[0] = R.EPS
    ev = evaluate(p, lin, u, m)
    obj0, mv0 = ev.obj, ev.max_violation
    hist, n_ipm, it, conv = [], 0, 0, False
    for it in range(max_scp):
        A, b = rows(p, lin, u, m)
        P, q, G, h = R.qp_matrices(Phi0, Psi0, A, b, p.u_lim)
        res = R.qp_solve(P, q, G, h, p.u_lim, N, polish=polish)
        n_ipm += res.iters
        u_lin, u = u, res.z[:N].copy()
        ev = evaluate(p, lin, u, m)
        delta = (obj0 + R.SLACK_WEIGHT * mv0) - (ev.obj + R.SLACK_WEIGHT * ev.max_violation)
        obj0, mv0 = ev.obj, ev.max_violation
        if keep_history:
            hist.append(dict(u_lin=u_lin, A=A, b=b, z=res.z.copy(), obj=ev.obj,
                             maxviol=ev.max_violation, delta=delta, certified=res.certified))
        if nV == 1 and abs(delta) < R.DELTA_TOL and ev.max_violation > R.CONSTRAINT_TOL:
            conv = True
            break
        if abs(delta) < R.DELTA_TOL and ev.max_violation <= R.CONSTRAINT_TOL:
            conv = True
            break
    traj, U = R.forward_u(lin, u, nV, Hp)
    r = R.SCPResult(u=u, traj=traj, U=U, feasible=ev.feasible, obj=ev.obj,
                    max_violation=ev.max_violation, sum_violations=ev.sum_violations,
                    n_scp=it + 1, n_ipm=n_ipm, converged=conv, history=hist, lin=lin)
    r.evaluation = ev
    return r
