/*
 * scpqp_margin.h — chance-constrained obstacle margins: the trackers' covariances, pushed
 * through the very horizon the planner is told, become a safety margin per (realisation,
 * obstacle, horizon step) that the solve adds to its obstacle safety distance
 * (csrc/margin.hip), and the two entry points that hand the array to the solve and to the
 * evaluation as it is written (scpqp_solve_margin, scpqp_evaluate_margin, below).
 *
 * The trackers of scpqp_tracker_accel.h and scpqp_imm.h carry a 6 x 6 covariance per
 * (realisation, obstacle, mode) and tell the planner one point per horizon step.  The planner
 * then keeps the same distance from an obstacle it has watched for ten steps as from one it
 * first saw a step ago, and the same from one whose hypotheses lie metres apart at the end of
 * the horizon.  This step says how far from the told point the obstacle may be.
 *
 * Inputs.  M = n_modes, 1 <= M <= SCPQP_IMM_MAX_MODES = 4, the same for every lane of a call.
 *   trk [B][n_obst][M][14]     the tuning of mode j (the rows of scpqp_tracker_accel.h)
 *   x   [B][n_obst][M][6]      the estimate of every mode
 *   cov [B][n_obst][M][6][6]   P of every mode; only the upper triangles are read
 *   mu  [B][n_obst][M]         the mode probabilities, or NULL when M == 1 (= 1)
 * With M = 1 and mu == NULL the state arrays of scpqp_obstacles_track_accel pass as they are;
 * with M = 1..4 so do x_imm, cov and mu of scpqp_obstacles_track_imm.  The step is called
 * after the tracker step of the same MPC step, with the same lead, dt and hp.  Nothing of the
 * state is written.
 *
 * Per lane (b, o), with tau_k = (k + 1) * dt + lead, k = 0..hp-1, and point(s)[k] the two
 * coordinates of step 4 of scpqp_tracker_accel.h from the state s = (x, y, h, s, w, a) under
 * the mode's row (s0 = max(s, 0), the clamps on w and a, the holds, the three pieces on
 * `advance` of csrc/scpqp_manoeuvre_pose.h, its stop rule):
 *
 * 1. Per mode j with mu_j > 0 (a mode with mu_j exactly 0 is skipped, as in the outputs of
 *    scpqp_imm.h):
 *      L_j     = the lower Cholesky factor of P_j, P_j = L_j L_j', column by column:
 *                d = P[c][c] - sum_{k<c} L[c][k]^2, L[c][c] = sqrt(d),
 *                L[i][c] = (P[i][c] - sum_{k<c} L[i][k] L[c][k]) / L[c][c]
 *      sigma_i = x_j + sqrt(6) L_j[:, i] and x_j - sqrt(6) L_j[:, i], i = 0..5: twelve states
 *      c_j[k]  = point(x_j)[k]
 *      S_j[k]  = (1 / 12) sum_i e_i e_i', e_i = point(sigma_i)[k] - c_j[k], over the twelve,
 *                plus tau_k Q_POS_j^2 on both diagonal entries.
 *    S_j is the second moment about the point the planner is told, not about the mean of the
 *    sigma points.  It is taken through the horizon function itself, so the clamps, the holds
 *    and the stop rule need no Jacobian: where a braking obstacle stops is where a first-order
 *    propagation fails.
 * 2. Mix, every sum in mode order over the modes with mu_j > 0:
 *      cbar[k]  = sum_j mu_j c_j[k]
 *      Sigma[k] = sum_j mu_j (S_j[k] + (c_j[k] - cbar[k]) (c_j[k] - cbar[k])')
 *    The second term is the spread between the hypotheses: the set the mean hides.  cbar is
 *    the point scpqp_obstacles_track_imm writes.  mu is used as given (it is not normalised).
 * 3. With Sigma = [[Sxx, Sxy], [Sxy, Syy]]:
 *      lam             = (Sxx + Syy) / 2 + hypot((Sxx - Syy) / 2, Sxy)   (the larger eigenvalue)
 *      margin[b][o][k] = min(kappa * sqrt(lam), m_max)
 *      sigma_out[b][o][k][0..2] = Sxx, Sxy, Syy                          (when not NULL)
 *
 * Off lane: all M rows of trk all-zero (a -0.0 compares equal).  margin and sigma_out are
 * exactly 0 and the lane's x, cov and mu are not looked at (they may hold anything).
 *
 * Trouble turns the lane's margin and sigma_out to NaN, touches nothing of any other lane,
 * and the call returns 0, as the NaN obst block of the trackers; scpqp_solve_margin then reports
 * SCPQP_ST_INVALID for that problem.  Trouble is any of
 *   - a lane that is not initialised (x[b][o][0][0] is NaN);
 *   - a bad row in any mode (the rule of scpqp_tracker_accel.h: a non-finite or negative
 *     field, or a row that is not off with some R_* = 0);
 *   - off and non-off rows mixed;
 *   - a non-finite entry of x, of the upper triangle of P or of mu, in any mode, skipped
 *     ones included;
 *   - a negative mu_j, or no positive mu_j;
 *   - a Cholesky pivot d <= 0 or not finite, in a mode with mu_j > 0;
 *   - a lam that is not finite (an overflow on the way).
 *
 * What the margin does not know.  The process noise on speed, turn rate and acceleration that
 * accumulates over the horizon: only Q_POS enters, as tau_k Q_POS^2.  Non-Gaussian tails: the
 * twelve sigma points match a Gaussian's first two moments and nothing beyond.  The vehicles'
 * own state uncertainty.  The footprint (the dsafe tables stay the controller's knowledge).
 * kappa is a distance in sigmas of the larger principal axis: for a two-dimensional Gaussian
 * of covariance Sigma the probability of lying farther than kappa sqrt(lam) from its mean is
 * at most exp(-kappa^2 / 2), with equality for a circular one; p_miss asks for
 * kappa = sqrt(-2 ln p_miss).  There are no margins between vehicles and none per variant.
 *
 * Conventions of scpqp_sensing.h: device pointers, asynchronous on `stream`, 0 or a negative
 * SCPQP_E_* code with the message in scpqp_last_error().  Every argument is validated on the
 * host before any HIP call.  B = 0 is a no-op (the arrays may then be NULL).
 */
#ifndef SCPQP_MARGIN_H
#define SCPQP_MARGIN_H

#include "scpqp_imm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The margins of every lane, as described above.  Sizes as scpqp_obstacles_track_imm:
 * 1 <= n_obst <= SCPQP_MAX_OBST, 1 <= hp <= SCPQP_MAX_HP, 1 <= n_modes <= SCPQP_IMM_MAX_MODES,
 * B * n_obst * n_modes * 36 and B * n_obst * 3 * hp must fit int32 (SCPQP_E_SIZE).  lead and
 * dt finite; kappa and m_max finite and >= 0.  At B > 0, trk, x, cov and margin must be
 * non-NULL, and mu unless n_modes == 1; sigma_out may be NULL. */
int scpqp_obstacles_margin(int32_t B, int32_t n_obst, int32_t hp, int32_t n_modes,
                           const double* trk, const double* x, const double* cov,
                           const double* mu, double lead, double dt, double kappa, double m_max,
                           double* margin, double* sigma_out, void* stream);

/* scpqp_solve and scpqp_evaluate of scpqp.h with obstacle margins.  obst_margin
 * [B][n_obst][hp_b], a DEVICE pointer: metres added to the obstacle safety distance of problem
 * b, obstacle o, horizon step k, in a slot of n_obst * hp_max doubles per problem with the
 * problem's own horizon as the packed prefix, as scpqp_batch_in.obst (the array
 * scpqp_obstacles_margin writes at hp = hp_max passes as it is).  Wherever the solve and the
 * evaluation use (dsafe_obs[v][o] + dsafe_extra)^2 for an obstacle row they use
 * (dsafe_obs[v][o] + dsafe_extra + obst_margin[b][o][k])^2 with the problem's variant: the
 * evaluation of the QCQP (c_obs, violations, feasibility) and the row linearisation (the
 * trace's h_r carries it).  Rows between vehicles, the obstacle quirk and its repetitions are
 * untouched.
 *   - obst_margin == NULL: every output is bitwise what scpqp_solve / scpqp_evaluate write, and
 *     an all-zero array gives bitwise the same.
 *   - A problem with a non-finite or negative entry among the n_obst * hp_b entries of its
 *     prefix reports SCPQP_ST_INVALID with zero counters and nothing else of it is written (the
 *     rule of a horizon outside its slot or a variant outside its table; scpqp_evaluate_margin
 *     has no status word and writes nothing of it).  Entries past the prefix are never read.
 *   - With n_obst == 0 the pointer is ignored.
 * Everything else (arguments, error codes, the memory plan, the kernel a call runs) is that of
 * scpqp_solve and scpqp_evaluate.  scpqp_batch_in itself is unchanged: callers built against
 * scpqp.h alone are unaffected. */
int scpqp_solve_margin(scpqp_handle* h, int32_t B, const scpqp_batch_in* in,
                       const double* obst_margin, const scpqp_batch_out* out, void* stream);
int scpqp_evaluate_margin(scpqp_handle* h, int32_t B, const scpqp_batch_in* in,
                          const double* obst_margin, const double* u, const scpqp_eval_out* out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_MARGIN_H */
