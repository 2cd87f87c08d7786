/*
 * scpqp_imm.h — interacting-multiple-model obstacle tracker: a bank of up to four six-state
 * filters per (realisation, obstacle) between the obstacle sensing and the obstacle prediction
 * of closed-loop rollouts (csrc/imm.hip).
 *
 * The filter of scpqp_tracker_accel.h runs one tuning for a whole rollout, and no one tuning
 * is right for an obstacle that cruises, then turns, then brakes: a learnt arc carried over
 * the horizon loses against a weaving obstacle, and a filter that starts at a = 0 follows the
 * onset of a braking only as fast as its Q_ACCEL allows.  This tracker runs several
 * hypotheses side by side, lets a Markov chain say how often the obstacle changes its mind,
 * moves the probabilities by each hypothesis' likelihood of the measurement, and tells the
 * planner the probability-weighted prediction.  scpqp_tracker.h and scpqp_tracker_accel.h are
 * unchanged and stay available; a lane runs one of the three.
 *
 * Modes.  M = n_modes, 1 <= M <= SCPQP_IMM_MAX_MODES = 4, the same for every lane of a call.
 * Every mode is the filter of scpqp_tracker_accel.h: its state (SCPQP_TRKA_NS = 6), its
 * measurement z and the draws behind it (no new Philox site: every mode of a lane sees the
 * one measurement the two single filters and the untracked prediction of the same step would
 * have seen), its F, its update, its clamps and its holds.  Every mode has its own row of
 * SCPQP_TRKA_NP = 14 fields, so the modes differ in process noise, initial sigmas, clamps and
 * holds: a "straight" mode has both holds 0 and small Q_YAW, Q_ACCEL; an "arc" mode holds w;
 * a "brake" mode holds a and has a large Q_ACCEL.
 *
 * Rows.
 *   trk [B][n_obst][M][14]    the tuning of mode j of lane (b, o)
 *   sw  [B][n_obst][M + 1][M] row 0: the initial probabilities mu0; rows 1..M: the transition
 *                             matrix Pi, Pi[i][j] = P(mode j at this call | mode i at the
 *                             previous one) at sw[b][o][1 + i][j]
 *
 * State carried between steps (in/out, caller-owned):
 *   x_imm [B][n_obst][M][6]     the estimate of every mode.  The caller fills it with NaN
 *                               before the first step: x_imm[b][o][0][0] being NaN means "not
 *                               initialised".
 *   cov   [B][n_obst][M][6][6]  P of every mode, symmetric.  Only the upper triangles are
 *                               read; both triangles are written.
 *   mu    [B][n_obst][M]        the mode probabilities.  Not read on a lane that is not
 *                               initialised.
 *
 * One call per MPC step, scpqp_obstacles_track_imm.  T = t_since >= 0 as in
 * scpqp_tracker_accel.h, a scalar.  Per lane (b, o), with i, j = 0..M-1 and every sum over the
 * modes taken in mode order, starting from 0:
 *
 * 1. Not initialised.  Every mode initialises as step 2 of scpqp_tracker_accel.h with its own
 *    row: x_j = (z, 0, 0), P_j = diag(R_j, P0_YAW_j^2, P0_ACCEL_j^2).  mu = mu0, every
 *    nis_j = NaN.  Continue at step 5.
 * 2. Mix, only when T > 0.  Pi applies per call, whatever the call's length: it is not
 *    rescaled by T.
 *      c_j     = sum_i Pi[i][j] mu_i
 *      w_{i|j} = (Pi[i][j] mu_i) / c_j; where c_j == 0 the weights are delta_ij, so a dead
 *                mode keeps its own state
 *      x0_j    = sum_i w_{i|j} x_i
 *      P0_j    = sum_i w_{i|j} (P_i + (x_i - x0_j)(x_i - x0_j)'), then (P0_j + P0_j') / 2
 *    Heading differences are not wrapped, as in the filters.  A term whose weight is exactly
 *    0 is skipped, not multiplied (a non-finite state of a mode that cannot be reached from
 *    does not spread).  With T == 0: c_j = mu_j, x0_j = x_j, P0_j = P_j.
 * 3. Filter.  Every mode runs step 1 (predict over T with its own Q) and step 3 (update with
 *    z and its own R) of scpqp_tracker_accel.h from (x0_j, P0_j), dead modes included, and
 *    keeps nis_j and the diagonal of the Cholesky factor L_j of S_j.
 * 4. Probabilities.
 *      l_j  = -nis_j / 2 - sum_k log L_j,kk          (the log-likelihood up to a constant)
 *      mu_j = c_j exp(l_j - max l) / sum_j' c_j' exp(l_j' - max l)
 *    The maximum and the sum are taken over the modes with c_j > 0; the modes with c_j == 0
 *    stay at exactly 0.  No mode with c_j > 0 (the caller handed in a mu without a positive
 *    entry) is trouble, step 6.
 * 5. Outputs.  Every mode's horizon is step 4 of scpqp_tracker_accel.h from its own estimate
 *    with its own clamps and holds, point_j[k].
 *      obst_out[b][o][0 / 1][k] = sum_j mu_j point_j[k]
 *      x_hat [B][n_obst][6]     = sum_j mu_j x_j
 *    The modes with mu_j exactly 0 are skipped.  nis [B][n_obst][M] (may be NULL) receives
 *    nis_j.  z_out [B][n_obst][4] (may be NULL) follows the z_out rule of
 *    scpqp_tracker_accel.h with "a bad tracker row" read as "a bad lane" below.
 * 6. Trouble.  Trouble in any mode (step 5 of scpqp_tracker_accel.h: a Cholesky pivot, a
 *    non-finite estimate, P or nis, a bad obstacle row or osense row), a probability that is
 *    not finite or no mode with c_j > 0 turns the whole lane to NaN: every mode's x_imm and
 *    cov, mu, x_hat, nis and the [2][hp] block.  The lane initialises itself again on the next call.  The call
 *    returns 0.
 *
 * Off lane: all M rows of trk all-zero (a -0.0 compares equal).  Its sw is not read.  There is
 * no filter: the lane's obst block is bitwise what scpqp_obstacles_predict writes when osense
 * is NULL and what scpqp_obstacles_predict_sensed writes otherwise (the entry point launches
 * that very kernel into obst_out first, and this tracker's kernel skips the off lanes).
 * x_imm, cov and mu of the lane are left alone; x_hat and nis are NaN.
 *
 * Bad lane: any mode's row is bad by the rule of scpqp_tracker_accel.h; off and non-off rows
 * are mixed; any entry of sw is non-finite or negative; mu0 or a row of Pi does not sum to 1
 * within SCPQP_IMM_SUM_TOL = 1e-12 (the sum in mode order from 0).  A bad lane writes NaN to
 * its own x_imm, cov, mu, x_hat, nis and obst block, touches nothing of any other lane, and
 * the call returns 0.
 *
 * What the tracker still does not know.  The weighted mean of two diverging hypotheses lies
 * between them, where neither hypothesis puts the obstacle: the planner is told one point per
 * time, not a set.  Pi is a tuning per call, not a rate: calls of another length need another
 * Pi.  The footprint (LENGTH, WIDTH: the dsafe tables stay the controller's knowledge).
 * There are no rows per variant and no sampler: a bank is chosen, not drawn.
 *
 * Conventions of scpqp_sensing.h: device pointers, asynchronous on `stream`, 0 or a negative
 * SCPQP_E_* code with the message in scpqp_last_error().  Every argument is validated on the
 * host before any HIP call.  B = 0 is a no-op (the arrays may then be NULL).
 */
#ifndef SCPQP_IMM_H
#define SCPQP_IMM_H

#include "scpqp_tracker_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_IMM_MAX_MODES 4
#define SCPQP_IMM_SUM_TOL 1e-12

/* One step of every lane's bank, as described above.  rows [B][n_obst][SCPQP_OBST_NP], osense
 * [B][n_obst][SCPQP_OSENSE_NP] or NULL, trk and sw as above.  Sizes and t_meas, lead, dt as
 * scpqp_obstacles_predict; 1 <= n_modes <= SCPQP_IMM_MAX_MODES; t_since finite and >= 0.
 * B * n_obst * n_modes * 36 and B * n_obst * 2 * hp must fit int32 (SCPQP_E_SIZE).  At B > 0,
 * rows, trk, sw, x_imm, cov, mu, x_hat and obst_out must be non-NULL, and st if osense is
 * given; z_out and nis may be NULL. */
int scpqp_obstacles_track_imm(int32_t B, int32_t n_obst, int32_t hp, int32_t n_modes,
                              const double* rows, const double* osense,
                              const scpqp_sense_stream* st, const double* trk, const double* sw,
                              double t_meas, double t_since, double lead, double dt,
                              double* x_imm, double* cov, double* mu, double* x_hat,
                              double* z_out, double* nis, double* obst_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_IMM_H */
