/*
 * scpqp_yield.h — right of way and graded braking for the speed governor: a longitudinal
 * command per (realisation, vehicle) of closed-loop rollouts, taken from the planner's own plan
 * (csrc/yield.hip).
 *
 * The speed governor (scpqp_governor.h) brakes every vehicle of a conflicting pair, fully.  Here
 * every vehicle carries a rank, and in a vehicle-vehicle conflict only the side without right of
 * way yields; and the deceleration is sized to stop at the last plan point before the conflict,
 * between a gentlest and a largest value.  With equal ranks, A_EASE = A_BRAKE and S_STAND = 0
 * scpqp_yield_step gives what scpqp_governor_step gives, bit for bit: nobody outranks anybody,
 * and the graded deceleration is pinned at A_BRAKE.
 *
 * Rows.  yld[B][n_veh][SCPQP_YLD_NP], SCPQP_YLD_NP = 10 doubles.  Indices 0..6 are the
 * governor's seven (SCPQP_GOV_*), with the same meaning, units and order:
 *
 *   index      unit    meaning
 *   0 V_REF    m/s     cruise speed
 *   1 A_ACC    m/s^2   largest acceleration
 *   2 A_BRAKE  m/s^2   largest deceleration (a magnitude)
 *   3 K_V      1/s     gain of the speed loop
 *   4 J_MAX    m/s^3   largest change of the command per second of hold time; +inf: no slew
 *                      limit
 *   5 LOOK     steps   how many plan steps are examined (an integer-valued double)
 *   6 BAND     m       clearance demanded on top of the required distance
 *   7 PRIO     -       rank, an integer-valued double in 0 .. 2^20 (SCPQP_YLD_PRIO_MAX); the
 *                      larger rank has right of way
 *   8 A_EASE   m/s^2   gentlest deceleration commanded on a conflict (a magnitude), <= A_BRAKE
 *   9 S_STAND  m/s     another vehicle at or below this speed is standing and has no rank;
 *                      0: rule off
 *
 * One call per MPC step, after the solve, scpqp_yield_step.  Its inputs x0, traj, obst,
 * obst_margin, hp, dreq_obs, dreq_veh, t_hold and t_back are those of scpqp_governor_step, in
 * the same slots, with yld in place of gov.
 *
 * Outputs, each [B][n_veh]: a_cmd the commanded acceleration; k_conf (int32) the first step
 * with a conflict that counts; k_any (int32) the first step with any conflict; who (int32) whom
 * the lane yields to; clear the smallest clearance found; d_stop the length of the plan before
 * the conflict.  All but a_cmd may be NULL.
 *
 * Per lane (b, v), with s = x0[b][v][3] and a_now = x0[b][v][4]:
 *
 * 1. Own row.  Off row: all ten fields exactly 0 (a -0.0 compares equal).  a_cmd = a_now bit for
 *    bit, k_conf = k_any = who = -1, clear = d_stop = NaN, and nothing else is read.  Bad lane:
 *    the governor's rules on fields 0..6, the state and hp[b] (a field negative, or non-finite
 *    other than J_MAX = +inf; LOOK not an integer or above SCPQP_MAX_HP; s or a_now non-finite;
 *    a horizon hp[b] outside 1..hp_max), or PRIO not an integer in 0 .. 2^20, A_EASE or S_STAND
 *    negative or non-finite, or A_EASE > A_BRAKE.  The lane writes a_cmd = NaN,
 *    k_conf = k_any = who = -2, clear = d_stop = NaN, touches nothing of any other lane, and the
 *    call returns 0.  An off row is off whatever its state holds.
 * 2. Who counts.  Every obstacle counts.  Another vehicle w counts unless all three hold:
 *      (a) w's row is neither off nor bad by its fields alone (its state and hp[b] are not
 *          asked): a vehicle without a governor never yields, so it is yielded to;
 *      (b) PRIO_v > PRIO_w;
 *      (c) w is not standing.  w is standing iff S_STAND_v > 0 and not x0[b][w][3] > S_STAND_v:
 *          a speed that is not a number stands.
 * 3. Clearance.  The pairs (k, other), k < min(LOOK, hp_b), the clearance
 *      c = |p_v(k) - q(k)| - (required + BAND)
 *    and the non-finite rule (c = -inf) are the governor's step 1, unchanged.  clear is the
 *    minimum of c over all pairs, +inf when nothing was examined.  k_any is the first step with
 *    any c < 0, else -1.  k_conf is the first step with a c < 0 against an other that counts,
 *    else -1.  A pair with a non-finite examined entry, or a c that is not a number, counts
 *    whatever the ranks.  who is the smallest j with c < 0 at step k_conf among those that
 *    count, j = o for obstacle o and j = n_obst + w for vehicle w; else -1.  k_conf and who are
 *    the two halves of the minimum of the integer key k (n_obst + n_veh) + j, and k_any and
 *    clear are minima as well, so none depends on how the device maps the pairs to its threads.
 * 4. Wish.  Without a counted conflict: d_stop = +inf and
 *      a_des = min(max(K_V (V_REF - s), -A_BRAKE), A_ACC).
 *    With one:
 *      d_stop = sum_{j=0}^{k_conf-1} |p_v(j) - p_v(j-1)|,   p_v(-1) = (x0[0], x0[1])
 *    the length of the plan from its start to the last point before the conflict, 0 at
 *    k_conf = 0;
 *      a_need = max(s, 0)^2 / (2 d_stop), +inf where d_stop is 0 or not a finite number
 *      a_des  = -min(A_BRAKE, max(A_EASE, a_need)).
 * 5. Slew limit and stop rule: the governor's steps 3 and 4, verbatim.
 *      a_cmd = min(max(a_des, a_now - J_MAX t_hold), a_now + J_MAX t_hold); skipped when J_MAX
 *      is +inf;
 *      s_app = max(s - a_now t_back, 0);  a_cmd = max(a_cmd, -s_app / t_hold).
 *
 * What it does not know.  The ranks are static: there is no first-come rule and no negotiation,
 * and a rank does not change when the situation does.  A vehicle with right of way is not told
 * to hurry: it keeps its speed loop while the other waits.  There is no hysteresis beyond the
 * slew limit: a conflict that flickers gives a command that flickers, and a vehicle that was
 * standing loses that status the moment it moves.  d_stop is measured on the plan's points, not
 * to the conflict itself: the stop aims at the last point before the conflicting one, up to a
 * plan step short of where the required distance is first missed.  As the governor it uses the
 * plan's points only: not the footprints, not the obstacles' speeds, no time to collision.
 * There are no rows per variant and no sampler: a tuning is chosen, not drawn.
 *
 * Conventions of scpqp_governor.h: device pointers, asynchronous on `stream`, 0 or a negative
 * SCPQP_E_* code with the message in scpqp_last_error().  Every argument is validated on the
 * host before any HIP call.  B = 0 is a no-op (the arrays may then be NULL).
 */
#ifndef SCPQP_YIELD_H
#define SCPQP_YIELD_H

#include "scpqp_governor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_YLD_NP 10
#define SCPQP_YLD_PRIO 7
#define SCPQP_YLD_A_EASE 8
#define SCPQP_YLD_S_STAND 9
#define SCPQP_YLD_PRIO_MAX 1048576 /* 2^20 */

/* One step of every lane, as described above.  1 <= n_veh <= SCPQP_MAX_VEH,
 * 0 <= n_obst <= SCPQP_MAX_OBST, 1 <= hp_max <= SCPQP_MAX_HP, B >= 0; t_hold finite and > 0,
 * t_back finite and >= 0.  B * n_veh * 2 * hp_max, B * n_obst * 2 * hp_max and
 * B * n_veh * max(n_veh, n_obst, SCPQP_YLD_NP) must fit int32 (SCPQP_E_SIZE).  At B > 0, x0,
 * traj, dreq_veh, yld and a_cmd must be non-NULL, and obst and dreq_obs if n_obst > 0;
 * obst_margin, hp, k_conf, k_any, who, clear and d_stop may be NULL. */
int scpqp_yield_step(int32_t n_veh, int32_t n_obst, int32_t hp_max, int32_t B, double t_hold,
                     double t_back, const double* x0, const double* traj, const double* obst,
                     const double* obst_margin, const int32_t* hp, const double* dreq_obs,
                     const double* dreq_veh, const double* yld, double* a_cmd, int32_t* k_conf,
                     int32_t* k_any, int32_t* who, double* clear, double* d_stop, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_YIELD_H */
