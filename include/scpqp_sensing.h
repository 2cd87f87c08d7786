/*
 * scpqp_sensing.h — sensing truth: noisy, biased, late and lost measurements of
 * closed-loop rollouts (csrc/sensing.hip).
 *
 * The reference's controller measures the realised state exactly: x_measured is
 * read straight out of the vehicle path (main.py:112), and the obstacle positions
 * it extrapolates (main.py:123, MPC_Iter.py:45-51) are the true ones.  A sensing
 * truth gives every (realisation, vehicle) its own sensor: noise on position,
 * heading, speed and steering angle, a compass offset, an odometer scale, a
 * probability that a step's measurement is lost and an extra latency; and every
 * (realisation, obstacle) a noise on the pose and speed the controller measures.
 * The controller does not know the rows: its delay compensation, solve and
 * clipping take the measurement as the state, and it does not know that a
 * measurement is stale or held.  The world (plant, metrics, plotted paths) keeps
 * the true state and the true obstacle rows.
 *
 * Vehicle rows.  sense[B][n_veh][SCPQP_SENSE_NP], SCPQP_SENSE_NP = 8 doubles:
 *
 *   index           unit   nominal  meaning
 *   0 SIG_POS       m      0        sigma of independent noise on x and on y
 *   1 SIG_HEADING   rad    0        sigma on state 2
 *   2 SIG_SPEED     m/s    0        sigma on state 3
 *   3 SIG_STEER     rad    0        sigma on state 5
 *   4 BIAS_HEADING  rad    0        constant offset on state 2
 *   5 SCALE_SPEED   -      1        odometer scale on state 3
 *   6 P_DROP        -      0        probability that this step's measurement is lost
 *   7 LAG           ticks  0        extra latency, a whole number of ticks >= 0
 *
 * State 4 (Model.py:72, the acceleration) is passed through unchanged.
 *
 * The measurement of lane (b, v) at MPC step `epoch`
 * (x_path [B][n_veh][n_ticks + 1][6], the layout of scpqp_plant_step):
 *
 *   k     = max(0, k_meas - (int)LAG)
 *   x     = x_path[b][v][k][0..5]
 *   m[0]  = x[0] + SIG_POS * z0(c0 = 0)
 *   m[1]  = x[1] + SIG_POS * z1(c0 = 0)
 *   m[2]  = (x[2] + BIAS_HEADING) + SIG_HEADING * z0(c0 = 1)
 *   m[3]  = SCALE_SPEED * x[3] + SIG_SPEED * z1(c0 = 1)
 *   m[4]  = x[4]
 *   m[5]  = x[5] + SIG_STEER * z0(c0 = 2)
 *   lost  = u2(c0 = 3) < P_DROP  and  x_held[b][v][0] is not NaN
 *
 * Every product and every sum is its own rounding (__dmul_rn / __dadd_rn, no
 * fused multiply-add), so a plain fp64 evaluation differs only through the
 * normal draw.  z0, z1 are the normal pair and u2 the [0, 1) uniform of one
 * Philox4x32-10 call, mapped exactly as scpqp_noise.h maps them:
 *
 *   key      (seed & 0xffffffff, seed >> 32)
 *   counter  c0 as above   c1 = epoch
 *            c2 = (SCPQP_NOISE_SITE_SENSE_DRAW << 24) | v   c3 = b_offset + b
 *
 * x_held [B][n_veh][6] is in/out and carries the last delivered measurement
 * between steps.  If `lost`, the output is x_held, unchanged; otherwise the
 * output is m and x_held becomes m.  A caller fills x_held with NaN before the
 * first step, so the first measurement is always delivered; P_DROP = 1 then
 * holds that first measurement for ever, and P_DROP = 0 never loses one
 * (u2 < 0 is false).  delivered [B][n_veh] (int32, may be NULL) receives 1 or 0.
 *
 * Nominal row: exactly (0, 0, 0, 0, 0, 1, 0, 0).  The lane copies the six
 * doubles of x_path[b][v][k_meas] bit for bit (the sign of a zero included,
 * which the arithmetic above would not keep), stores them to x_held, draws
 * nothing and reports delivered.
 *
 * Bad row: any field non-finite, a sigma < 0, P_DROP outside [0, 1], LAG < 0 or
 * not a whole number.  The lane writes NaN to its six outputs and to
 * x_held[b][v] and reports delivered = 0.  It touches nothing of any other lane
 * and the call returns 0: numerical trouble never aborts a batch.
 *
 * Sampler.  scpqp_sense_sample draws field f of (b, v) from ONE Philox call at
 * counter (f, 0, (SCPQP_NOISE_SITE_SENSE << 24) | v, b_offset + b); kinds, clamp
 * and value formula are those of scpqp_truth.h.  After clamping, LAG is rounded
 * to the nearest whole number (rint); so is a FIXED LAG.
 *
 * Obstacle sensing.  osense[B][n_obst][SCPQP_OSENSE_NP] holds SIG_POS,
 * SIG_HEADING, SIG_SPEED.  scpqp_obstacles_predict_sensed is
 * scpqp_obstacles_predict (scpqp_obstacles.h) from the MEASURED pose and speed:
 *
 *   xm = x(t_meas) + SIG_POS * z0(c0 = 0)     ym = y(t_meas) + SIG_POS * z1(c0 = 0)
 *   hm = h(t_meas) + SIG_HEADING * z0(c0 = 1) sm = s + SIG_SPEED * z1(c0 = 1)
 *   obst[b][o][0][k] = step_k * cos hm + xm,  obst[b][o][1][k] = step_k * sin hm + ym
 *   step_k = ((k + 1) * dt + lead) * sm
 *   counter  c1 = epoch   c2 = (SCPQP_NOISE_SITE_SENSE_OBST << 24) | o   c3 = b_offset + b
 *
 * An all-zero osense row takes the code path of scpqp_obstacles_predict and
 * gives its output bitwise.  A bad osense row (a non-finite or negative field)
 * or a bad obstacle row writes NaN to that obstacle's [2][hp] block only.
 *
 * Sites.  5 (row sampler), 6 (per-step vehicle draws) and 7 (per-step obstacle
 * draws) are disjoint from the sites 0..2 of scpqp_noise.h, 3 of scpqp_truth.h
 * and 4 of scpqp_obstacles.h: a sensing seed equal to the noise, truth or
 * obstacle seed shares no counter with them.
 *
 * Conventions of scpqp_obstacles.h: device pointers, asynchronous on `stream`,
 * 0 or a negative SCPQP_E_* code with the message in scpqp_last_error().  Every
 * argument is validated on the host before any HIP call.  B = 0 is a no-op (the
 * arrays may then be NULL).
 */
#ifndef SCPQP_SENSING_H
#define SCPQP_SENSING_H

#include "scpqp_obstacles.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_SENSE_NP 8
#define SCPQP_SENSE_SIG_POS 0
#define SCPQP_SENSE_SIG_HEADING 1
#define SCPQP_SENSE_SIG_SPEED 2
#define SCPQP_SENSE_SIG_STEER 3
#define SCPQP_SENSE_BIAS_HEADING 4
#define SCPQP_SENSE_SCALE_SPEED 5
#define SCPQP_SENSE_P_DROP 6
#define SCPQP_SENSE_LAG 7

#define SCPQP_OSENSE_NP 3
#define SCPQP_OSENSE_SIG_POS 0
#define SCPQP_OSENSE_SIG_HEADING 1
#define SCPQP_OSENSE_SIG_SPEED 2

#define SCPQP_NOISE_SITE_SENSE 5
#define SCPQP_NOISE_SITE_SENSE_DRAW 6
#define SCPQP_NOISE_SITE_SENSE_OBST 7

typedef struct scpqp_sense_stream {
    uint64_t seed;
    uint32_t epoch;      /* c1: the MPC step index */
    uint32_t b_offset;   /* c3 = b_offset + b      */
} scpqp_sense_stream;

typedef struct scpqp_sense_dist {
    int32_t  n_veh;      /* 1..SCPQP_MAX_VEH */
    int32_t  pad0;
    double   mean[SCPQP_SENSE_NP][SCPQP_MAX_VEH];
    scpqp_truth_field field[SCPQP_SENSE_NP];
    uint64_t seed;
    uint32_t b_offset;   /* c3 = b_offset + b */
    uint32_t pad1;
} scpqp_sense_dist;

/* x_meas_out [B][n_veh][6] from x_path [B][n_veh][n_ticks + 1][6] as described above.
 * n_veh in 1..SCPQP_MAX_VEH; n_ticks >= 0 and 0 <= k_meas <= n_ticks (n_ticks = 0 is the
 * step-0 form: the "path" is the state itself).  B * n_veh * (n_ticks + 1) * 6 must fit
 * int32 (SCPQP_E_SIZE).  x_path, sense, st, x_held and x_meas_out must be non-NULL at
 * B > 0; delivered may be NULL. */
int scpqp_sense_measure(int32_t B, int32_t n_veh, int32_t n_ticks, int32_t k_meas,
                        const double* x_path, const double* sense, const scpqp_sense_stream* st,
                        double* x_held, int32_t* delivered, double* x_meas_out, void* stream);

/* sense[b][v] = (0, 0, 0, 0, 0, 1, 0, 0) */
int scpqp_sense_fill_nominal(int32_t B, int32_t n_veh, double* sense, void* stream);

/* sense[b][v][f] drawn as described above.  SCPQP_E_ARG (the message names the field)
 * unless: n_veh in 1..SCPQP_MAX_VEH; every kind in range; every spread finite and >= 0;
 * lo <= hi; every mean[f][v], v < n_veh, finite; and, with floor(f, v) = mean[f][v] of a
 * FIXED field and lo otherwise: every sigma's floor >= 0, P_DROP's floor in [0, 1] and its
 * hi (a FIXED field: its mean) in [0, 1], LAG's floor >= 0: the sampler never emits a bad
 * row. */
int scpqp_sense_sample(const scpqp_sense_dist* d, int32_t B, double* sense, void* stream);

/* scpqp_obstacles_predict from the measured pose and speed: obst_out [B][n_obst][2][hp]
 * from rows [B][n_obst][SCPQP_OBST_NP] and osense [B][n_obst][SCPQP_OSENSE_NP].  Sizes and
 * t_meas, lead, dt as scpqp_obstacles_predict. */
int scpqp_obstacles_predict_sensed(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                                   const double* osense, const scpqp_sense_stream* st,
                                   double t_meas, double lead, double dt, double* obst_out,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_SENSING_H */
