/*
 * scpqp_obstacles.h — obstacle truth: per-realisation obstacle motion of
 * closed-loop rollouts (csrc/obstacles.hip, csrc/metrics.hip).
 *
 * The reference moves every obstacle on a straight line at constant speed
 * (main.py:61-71) and the controller extrapolates it the same way from the
 * position it measures (main.py:123, MPC_Iter.py:45-51), so the prediction is
 * always right.  An obstacle truth gives every (realisation, obstacle) its own
 * start pose, speed, footprint and turn rate.  The world (the realised-path
 * metrics, the plotted obstacle path) moves the obstacle by its row; the
 * controller keeps the straight-line extrapolation from what it measures and
 * never sees the turn rate.
 *
 * A row holds SCPQP_OBST_NP = 7 doubles: rows[B][n_obst][SCPQP_OBST_NP].
 *
 *   index        field                        nominal
 *   0 X, 1 Y     position at t = 0, m         scenario.obstacles[o][0:2]
 *   2 HEADING    heading at t = 0, rad        [2]
 *   3 SPEED      constant speed, m/s          [3]
 *   4 LENGTH     footprint length, m          [4]
 *   5 WIDTH      footprint width, m           [5]
 *   6 YAW_RATE   constant turn rate w, rad/s  0
 *
 * Pose at time t (constant turn rate and speed, closed form).  With
 * a = 0.5 * w * t:
 *
 *   x(t) = x + (s * t) * sinc(a) * cos(h + a)
 *   y(t) = y + (s * t) * sinc(a) * sin(h + a)
 *   h(t) = h + w * t
 *   sinc(a) = 1 - a * a / 6  for |a| < 1e-4,  sin(a) / a  otherwise
 *
 * (the chord of the arc: length 2 (s / w) sin a, direction h + a).  The series
 * error a^4 / 120 is below 1e-18 at the switch, which is continuous to one unit
 * in the last place.
 *   - A row with YAW_RATE == 0.0 exactly is evaluated with the straight-line
 *     expression of scpqp_metrics.h instead,  t * s * cos h + x,  t * s * sin h + y,
 *     h(t) = h:  the nominal row gives bitwise what the constant obstacles of
 *     scpqp_metrics_params give.  (In fp64 the arc form reduces to it.)
 *   - The time of global tick g is  t = g * tick_length  (one rounding), in the
 *     metrics and in scpqp_obstacles_pose alike.
 *   - No rounding order beyond this is promised: the device contracts a * b + c
 *     into one fused multiply-add where it can, and its sincos is within an ulp.
 *     A plain fp64 evaluation agrees to a few units in the last place of the
 *     coordinates.
 *
 * What the controller knows (scpqp_obstacles_predict).  It measures the true
 * pose at t_meas and extrapolates straight from it with the measured heading
 * and the row's speed:
 *
 *   obst[b][o][0][k] = step_k * cos h(t_meas) + x(t_meas)
 *   obst[b][o][1][k] = step_k * sin h(t_meas) + y(t_meas)
 *   step_k = ((k + 1) * dt + lead) * s,    lead = delay_x + dt + delay_u
 *
 * The dsafe_obs tables stay the scenario's (or the variant's): they are the
 * controller's knowledge.  LENGTH and WIDTH of a row enter only the realised
 * footprint of the metrics.
 *
 * Bad row: any field non-finite, or LENGTH < 0, or WIDTH < 0.
 *   - predict writes NaN to that obstacle's [2][hp] block, pose to its
 *     [n_ticks + 1][3] block; no other output is touched.
 *   - the metrics leave a realisation with any bad row untouched (accumulator
 *     and dense outputs; after a reset: the reset values), the rule of
 *     scpqp_variants.h for a variant index outside the table.
 *   - the calls return 0: numerical trouble never aborts a batch.
 *
 * Sampler.  scpqp_obstacles_sample draws field f of (b, o) from ONE
 * Philox4x32-10 call (generator, key and the u1 / u2 / Box-Muller mapping of
 * scpqp_noise.h; the kinds and the field description of scpqp_truth.h):
 *
 *   key      (seed & 0xffffffff, seed >> 32)
 *   counter  c0 = f   c1 = 0   c2 = (SCPQP_NOISE_SITE_OBSTACLE << 24) | o
 *            c3 = b_offset + b
 *
 * Site 4 is disjoint from the sites 0..3, so an obstacle seed equal to the
 * noise or the truth seed shares no counter with them.
 *
 *   FIXED    mean[f][o] exactly (spread, lo, hi ignored; no draw)
 *   UNIFORM  xi = 2 u2 - 1
 *   NORMAL   xi = sqrt(-2 ln u1) cos(2 pi u2)
 *   value    fmin(fmax(__dadd_rn(mean, __dmul_rn(spread, xi)), lo), hi)
 *
 * c3 is the global realisation index: a batch sharded over calls or ranks
 * (b_offset = first realisation of the call) samples what one call would.
 *
 * Conventions of scpqp.h: device pointers, asynchronous on `stream`, 0 or a
 * negative SCPQP_E_* code with the message in scpqp_last_error().  Every
 * argument is validated on the host before any HIP call.  B = 0 is a no-op
 * (the arrays may then be NULL).
 */
#ifndef SCPQP_OBSTACLES_H
#define SCPQP_OBSTACLES_H

#include "scpqp_metrics.h"
#include "scpqp_truth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_OBST_NP 7
#define SCPQP_OBST_X 0
#define SCPQP_OBST_Y 1
#define SCPQP_OBST_HEADING 2
#define SCPQP_OBST_SPEED 3
#define SCPQP_OBST_LENGTH 4
#define SCPQP_OBST_WIDTH 5
#define SCPQP_OBST_YAW_RATE 6

#define SCPQP_NOISE_SITE_OBSTACLE 4

typedef struct scpqp_obstacles_dist {
    int32_t  n_obst;     /* 1..SCPQP_MAX_OBST */
    int32_t  pad0;
    double   mean[SCPQP_OBST_NP][SCPQP_MAX_OBST];
    scpqp_truth_field field[SCPQP_OBST_NP];
    uint64_t seed;
    uint32_t b_offset;   /* c3 = b_offset + b */
    uint32_t pad1;
} scpqp_obstacles_dist;

/* The controller's prediction obst_out [B][n_obst][2][hp] (the layout of
 * scpqp_batch_in.obst) from rows [B][n_obst][SCPQP_OBST_NP]; one horizon per call.
 * n_obst in 1..SCPQP_MAX_OBST, hp in 1..SCPQP_MAX_HP; t_meas, lead and dt finite.
 * B * n_obst * 2 * hp must fit int32 (SCPQP_E_SIZE). */
int scpqp_obstacles_predict(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                            double t_meas, double lead, double dt, double* obst_out, void* stream);

/* pose_out [B][n_obst][n_ticks + 1][3]: x, y, heading at the global ticks
 * tick0 .. tick0 + n_ticks (t = tick * tick_length).  tick_length finite and > 0,
 * tick0 >= 0, n_ticks >= 0; the output size must fit int32 (SCPQP_E_SIZE). */
int scpqp_obstacles_pose(int32_t B, int32_t n_obst, const double* rows, double tick_length,
                         int32_t tick0, int32_t n_ticks, double* pose_out, void* stream);

/* rows[b][o] = (obstacles_host[o][0..5], 0) for every b.  obstacles_host is a HOST array
 * [n_obst][6] (x y heading speed length width, as scpqp_metrics_params.obstacles), copied
 * before the call returns; a row that would be bad is refused (SCPQP_E_ARG). */
int scpqp_obstacles_fill_nominal(int32_t n_obst, const double* obstacles_host, int32_t B,
                                 double* rows, void* stream);

/* rows[b][o][f] drawn as described above.  SCPQP_E_ARG (the message names the field)
 * unless: n_obst in 1..SCPQP_MAX_OBST; every kind in range; every spread finite and >= 0;
 * lo <= hi; every mean[f][o], o < n_obst, finite; and, with floor(f, o) = mean[f][o] of a
 * FIXED field and lo otherwise, floor(LENGTH, o) >= 0 and floor(WIDTH, o) >= 0: the
 * sampler never emits a bad row. */
int scpqp_obstacles_sample(const scpqp_obstacles_dist* d, int32_t B, double* rows, void* stream);

/* scpqp_metrics_accumulate_variants with obstacle o of realisation b posed by rows[b][o]
 * at t = (tick0 + k) * tick_length: the rectangle is centred at (x(t), y(t)), rotated by
 * h(t), and its half extents are LENGTH / 2, WIDTH / 2 of the row.  The handle's constant
 * obstacles are not read; gaps, margins against the variant's dsafe_obs, the argmin order
 * and the collision ticks are those of scpqp_metrics.h.  rows [B][n_obst][SCPQP_OBST_NP]
 * (n_obst the handle's, >= 1) must be non-NULL: callers without rows keep the existing
 * entry points.  variant may be NULL (entry 0). */
int scpqp_metrics_accumulate_obstacles(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                                       int32_t k_first, const double* x_path,
                                       const scpqp_metrics_acc* acc,
                                       const scpqp_metrics_dense* dense, const int32_t* variant,
                                       const double* rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_OBSTACLES_H */
