/*
 * scpqp_metrics.h — realised-path metrics of closed-loop rollouts, accumulated
 * on the device step by step (csrc/metrics.hip).
 *
 * The reference draws each vehicle and obstacle as a rectangle Length x Width
 * centred at (x, y) and rotated by the heading (plotOnline.py:91-101, :120-132;
 * draw_video.py:106).  That footprint is what "collision" means here.
 *
 * Per call the kernel reads one MPC step's plant path x_path [B][n_veh][K][6]
 * (K = n_ticks + 1, the layout scpqp_plant_step writes); entry k is global
 * tick tick0 + k.
 *
 * Footprint gap of two rectangles A, B (centre c, heading h, half extents
 * hx = length / 2, hy = width / 2, axes x1 = (cos h, sin h), x2 = (-sin h, cos h)):
 *   separated on axis n  <=>  |n.(cB - cA)| > rA(n) + rB(n),
 *                             rX(n) = hx |n.x1| + hy |n.x2|       (strict: touching overlaps)
 *   n over {a1, a2, b1, b2}.  Separated on no axis: gap = 0.0 exactly (a collision).
 *   Otherwise gap = min over the 4 corners of A of their distance to B and the 4
 *   corners of B of their distance to A; a corner p in the other rectangle's frame
 *   is hypot(max(|px| - hx, 0), max(|py| - hy, 0)) away.  For disjoint convex
 *   polygons this vertex-to-polygon minimum is the exact distance.
 *   A tick is a collision tick when any of its gaps is 0.0.
 * Vehicle pairs (v, w), v < w, are numbered lexicographically.  Obstacle o at
 * global tick g is centred at (t s cos oh + ox, t s sin oh + oy), t = g *
 * tick_length (main.py:68-75), with constant heading oh.
 * Margins: centre distance - dsafe_veh[v][w], centre distance - dsafe_obs[v][o].
 * Cross-track error of vehicle v: min over the segments of its reference polyline
 * of the point-segment distance with the projection parameter clamped to [0, 1],
 * except the lower clamp of the first segment and the upper clamp of the last (the
 * end segments extend as lines: running past the end of the line costs nothing).
 *
 * Accumulator, per realisation, over the entries k_first <= k <= n_ticks (the
 * rollout passes k_first = 0 in step 0 and 1 afterwards: entry 0 of a step is the
 * previous step's last entry):
 *   min_gap_*, min_margin_*      +inf after reset (the _obs fields stay so with n_obst = 0)
 *   argmin_gap_veh [B][3]        (global tick, v, w), -1 after reset.  Among equal gaps
 *   argmin_gap_obs [B][3]        (global tick, v, o)  the lexicographically smallest triple
 *                                wins; across calls only a strictly smaller gap replaces.
 *   first_collision_tick         -1 after reset; the smallest global collision tick
 *   n_collision_ticks, n_ticks_seen
 *   max_xtrack, sum_sq_xtrack [B][n_veh]   0 after reset; the sum adds e*e tick by tick
 *                                in ascending tick order (two roundings per tick)
 * A realisation's results depend on its own path alone: not on B, the launch
 * grid, or how a batch is cut into calls.
 *
 * Conventions of scpqp.h: asynchronous on `stream`, 0 or a negative SCPQP_E_*
 * code with the message in scpqp_last_error().  Every argument is validated
 * before any HIP call.  The handle owns only the device copy of the constants.
 */
#ifndef SCPQP_METRICS_H
#define SCPQP_METRICS_H

#include "scpqp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scpqp_metrics_params {   /* host pointers, copied at create */
    int32_t n_veh;                /* 1..SCPQP_MAX_VEH                       */
    int32_t n_obst;               /* 0..SCPQP_MAX_OBST                      */
    int32_t ref_max_pts;          /* 2..SCPQP_MAX_REFPTS                    */
    int32_t pad0;
    double tick_length;           /* > 0                                    */
    const double* length;         /* [n_veh]                                */
    const double* width;          /* [n_veh]                                */
    const double* dsafe_veh;      /* [n_veh*n_veh]                          */
    const double* dsafe_obs;      /* [n_veh*n_obst] or NULL (n_obst = 0)    */
    const double* obstacles;      /* [n_obst][6] x y heading speed length width, or NULL */
    const double* ref_polyline;   /* [n_veh][ref_max_pts][2]                */
    const int32_t* ref_npts;      /* [n_veh], each in 2..ref_max_pts        */
} scpqp_metrics_params;

typedef struct scpqp_metrics_acc {      /* caller-owned device pointers, none NULL */
    double*  min_gap_veh;           /* [B]        */
    double*  min_gap_obs;           /* [B]        */
    double*  min_margin_veh;        /* [B]        */
    double*  min_margin_obs;        /* [B]        */
    int32_t* argmin_gap_veh;        /* [B][3]     */
    int32_t* argmin_gap_obs;        /* [B][3]     */
    int32_t* first_collision_tick;  /* [B]        */
    int32_t* n_collision_ticks;     /* [B]        */
    int32_t* n_ticks_seen;          /* [B]        */
    double*  max_xtrack;            /* [B][n_veh] */
    double*  sum_sq_xtrack;         /* [B][n_veh] */
} scpqp_metrics_acc;

/* Dense outputs of one call (device pointers, any may be NULL), written for every
 * k in 0..n_ticks regardless of k_first. */
typedef struct scpqp_metrics_dense {
    double* gap_veh;   /* [B][K][n_veh*(n_veh-1)/2] */
    double* gap_obs;   /* [B][K][n_veh][n_obst]     */
    double* xtrack;    /* [B][K][n_veh]             */
} scpqp_metrics_dense;

typedef struct scpqp_metrics scpqp_metrics;

int scpqp_metrics_create(const scpqp_metrics_params* p, int device, scpqp_metrics** out);
int scpqp_metrics_destroy(scpqp_metrics* m);   /* NULL: returns 0 */

/* Set the first B entries of every accumulator array to their reset values. */
int scpqp_metrics_reset(scpqp_metrics* m, int32_t B, const scpqp_metrics_acc* acc, void* stream);

/* Merge the entries k_first..n_ticks of x_path into acc (may be NULL when dense is
 * given) and write the dense outputs asked for.  k_first in {0, 1}, n_ticks >= 0,
 * tick0 >= 0; B * n_veh * (n_ticks + 1) * 6 and every dense size must fit int32
 * (SCPQP_E_SIZE otherwise).  B = 0 is a no-op. */
int scpqp_metrics_accumulate(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                             int32_t k_first, const double* x_path, const scpqp_metrics_acc* acc,
                             const scpqp_metrics_dense* dense, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_METRICS_H */
