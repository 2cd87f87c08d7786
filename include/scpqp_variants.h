/*
 * scpqp_variants.h — scenario variants: several sets of scenario-level
 * parameters in one launch, chosen per problem.
 *
 * A variant is one complete set of the parameters that may differ between the
 * problems of a launch:
 *   solver (scpqp_params):          lf, lr, q, q_final, r, dsafe_veh, dsafe_obs,
 *                                   dsafe_extra, ref_polyline, ref_npts, ref_max_pts
 *   metrics (scpqp_metrics_params): length, width, dsafe_veh, dsafe_obs, obstacles,
 *                                   ref_polyline, ref_npts, ref_max_pts
 * Everything else must equal the handle's and is rejected otherwise (SCPQP_E_ARG,
 * the message names the field): the sizes n_veh, n_obst (and hp_max, which the
 * handle keeps), dt, u_lim, the tolerances, caps and flags of scpqp_params;
 * n_veh, n_obst and tick_length of scpqp_metrics_params.
 *
 * The handle holds a device table of parameter blocks.  After create the table
 * is the one block create built (entry 0).  Problem b of a call uses entry
 * variant[b] (scpqp_batch_in.variant, a device array [B]; NULL: entry 0).
 * An index outside [0, n):
 *   solver   the problem reports SCPQP_ST_INVALID with zero counters and nothing
 *            else of it is written (the rule of a horizon outside its slot);
 *   metrics  the realisation's accumulator entries and dense outputs are left
 *            untouched (after a reset: the reset values).
 *
 * Conventions of scpqp.h.  Every argument is validated on the host before any
 * HIP call.
 */
#ifndef SCPQP_VARIANTS_H
#define SCPQP_VARIANTS_H

#include "scpqp.h"
#include "scpqp_metrics.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Install a table of n >= 1 parameter blocks, replacing the previous table.  Block k
 * is byte for byte what a handle created from params[k] holds.  Synchronises the
 * device before the old table is freed: not asynchronous. */
int scpqp_set_variants(scpqp_handle* h, int32_t n, const scpqp_params* params);

/* The metrics counterpart (same rules; entry k as scpqp_metrics_create builds it). */
int scpqp_metrics_set_variants(scpqp_metrics* m, int32_t n, const scpqp_metrics_params* params);

/* scpqp_metrics_accumulate with realisation b measured against table entry variant[b]
 * (device, [B]; NULL: entry 0). */
int scpqp_metrics_accumulate_variants(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                                      int32_t k_first, const double* x_path,
                                      const scpqp_metrics_acc* acc,
                                      const scpqp_metrics_dense* dense, const int32_t* variant,
                                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_VARIANTS_H */
