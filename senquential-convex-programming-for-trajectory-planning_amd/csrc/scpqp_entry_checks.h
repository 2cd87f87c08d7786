// scpqp_entry_checks.h — host side: the argument checks that several C-ABI entry points share,
// in the order and with the texts their headers under include/ promise.  Each returns the code
// of scpqp_fail_ (< 0), 0 to go on, or SCPQP_NOTHING_TO_DO (> 0) for an empty batch, which the
// entry point turns into 0.
#ifndef SCPQP_ENTRY_CHECKS_H
#define SCPQP_ENTRY_CHECKS_H

#include <initializer_list>
#include <math.h>

#include "scpqp_imm.h"
#include "scpqp_yield.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace scpqp_host {

constexpr int SCPQP_NOTHING_TO_DO = 1;

struct Required {
    const void* p;
    const char* null_msg;
};

static inline int check_stream(const scpqp_sense_stream* st) {
    if (!st) return scpqp_fail_(SCPQP_E_ARG, "null sensing stream");
    return 0;
}

// scpqp_governor_step and scpqp_yield_step: everything before the launch.  np: the doubles of
// a row; rows_null_msg: the text for a null rows array.
static inline int conflict_step_checks(int32_t n_veh, int32_t n_obst, int32_t hp_max, int32_t B,
                                       double t_hold, double t_back, const double* x0,
                                       const double* traj, const double* obst,
                                       const double* dreq_obs, const double* dreq_veh,
                                       const double* rows, int np, const char* rows_null_msg,
                                       const double* a_cmd) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_veh < 1 || n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    if (n_obst < 0 || n_obst > SCPQP_MAX_OBST) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    if (hp_max < 1 || hp_max > SCPQP_MAX_HP) return scpqp_fail_(SCPQP_E_ARG, "hp_max out of range");
    if (!isfinite(t_hold) || !(t_hold > 0.0))
        return scpqp_fail_(SCPQP_E_ARG, "t_hold must be finite and > 0");
    if (!isfinite(t_back) || !(t_back >= 0.0))
        return scpqp_fail_(SCPQP_E_ARG, "t_back must be finite and >= 0");
    const long long n = (long long)B * n_veh;
    if (2 * n * hp_max > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * 2 * hp_max too large");
    if (2LL * B * n_obst * hp_max > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 2 * hp_max too large");
    const int widest = n_veh > n_obst ? (n_veh > np ? n_veh : np) : (n_obst > np ? n_obst : np);
    if (n * widest > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * row width too large");
    if (B == 0) return SCPQP_NOTHING_TO_DO;
    if (!x0) return scpqp_fail_(SCPQP_E_ARG, "null x0 array");
    if (!traj) return scpqp_fail_(SCPQP_E_ARG, "null traj array");
    if (!obst && n_obst > 0) return scpqp_fail_(SCPQP_E_ARG, "null obst array with n_obst > 0");
    if (!dreq_obs && n_obst > 0) return scpqp_fail_(SCPQP_E_ARG, "null dreq_obs array with n_obst > 0");
    if (!dreq_veh) return scpqp_fail_(SCPQP_E_ARG, "null dreq_veh array");
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, rows_null_msg);
    if (!a_cmd) return scpqp_fail_(SCPQP_E_ARG, "null a_cmd array");
    return 0;
}

// scpqp_obstacles_track, _track_accel and _track_imm: everything before the tracker's own
// launch.  n_modes: 1 for the single filters; per_lane: the doubles of covariance per (b, o),
// size_msg the text when they overflow; state: the tracker's own arrays, checked in order
// between trk and obst_out.  Then every block as the untracked controller predicts it: the
// lanes with a tracker overwrite theirs afterwards, in stream order, so an off row takes the
// code path of scpqp_obstacles_predict(_sensed) itself, bitwise, whatever the compiler makes
// of either kernel.
static inline int track_begin(int32_t B, int32_t n_obst, int32_t hp, int32_t n_modes,
                              long long per_lane, const char* size_msg, const double* rows,
                              const double* osense, const scpqp_sense_stream* st,
                              const double* trk, std::initializer_list<Required> state,
                              double t_meas, double t_since, double lead, double dt,
                              double* obst_out, void* stream) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_obst < 1 || n_obst > SCPQP_MAX_OBST) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    if (hp < 1 || hp > SCPQP_MAX_HP) return scpqp_fail_(SCPQP_E_ARG, "hp out of range");
    if (n_modes < 1 || n_modes > SCPQP_IMM_MAX_MODES)
        return scpqp_fail_(SCPQP_E_ARG, "n_modes out of range");
    if (!isfinite(t_meas) || !isfinite(lead) || !isfinite(dt))
        return scpqp_fail_(SCPQP_E_ARG, "t_meas, lead and dt must be finite");
    if (!(t_since >= 0.0) || !isfinite(t_since))
        return scpqp_fail_(SCPQP_E_ARG, "t_since must be finite and >= 0");
    const long long n = (long long)B * n_obst;
    if (n * per_lane > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, size_msg);
    if (2 * n * hp > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 2 * hp too large");
    if (B == 0) return SCPQP_NOTHING_TO_DO;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (osense)
        if (int rc = check_stream(st)) return rc;
    if (!trk) return scpqp_fail_(SCPQP_E_ARG, "null trk rows array");
    for (const Required& a : state)
        if (!a.p) return scpqp_fail_(SCPQP_E_ARG, a.null_msg);
    if (!obst_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    if (osense)
        return scpqp_obstacles_predict_sensed(B, n_obst, hp, rows, osense, st, t_meas, lead, dt,
                                              obst_out, stream);
    return scpqp_obstacles_predict(B, n_obst, hp, rows, t_meas, lead, dt, obst_out, stream);
}

}  // namespace scpqp_host

#endif  // SCPQP_ENTRY_CHECKS_H
