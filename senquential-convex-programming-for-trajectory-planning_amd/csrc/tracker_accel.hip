// tracker_accel.hip — obstacle tracker with an acceleration state on MI355X (fp64): the
// per-(realisation, obstacle) six-state extended Kalman filter of
// include/scpqp_tracker_accel.h.
//
//   scpqp_obstacles_track_accel   one tracker step of every lane: the untracked prediction
//                                 into obst_out (the existing kernels, for the off lanes),
//                                 then per lane measure, predict over t_since on one
//                                 manoeuvre piece, initialise or correct, and the horizon in
//                                 up to three pieces
//
// One lane per (b, o), 256 threads per workgroup, in the launch shape of tracker.hip.  The
// flow is closed-form (advance of scpqp_manoeuvre_pose.h, the manoeuvring truth's own), so a
// step is one Jacobian, one covariance product, one 4 x 4 Cholesky, two boundary states and
// hp pieces.  P is carried in registers (every 6 x 6 and 4 x 4 loop below is fully unrolled
// with compile-time indices, so no per-thread array is indexed at run time), the two products
// F P and (F P) F' touch only F's twelve off-diagonal nonzeros, and the update works on the
// 4 x 4 S and the 6 x 4 gain without forming H = [I4 | 0].  The horizon keeps its three
// start states in scalars and selects among them.  No LDS.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_ekf.h"
#include "scpqp_entry_checks.h"
#include "scpqp_sense_draw.h"
#include "scpqp_tracker_accel.h"

namespace {

using namespace scpqp_trka_dev;   // scpqp_ekf.h: NS, NZ, NP, State, transition, propagate
using scpqp_ekf_dev::correct;

constexpr int PT = 256;   // threads per workgroup

// one lane per (b, o).  obst_out already holds the untracked prediction of every lane.
__global__ __launch_bounds__(PT) void track_accel_kernel(int n, int nO, int hp,
                                                         const double* __restrict__ rows,
                                                         const double* __restrict__ osense,
                                                         scpqp_sense_stream st,
                                                         const double* __restrict__ trk,
                                                         double t_meas, double T, double lead,
                                                         double dt, double* __restrict__ x_trk,
                                                         double* __restrict__ cov,
                                                         double* __restrict__ z_out,
                                                         double* __restrict__ nis_out,
                                                         double* __restrict__ out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const int b = g / nO, ob = g - b * nO;
    const double* r = rows + (size_t)g * SCPQP_OBST_NP;
    double* xt = x_trk + (size_t)g * NS;
    double* pc = cov + (size_t)g * NS * NS;
    double* o = out + (size_t)g * 2 * hp;
    double row[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) row[f] = trk[(size_t)g * NP + f];

    bool bad = false, off = true, r_zero = false;
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        bad |= !isfinite(row[f]) || row[f] < 0.0;
        off &= row[f] == 0.0;
    }
#pragma unroll
    for (int f = SCPQP_TRKA_R_POS; f <= SCPQP_TRKA_R_SPEED; ++f) r_zero |= row[f] == 0.0;
    bad |= !off && r_zero;
    off = off && !bad;

    double zm[NZ] = {NAN, NAN, NAN, NAN};
    const bool bad_meas = scpqp_sense_dev::measure_obstacle(r, osense, g, st, b, ob, t_meas, zm);
    if (z_out) {
#pragma unroll
        for (int i = 0; i < NZ; ++i) z_out[(size_t)g * NZ + i] = zm[i];
    }
    if (off) {
        // no filter: the block the untracked prediction wrote before this launch stays
        if (nis_out) nis_out[g] = NAN;
        return;
    }

    double x[NS], P[NS][NS];
    bool ok = !bad && !bad_meas;
    double nis = NAN;
    if (ok) {
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = xt[i];
        const bool init = x[0] == x[0];
        const double r2[NZ] = {row[0] * row[0], row[0] * row[0], row[1] * row[1], row[2] * row[2]};
        if (init) {
#pragma unroll
            for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
                for (int c = rr; c < NS; ++c) P[rr][c] = P[c][rr] = pc[rr * NS + c];
            }
            const double tq[NS] = {T * (row[3] * row[3]), T * (row[3] * row[3]),
                                   T * (row[4] * row[4]), T * (row[5] * row[5]),
                                   T * (row[6] * row[6]), T * (row[7] * row[7])};
            // F is taken at the estimate the flow starts from
            const double s0 = fmax(x[3], 0.0);
            propagate(P, transition(x[2], s0, x[4], x[5], T), tq);
            State q{x[0], x[1], x[2], s0, x[4]};
            scpqp_man_dev::advance(q, x[5], x[4], T);
            x[0] = q.x;
            x[1] = q.y;
            x[2] = q.h;
            x[3] = q.s;
            ok = correct(x, P, zm, r2, nis);
            ok = ok && isfinite(nis);
        } else {
#pragma unroll
            for (int i = 0; i < NZ; ++i) x[i] = zm[i];
            x[4] = 0.0;
            x[5] = 0.0;
#pragma unroll
            for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
                for (int c = 0; c < NS; ++c) P[rr][c] = 0.0;
            }
#pragma unroll
            for (int i = 0; i < NZ; ++i) P[i][i] = r2[i];
            P[4][4] = row[SCPQP_TRKA_P0_YAW] * row[SCPQP_TRKA_P0_YAW];
            P[5][5] = row[SCPQP_TRKA_P0_ACCEL] * row[SCPQP_TRKA_P0_ACCEL];
        }
    }
    if (ok) {
#pragma unroll
        for (int i = 0; i < NS; ++i) ok &= isfinite(x[i]);
#pragma unroll
        for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
            for (int c = rr; c < NS; ++c) ok &= isfinite(P[rr][c]);
        }
    }
    if (!ok) {
        // a bad row or trouble: the lane starts again on the next call
#pragma unroll
        for (int i = 0; i < NS; ++i) xt[i] = NAN;
#pragma unroll
        for (int k = 0; k < NS * NS; ++k) pc[k] = NAN;
        if (nis_out) nis_out[g] = NAN;
        for (int k = 0; k < 2 * hp; ++k) o[k] = NAN;
        return;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) xt[i] = x[i];
#pragma unroll
    for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
        for (int c = 0; c < NS; ++c) pc[rr * NS + c] = P[rr][c];
    }
    if (nis_out) nis_out[g] = nis;

    // the horizon in up to three pieces: the start states q0, q1, q2 once per lane
    const double wc = fmin(fmax(x[4], -row[SCPQP_TRKA_W_CLAMP]), row[SCPQP_TRKA_W_CLAMP]);
    const double ac = fmin(fmax(x[5], -row[SCPQP_TRKA_A_CLAMP]), row[SCPQP_TRKA_A_CLAMP]);
    const double wh = row[SCPQP_TRKA_W_HOLD], ah = row[SCPQP_TRKA_A_HOLD];
    const double t1 = fmin(wh, ah), t2 = fmax(wh, ah);
    const double a2 = ah > wh ? ac : 0.0, w2 = ah > wh ? 0.0 : wc;
    const State q0{x[0], x[1], x[2], fmax(x[3], 0.0), wc};
    State q1 = q0;
    scpqp_man_dev::advance(q1, ac, wc, t1);
    State q2 = q1;
    scpqp_man_dev::advance(q2, a2, w2, t2 - t1);
    for (int k = 0; k < hp; ++k) {
        const double tau = (double)(k + 1) * dt + lead;
        const bool in1 = tau < t1, in2 = tau < t2;
        State q;
        q.x = in1 ? q0.x : (in2 ? q1.x : q2.x);
        q.y = in1 ? q0.y : (in2 ? q1.y : q2.y);
        q.h = in1 ? q0.h : (in2 ? q1.h : q2.h);
        q.s = in1 ? q0.s : (in2 ? q1.s : q2.s);
        q.w = 0.0;
        scpqp_man_dev::advance(q, in1 ? ac : (in2 ? a2 : 0.0), in1 ? wc : (in2 ? w2 : 0.0),
                               in1 ? tau : (in2 ? tau - t1 : tau - t2));
        o[k] = q.x;
        o[hp + k] = q.y;
    }
}

}  // namespace

extern "C" {

int scpqp_obstacles_track_accel(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                                const double* osense, const scpqp_sense_stream* st,
                                const double* trk, double t_meas, double t_since, double lead,
                                double dt, double* x_trk, double* cov, double* z_out,
                                double* nis, double* obst_out, void* stream) {
    if (int rc = scpqp_host::track_begin(B, n_obst, hp, 1, NS * NS, "B * n_obst * 36 too large",
                                         rows, osense, st, trk,
                                         {{x_trk, "null x_trk array"}, {cov, "null cov array"}},
                                         t_meas, t_since, lead, dt, obst_out, stream))
        return rc < 0 ? rc : 0;
    const long long n = (long long)B * n_obst;
    const scpqp_sense_stream none = {0, 0, 0};
    hipLaunchKernelGGL(track_accel_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, n_obst, hp, rows, osense,
                       osense ? *st : none, trk, t_meas, t_since, lead, dt, x_trk, cov, z_out, nis,
                       obst_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
