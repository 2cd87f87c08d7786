// tracker.hip — obstacle tracker on MI355X (fp64): the per-(realisation, obstacle)
// extended Kalman filter of include/scpqp_tracker.h.
//
//   scpqp_obstacles_track   one tracker step of every lane: the untracked prediction into
//                           obst_out (the existing kernels, for the off lanes), then per
//                           lane measure, predict over t_since, initialise or correct, and
//                           the horizon on the arc of the estimate
//
// One lane per (b, o), 256 threads per workgroup, in the launch shape of estimator.hip.
// The flow is closed-form (pose_at of scpqp_obstacle_pose.h, the obstacle truth's own), so
// a step is one Jacobian, one covariance product, one 4 x 4 Cholesky and hp poses.  P is
// carried in registers (every 5 x 5 and 4 x 4 loop below is fully unrolled with
// compile-time indices, so no per-thread array is indexed at run time), the two products
// F P and (F P) F' touch only F's seven off-diagonal nonzeros, and the update works on the
// 4 x 4 S and the 5 x 4 gain without forming H = [I4 | 0].  No LDS.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_ekf.h"
#include "scpqp_entry_checks.h"
#include "scpqp_obstacle_pose.h"
#include "scpqp_sense_draw.h"
#include "scpqp_tracker.h"

namespace {

constexpr int NS = SCPQP_TRK_NS;
constexpr int NZ = SCPQP_TRK_NZ;
constexpr int NP = SCPQP_TRK_NP;
constexpr int PT = 256;   // threads per workgroup

using scpqp_ekf_dev::correct;
using scpqp_obst_dev::Pose;

// the pose of (x, y, h, s, w) after t on the obstacle truth's own flow
__device__ __forceinline__ Pose flow(double x, double y, double h, double s, double w, double t) {
    const double r[SCPQP_OBST_NP] = {x, y, h, s, 0.0, 0.0, w};
    return scpqp_obst_dev::pose_at(r, t);
}

// the nonzeros of F off the unit diagonal
struct Trans {
    double f02, f03, f04, f12, f13, f14, f24;
};

// include/scpqp_tracker.h, step 1, at the estimate (h, s, w)
__device__ __forceinline__ Trans transition(double h, double s, double w, double T) {
    const double a = 0.5 * w * T, c = s * T;
    const double g = fabs(a) < 1e-4 ? 1.0 - a * a / 6.0 : sin(a) / a;
    const double a2 = a * a;
    const double gp = fabs(a) < SCPQP_TRK_DSINC_SWITCH
                          ? a * (-1.0 / 3.0 + a2 * (1.0 / 30.0 - a2 * (1.0 / 840.0)))
                          : (a * cos(a) - sin(a)) / a2;
    double sa, ca;
    sincos(h + a, &sa, &ca);
    const double hT = 0.5 * T;
    Trans f;
    f.f02 = -c * g * sa;
    f.f03 = T * g * ca;
    f.f04 = c * hT * (gp * ca - g * sa);
    f.f12 = c * g * ca;
    f.f13 = T * g * sa;
    f.f14 = c * hT * (gp * sa + g * ca);
    f.f24 = T;
    return f;
}

// P <- F P F' + T Q on the upper triangle of a symmetric P, mirrored below: the
// symmetrisation (P + P') / 2 of the definition is then the identity
__device__ __forceinline__ void propagate(double (&P)[NS][NS], const Trans& f,
                                          const double (&tq)[NS]) {
    double M[NS][NS];   // F P
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        M[0][c] = P[0][c] + f.f02 * P[2][c] + f.f03 * P[3][c] + f.f04 * P[4][c];
        M[1][c] = P[1][c] + f.f12 * P[2][c] + f.f13 * P[3][c] + f.f14 * P[4][c];
        M[2][c] = P[2][c] + f.f24 * P[4][c];
        M[3][c] = P[3][c];
        M[4][c] = P[4][c];
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        if (r <= 0) P[r][0] = M[r][0] + f.f02 * M[r][2] + f.f03 * M[r][3] + f.f04 * M[r][4];
        if (r <= 1) P[r][1] = M[r][1] + f.f12 * M[r][2] + f.f13 * M[r][3] + f.f14 * M[r][4];
        if (r <= 2) P[r][2] = M[r][2] + f.f24 * M[r][4];
        if (r <= 3) P[r][3] = M[r][3];
        P[r][4] = M[r][4];
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        P[r][r] += tq[r];
#pragma unroll
        for (int c = 0; c < r; ++c) P[r][c] = P[c][r];
    }
}

// one lane per (b, o).  obst_out already holds the untracked prediction of every lane.
__global__ __launch_bounds__(PT) void track_kernel(int n, int nO, int hp,
                                                   const double* __restrict__ rows,
                                                   const double* __restrict__ osense,
                                                   scpqp_sense_stream st,
                                                   const double* __restrict__ trk, double t_meas,
                                                   double T, double lead, double dt,
                                                   double* __restrict__ x_trk,
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
    for (int f = SCPQP_TRK_R_POS; f <= SCPQP_TRK_R_SPEED; ++f) r_zero |= row[f] == 0.0;
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
                                   T * (row[6] * row[6])};
            // F is taken at the estimate the flow starts from
            propagate(P, transition(x[2], x[3], x[4], T), tq);
            const Pose p = flow(x[0], x[1], x[2], x[3], x[4], T);
            x[0] = p.x;
            x[1] = p.y;
            x[2] = p.h;
            ok = correct(x, P, zm, r2, nis);
            ok = ok && isfinite(nis);
        } else {
#pragma unroll
            for (int i = 0; i < NZ; ++i) x[i] = zm[i];
            x[4] = 0.0;
#pragma unroll
            for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
                for (int c = 0; c < NS; ++c) P[rr][c] = 0.0;
            }
#pragma unroll
            for (int i = 0; i < NZ; ++i) P[i][i] = r2[i];
            P[4][4] = row[SCPQP_TRK_P0_YAW] * row[SCPQP_TRK_P0_YAW];
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
    // the horizon on the arc of the estimate
    const double wc = fmin(fmax(x[4], -row[SCPQP_TRK_W_CLAMP]), row[SCPQP_TRK_W_CLAMP]);
    for (int k = 0; k < hp; ++k) {
        const Pose p = flow(x[0], x[1], x[2], x[3], wc, (double)(k + 1) * dt + lead);
        o[k] = p.x;
        o[hp + k] = p.y;
    }
}

}  // namespace

extern "C" {

int scpqp_obstacles_track(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                          const double* osense, const scpqp_sense_stream* st, const double* trk,
                          double t_meas, double t_since, double lead, double dt,
                          double* x_trk, double* cov, double* z_out, double* nis,
                          double* obst_out, void* stream) {
    if (int rc = scpqp_host::track_begin(B, n_obst, hp, 1, NS * NS, "B * n_obst * 25 too large",
                                         rows, osense, st, trk,
                                         {{x_trk, "null x_trk array"}, {cov, "null cov array"}},
                                         t_meas, t_since, lead, dt, obst_out, stream))
        return rc < 0 ? rc : 0;
    const long long n = (long long)B * n_obst;
    const scpqp_sense_stream none = {0, 0, 0};
    hipLaunchKernelGGL(track_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, n_obst, hp, rows, osense,
                       osense ? *st : none, trk, t_meas, t_since, lead, dt, x_trk, cov, z_out, nis,
                       obst_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
