// estimator.hip — state estimator on MI355X (fp64): the per-(realisation, vehicle)
// extended Kalman filter of include/scpqp_estimator.h.
//
//   scpqp_est_step   one filter step of every lane: predict over the ticks since the
//                    previous step with the commands that acted, then initialise on or
//                    correct with this step's measurement
//
// One lane per (b, v), 256 threads per workgroup, in the launch shape of plant.hip.  The
// prediction is the one long dependent chain the filter adds to a rollout step: per tick
// steps_for(tick, h_max) RK4 steps of the nominal vehicle (scpqp_bicycle.h: plant.hip's
// own integrator) and one covariance product.  P is carried as its upper triangle in
// registers (every 5 x 5 loop below is fully unrolled with compile-time indices, so no
// per-thread array is indexed at run time), F = I + T A + T^2/2 A A is formed from the
// nine nonzeros of A in closed form, and the two products F P and (F P) F' touch only
// F's nonzeros.  No LDS.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_bicycle.h"
#include "scpqp_ekf.h"
#include "scpqp_estimator.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

using namespace scpqp_plant_dev;   // NX, Veh, flow, steps_for
using scpqp_ekf_dev::correct;      // with every state measured: H = I

constexpr int NS = SCPQP_EST_NS;
constexpr int NP = SCPQP_EST_NP;
constexpr int PT = 256;   // threads per workgroup

// the nonzeros of F = I + T A + T^2/2 A A off the unit diagonal (F33 = 1, F44 = f44)
struct Trans {
    double f02, f03, f04, f12, f13, f14, f23, f24, f44;
};

// Model.py:46-52 at x, restricted to (x, y, heading, speed, steering angle)
__device__ __forceinline__ Trans transition(const double (&x)[NX], double lf, double lr, double T) {
    const double L = lf + lr, rho = lr / L;
    const double v = x[3];
    const double t = tan(x[5]);
    const double sec2 = t * t + 1.0;
    const double kap = sqrt(rho * rho * t * t + 1.0);
    const double th = x[2] + atan(rho * t);
    const double sth = sin(th), cth = cos(th);
    const double a02 = -v * sth * kap, a03 = cth * kap;
    const double a04 = rho * rho * v * cth * t * sec2 / kap - rho * v * sth * sec2 / kap;
    const double a12 = v * cth * kap, a13 = sth * kap;
    const double a14 = rho * v * cth * sec2 / kap + rho * rho * v * sth * t * sec2 / kap;
    const double a23 = t / L, a24 = v * sec2 / L, a44 = -10.0;
    // A A: row 0 = a02 row 2 + a04 row 4, row 1 likewise, row 2 = a24 row 4, row 4 = a44 row 4
    const double h2 = 0.5 * T * T;
    Trans f;
    f.f02 = T * a02;
    f.f03 = T * a03 + h2 * (a02 * a23);
    f.f04 = T * a04 + h2 * (a02 * a24 + a04 * a44);
    f.f12 = T * a12;
    f.f13 = T * a13 + h2 * (a12 * a23);
    f.f14 = T * a14 + h2 * (a12 * a24 + a14 * a44);
    f.f23 = T * a23;
    f.f24 = T * a24 + h2 * (a24 * a44);
    f.f44 = 1.0 + T * a44 + h2 * (a44 * a44);
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
        M[2][c] = P[2][c] + f.f23 * P[3][c] + f.f24 * P[4][c];
        M[3][c] = P[3][c];
        M[4][c] = f.f44 * P[4][c];
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        if (r <= 0) P[r][0] = M[r][0] + f.f02 * M[r][2] + f.f03 * M[r][3] + f.f04 * M[r][4];
        if (r <= 1) P[r][1] = M[r][1] + f.f12 * M[r][2] + f.f13 * M[r][3] + f.f14 * M[r][4];
        if (r <= 2) P[r][2] = M[r][2] + f.f23 * M[r][3] + f.f24 * M[r][4];
        if (r <= 3) P[r][3] = M[r][3];
        P[r][4] = f.f44 * M[r][4];
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        P[r][r] += tq[r];
#pragma unroll
        for (int c = 0; c < r; ++c) P[r][c] = P[c][r];
    }
}

// one lane per (b, v)
__global__ __launch_bounds__(PT) void est_kernel(scpqp_plant_params p, int n, int n_span,
                                                 double tick, double hmax,
                                                 const double* __restrict__ u_span,
                                                 const double* __restrict__ x_meas,
                                                 const int32_t* __restrict__ delivered,
                                                 const double* __restrict__ est,
                                                 double* __restrict__ x_est,
                                                 double* __restrict__ cov,
                                                 double* __restrict__ nis_out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const int v = g % p.n_veh;
    double row[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) row[f] = est[(size_t)g * NP + f];
    double* xe = x_est + (size_t)g * NX;
    double* pc = cov + (size_t)g * NS * NS;

    bool bad = false, off = true, r_zero = false;
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        bad |= !isfinite(row[f]) || row[f] < 0.0;
        off &= row[f] == 0.0;
    }
#pragma unroll
    for (int f = SCPQP_EST_R_POS; f <= SCPQP_EST_R_STEER; ++f) r_zero |= row[f] == 0.0;
    bad |= !off && r_zero;
    if (!bad && off) {
        // no filter: the measurement, bit for bit
#pragma unroll
        for (int i = 0; i < NX; ++i) xe[i] = x_meas[(size_t)g * NX + i];
        if (nis_out) nis_out[g] = NAN;
        return;
    }

    // states (0, 1, 2, 3, 5) of the model are the filter's 0..4
    const double tq[NS] = {tick * (row[4] * row[4]), tick * (row[4] * row[4]),
                           tick * (row[5] * row[5]), tick * (row[6] * row[6]),
                           tick * (row[7] * row[7])};
    double x[NX], P[NS][NS];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = xe[i];
    const bool init = x[0] == x[0];
    bool ok = !bad;
    double nis = NAN;
    if (ok && init) {
#pragma unroll
        for (int r = 0; r < NS; ++r) {
#pragma unroll
            for (int c = r; c < NS; ++c) P[r][c] = P[c][r] = pc[r * NS + c];
        }
        Veh q{p.lf[v], p.lr[v], 0.0, 0.0, 0.0};
        Stream ns{};
        const int nrk = steps_for(tick, hmax);
        for (int j = 0; j < n_span; ++j) {
            q.uref = u_span[(size_t)g * n_span + j];
            // F is taken at the estimate the tick starts from, so P goes first and
            // nothing of F lives across the integration
            propagate(P, transition(x, q.lf, q.lr, tick), tq);
            flow<false>(x, q, tick, nrk, ns);
        }
    }
    // the measurement and R are first needed here: they hold no register over the loop
    double m[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) m[i] = x_meas[(size_t)g * NX + i];
    const double r2[NS] = {row[0] * row[0], row[0] * row[0], row[1] * row[1], row[2] * row[2],
                           row[3] * row[3]};
    bool counts = !delivered || delivered[g] == 1;
#pragma unroll
    for (int i = 0; i < NX; ++i) counts &= isfinite(m[i]);
    if (ok && counts) {
        if (!init) {
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = m[i];
#pragma unroll
            for (int r = 0; r < NS; ++r) {
#pragma unroll
                for (int c = 0; c < NS; ++c) P[r][c] = r == c ? r2[r] : 0.0;
            }
        } else {
            double xs[NS] = {x[0], x[1], x[2], x[3], x[5]};
            const double ms[NS] = {m[0], m[1], m[2], m[3], m[5]};
            ok = correct(xs, P, ms, r2, nis);
            x[0] = xs[0];
            x[1] = xs[1];
            x[2] = xs[2];
            x[3] = xs[3];
            x[4] = m[4];
            x[5] = xs[4];
            ok = ok && isfinite(nis);
        }
    }
    if (ok && !init && !counts) {
        // neither initialised nor measured: stays NaN
#pragma unroll
        for (int i = 0; i < NX; ++i) xe[i] = NAN;
        if (nis_out) nis_out[g] = NAN;
        return;
    }
    if (ok) {
#pragma unroll
        for (int i = 0; i < NX; ++i) ok &= isfinite(x[i]);
#pragma unroll
        for (int r = 0; r < NS; ++r) {
#pragma unroll
            for (int c = r; c < NS; ++c) ok &= isfinite(P[r][c]);
        }
    }
    if (!ok) {
        // a bad row or trouble: the lane starts again on its next measurement
#pragma unroll
        for (int i = 0; i < NX; ++i) xe[i] = NAN;
#pragma unroll
        for (int k = 0; k < NS * NS; ++k) pc[k] = NAN;
        if (nis_out) nis_out[g] = NAN;
        return;
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) xe[i] = x[i];
#pragma unroll
    for (int r = 0; r < NS; ++r) {
#pragma unroll
        for (int c = 0; c < NS; ++c) pc[r * NS + c] = P[r][c];
    }
    if (nis_out) nis_out[g] = nis;
}

}  // namespace

extern "C" {

int scpqp_est_step(const scpqp_plant_params* p, int32_t B, int32_t n_span, double tick,
                   double h_max, const double* u_span, const double* x_meas,
                   const int32_t* delivered, const double* est, double* x_est, double* cov,
                   double* nis, void* stream) {
    if (!p) return scpqp_fail_(SCPQP_E_ARG, "null plant params");
    if (p->n_veh < 1 || p->n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    for (int v = 0; v < p->n_veh; ++v)
        if (!(p->lf[v] + p->lr[v] > 0.0)) return scpqp_fail_(SCPQP_E_ARG, "lf + lr must be > 0");
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_span < 0) return scpqp_fail_(SCPQP_E_ARG, "n_span < 0");
    if (!(tick > 0.0) || !isfinite(tick)) return scpqp_fail_(SCPQP_E_ARG, "tick must be finite and > 0");
    if (!(h_max > 0.0) || !isfinite(h_max)) return scpqp_fail_(SCPQP_E_ARG, "h_max must be finite and > 0");
    const long long n = (long long)B * p->n_veh;
    if (n * NS * NS > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * 25 too large");
    if (n * n_span > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * n_span too large");
    if (B == 0) return 0;
    if (n_span > 0 && !u_span) return scpqp_fail_(SCPQP_E_ARG, "null u_span array");
    if (!x_meas) return scpqp_fail_(SCPQP_E_ARG, "null x_meas array");
    if (!est) return scpqp_fail_(SCPQP_E_ARG, "null est rows array");
    if (!x_est) return scpqp_fail_(SCPQP_E_ARG, "null x_est array");
    if (!cov) return scpqp_fail_(SCPQP_E_ARG, "null cov array");
    hipLaunchKernelGGL(est_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *p, (int)n, n_span, tick, h_max, u_span,
                       x_meas, delivered, est, x_est, cov, nis);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
