// scpqp_ekf.h — the filter steps the rollout kernels share (device side).
//
//   scpqp_ekf_dev    the Cholesky-based measurement update on H = [I_NZ | 0], for
//                    estimator.hip, tracker.hip, tracker_accel.hip and imm.hip
//   scpqp_trka_dev   the six-state transition and covariance product of
//                    include/scpqp_tracker_accel.h, for tracker_accel.hip and imm.hip
//
// Every loop is fully unrolled with compile-time indices, so x and P stay in registers.  No
// function here exchanges between lanes (the rule at the top of imm.hip); the only early
// return is the bad pivot of `correct`, as before it moved here.
#ifndef SCPQP_EKF_H
#define SCPQP_EKF_H

#include <hip/hip_runtime.h>

#include <math.h>

#include "scpqp_manoeuvre_pose.h"
#include "scpqp_tracker_accel.h"

namespace scpqp_ekf_dev {

// the measurement update with H = [I_NZ | 0] on a symmetric P; false on a bad pivot.  LD:
// *logdet receives sum_k log L_kk.
template <bool LD = false, int NS, int NZ>
__device__ __forceinline__ bool correct(double (&x)[NS], double (&P)[NS][NS],
                                        const double (&zm)[NZ], const double (&r2)[NZ],
                                        double& nis, double* logdet = nullptr) {
    double Lc[NZ][NZ], inv[NZ];
    bool ok = true;
    // S = P[0:NZ, 0:NZ] + R = L L'
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
        double d = P[j][j] + r2[j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= Lc[j][k] * Lc[j][k];
        ok &= d > 0.0 && isfinite(d);
        Lc[j][j] = sqrt(d);
        inv[j] = 1.0 / Lc[j][j];
#pragma unroll
        for (int i = j + 1; i < NZ; ++i) {
            double s = P[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= Lc[i][k] * Lc[j][k];
            Lc[i][j] = s * inv[j];
        }
    }
    if (!ok) return false;
    if constexpr (LD) {
        *logdet = 0.0;
#pragma unroll
        for (int j = 0; j < NZ; ++j) *logdet += log(Lc[j][j]);
    }
    // v = L^-1 y, nis = v' v, w = L'^-1 v = S^-1 y
    double v[NZ], w[NZ];
    nis = 0.0;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        double s = zm[i] - x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= Lc[i][k] * v[k];
        v[i] = s * inv[i];
        nis += v[i] * v[i];
    }
#pragma unroll
    for (int i = NZ - 1; i >= 0; --i) {
        double s = v[i];
#pragma unroll
        for (int k = i + 1; k < NZ; ++k) s -= Lc[k][i] * w[k];
        w[i] = s * inv[i];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < NZ; ++k) s += P[i][k] * w[k];
        x[i] = s;
    }
    // W = L^-1 P[0:NZ, :], P <- P - W' W = P - P[:, 0:NZ] S^-1 P[0:NZ, :]
    double W[NZ][NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
#pragma unroll
        for (int i = 0; i < NZ; ++i) {
            double s = P[i][c];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= Lc[i][k] * W[k][c];
            W[i][c] = s * inv[i];
        }
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
#pragma unroll
        for (int c = r; c < NS; ++c) {
            double s = P[r][c];
#pragma unroll
            for (int k = 0; k < NZ; ++k) s -= W[k][r] * W[k][c];
            P[r][c] = s;
        }
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
#pragma unroll
        for (int c = 0; c < r; ++c) P[r][c] = P[c][r];
    }
    return true;
}

}  // namespace scpqp_ekf_dev

namespace scpqp_trka_dev {

constexpr int NS = SCPQP_TRKA_NS;
constexpr int NZ = SCPQP_TRKA_NZ;
constexpr int NP = SCPQP_TRKA_NP;

using scpqp_man_dev::State;

// p'(theta) and r'(theta) of include/scpqp_tracker_accel.h
__device__ __forceinline__ void dpr_of(double th, double& dp, double& dr) {
    const double t2 = th * th;
    if (fabs(th) < SCPQP_TRKA_DPR_SWITCH) {
        dp = -th * (1.0 / 4.0 - t2 * (1.0 / 36.0 - t2 * (1.0 / 960.0 - t2 * (1.0 / 50400.0 -
             t2 * (1.0 / 4354560.0 - t2 * (1.0 / 558835200.0))))));
        dr = 1.0 / 3.0 - t2 * (1.0 / 10.0 - t2 * (1.0 / 168.0 - t2 * (1.0 / 6480.0 -
             t2 * (1.0 / 443520.0 - t2 * (1.0 / 47174400.0)))));
        return;
    }
    double sn, cs;
    sincos(th, &sn, &cs);
    const double t3 = t2 * th;
    dp = (t2 * cs - 2.0 * th * sn - 2.0 * cs + 2.0) / t3;
    dr = ((t2 - 2.0) * sn + 2.0 * th * cs) / t3;
}

// the nonzeros of F off the unit diagonal
struct Trans {
    double f02, f03, f04, f05, f12, f13, f14, f15, f24, f35;
};

// include/scpqp_tracker_accel.h, step 1, at the estimate (h, s0, w, a) over T
__device__ __forceinline__ Trans transition(double h, double s0, double w, double a, double T) {
    const double stop = a < 0.0 ? s0 / -a : (a == 0.0 && s0 == 0.0 ? 0.0 : INFINITY);
    const double Te = T >= stop ? stop : T;
    const double th = w * Te, A = 0.5 * th, c = s0 * Te;
    const double g = fabs(A) < 1e-4 ? 1.0 - A * A / 6.0 : sin(A) / A;
    const double A2 = A * A;
    const double gp = fabs(A) < SCPQP_TRK_DSINC_SWITCH
                          ? A * (-1.0 / 3.0 + A2 * (1.0 / 30.0 - A2 * (1.0 / 840.0)))
                          : (A * cos(A) - sin(A)) / A2;
    double sa, ca, sh, ch, dp, dr;
    sincos(h + A, &sa, &ca);
    sincos(h, &sh, &ch);
    const double p = scpqp_man_dev::p_of(th), r = scpqp_man_dev::r_of(th);
    dpr_of(th, dp, dr);
    const double hT = 0.5 * Te, Te2 = Te * Te, aT3 = a * (Te2 * Te);
    Trans f;
    f.f03 = Te * g * ca;
    f.f13 = Te * g * sa;
    f.f05 = Te2 * (p * ch - r * sh);
    f.f15 = Te2 * (p * sh + r * ch);
    f.f02 = -(c * g * sa + a * f.f15);
    f.f12 = c * g * ca + a * f.f05;
    f.f04 = c * hT * (gp * ca - g * sa) + aT3 * (dp * ch - dr * sh);
    f.f14 = c * hT * (gp * sa + g * ca) + aT3 * (dp * sh + dr * ch);
    f.f24 = Te;
    f.f35 = Te;
    return f;
}

// P <- F P F' + T Q on the upper triangle of a symmetric P, mirrored below: the
// symmetrisation (P + P') / 2 of the definition is then the identity
__device__ __forceinline__ void propagate(double (&P)[NS][NS], const Trans& f,
                                          const double (&tq)[NS]) {
    double M[NS][NS];   // F P
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        M[0][c] = P[0][c] + f.f02 * P[2][c] + f.f03 * P[3][c] + f.f04 * P[4][c] + f.f05 * P[5][c];
        M[1][c] = P[1][c] + f.f12 * P[2][c] + f.f13 * P[3][c] + f.f14 * P[4][c] + f.f15 * P[5][c];
        M[2][c] = P[2][c] + f.f24 * P[4][c];
        M[3][c] = P[3][c] + f.f35 * P[5][c];
        M[4][c] = P[4][c];
        M[5][c] = P[5][c];
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        if (r <= 0)
            P[r][0] = M[r][0] + f.f02 * M[r][2] + f.f03 * M[r][3] + f.f04 * M[r][4] + f.f05 * M[r][5];
        if (r <= 1)
            P[r][1] = M[r][1] + f.f12 * M[r][2] + f.f13 * M[r][3] + f.f14 * M[r][4] + f.f15 * M[r][5];
        if (r <= 2) P[r][2] = M[r][2] + f.f24 * M[r][4];
        if (r <= 3) P[r][3] = M[r][3] + f.f35 * M[r][5];
        if (r <= 4) P[r][4] = M[r][4];
        P[r][5] = M[r][5];
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        P[r][r] += tq[r];
#pragma unroll
        for (int c = 0; c < r; ++c) P[r][c] = P[c][r];
    }
}

}  // namespace scpqp_trka_dev

#endif  // SCPQP_EKF_H
