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

#include "scpqp_manoeuvre_pose.h"
#include "scpqp_obstacle_pose.h"
#include "scpqp_philox.h"
#include "scpqp_tracker_accel.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

constexpr int NS = SCPQP_TRKA_NS;
constexpr int NZ = SCPQP_TRKA_NZ;
constexpr int NP = SCPQP_TRKA_NP;
constexpr int ONP = SCPQP_OSENSE_NP;
constexpr int PT = 256;   // threads per workgroup

using scpqp_man_dev::State;
using scpqp_obst_dev::Pose;

// a * b + c in two roundings (include/scpqp_sensing.h: every product and every sum is its
// own rounding), spelled with the operators under contract(off) as in sensing.hip
__device__ __forceinline__ double mul_add_2r(double a, double b, double c) {
#pragma clang fp contract(off)
    const double ab = a * b;
    return ab + c;
}

__device__ __forceinline__ double mul_1r(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}

// the normal pair of the Philox call at counter (c0, epoch, c2, b_global), mapped as
// sensing.hip maps it
__device__ __forceinline__ void draw_at(const scpqp_sense_stream& st, uint32_t c0, uint32_t c2,
                                        uint32_t b_global, double& z0, double& z1) {
    uint32_t c[4] = {c0, st.epoch, c2, b_global};
    scpqp_noise_dev::philox4x32_10(c, (uint32_t)st.seed, (uint32_t)(st.seed >> 32));
    double u1, u2;
    scpqp_noise_dev::uniforms(c, u1, u2);
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    z0 = mul_1r(r, cs);
    z1 = mul_1r(r, sn);
}

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

// the measurement update with H = [I4 | 0] on a symmetric P; false on a bad pivot
__device__ __forceinline__ bool correct(double (&x)[NS], double (&P)[NS][NS],
                                        const double (&zm)[NZ], const double (&r2)[NZ],
                                        double& nis) {
    double Lc[NZ][NZ], inv[NZ];
    bool ok = true;
    // S = P[0:4, 0:4] + R = L L'
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
    // W = L^-1 P[0:4, :], P <- P - W' W = P - P[:, 0:4] S^-1 P[0:4, :]
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

    // the measurement of scpqp_obstacles_predict_sensed
    double sp = 0.0, sh = 0.0, ss = 0.0;
    if (osense) {
        sp = osense[(size_t)g * ONP + SCPQP_OSENSE_SIG_POS];
        sh = osense[(size_t)g * ONP + SCPQP_OSENSE_SIG_HEADING];
        ss = osense[(size_t)g * ONP + SCPQP_OSENSE_SIG_SPEED];
    }
    const bool bad_meas = !isfinite(sp) || !isfinite(sh) || !isfinite(ss) || sp < 0.0 ||
                          sh < 0.0 || ss < 0.0 || scpqp_obst_dev::bad_row(r);
    double zm[NZ] = {NAN, NAN, NAN, NAN};
    if (!bad_meas) {
        const Pose p = scpqp_obst_dev::pose_at(r, t_meas);
        zm[0] = p.x;
        zm[1] = p.y;
        zm[2] = p.h;
        zm[3] = r[SCPQP_OBST_SPEED];
        if (!(sp == 0.0 && sh == 0.0 && ss == 0.0)) {
            const uint32_t c2 = ((uint32_t)SCPQP_NOISE_SITE_SENSE_OBST << 24) | (uint32_t)ob;
            const uint32_t bg = st.b_offset + (uint32_t)b;
            double a0, a1, b0, b1;
            draw_at(st, 0u, c2, bg, a0, a1);
            draw_at(st, 1u, c2, bg, b0, b1);
            zm[0] = mul_add_2r(sp, a0, zm[0]);
            zm[1] = mul_add_2r(sp, a1, zm[1]);
            zm[2] = mul_add_2r(sh, b0, zm[2]);
            zm[3] = mul_add_2r(ss, b1, zm[3]);
        }
    }
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
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_obst < 1 || n_obst > SCPQP_MAX_OBST) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    if (hp < 1 || hp > SCPQP_MAX_HP) return scpqp_fail_(SCPQP_E_ARG, "hp out of range");
    if (!isfinite(t_meas) || !isfinite(lead) || !isfinite(dt))
        return scpqp_fail_(SCPQP_E_ARG, "t_meas, lead and dt must be finite");
    if (!(t_since >= 0.0) || !isfinite(t_since))
        return scpqp_fail_(SCPQP_E_ARG, "t_since must be finite and >= 0");
    const long long n = (long long)B * n_obst;
    if (n * NS * NS > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 36 too large");
    if (2 * n * hp > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 2 * hp too large");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (osense && !st) return scpqp_fail_(SCPQP_E_ARG, "null sensing stream");
    if (!trk) return scpqp_fail_(SCPQP_E_ARG, "null trk rows array");
    if (!x_trk) return scpqp_fail_(SCPQP_E_ARG, "null x_trk array");
    if (!cov) return scpqp_fail_(SCPQP_E_ARG, "null cov array");
    if (!obst_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    // every block as the untracked controller predicts it; then, in stream order, the lanes
    // with a tracker overwrite theirs (scpqp_obstacles_track does the same)
    if (osense) {
        if (int rc = scpqp_obstacles_predict_sensed(B, n_obst, hp, rows, osense, st, t_meas, lead,
                                                    dt, obst_out, stream))
            return rc;
    } else {
        if (int rc = scpqp_obstacles_predict(B, n_obst, hp, rows, t_meas, lead, dt, obst_out, stream))
            return rc;
    }
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
