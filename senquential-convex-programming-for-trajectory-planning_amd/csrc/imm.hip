// imm.hip — interacting-multiple-model obstacle tracker on MI355X (fp64): the bank of up to
// four six-state filters per (realisation, obstacle) of include/scpqp_imm.h.
//
//   scpqp_obstacles_track_imm   one step of every lane's bank: the untracked prediction into
//                               obst_out (the existing kernels, for the off lanes), then per
//                               lane measure, mix, predict and correct every mode, move the
//                               probabilities, and the probability-weighted horizon
//
// One thread per (b, o, mode): the four threads of a quad belong to one (b, o), n_modes of them
// carry a mode, 64 (b, o) per workgroup of 256.  Every mode's estimate and covariance stay in
// its thread's registers, as in tracker_accel.hip (every 6 x 6 and 4 x 4 loop is fully
// unrolled with compile-time indices).  The mixing, the probability update and the weighted
// outputs exchange x, the upper triangle of P, c, l, mu and the horizon points between the
// quad's threads with __shfl of width 4.  No LDS, no scratch.
//
// No thread leaves before the last exchange: threads past the batch and quad threads without
// a mode run on clamped addresses (they read what another thread reads and store nothing),
// off and bad lanes compute and discard, and every exchange is written as a statement of its
// own, outside any && or ||.  Whatever condition the compiler still puts around an exchange
// is the same for the four threads of a quad, and an exchange of width 4 reads only inside
// its quad.  Every reduction over the modes is taken in mode order by every thread of the quad.
//
// The predict, transition and update functions restate those of tracker_accel.hip (which is
// not edited); the update also returns sum_k log L_kk.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_imm.h"
#include "scpqp_manoeuvre_pose.h"
#include "scpqp_obstacle_pose.h"
#include "scpqp_philox.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

constexpr int NS = SCPQP_TRKA_NS;
constexpr int NZ = SCPQP_TRKA_NZ;
constexpr int NP = SCPQP_TRKA_NP;
constexpr int ONP = SCPQP_OSENSE_NP;
constexpr int MM = SCPQP_IMM_MAX_MODES;
constexpr int PT = 256;   // threads per workgroup: PT / MM lanes (b, o)

static_assert(MM == 4, "the quad layout carries four modes");

using scpqp_man_dev::State;
using scpqp_obst_dev::Pose;

// a * b + c in two roundings (include/scpqp_sensing.h), as in sensing.hip
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

// P <- F P F' + T Q on the upper triangle of a symmetric P, mirrored below
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

// the measurement update with H = [I4 | 0] on a symmetric P; false on a bad pivot.  logdet
// receives sum_k log L_kk.
__device__ __forceinline__ bool correct(double (&x)[NS], double (&P)[NS][NS],
                                        const double (&zm)[NZ], const double (&r2)[NZ],
                                        double& nis, double& logdet) {
    double Lc[NZ][NZ], inv[NZ];
    bool ok = true;
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
    logdet = 0.0;
#pragma unroll
    for (int j = 0; j < NZ; ++j) logdet += log(Lc[j][j]);
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

// the value thread `i` of this thread's quad holds
__device__ __forceinline__ double quad(double v, int i) { return __shfl(v, i, MM); }
__device__ __forceinline__ int quad(int v, int i) { return __shfl(v, i, MM); }

// OR of `flag` over the quad's threads that carry a mode
__device__ __forceinline__ bool quad_any(bool flag, int M) {
    bool any = false;
#pragma unroll
    for (int i = 0; i < MM; ++i) {
        const int v = quad((int)flag, i);
        any |= i < M && v != 0;
    }
    return any;
}

// one thread per (b, o, mode).  obst_out already holds the untracked prediction of every lane.
__global__ __launch_bounds__(PT) void track_imm_kernel(
    int n, int nO, int hp, int M, const double* __restrict__ rows,
    const double* __restrict__ osense, scpqp_sense_stream st, const double* __restrict__ trk,
    const double* __restrict__ sw, double t_meas, double T, double lead, double dt,
    double* __restrict__ x_imm, double* __restrict__ cov, double* __restrict__ mu_io,
    double* __restrict__ x_hat, double* __restrict__ z_out, double* __restrict__ nis_out,
    double* __restrict__ out) {
    const int tid = blockIdx.x * PT + threadIdx.x;
    const int m = tid & (MM - 1);
    const bool in = (tid >> 2) < n;          // the same for the whole quad
    const int g = in ? tid >> 2 : n - 1;     // clamped: the reads stay inside the arrays
    const bool has = m < M;
    const int mj = has ? m : 0;              // clamped likewise
    const int b = g / nO, ob = g - b * nO;
    const size_t gm = (size_t)g * M + mj;
    const double* r = rows + (size_t)g * SCPQP_OBST_NP;
    const double* swl = sw + (size_t)g * (M + 1) * M;
    double row[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) row[f] = trk[gm * NP + f];

    // the row of this mode, then the lane
    bool bad_row = false, off_row = true, r_zero = false;
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        bad_row |= !isfinite(row[f]) || row[f] < 0.0;
        off_row &= row[f] == 0.0;
    }
#pragma unroll
    for (int f = SCPQP_TRKA_R_POS; f <= SCPQP_TRKA_R_SPEED; ++f) r_zero |= row[f] == 0.0;
    bad_row |= !off_row && r_zero;
    // mu0, this mode's row of Pi (checked here) and its column of Pi (used below)
    double mu0 = 0.0, pi[MM], s0sum = 0.0, s1sum = 0.0;
    bool bad_sw = false;
#pragma unroll
    for (int i = 0; i < MM; ++i) {
        pi[i] = 0.0;
        if (i < M) {
            const double a0 = swl[i], a1 = swl[(size_t)(1 + mj) * M + i];
            bad_sw |= !isfinite(a0) || a0 < 0.0 || !isfinite(a1) || a1 < 0.0;
            s0sum += a0;
            s1sum += a1;
            pi[i] = swl[(size_t)(1 + i) * M + mj];
            if (i == mj) mu0 = a0;
        }
    }
    bad_sw |= !(fabs(s0sum - 1.0) <= SCPQP_IMM_SUM_TOL) || !(fabs(s1sum - 1.0) <= SCPQP_IMM_SUM_TOL);
    const bool any_on = quad_any(!off_row, M), any_off = quad_any(off_row, M);
    const bool any_bad_row = quad_any(bad_row, M), any_bad_sw = quad_any(bad_sw, M);
    const bool off = !any_on;
    const bool bad = !off && (any_bad_row || any_off || any_bad_sw);

    // the measurement of scpqp_obstacles_predict_sensed, the same in every thread of the quad
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
    if (z_out && in && m == 0) {
#pragma unroll
        for (int i = 0; i < NZ; ++i) z_out[(size_t)g * NZ + i] = zm[i];
    }

    // the state of this mode; init: the lane has been initialised (mode 0's x says so)
    double x[NS], P[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] = x_imm[gm * NS + i];
#pragma unroll
    for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
        for (int c = rr; c < NS; ++c) P[rr][c] = P[c][rr] = cov[gm * NS * NS + rr * NS + c];
    }
    const double x00 = x_imm[(size_t)g * M * NS];
    const bool init = x00 == x00;
    const double mu_prev = mu_io[gm];

    // 2. mix: c_j and the weights w_{i|j} of this mode j
    const bool mix = T > 0.0;
    double cj = 0.0, wt[MM];
#pragma unroll
    for (int i = 0; i < MM; ++i) {
        const double mui = quad(mu_prev, i);
        wt[i] = i < M ? pi[i] * mui : 0.0;
        if (i < M) cj += wt[i];
    }
#pragma unroll
    for (int i = 0; i < MM; ++i) wt[i] = cj == 0.0 ? (i == mj ? 1.0 : 0.0) : wt[i] / cj;
    double xm[NS], Pm[NS][NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) xm[k] = 0.0;
#pragma unroll
    for (int i = 0; i < MM; ++i) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const double xi = quad(x[k], i);
            xm[k] = wt[i] != 0.0 ? xm[k] + wt[i] * xi : xm[k];
        }
    }
#pragma unroll
    for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
        for (int c = rr; c < NS; ++c) Pm[rr][c] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < MM; ++i) {
        double d[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) d[k] = quad(x[k], i) - xm[k];
#pragma unroll
        for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
            for (int c = rr; c < NS; ++c) {
                const double pi_rc = quad(P[rr][c], i);
                Pm[rr][c] = wt[i] != 0.0 ? Pm[rr][c] + wt[i] * (pi_rc + d[rr] * d[c]) : Pm[rr][c];
            }
        }
    }
    if (mix) {
#pragma unroll
        for (int k = 0; k < NS; ++k) x[k] = xm[k];
#pragma unroll
        for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
            for (int c = rr; c < NS; ++c) P[rr][c] = P[c][rr] = Pm[rr][c];
        }
    } else {
        cj = mu_prev;
    }

    // 3. filter this mode, or 1. initialise it
    const double r2[NZ] = {row[0] * row[0], row[0] * row[0], row[1] * row[1], row[2] * row[2]};
    double nis = NAN, logdet = 0.0;
    bool okj = true;
    if (init) {
        const double tq[NS] = {T * (row[3] * row[3]), T * (row[3] * row[3]),
                               T * (row[4] * row[4]), T * (row[5] * row[5]),
                               T * (row[6] * row[6]), T * (row[7] * row[7])};
        const double s0 = fmax(x[3], 0.0);
        propagate(P, transition(x[2], s0, x[4], x[5], T), tq);
        State q{x[0], x[1], x[2], s0, x[4]};
        scpqp_man_dev::advance(q, x[5], x[4], T);
        x[0] = q.x;
        x[1] = q.y;
        x[2] = q.h;
        x[3] = q.s;
        okj = correct(x, P, zm, r2, nis, logdet);
        okj = okj && isfinite(nis);
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
#pragma unroll
    for (int i = 0; i < NS; ++i) okj &= isfinite(x[i]);
#pragma unroll
    for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
        for (int c = rr; c < NS; ++c) okj &= isfinite(P[rr][c]);
    }

    // 4. probabilities: the maximum and the sum over the modes with c > 0, in mode order
    const double lj = -0.5 * nis - logdet;
    double lmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < MM; ++i) {
        const double li = quad(lj, i), ci = quad(cj, i);
        if (i < M && ci > 0.0) lmax = fmax(lmax, li);
    }
    const double ej = cj * exp(lj - lmax);
    double esum = 0.0;
#pragma unroll
    for (int i = 0; i < MM; ++i) {
        const double ei = quad(ej, i), ci = quad(cj, i);
        if (i < M && ci > 0.0) esum += ei;
    }
    const double mu = init ? (cj > 0.0 ? ej / esum : 0.0) : mu0;
    // trouble: in any mode, a probability that is not finite, or no mode with c > 0
    const bool any_trouble = quad_any(!okj || !isfinite(mu), M);
    const bool any_alive = quad_any(cj > 0.0, M);
    const bool live = in && !off && !bad && !bad_meas && !any_trouble && (!init || any_alive);

    // 5. the combined estimate and this mode's state
    double mus[MM];
#pragma unroll
    for (int i = 0; i < MM; ++i) {
        const double v = quad(mu, i);
        mus[i] = i < M ? v : 0.0;
    }
    double xh[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        xh[k] = 0.0;
#pragma unroll
        for (int i = 0; i < MM; ++i) {
            const double xi = quad(x[k], i);
            xh[k] = mus[i] != 0.0 ? xh[k] + mus[i] * xi : xh[k];
        }
    }
    const bool store = in && !off;   // an off lane keeps its state and its block
    if (in && m == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) x_hat[(size_t)g * NS + k] = live ? xh[k] : NAN;
    }
    if (in && has && nis_out) nis_out[gm] = live ? nis : NAN;
    if (store && has) {
#pragma unroll
        for (int i = 0; i < NS; ++i) x_imm[gm * NS + i] = live ? x[i] : NAN;
#pragma unroll
        for (int rr = 0; rr < NS; ++rr) {
#pragma unroll
            for (int c = 0; c < NS; ++c) cov[gm * NS * NS + rr * NS + c] = live ? P[rr][c] : NAN;
        }
        mu_io[gm] = live ? mu : NAN;
    }

    // this mode's horizon in up to three pieces, summed over the quad
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
    double* o = out + (size_t)g * 2 * hp;
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
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int i = 0; i < MM; ++i) {
            const double px = quad(q.x, i), py = quad(q.y, i);
            sx = mus[i] != 0.0 ? sx + mus[i] * px : sx;
            sy = mus[i] != 0.0 ? sy + mus[i] * py : sy;
        }
        // thread 0 of the quad writes x, thread 1 writes y
        if (store && m == 0) o[k] = live ? sx : NAN;
        if (store && m == 1) o[hp + k] = live ? sy : NAN;
    }
}

}  // namespace

extern "C" {

int scpqp_obstacles_track_imm(int32_t B, int32_t n_obst, int32_t hp, int32_t n_modes,
                              const double* rows, const double* osense,
                              const scpqp_sense_stream* st, const double* trk, const double* sw,
                              double t_meas, double t_since, double lead, double dt,
                              double* x_imm, double* cov, double* mu, double* x_hat,
                              double* z_out, double* nis, double* obst_out, void* stream) {
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
    if (n * n_modes * NS * NS > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * n_modes * 36 too large");
    if (2 * n * hp > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 2 * hp too large");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (osense && !st) return scpqp_fail_(SCPQP_E_ARG, "null sensing stream");
    if (!trk) return scpqp_fail_(SCPQP_E_ARG, "null trk rows array");
    if (!sw) return scpqp_fail_(SCPQP_E_ARG, "null sw array");
    if (!x_imm) return scpqp_fail_(SCPQP_E_ARG, "null x_imm array");
    if (!cov) return scpqp_fail_(SCPQP_E_ARG, "null cov array");
    if (!mu) return scpqp_fail_(SCPQP_E_ARG, "null mu array");
    if (!x_hat) return scpqp_fail_(SCPQP_E_ARG, "null x_hat array");
    if (!obst_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    // every block as the untracked controller predicts it; then, in stream order, the lanes
    // with a bank overwrite theirs (scpqp_obstacles_track_accel does the same)
    if (osense) {
        if (int rc = scpqp_obstacles_predict_sensed(B, n_obst, hp, rows, osense, st, t_meas, lead,
                                                    dt, obst_out, stream))
            return rc;
    } else {
        if (int rc = scpqp_obstacles_predict(B, n_obst, hp, rows, t_meas, lead, dt, obst_out, stream))
            return rc;
    }
    const scpqp_sense_stream none = {0, 0, 0};
    const long long threads = n * MM;
    hipLaunchKernelGGL(track_imm_kernel, dim3((unsigned)((threads + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, n_obst, hp, (int)n_modes, rows,
                       osense, osense ? *st : none, trk, sw, t_meas, t_since, lead, dt, x_imm, cov,
                       mu, x_hat, z_out, nis, obst_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
