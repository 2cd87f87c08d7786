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
// The transition, the covariance product and the update are those of tracker_accel.hip
// (scpqp_ekf.h), the update with sum_k log L_kk; the measurement is the one of every tracker
// (scpqp_sense_draw.h).  A helper used here must keep the rule above: no exchange and no early
// exit under a condition that differs within a quad.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_ekf.h"
#include "scpqp_entry_checks.h"
#include "scpqp_imm.h"
#include "scpqp_sense_draw.h"

namespace {

using namespace scpqp_trka_dev;   // scpqp_ekf.h: NS, NZ, NP, State, transition, propagate

constexpr int MM = SCPQP_IMM_MAX_MODES;
constexpr int PT = 256;   // threads per workgroup: PT / MM lanes (b, o)

static_assert(MM == 4, "the quad layout carries four modes");

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

    // the measurement, the same in every thread of the quad
    double zm[NZ] = {NAN, NAN, NAN, NAN};
    const bool bad_meas = scpqp_sense_dev::measure_obstacle(r, osense, g, st, b, ob, t_meas, zm);
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
        okj = scpqp_ekf_dev::correct<true>(x, P, zm, r2, nis, &logdet);
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
    if (int rc = scpqp_host::track_begin(
            B, n_obst, hp, n_modes, (long long)n_modes * NS * NS,
            "B * n_obst * n_modes * 36 too large", rows, osense, st, trk,
            {{sw, "null sw array"}, {x_imm, "null x_imm array"}, {cov, "null cov array"},
             {mu, "null mu array"}, {x_hat, "null x_hat array"}},
            t_meas, t_since, lead, dt, obst_out, stream))
        return rc < 0 ? rc : 0;
    const long long n = (long long)B * n_obst;
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
