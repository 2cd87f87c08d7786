// margin.hip — chance-constrained obstacle margins on MI355X (fp64): the trackers' covariances
// pushed through the planner's own obstacle horizon (include/scpqp_margin.h).
//
//   scpqp_obstacles_margin   per (realisation, obstacle, horizon step) the larger principal
//                            sigma of the mixed second moment about the told point, times
//                            kappa, capped at m_max
//
// Sixteen threads per (b, o, mode): twelve carry a sigma state each, the thirteenth carries the
// mode's estimate (the nominal point), three more repeat the nominal and add nothing.  The four
// groups of a (b, o) make one wave of 64, four (b, o) per workgroup of 256.  Every thread of a
// group factors the mode's P itself (a 6 x 6 Cholesky fully unrolled in registers: one group
// does it once), picks its column of L, and walks the horizon of its own state.  Per horizon
// step the nominal point comes from thread 12 by __shfl of width 16, the three entries of the
// second moment are summed over the group by a butterfly of width 16, and the modes are mixed
// by __shfl of width 64.  No LDS, no scratch.
//
// No thread leaves before the last exchange (the rule at the top of imm.hip): waves past the
// batch and groups without a mode run on clamped addresses and store nothing, off and trouble
// lanes compute and discard, the loop over the horizon has the same trip count in every thread,
// and every exchange is a statement of its own, outside any && or ||.
//
// The horizon is step 4 of include/scpqp_tracker_accel.h on `advance` of
// scpqp_manoeuvre_pose.h, in the text of tracker_accel.hip and imm.hip.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_manoeuvre_pose.h"
#include "scpqp_margin.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

constexpr int NS = SCPQP_TRKA_NS;
constexpr int NP = SCPQP_TRKA_NP;
constexpr int MM = SCPQP_IMM_MAX_MODES;
constexpr int GW = 16;        // threads per (b, o, mode)
constexpr int LW = MM * GW;   // threads per (b, o): one wave
constexpr int PT = 256;       // threads per workgroup: PT / LW lanes (b, o)
constexpr int NOMINAL = 12;   // the group's thread that carries the estimate itself

static_assert(LW == 64, "one wave per (b, o)");

using scpqp_man_dev::State;

// the sum of v over this thread's group of sixteen, the same in every thread of the group
__device__ __forceinline__ double group_sum(double v) {
    v += __shfl_xor(v, 8, GW);
    v += __shfl_xor(v, 4, GW);
    v += __shfl_xor(v, 2, GW);
    v += __shfl_xor(v, 1, GW);
    return v;
}

// OR of `flag` over the groups of the wave that carry a mode
__device__ __forceinline__ bool lane_any(bool flag, int M) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        const int v = __shfl((int)flag, j * GW, LW);
        any |= j < M && v != 0;
    }
    return any;
}

__global__ __launch_bounds__(PT) void margin_kernel(
    int n, int hp, int M, const double* __restrict__ trk, const double* __restrict__ xs,
    const double* __restrict__ cov, const double* __restrict__ mus, double lead, double dt,
    double kappa, double m_max, double* __restrict__ margin, double* __restrict__ sigma_out) {
    const long long lane = (long long)blockIdx.x * (PT / LW) + (threadIdx.x >> 6);
    const int m = (threadIdx.x >> 4) & (MM - 1), sub = threadIdx.x & (GW - 1);
    const bool in = lane < n;                     // the same for the whole wave
    const int g = in ? (int)lane : n - 1;         // clamped: the reads stay inside the arrays
    const bool has = m < M;
    const int mj = has ? m : 0;                   // clamped likewise
    const size_t gm = (size_t)g * M + mj;

    double row[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) row[f] = trk[gm * NP + f];
    bool bad_row = false, off_row = true, r_zero = false;
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        bad_row |= !isfinite(row[f]) || row[f] < 0.0;
        off_row &= row[f] == 0.0;
    }
#pragma unroll
    for (int f = SCPQP_TRKA_R_POS; f <= SCPQP_TRKA_R_SPEED; ++f) r_zero |= row[f] == 0.0;
    bad_row |= !off_row && r_zero;

    // the state of this group's mode
    double x[NS], L[NS][NS];
    bool fin = true;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        x[i] = xs[gm * NS + i];
        fin &= isfinite(x[i]);
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
#pragma unroll
        for (int c = r; c < NS; ++c) {
            L[c][r] = cov[gm * NS * NS + r * NS + c];   // P's upper triangle, kept as its lower
            fin &= isfinite(L[c][r]);
        }
    }
    const double x00 = xs[(size_t)g * M * NS];
    const bool init = x00 == x00;
    const double mu = mus ? mus[gm] : 1.0;
    const bool bad_mu = !isfinite(mu) || mu < 0.0;
    const bool used = has && mu > 0.0;

    // L of P = L L', in place, column by column
    bool piv = true;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < c; ++k) s += L[c][k] * L[c][k];
        const double d = L[c][c] - s;
        piv &= d > 0.0 && isfinite(d);
        L[c][c] = sqrt(d);
#pragma unroll
        for (int i = c + 1; i < NS; ++i) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < c; ++k) t += L[i][k] * L[c][k];
            L[i][c] = (L[i][c] - t) / L[c][c];
        }
    }

    const bool any_on = lane_any(!off_row, M), any_off = lane_any(off_row, M);
    const bool any_bad = lane_any(bad_row || !fin || bad_mu || (used && !piv), M);
    const bool any_used = lane_any(used, M);
    const bool off = !any_on;
    bool ok = !off && !any_off && !any_bad && any_used && init;

    // this thread's state: x +- sqrt(6) L[:, col], or x itself
    const int col = sub < 6 ? sub : sub - 6;
    const double sg = sub < 6 ? 2.449489742783178 : (sub < NOMINAL ? -2.449489742783178 : 0.0);
    double sx[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double lc = 0.0;
#pragma unroll
        for (int c = 0; c <= i; ++c) lc = col == c ? L[i][c] : lc;
        sx[i] = sub < NOMINAL ? x[i] + sg * lc : x[i];
    }

    // the horizon of this state in up to three pieces
    const double wc = fmin(fmax(sx[4], -row[SCPQP_TRKA_W_CLAMP]), row[SCPQP_TRKA_W_CLAMP]);
    const double ac = fmin(fmax(sx[5], -row[SCPQP_TRKA_A_CLAMP]), row[SCPQP_TRKA_A_CLAMP]);
    const double wh = row[SCPQP_TRKA_W_HOLD], ah = row[SCPQP_TRKA_A_HOLD];
    const double t1 = fmin(wh, ah), t2 = fmax(wh, ah);
    const double a2 = ah > wh ? ac : 0.0, w2 = ah > wh ? 0.0 : wc;
    const State q0{sx[0], sx[1], sx[2], fmax(sx[3], 0.0), wc};
    State q1 = q0;
    scpqp_man_dev::advance(q1, ac, wc, t1);
    State q2 = q1;
    scpqp_man_dev::advance(q2, a2, w2, t2 - t1);
    const double qpos2 = row[SCPQP_TRKA_Q_POS] * row[SCPQP_TRKA_Q_POS];
    const bool writer = in && threadIdx.x % LW == 0;
    double* mo = margin + (size_t)g * hp;
    double* so = sigma_out ? sigma_out + (size_t)g * hp * 3 : nullptr;
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
        // 1. the second moment of the group's twelve about its nominal point
        const double cx = __shfl(q.x, NOMINAL, GW);
        const double cy = __shfl(q.y, NOMINAL, GW);
        const double ex = sub < NOMINAL ? q.x - cx : 0.0, ey = sub < NOMINAL ? q.y - cy : 0.0;
        const double sxx = group_sum(ex * ex) * (1.0 / 12.0) + tau * qpos2;
        const double sxy = group_sum(ex * ey) * (1.0 / 12.0);
        const double syy = group_sum(ey * ey) * (1.0 / 12.0) + tau * qpos2;
        // 2. the mix over the modes with mu > 0, in mode order
        double mw[MM], mcx[MM], mcy[MM], bx = 0.0, by = 0.0;
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            const double muj = __shfl(mu, j * GW, LW);
            mcx[j] = __shfl(cx, j * GW, LW);
            mcy[j] = __shfl(cy, j * GW, LW);
            mw[j] = j < M && muj > 0.0 ? muj : 0.0;
            bx = mw[j] != 0.0 ? bx + mw[j] * mcx[j] : bx;
            by = mw[j] != 0.0 ? by + mw[j] * mcy[j] : by;
        }
        double Sxx = 0.0, Sxy = 0.0, Syy = 0.0;
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            const double jxx = __shfl(sxx, j * GW, LW);
            const double jxy = __shfl(sxy, j * GW, LW);
            const double jyy = __shfl(syy, j * GW, LW);
            const double dx = mcx[j] - bx, dy = mcy[j] - by;
            Sxx = mw[j] != 0.0 ? Sxx + mw[j] * (jxx + dx * dx) : Sxx;
            Sxy = mw[j] != 0.0 ? Sxy + mw[j] * (jxy + dx * dy) : Sxy;
            Syy = mw[j] != 0.0 ? Syy + mw[j] * (jyy + dy * dy) : Syy;
        }
        // 3. the larger eigenvalue
        const double lam = 0.5 * (Sxx + Syy) + hypot(0.5 * (Sxx - Syy), Sxy);
        const bool good = ok && isfinite(lam);
        if (writer) {
            mo[k] = off ? 0.0 : (good ? fmin(kappa * sqrt(lam), m_max) : NAN);
            if (so) {
                so[3 * k] = off ? 0.0 : (good ? Sxx : NAN);
                so[3 * k + 1] = off ? 0.0 : (good ? Sxy : NAN);
                so[3 * k + 2] = off ? 0.0 : (good ? Syy : NAN);
            }
        }
    }
}

}  // namespace

extern "C" {

int scpqp_obstacles_margin(int32_t B, int32_t n_obst, int32_t hp, int32_t n_modes,
                           const double* trk, const double* x, const double* cov,
                           const double* mu, double lead, double dt, double kappa, double m_max,
                           double* margin, double* sigma_out, void* stream) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_obst < 1 || n_obst > SCPQP_MAX_OBST) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    if (hp < 1 || hp > SCPQP_MAX_HP) return scpqp_fail_(SCPQP_E_ARG, "hp out of range");
    if (n_modes < 1 || n_modes > SCPQP_IMM_MAX_MODES)
        return scpqp_fail_(SCPQP_E_ARG, "n_modes out of range");
    if (!isfinite(lead) || !isfinite(dt)) return scpqp_fail_(SCPQP_E_ARG, "lead and dt must be finite");
    if (!(kappa >= 0.0) || !isfinite(kappa))
        return scpqp_fail_(SCPQP_E_ARG, "kappa must be finite and >= 0");
    if (!(m_max >= 0.0) || !isfinite(m_max))
        return scpqp_fail_(SCPQP_E_ARG, "m_max must be finite and >= 0");
    const long long n = (long long)B * n_obst;
    if (n * n_modes * NS * NS > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * n_modes * 36 too large");
    if (3 * n * hp > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 3 * hp too large");
    if (B == 0) return 0;
    if (!trk) return scpqp_fail_(SCPQP_E_ARG, "null trk rows array");
    if (!x) return scpqp_fail_(SCPQP_E_ARG, "null x array");
    if (!cov) return scpqp_fail_(SCPQP_E_ARG, "null cov array");
    if (!mu && n_modes != 1) return scpqp_fail_(SCPQP_E_ARG, "null mu array with n_modes > 1");
    if (!margin) return scpqp_fail_(SCPQP_E_ARG, "null margin array");
    constexpr int per = PT / LW;
    hipLaunchKernelGGL(margin_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, hp, (int)n_modes, trk, x, cov, mu,
                       lead, dt, kappa, m_max, margin, sigma_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
