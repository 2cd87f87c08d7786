// metrics.hip — realised-path metrics of closed-loop rollouts on MI355X (fp64).
//
//   scpqp_metrics_accumulate  one MPC step's plant path x_path [B][n_veh][K][6] ->
//                             footprint gaps (vehicle-vehicle, vehicle-obstacle),
//                             margins to the planner's dsafe and cross-track errors,
//                             merged into a per-realisation accumulator and/or
//                             written densely (include/scpqp_metrics.h)
//
// Work decomposition: one wave64 (one 64-thread workgroup) owns one realisation.
//   1. stage   lanes stride over the (tick, vehicle) entries: x, y, cos h, sin h go
//              to LDS, the cross-track error of the entry is computed and kept there
//   2. pairs   lanes stride over the (tick, pair) and (tick, vehicle, obstacle) items
//              in lexicographic order; each lane keeps its smallest gap with the item
//              index, so a strict "<" inside the lane keeps the earliest item
//   3. ticks   lane v adds vehicle v's squared cross-track errors tick by tick (a
//              fixed order: the sum does not depend on anything but the path); lanes
//              stride over the ticks' collision flags
//   4. merge   a shuffle butterfly with the total order (gap, tick, item) reduces the
//              lanes; lane 0 merges into the realisation's accumulator with plain
//              loads and stores.  No atomics, nothing shared between realisations.
// Steps 1-3 run per chunk of ticks (ENT_CAP staged entries: the whole step for up
// to 16 vehicles x 42 ticks); lane state carries over the chunks, so the chunking
// does not show in any result.
//
// scpqp_metrics_accumulate_obstacles (include/scpqp_obstacles.h) runs the same kernel
// instantiated with kRows: obstacle o of realisation b is posed by its own row at the
// tick's time, per (tick, vehicle, obstacle) item and in registers.  The constant
// obstacles' once-per-workgroup cos / sin staging cannot serve a pose that depends on the
// tick, and staging [ticks][n_obst] poses would bound the chunk by ticks x n_obst as well
// (frog's 22 obstacles: 30 ticks, its 41-entry step cut in two) for 21 KB more LDS.  The
// per-item pose repeats a row's sincos n_veh times per tick; the scenarios with obstacles
// have 1 and 5 vehicles, and the chunking stays that of the constant obstacles, so the
// nominal rows give bitwise what those give.  The instantiation without kRows is the
// kernel the other entry points have always launched.
//
// scpqp_metrics_accumulate_posed (include/scpqp_manoeuvres.h) is the third instantiation,
// kPosed: obstacle o of realisation b at tick k is read from the dense poses
// pose[b][o][k][0..2] the caller computed (scpqp_manoeuvres_pose), and sized by its row.  The
// poses stay in global memory (each is read n_veh times, from L2), so the chunking is again
// that of the constant obstacles; the item costs one sincos of the heading.
#include <hip/hip_runtime.h>

#include <math.h>

#include <vector>

#include "scpqp_manoeuvres.h"
#include "scpqp_metrics.h"
#include "scpqp_obstacle_pose.h"
#include "scpqp_obstacles.h"
#include "scpqp_variants.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

constexpr int WAVE = 64;
constexpr int ENT_CAP = 672;   // staged (tick, vehicle) entries per chunk
constexpr int MAXV = SCPQP_MAX_VEH, MAXO = SCPQP_MAX_OBST, MAXP = SCPQP_MAX_REFPTS;
constexpr int MAX_PAIR = MAXV * (MAXV - 1) / 2;
constexpr int NX = 6;

struct DevConst {
    int n_veh, n_obst, n_pair, pad;
    double tick_length;
    double hx[MAXV], hy[MAXV];          // Length / 2, Width / 2
    double dsafe_veh[MAXV * MAXV];      // [v * n_veh + w]
    double dsafe_obs[MAXV * MAXO];      // [v * n_obst + o]
    double obst[MAXO][6];               // x y heading speed length width
    double ref[MAXV][MAXP][2];
    int npts[MAXV];
    unsigned char pair_v[MAX_PAIR], pair_w[MAX_PAIR];   // pair index -> (v, w), v < w
};

struct Rect {
    double cx, cy, c, s, hx, hy;        // centre, cos / sin of the heading, half extents
};

// r_X(n) = hx |n.x1| + hy |n.x2|, x1 = (c, s), x2 = (-s, c)
__device__ __forceinline__ double radius(const Rect& r, double nx, double ny) {
    return r.hx * fabs(nx * r.c + ny * r.s) + r.hy * fabs(ny * r.c - nx * r.s);
}

__device__ __forceinline__ bool separated(const Rect& a, const Rect& b, double dx, double dy,
                                          double nx, double ny) {
    return fabs(nx * dx + ny * dy) > radius(a, nx, ny) + radius(b, nx, ny);
}

// smallest distance of a's four corners to the rectangle b
__device__ __forceinline__ double corners_to(const Rect& a, const Rect& b) {
    double best = INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double sx = (i & 2) ? -1.0 : 1.0, sy = (i & 1) ? -1.0 : 1.0;
        const double qx = a.cx + sx * a.hx * a.c - sy * a.hy * a.s;
        const double qy = a.cy + sx * a.hx * a.s + sy * a.hy * a.c;
        const double rx = qx - b.cx, ry = qy - b.cy;
        const double px = rx * b.c + ry * b.s, py = ry * b.c - rx * b.s;
        best = fmin(best, hypot(fmax(fabs(px) - b.hx, 0.0), fmax(fabs(py) - b.hy, 0.0)));
    }
    return best;
}

__device__ __forceinline__ double footprint_gap(const Rect& a, const Rect& b) {
    const double dx = b.cx - a.cx, dy = b.cy - a.cy;
    const bool sep = separated(a, b, dx, dy, a.c, a.s) || separated(a, b, dx, dy, -a.s, a.c) ||
                     separated(a, b, dx, dy, b.c, b.s) || separated(a, b, dx, dy, -b.s, b.c);
    if (!sep) return 0.0;
    return fmin(corners_to(a, b), corners_to(b, a));
}

// distance of (px, py) to vehicle v's reference polyline, end segments extended
__device__ __forceinline__ double cross_track(const DevConst* __restrict__ P, int v, double px,
                                              double py) {
    const int n = P->npts[v];
    double best = INFINITY;
    for (int j = 0; j + 1 < n; ++j) {
        const double ax = P->ref[v][j][0], ay = P->ref[v][j][1];
        const double ex = P->ref[v][j + 1][0] - ax, ey = P->ref[v][j + 1][1] - ay;
        const double l2 = ex * ex + ey * ey;
        double t = l2 > 0.0 ? ((px - ax) * ex + (py - ay) * ey) / l2 : 0.0;
        if (j > 0) t = fmax(t, 0.0);
        if (j + 2 < n) t = fmin(t, 1.0);
        best = fmin(best, hypot(px - (ax + t * ex), py - (ay + t * ey)));
    }
    return best;
}

// lane-local running minimum with its (global tick, item) key
struct Best {
    double g;
    int tick, item;
};

__device__ __forceinline__ bool before(double g, int tick, int item, const Best& b) {
    return g < b.g || (g == b.g && (tick < b.tick || (tick == b.tick && item < b.item)));
}

__device__ __forceinline__ void wave_min(Best& b) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const double g = __shfl_xor(b.g, m, WAVE);
        const int t = __shfl_xor(b.tick, m, WAVE), it = __shfl_xor(b.item, m, WAVE);
        if (before(g, t, it, b)) b = Best{g, t, it};
    }
}

__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) x = fmin(x, __shfl_xor(x, m, WAVE));
    return x;
}

// where the obstacles of a realisation come from
enum ObstSrc { kConst = 0, kRowsSrc = 1, kPosed = 2 };

// the arguments of the source: the rows (kRows, kPosed; not read otherwise) and, for kPosed
// alone, the dense poses, so that the two other instantiations keep their argument list
template <int kSrc>
struct SrcArgs {
    const double* rows;
};
template <>
struct SrcArgs<kPosed> {
    const double* rows;
    const double* pose;
};

// kRows: obstacle o of realisation b is rows[b][o] (include/scpqp_obstacles.h) instead of
// the constants' P->obst[o]; kPosed: it is at src.pose[b][o][k] with the row's extents
// (include/scpqp_manoeuvres.h)
template <int kSrc>
__global__ __launch_bounds__(WAVE) void metrics_kernel(const DevConst* __restrict__ table, int n_var,
                                                       const int* __restrict__ variant, int n_ticks,
                                                       int tick0, int k_first,
                                                       const double* __restrict__ x_path,
                                                       scpqp_metrics_acc acc, bool have_acc,
                                                       scpqp_metrics_dense dense,
                                                       const SrcArgs<kSrc> src) {
    constexpr bool kRows = kSrc == kRowsSrc;
    const double* __restrict__ rows = src.rows;
    __shared__ double pose[ENT_CAP][4];     // x, y, cos h, sin h of entry (tick, vehicle)
    __shared__ double xt[ENT_CAP];          // its cross-track error
    __shared__ int coll[ENT_CAP];           // per tick of the chunk: any gap of 0
    __shared__ double ocs[MAXO][2];         // cos / sin of the obstacle headings

    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    // the realisation's constants; an index outside the table leaves the realisation's
    // accumulator and dense outputs untouched (the whole workgroup leaves: b is uniform)
    const int var = variant ? variant[b] : 0;
    if (var < 0 || var >= n_var) return;
    const DevConst* __restrict__ P = table + var;
    const int nV = P->n_veh, nO = P->n_obst, nP = P->n_pair, K = n_ticks + 1;
    const int nVO = nV * nO;
    const int chunk = ENT_CAP / nV;         // ticks per chunk (>= 42)
    const double* xb = x_path + b * nV * K * NX;
    const double* rb = nullptr;             // kRows, kPosed: the realisation's rows [nO][7]
    const double* posed = nullptr;          // kPosed: its poses [nO][K][3]

    if constexpr (kRows) {
        // a bad row leaves the realisation untouched, like a bad variant index: the lanes
        // stride over the rows and the whole wave leaves together
        rb = rows + b * nO * SCPQP_OBST_NP;
        bool bad = false;
        for (int o = lane; o < nO; o += WAVE) bad |= scpqp_obst_dev::bad_row(rb + o * SCPQP_OBST_NP);
        if (__any(bad)) return;
    } else if constexpr (kSrc == kPosed) {
        // likewise a bad row or a pose entry that is not finite (a bad lane's block is NaN)
        rb = rows + b * nO * SCPQP_OBST_NP;
        posed = src.pose + b * nO * K * 3;
        bool bad = false;
        for (int o = lane; o < nO; o += WAVE) bad |= scpqp_obst_dev::bad_row(rb + o * SCPQP_OBST_NP);
        for (int e = lane; e < nO * K * 3; e += WAVE) bad |= !isfinite(posed[e]);
        if (__any(bad)) return;
    } else {
        for (int o = lane; o < nO; o += WAVE) sincos(P->obst[o][2], &ocs[o][1], &ocs[o][0]);
    }

    Best bv{INFINITY, 0x7fffffff, 0x7fffffff}, bo{INFINITY, 0x7fffffff, 0x7fffffff};
    double mv = INFINITY, mo = INFINITY;    // margins
    double xmax = 0.0, xsum = 0.0;          // lane v < nV: vehicle v's cross-track state
    int ncoll = 0, first = 0x7fffffff;
    if (have_acc && lane < nV) {
        xmax = acc.max_xtrack[b * nV + lane];
        xsum = acc.sum_sq_xtrack[b * nV + lane];
    }

    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int nT = min(chunk, K - k0);
        // 1. stage the chunk's poses and cross-track errors
        for (int e = lane; e < nT * nV; e += WAVE) {
            const int kk = e / nV, v = e - kk * nV, k = k0 + kk;
            const double* x = xb + ((size_t)v * K + k) * NX;
            const double px = x[0], py = x[1];
            double s, c;
            sincos(x[2], &s, &c);
            pose[e][0] = px;
            pose[e][1] = py;
            pose[e][2] = c;
            pose[e][3] = s;
            const double d = cross_track(P, v, px, py);
            xt[e] = d;
            if (dense.xtrack) dense.xtrack[(b * K + k) * nV + v] = d;
        }
        for (int kk = lane; kk < nT; kk += WAVE) coll[kk] = 0;
        __syncthreads();
        // 2a. vehicle pairs
        for (int it = lane; it < nT * nP; it += WAVE) {
            const int kk = it / nP, p = it - kk * nP, k = k0 + kk;
            const int v = P->pair_v[p], w = P->pair_w[p];
            const double* pa = pose[kk * nV + v];
            const double* pb = pose[kk * nV + w];
            const Rect A{pa[0], pa[1], pa[2], pa[3], P->hx[v], P->hy[v]};
            const Rect Bq{pb[0], pb[1], pb[2], pb[3], P->hx[w], P->hy[w]};
            const double g = footprint_gap(A, Bq);
            if (dense.gap_veh) dense.gap_veh[(b * K + k) * nP + p] = g;
            if (k >= k_first) {
                if (before(g, tick0 + k, p, bv)) bv = Best{g, tick0 + k, p};
                if (g == 0.0) coll[kk] = 1;
                mv = fmin(mv, hypot(Bq.cx - A.cx, Bq.cy - A.cy) - P->dsafe_veh[v * nV + w]);
            }
        }
        // 2b. vehicle-obstacle items
        for (int it = lane; it < nT * nVO; it += WAVE) {
            const int kk = it / nVO, q = it - kk * nVO, k = k0 + kk;
            const int v = q / nO, o = q - v * nO;
            const double* pa = pose[kk * nV + v];
            const Rect A{pa[0], pa[1], pa[2], pa[3], P->hx[v], P->hy[v]};
            const double t = (double)(tick0 + k) * P->tick_length;
            Rect O;
            if constexpr (kRows) {
                const double* ob = rb + o * SCPQP_OBST_NP;
                const scpqp_obst_dev::Pose q = scpqp_obst_dev::pose_at(ob, t);
                O = Rect{q.x, q.y, q.c, q.s, ob[SCPQP_OBST_LENGTH] * 0.5, ob[SCPQP_OBST_WIDTH] * 0.5};
            } else if constexpr (kSrc == kPosed) {
                const double* ob = rb + o * SCPQP_OBST_NP;
                const double* q = posed + ((size_t)o * K + k) * 3;
                double s, c;
                sincos(q[2], &s, &c);
                O = Rect{q[0], q[1], c, s, ob[SCPQP_OBST_LENGTH] * 0.5, ob[SCPQP_OBST_WIDTH] * 0.5};
            } else {
                const double* ob = P->obst[o];
                O = Rect{t * ob[3] * ocs[o][0] + ob[0], t * ob[3] * ocs[o][1] + ob[1], ocs[o][0],
                         ocs[o][1], ob[4] * 0.5, ob[5] * 0.5};
            }
            const double g = footprint_gap(A, O);
            if (dense.gap_obs) dense.gap_obs[(b * K + k) * nVO + q] = g;
            if (k >= k_first) {
                if (before(g, tick0 + k, q, bo)) bo = Best{g, tick0 + k, q};
                if (g == 0.0) coll[kk] = 1;
                mo = fmin(mo, hypot(O.cx - A.cx, O.cy - A.cy) - P->dsafe_obs[q]);
            }
        }
        __syncthreads();
        // 3. per vehicle in tick order; per tick the collision flag
        if (lane < nV) {
            for (int kk = max(0, k_first - k0); kk < nT; ++kk) {
                const double d = xt[kk * nV + lane];
                xmax = fmax(xmax, d);
                xsum = __dadd_rn(xsum, __dmul_rn(d, d));
            }
        }
        for (int kk = lane; kk < nT; kk += WAVE) {
            if (k0 + kk >= k_first && coll[kk]) {
                ++ncoll;
                first = min(first, tick0 + k0 + kk);
            }
        }
        __syncthreads();
    }
    if (!have_acc) return;
    // 4. reduce the lanes and merge into the realisation's accumulator
    wave_min(bv);
    wave_min(bo);
    mv = wave_min(mv);
    mo = wave_min(mo);
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        ncoll += __shfl_xor(ncoll, m, WAVE);
        first = min(first, __shfl_xor(first, m, WAVE));
    }
    if (lane < nV) {
        acc.max_xtrack[b * nV + lane] = xmax;
        acc.sum_sq_xtrack[b * nV + lane] = xsum;
    }
    if (lane == 0) {
        if (bv.g < acc.min_gap_veh[b]) {
            acc.min_gap_veh[b] = bv.g;
            acc.argmin_gap_veh[b * 3 + 0] = bv.tick;
            acc.argmin_gap_veh[b * 3 + 1] = P->pair_v[bv.item];
            acc.argmin_gap_veh[b * 3 + 2] = P->pair_w[bv.item];
        }
        if (bo.g < acc.min_gap_obs[b]) {
            acc.min_gap_obs[b] = bo.g;
            acc.argmin_gap_obs[b * 3 + 0] = bo.tick;
            acc.argmin_gap_obs[b * 3 + 1] = bo.item / nO;
            acc.argmin_gap_obs[b * 3 + 2] = bo.item % nO;
        }
        acc.min_margin_veh[b] = fmin(acc.min_margin_veh[b], mv);
        acc.min_margin_obs[b] = fmin(acc.min_margin_obs[b], mo);
        if (ncoll) {
            const int old = acc.first_collision_tick[b];
            acc.first_collision_tick[b] = old < 0 ? first : min(old, first);
            acc.n_collision_ticks[b] += ncoll;
        }
        acc.n_ticks_seen[b] += K - k_first;
    }
}

__global__ __launch_bounds__(256) void metrics_reset_kernel(int B, int nV, scpqp_metrics_acc acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * nV) {
        acc.max_xtrack[i] = 0.0;
        acc.sum_sq_xtrack[i] = 0.0;
    }
    if (i < B * 3) {
        acc.argmin_gap_veh[i] = -1;
        acc.argmin_gap_obs[i] = -1;
    }
    if (i < B) {
        acc.min_gap_veh[i] = INFINITY;
        acc.min_gap_obs[i] = INFINITY;
        acc.min_margin_veh[i] = INFINITY;
        acc.min_margin_obs[i] = INFINITY;
        acc.first_collision_tick[i] = -1;
        acc.n_collision_ticks[i] = 0;
        acc.n_ticks_seen[i] = 0;
    }
}

int check_acc(const scpqp_metrics_acc* a) {
    if (!a->min_gap_veh || !a->min_gap_obs || !a->min_margin_veh || !a->min_margin_obs ||
        !a->argmin_gap_veh || !a->argmin_gap_obs || !a->first_collision_tick ||
        !a->n_collision_ticks || !a->n_ticks_seen || !a->max_xtrack || !a->sum_sq_xtrack)
        return scpqp_fail_(SCPQP_E_ARG, "null array in the accumulator");
    return 0;
}

int launched() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // namespace

struct scpqp_metrics {
    int device;
    int n_veh, n_obst, n_pair;
    DevConst* dev;        // the constants table: n_var blocks (scpqp_metrics_set_variants)
    int n_var;
    double tick_length;
};

namespace {

// the checks of one scpqp_metrics_params that need no other state (create, set_variants)
int check_params(const scpqp_metrics_params* p) {
    if (p->n_veh < 1 || p->n_veh > MAXV) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    if (p->n_obst < 0 || p->n_obst > MAXO) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    if (p->ref_max_pts < 2 || p->ref_max_pts > MAXP)
        return scpqp_fail_(SCPQP_E_ARG, "ref_max_pts out of range");
    if (!(p->tick_length > 0.0) || isinf(p->tick_length))
        return scpqp_fail_(SCPQP_E_ARG, "tick_length must be finite and > 0");
    return 0;
}

// The device constants of one scpqp_metrics_params (checked by check_params): what
// create uploads, and entry k of the table scpqp_metrics_set_variants installs.
int fill_const(const scpqp_metrics_params* p, DevConst* c) {
    if (!p->length || !p->width || !p->dsafe_veh || !p->ref_polyline || !p->ref_npts)
        return scpqp_fail_(SCPQP_E_ARG, "null array");
    if (p->n_obst > 0 && (!p->dsafe_obs || !p->obstacles))
        return scpqp_fail_(SCPQP_E_ARG, "null obstacle array");
    const int nV = p->n_veh, nO = p->n_obst;
    *c = DevConst();
    c->n_veh = nV;
    c->n_obst = nO;
    c->n_pair = nV * (nV - 1) / 2;
    c->tick_length = p->tick_length;
    for (int v = 0; v < nV; ++v) {
        if (!(p->length[v] >= 0.0) || !(p->width[v] >= 0.0) || isinf(p->length[v]) ||
            isinf(p->width[v]))
            return scpqp_fail_(SCPQP_E_ARG, "length / width must be finite and >= 0");
        if (p->ref_npts[v] < 2 || p->ref_npts[v] > p->ref_max_pts)
            return scpqp_fail_(SCPQP_E_ARG, "ref_npts must be in 2..ref_max_pts");
        c->hx[v] = p->length[v] / 2;
        c->hy[v] = p->width[v] / 2;
        c->npts[v] = p->ref_npts[v];
        for (int j = 0; j < p->ref_npts[v]; ++j)
            for (int d = 0; d < 2; ++d)
                c->ref[v][j][d] = p->ref_polyline[((size_t)v * p->ref_max_pts + j) * 2 + d];
        for (int w = 0; w < nV; ++w) c->dsafe_veh[v * nV + w] = p->dsafe_veh[v * nV + w];
        for (int o = 0; o < nO; ++o) c->dsafe_obs[v * nO + o] = p->dsafe_obs[v * nO + o];
    }
    for (int o = 0; o < nO; ++o)
        for (int d = 0; d < 6; ++d) c->obst[o][d] = p->obstacles[o * 6 + d];
    int q = 0;
    for (int v = 0; v < nV; ++v)
        for (int w = v + 1; w < nV; ++w, ++q) {
            c->pair_v[q] = (unsigned char)v;
            c->pair_w[q] = (unsigned char)w;
        }
    return 0;
}

int accumulate(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0, int32_t k_first,
               const double* x_path, const scpqp_metrics_acc* acc, const scpqp_metrics_dense* dense,
               const int32_t* variant, bool with_rows, const double* rows, void* stream);

int accumulate_from(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0, int32_t k_first,
                    const double* x_path, const scpqp_metrics_acc* acc,
                    const scpqp_metrics_dense* dense, const int32_t* variant, int src,
                    const double* rows, const double* pose, void* stream);

}  // namespace

extern "C" {

int scpqp_metrics_create(const scpqp_metrics_params* p, int device, scpqp_metrics** out) {
    if (!p || !out) return scpqp_fail_(SCPQP_E_ARG, "null argument");
    *out = nullptr;
    if (int rc = check_params(p)) return rc;
    if (device < 0) return scpqp_fail_(SCPQP_E_ARG, "device < 0");
    DevConst* c = new DevConst();
    if (int rc = fill_const(p, c)) {
        delete c;
        return rc;
    }
    scpqp_metrics* m = new scpqp_metrics{device, p->n_veh, p->n_obst, c->n_pair, nullptr, 1, p->tick_length};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&m->dev, sizeof(DevConst));
    if (e == hipSuccess) e = hipMemcpy(m->dev, c, sizeof(DevConst), hipMemcpyHostToDevice);
    delete c;
    if (e != hipSuccess) {
        if (m->dev) (void)hipFree(m->dev);
        delete m;
        return scpqp_fail_(e == hipErrorOutOfMemory ? SCPQP_E_NOMEM : SCPQP_E_HIP,
                           hipGetErrorString(e));
    }
    *out = m;
    return 0;
}

int scpqp_metrics_set_variants(scpqp_metrics* m, int32_t n, const scpqp_metrics_params* params) {
    if (!params) return scpqp_fail_(SCPQP_E_ARG, "null params");
    if (n < 1) return scpqp_fail_(SCPQP_E_ARG, "n < 1: a table holds at least one variant");
    if (!m) return scpqp_fail_(SCPQP_E_ARG, "null metrics handle");
    std::vector<DevConst> table((size_t)n);
    for (int k = 0; k < n; ++k) {
        const scpqp_metrics_params* p = &params[k];
        if (int rc = check_params(p)) return rc;
        if (p->n_veh != m->n_veh) return scpqp_fail_(SCPQP_E_ARG, "variant differs from the handle in n_veh");
        if (p->n_obst != m->n_obst) return scpqp_fail_(SCPQP_E_ARG, "variant differs from the handle in n_obst");
        if (p->tick_length != m->tick_length)
            return scpqp_fail_(SCPQP_E_ARG, "variant differs from the handle in tick_length");
        if (int rc = fill_const(p, &table[k])) return rc;
    }
    // launches in flight read the old table: wait for them before it is freed
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    DevConst* dev = nullptr;
    if (e == hipSuccess) e = hipMalloc(&dev, sizeof(DevConst) * (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(dev, table.data(), sizeof(DevConst) * (size_t)n, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (dev) (void)hipFree(dev);
        return scpqp_fail_(e == hipErrorOutOfMemory ? SCPQP_E_NOMEM : SCPQP_E_HIP,
                           hipGetErrorString(e));
    }
    (void)hipFree(m->dev);
    m->dev = dev;
    m->n_var = n;
    return 0;
}

int scpqp_metrics_destroy(scpqp_metrics* m) {
    if (!m) return 0;
    (void)hipSetDevice(m->device);
    if (m->dev) (void)hipFree(m->dev);
    delete m;
    return 0;
}

int scpqp_metrics_reset(scpqp_metrics* m, int32_t B, const scpqp_metrics_acc* acc, void* stream) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (!m) return scpqp_fail_(SCPQP_E_ARG, "null metrics handle");
    if ((long long)B * (m->n_veh > 3 ? m->n_veh : 3) > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    if (B == 0) return 0;
    if (!acc) return scpqp_fail_(SCPQP_E_ARG, "null accumulator");
    if (int rc = check_acc(acc)) return rc;
    const int n = B * (m->n_veh > 3 ? m->n_veh : 3);
    hipLaunchKernelGGL(metrics_reset_kernel, dim3((n + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), B, m->n_veh, *acc);
    return launched();
}

int scpqp_metrics_accumulate(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                             int32_t k_first, const double* x_path, const scpqp_metrics_acc* acc,
                             const scpqp_metrics_dense* dense, void* stream) {
    return scpqp_metrics_accumulate_variants(m, B, n_ticks, tick0, k_first, x_path, acc, dense,
                                             nullptr, stream);
}

int scpqp_metrics_accumulate_variants(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                                      int32_t k_first, const double* x_path,
                                      const scpqp_metrics_acc* acc,
                                      const scpqp_metrics_dense* dense, const int32_t* variant,
                                      void* stream) {
    return accumulate(m, B, n_ticks, tick0, k_first, x_path, acc, dense, variant, false, nullptr,
                      stream);
}

int scpqp_metrics_accumulate_obstacles(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                                       int32_t k_first, const double* x_path,
                                       const scpqp_metrics_acc* acc,
                                       const scpqp_metrics_dense* dense, const int32_t* variant,
                                       const double* rows, void* stream) {
    return accumulate(m, B, n_ticks, tick0, k_first, x_path, acc, dense, variant, true, rows,
                      stream);
}

int scpqp_metrics_accumulate_posed(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                                   int32_t k_first, const double* x_path,
                                   const scpqp_metrics_acc* acc, const scpqp_metrics_dense* dense,
                                   const int32_t* variant, const double* rows, const double* pose,
                                   void* stream) {
    return accumulate_from(m, B, n_ticks, tick0, k_first, x_path, acc, dense, variant, kPosed, rows,
                           pose, stream);
}

}  // extern "C"

namespace {

// the body of the accumulate entry points of scpqp_metrics.h, scpqp_variants.h and
// scpqp_obstacles.h; with_rows: the obstacle rows of include/scpqp_obstacles.h pose the
// obstacles (rows non-NULL once there is work)
int accumulate(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0, int32_t k_first,
               const double* x_path, const scpqp_metrics_acc* acc, const scpqp_metrics_dense* dense,
               const int32_t* variant, bool with_rows, const double* rows, void* stream) {
    return accumulate_from(m, B, n_ticks, tick0, k_first, x_path, acc, dense, variant,
                           with_rows ? kRowsSrc : kConst, rows, nullptr, stream);
}

// src: where the obstacles come from (ObstSrc); kPosed reads the rows' extents and the dense
// poses [B][n_obst][n_ticks + 1][3] of include/scpqp_manoeuvres.h
int accumulate_from(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0, int32_t k_first,
                    const double* x_path, const scpqp_metrics_acc* acc,
                    const scpqp_metrics_dense* dense, const int32_t* variant, int src,
                    const double* rows, const double* pose, void* stream) {
    const bool with_rows = src != kConst;
    if (B < 0 || n_ticks < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size / n_ticks < 0");
    if (tick0 < 0) return scpqp_fail_(SCPQP_E_ARG, "tick0 < 0");
    if (k_first != 0 && k_first != 1) return scpqp_fail_(SCPQP_E_ARG, "k_first must be 0 or 1");
    const long long K = (long long)n_ticks + 1;
    if ((long long)tick0 + n_ticks > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "tick0 + n_ticks too large");
    if (!m) return scpqp_fail_(SCPQP_E_ARG, "null metrics handle");
    if (with_rows && m->n_obst < 1)
        return scpqp_fail_(SCPQP_E_ARG, "obstacle rows on a handle without obstacles");
    if (with_rows && (long long)B * m->n_obst * SCPQP_OBST_NP > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst too large");
    if (src == kPosed && (K > 0x7fffffffLL / 3 / m->n_obst ||
                          (long long)B * m->n_obst * K * 3 > 0x7fffffffLL))
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * (n_ticks + 1) * 3 too large");
    const long long per_tick = (long long)m->n_veh * NX > (long long)m->n_veh * m->n_obst
                                   ? (long long)m->n_veh * NX : (long long)m->n_veh * m->n_obst;
    const long long widest = per_tick > m->n_pair ? per_tick : m->n_pair;
    if (K > 0x7fffffffLL / widest || (long long)B * K > 0x7fffffffLL / widest)
        return scpqp_fail_(SCPQP_E_SIZE, "B * (n_ticks + 1) * items per tick too large");
    const bool any_dense = dense && (dense->gap_veh || dense->gap_obs || dense->xtrack);
    if (!acc && !any_dense)
        return scpqp_fail_(SCPQP_E_ARG, "nothing to do: null accumulator and no dense output");
    if (B == 0) return 0;
    if (!x_path) return scpqp_fail_(SCPQP_E_ARG, "null array");
    if (with_rows && !rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (src == kPosed && !pose) return scpqp_fail_(SCPQP_E_ARG, "null pose array");
    if (acc)
        if (int rc = check_acc(acc)) return rc;
    hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    const scpqp_metrics_acc a = acc ? *acc : scpqp_metrics_acc{};
    const scpqp_metrics_dense d = dense ? *dense : scpqp_metrics_dense{};
    if (src == kPosed)
        hipLaunchKernelGGL(metrics_kernel<kPosed>, dim3((unsigned)B), dim3(WAVE), 0,
                           static_cast<hipStream_t>(stream), m->dev, m->n_var, variant, n_ticks,
                           tick0, k_first, x_path, a, acc != nullptr, d, SrcArgs<kPosed>{rows, pose});
    else if (src == kRowsSrc)
        hipLaunchKernelGGL(metrics_kernel<kRowsSrc>, dim3((unsigned)B), dim3(WAVE), 0,
                           static_cast<hipStream_t>(stream), m->dev, m->n_var, variant, n_ticks,
                           tick0, k_first, x_path, a, acc != nullptr, d, SrcArgs<kRowsSrc>{rows});
    else
        hipLaunchKernelGGL(metrics_kernel<kConst>, dim3((unsigned)B), dim3(WAVE), 0,
                           static_cast<hipStream_t>(stream), m->dev, m->n_var, variant, n_ticks,
                           tick0, k_first, x_path, a, acc != nullptr, d, SrcArgs<kConst>{nullptr});
    return launched();
}

}  // namespace
