// Test harness (not linked into libscpqp.so): the KKT assembly and the IPM's vector phases of
// csrc/scpqp_kernel.h, each run alone on a given problem state, so that
// tests/test_gpu_qp_phases.py can hold what they leave behind to a high-precision reference
// (tests/qp_phase_mirror.py) and demand that they write nothing they do not own.
//
// One translation unit per kernel instantiation under test, -DQP_UNIT=1..6, and one with
// -DQP_UNIT=0 for the C entry points (tests/qp_phases_harness.py builds and binds them).
//
// Per case (QpCase) a workgroup of 256 threads
//   * builds the layout with lay_of from a Ctx, as every phase does;
//   * fills the launch's whole dynamic LDS and its workspace slice with a canary pattern;
//   * loads the problem state (g, the constraint rows and their table, z, dz, the seven
//     constraint-space vectors, rd, qs and the polish slot) into the plan's own layout;
//   * copies the LDS and the workspace out ("before");
//   * runs one site:
//       0  assemble(P, L, L.dd, rho)
//       1  g_apply(L, L.z, L.rp, false)        2  g_apply(L, L.z, L.rp, true)
//       3  ph_rhs_from_tv(c, rho)              4  ph_residuals(c)
//       5  ph_init_b(c)                        6  ph_back_affine_rhs(c, mu)
//       7  ph_back_update_residuals(c, smu, eta)
//   * copies the LDS and the workspace out again ("after") and the site's return value.
// The cases of a launch may differ in shape (V, O, slot horizon): each names its entry of the
// launch's parameter table.
#include "../../senquential-convex-programming-for-trajectory-planning_amd/csrc/scpqp_kernel.h"

#include <cstdint>

#ifndef QP_UNIT
#define QP_UNIT 0
#endif

struct QpCase {
    int Hb, site, pidx, lead, inoff, ooff, pad0, pad1;
    double rho, mu, smu, eta;
};
constexpr int kQpHdr = 8;   // doubles in front of a case's output: [0..3] the site's return value
constexpr int kQpUnits = 6;
constexpr int kQpSites = 8;
constexpr size_t kQpLdsLimit = 163840;
constexpr int kQpParams = 4 + 3 * SCPQP_MAX_VEH;   // uLim slackW polDelta polRho Q[] Qf[] R[]

// (HG, VG, RM, OCC, SH of the layout) of a unit; unit 3 (c5's kernel) runs the phases of the
// horizon's class (shapes 4-6), as the kernel's own dispatch does
__host__ __device__ constexpr bool qp_hg(int u) { return u >= 4; }
__host__ __device__ constexpr bool qp_vg(int u) { return u >= 2; }
__host__ __device__ constexpr int qp_rm(int u) { return u == 1 ? 1 : (u >= 5 ? 4 : 2); }
__host__ __device__ constexpr int qp_occ(int u) { return (u == 3 || u >= 5) ? 2 : 3; }
__host__ __device__ constexpr int qp_sh(int u) { return u == 2 ? 1 : (u == 3 ? 2 : (u == 6 ? 3 : 0)); }

// doubles of a case's input: g rowE rowW rowH z dz s lam rp dd sa la tv rd qs
__host__ __device__ inline int qp_in_doubles(int V, int O, int Hb) {
    const int N = V * Hb, n = N + 1, m = V * (V - 1) / 2 * Hb + V * O * Hb, mc = m + 2 * N + 1;
    return 2 * N + 4 * m + 2 * n + kVecs * mc + n + N;
}

// entry r of the row table, as setup_problem encodes it
__host__ __device__ inline int qp_rinfo(int r, int V, int O, int Hb) {
    const int mp = V * (V - 1) / 2 * Hb;
    int i, j, o, k;
    if (r < mp) {
        const int pi = r / Hb;
        k = r % Hb;
        int ii = 0, rem = pi;
        while (rem >= V - 1 - ii) { rem -= V - 1 - ii; ++ii; }
        i = ii;
        j = ii + 1 + rem;
        o = -1;
    } else {
        const int ro = r - mp;
        const int vo = ro / Hb;
        k = ro % Hb;
        i = vo / O;
        o = vo % O;
        j = -1;
    }
    return i | ((j + 1) << 8) | ((o + 1) << 16) | (k << 24);
}

typedef int (*QpLaunch)(int, const QpCase*, const DevParams*, const double*, double*, double*, int, int);

#if QP_UNIT != 0
namespace {
__device__ __forceinline__ double qp_canary(int region, int e) {
    return __longlong_as_double(0x7ff8c0de00000000ll | ((long long)region << 24) | (long long)e);
}

template <bool HG, bool VG, int RM, int OCC, int SH>
__device__ __noinline__ D4 qp_site(const QpCase& d, Ctx c) {
    const Lay<HG, VG, RM, OCC> L = lay_of<HG, VG, RM, OCC, SH>(c);
    const cParams& P = *c.P;
    D4 ret{0.0, 0.0, 0.0, 0.0};
    if (d.site == 0) {
        assemble(P, L, L.dd, d.rho);
    } else if (d.site == 1 || d.site == 2) {
        g_apply(L, L.z, L.rp, d.site == 2);
    } else if (d.site == 3) {
        ph_rhs_from_tv<HG, VG, RM, OCC, SH>(c, d.rho);
    } else if (d.site == 4) {
        ret = ph_residuals<HG, VG, RM, OCC, SH>(c);
    } else if (d.site == 5) {
        ph_init_b<HG, VG, RM, OCC, SH>(c);
    } else if (d.site == 6) {
        ret.a = ph_back_affine_rhs<HG, VG, RM, OCC, SH>(c, d.mu);
    } else {
        ret = ph_back_update_residuals<HG, VG, RM, OCC, SH>(c, d.smu, d.eta);
    }
    return ret;
}

template <bool HG, bool VG, int RM, int OCC, int SHL>
__global__ __launch_bounds__(NT, OCC) void qp_kernel(const QpCase* cases, const DevParams* Pd, const double* in,
                                                     double* out, double* wsAll, int ldsN, int wsN) {
    const QpCase d = cases[blockIdx.x];
    const int tid = threadIdx.x;
    const cParams* Pp = (const cParams*)(Pd + d.pidx);
    const cParams& P = *Pp;
    ldouble* lds = (ldouble*)smem_;
    gdouble* ws = (gdouble*)(wsAll + (size_t)blockIdx.x * wsN);
    const Ctx c{Pp, ws, d.Hb, d.lead};
    const Lay<HG, VG, RM, OCC> L = lay_of<HG, VG, RM, OCC, SHL>(c);
    for (int e = tid; e < ldsN; e += NT) lds[e] = qp_canary(1, e);
    for (int e = tid; e < wsN; e += NT) ws[e] = qp_canary(2, e);
    __syncthreads();
    const int N = L.N, n = L.n, m = L.m, mc = L.mc;
    const double* p = in + d.inoff;
    for (int e = tid; e < 2 * N; e += NT) L.g[e] = p[e];
    p += 2 * N;
    for (int e = tid; e < 2 * m; e += NT) L.rowE[e] = p[e];
    p += 2 * m;
    for (int e = tid; e < m; e += NT) {
        L.rowW[e] = p[e];
        L.rowH[e] = p[m + e];
        L.rinfo[e] = qp_rinfo(e, L.V, L.O, L.Hb);
    }
    p += 2 * m;
    for (int e = tid; e < n; e += NT) {
        L.z[e] = p[e];
        L.dz[e] = p[n + e];
    }
    p += 2 * n;
    for (int e = tid; e < mc; e += NT) {
        L.s[e] = p[e];
        L.lam[e] = p[mc + e];
        L.rp[e] = p[2 * mc + e];
        L.dd[e] = p[3 * mc + e];
        L.sa[e] = p[4 * mc + e];
        L.la[e] = p[5 * mc + e];
        L.tv[e] = p[6 * mc + e];
    }
    p += kVecs * mc;
    for (int e = tid; e < n; e += NT) L.rd[e] = p[e];
    p += n;
    for (int e = tid; e < N; e += NT) L.qs[e] = p[e];
    if (tid == 0) L.red[kIdlSlot] = 1.0 / P.polDelta;
    __syncthreads();
    double* o = out + d.ooff;
    for (int e = tid; e < ldsN; e += NT) o[kQpHdr + e] = lds[e];
    for (int e = tid; e < wsN; e += NT) o[kQpHdr + ldsN + e] = ws[e];
    __syncthreads();
    D4 ret;
    if constexpr (SHL == 2) {   // c5's kernel: the phases of the horizon's class
        if (d.Hb == 30) ret = qp_site<HG, VG, RM, OCC, 6>(d, c);
        else if (d.Hb == 20) ret = qp_site<HG, VG, RM, OCC, 5>(d, c);
        else if (d.Hb == 10) ret = qp_site<HG, VG, RM, OCC, 4>(d, c);
        else ret = qp_site<HG, VG, RM, OCC, SHL>(d, c);
    } else {
        ret = qp_site<HG, VG, RM, OCC, SHL>(d, c);
    }
    __syncthreads();
    o += kQpHdr + ldsN + wsN;
    for (int e = tid; e < ldsN; e += NT) o[e] = lds[e];
    for (int e = tid; e < wsN; e += NT) o[ldsN + e] = ws[e];
    if (tid == 0) {
        out[d.ooff] = ret.a;
        out[d.ooff + 1] = ret.b;
        out[d.ooff + 2] = ret.c;
        out[d.ooff + 3] = ret.d;
    }
}
}  // namespace

#define QP_CAT2(a, b) a##b
#define QP_CAT(a, b) QP_CAT2(a, b)
extern "C" int QP_CAT(qp_launch_, QP_UNIT)(int ncase, const QpCase* cases, const DevParams* P, const double* in,
                                           double* out, double* ws, int ldsN, int wsN) {
    auto k = qp_kernel<qp_hg(QP_UNIT), qp_vg(QP_UNIT), qp_rm(QP_UNIT), qp_occ(QP_UNIT), qp_sh(QP_UNIT)>;
    const size_t lds = (size_t)ldsN * sizeof(double);
    if (lds > kQpLdsLimit) return -1;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(ncase), dim3(NT), lds, 0, cases, P, in, out, ws, ldsN, wsN);
    return (int)hipGetLastError();
}

#else   // QP_UNIT == 0: the C entry points

extern "C" {
int qp_launch_1(int, const QpCase*, const DevParams*, const double*, double*, double*, int, int);
int qp_launch_2(int, const QpCase*, const DevParams*, const double*, double*, double*, int, int);
int qp_launch_3(int, const QpCase*, const DevParams*, const double*, double*, double*, int, int);
int qp_launch_4(int, const QpCase*, const DevParams*, const double*, double*, double*, int, int);
int qp_launch_5(int, const QpCase*, const DevParams*, const double*, double*, double*, int, int);
int qp_launch_6(int, const QpCase*, const DevParams*, const double*, double*, double*, int, int);

static bool qp_shape_ok(int unit, int V, int O, int HM) {
    if (unit < 1 || unit > kQpUnits || V < 1 || V > SCPQP_MAX_VEH || O < 0 || O > SCPQP_MAX_OBST) return false;
    if (HM < 1 || HM > SCPQP_MAX_HP) return false;
    const int n = V * HM + 1;
    if (n > 64 * qp_rm(unit)) return false;
    if (unit == 2 && (V != 4 || O != 0 || HM != 20)) return false;
    if (unit == 3 && (V != 4 || O != 0)) return false;
    if (unit == 6 && (V != 8 || O != 0 || HM != 30)) return false;
    // the plan sends W~ to the workspace exactly where the layout expects it there
    if (qp_hg(unit) && ((n + 63) / 64 == 4) != (qp_rm(unit) == 4)) return false;
    return true;
}
static Off qp_off(int unit, int V, int O, int HM) {
    return plan_offsets(V, O, HM, qp_hg(unit), qp_vg(unit), lean_plan(qp_hg(unit), qp_vg(unit), qp_occ(unit)));
}

// The plan of a unit at a shape, for the host's masks and reads: out[0..27] = LDS doubles,
// workspace doubles, the offsets g ya yb qs rowE rowW rowH rinfo z dz rhs rd dinv red H Wt vec
// pb, mcAlloc, then whether the factor / the vectors / W~ / the rows live in the workspace and
// tv in LDS, the row slots kept in registers (0: RowsMem), the reduction area's size.  0, or
// -1 for a shape the unit does not run.
int qp_plan(int unit, int V, int O, int HM, int Hb, int* out) {
    if (!qp_shape_ok(unit, V, O, HM) || Hb < 1 || Hb > HM) return -1;
    const Off f = qp_off(unit, V, O, HM);
    const bool hg = qp_hg(unit), vg = qp_vg(unit), lean = lean_plan(hg, vg, qp_occ(unit));
    const bool wg = (hg && vg && qp_rm(unit) == 4) || lean;
    int slots = 0;
    if (unit == 2) slots = row_slots<1>();
    if (unit == 6) slots = row_slots<3>();
    if (unit == 3) slots = Hb == 30 ? row_slots<6>() : (Hb == 20 ? row_slots<5>() : (Hb == 10 ? row_slots<4>() : 0));
    if (slots > kCarrySlots) slots = 0;
    const int v[28] = {f.persist + f.uni, f.ws, f.g, f.ya, f.yb, f.qs, f.rowE, f.rowW, f.rowH, f.rinfo,
                       f.z, f.dz, f.rhs, f.rd, f.dinv, f.red, f.H, f.Wt, f.vec, f.pb, f.mcAlloc,
                       hg ? 1 : 0, vg ? 1 : 0, wg ? 1 : 0, lean ? 1 : 0, tv_in_lds(hg, vg, lean) ? 1 : 0,
                       slots, red_size(hg)};
    for (int i = 0; i < 28; ++i) out[i] = v[i];
    return 0;
}
int qp_in_size(int V, int O, int Hb) { return qp_in_doubles(V, O, Hb); }
int qp_rinfo_host(int r, int V, int O, int Hb) { return qp_rinfo(r, V, O, Hb); }
int qp_roff(int i) { return roff(i); }
// the tile size assemble takes on a unit at (V, Hb): its switch, restated
int qp_tile_size(int unit, int V, int Hb) {
    if (!qp_hg(unit)) return 4;
    const int T4 = (Hb + 3) >> 2, PV = V * (V - 1) / 2;
    return V * (T4 * (T4 + 1) / 2) + PV * T4 * T4 >= 2 * NT ? 4 : 2;
}

// Run ncase cases on unit's kernel.  shapes: nshape x (V, O, HM); params: nshape x kQpParams
// doubles (uLim slackW polDelta polRho Q[] Qf[] R[]); every case names its shape (pidx) and its
// own horizon Hb <= HM (units 1, 3, 4 and 5: else Hb == HM).  ldsN / wsN: the launch's LDS
// and workspace doubles, at least every shape's own.  Output per case at ooff: kQpHdr doubles,
// then the "before" and the "after" image, each the LDS then the workspace slice.
int qp_run(int unit, int nshape, const int* shapes, const double* params, int ncase, const QpCase* cases,
           const double* in, long long nin, double* out, long long nout, int ldsN, int wsN) {
    static const QpLaunch table[kQpUnits] = {qp_launch_1, qp_launch_2, qp_launch_3,
                                             qp_launch_4, qp_launch_5, qp_launch_6};
    if (unit < 1 || unit > kQpUnits || nshape < 1 || ncase < 1 || ldsN < 1 || wsN < 0) return -2;
    if ((size_t)ldsN * sizeof(double) > kQpLdsLimit) return -6;
    for (int s = 0; s < nshape; ++s) {
        const int V = shapes[3 * s], O = shapes[3 * s + 1], HM = shapes[3 * s + 2];
        if (!qp_shape_ok(unit, V, O, HM)) return -2;
        const Off f = qp_off(unit, V, O, HM);
        if (f.persist + f.uni > ldsN || f.ws > wsN) return -6;
    }
    const bool ctH = unit == 2 || unit == 6;
    for (int c = 0; c < ncase; ++c) {
        const QpCase& d = cases[c];
        if (d.pidx < 0 || d.pidx >= nshape) return -3;
        const int V = shapes[3 * d.pidx], O = shapes[3 * d.pidx + 1], HM = shapes[3 * d.pidx + 2];
        if (d.Hb < 1 || d.Hb > HM || (ctH && d.Hb != HM)) return -3;
        if (d.lead < 0 || d.lead >= NWAVE || d.site < 0 || d.site >= kQpSites) return -3;
        if (d.inoff < 0 || d.inoff + (long long)qp_in_doubles(V, O, d.Hb) > nin) return -5;
        if (d.ooff < 0 || d.ooff + (long long)kQpHdr + 2ll * (ldsN + wsN) > nout) return -5;
    }
    DevParams* hp = (DevParams*)calloc(nshape, sizeof(DevParams));
    if (!hp) return -7;
    for (int s = 0; s < nshape; ++s) {
        const double* q = params + (size_t)s * kQpParams;
        hp[s].nV = shapes[3 * s]; hp[s].nO = shapes[3 * s + 1]; hp[s].hpMax = shapes[3 * s + 2];
        hp[s].uLim = q[0]; hp[s].slackW = q[1]; hp[s].polDelta = q[2]; hp[s].polRho = q[3];
        for (int v = 0; v < SCPQP_MAX_VEH; ++v) {
            hp[s].Q[v] = q[4 + v];
            hp[s].Qf[v] = q[4 + SCPQP_MAX_VEH + v];
            hp[s].R[v] = q[4 + 2 * SCPQP_MAX_VEH + v];
        }
    }
    QpCase* dc = nullptr;
    DevParams* dp = nullptr;
    double *din = nullptr, *dout = nullptr, *dws = nullptr;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; return r == hipSuccess; };
    const size_t wsBytes = (size_t)(wsN > 0 ? wsN : 1) * ncase * sizeof(double);
    if (chk(hipMalloc(&dc, ncase * sizeof(QpCase))) && chk(hipMalloc(&dp, nshape * sizeof(DevParams))) &&
        chk(hipMalloc(&din, nin * sizeof(double))) && chk(hipMalloc(&dout, nout * sizeof(double))) &&
        chk(hipMalloc(&dws, wsBytes)) &&
        chk(hipMemcpy(dc, cases, ncase * sizeof(QpCase), hipMemcpyHostToDevice)) &&
        chk(hipMemcpy(dp, hp, nshape * sizeof(DevParams), hipMemcpyHostToDevice)) &&
        chk(hipMemcpy(din, in, nin * sizeof(double), hipMemcpyHostToDevice)) &&
        chk(hipMemset(dout, 0, nout * sizeof(double)))) {
        const int rc = table[unit - 1](ncase, dc, dp, din, dout, dws, ldsN, wsN);
        if (rc != 0) e = rc > 0 ? (hipError_t)rc : hipErrorInvalidValue;
        else if (chk(hipDeviceSynchronize())) chk(hipMemcpy(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost));
    }
    (void)hipFree(dc); (void)hipFree(dp); (void)hipFree(din); (void)hipFree(dout); (void)hipFree(dws);
    free(hp);
    return (int)e;
}
}
#endif
