// Micro-benchmark of the triangular solve (Solver of csrc/scpqp_kernel.h) alone: cycles per
// L D L' solve for n = 41, 81 (c2) and 121 (c5's Hp 30), one workgroup alone and 3 workgroups
// per CU, with n a compile-time constant (the sweeps of the compiled shapes: step indices as
// template arguments, immediate-lane capture) and with n known at run time only (rolled
// chunk loops, select capture).  Variants are tried by editing Solver.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include tools/probe/solve_probe.hip -o tools/probe/solve_probe
#include "../../senquential-convex-programming-for-trajectory-planning_amd/csrc/scpqp_kernel.h"

#include <vector>

namespace {
// CT: n compiled in (Solver's NC = N), else passed at run time (NC = 0)
template <int N, bool CT>
__global__ __launch_bounds__(256, 3) void solve_probe(double* xout, long long* cyc, int n_rt, int reps) {
    constexpr int R = (N + 63) / 64;
    const int n = CT ? N : n_rt;
    ldouble* H = (ldouble*)smem_;
    const int hsz = pad2(roff(n + 1) + 16);
    ldouble* dinv = H + hsz;
    ldouble* b = dinv + pad2(n);
    ldouble* x = b + pad2(n);
    for (int e = threadIdx.x; e < hsz; e += 256) H[e] = 0.0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        for (int j = 0; j < i; ++j) H[roff(i) + j] = 0.3 * sin(0.7 * i + 1.3 * j) / (1.0 + 0.05 * (i - j));
        H[roff(i) + i] = 1.0;
        dinv[i] = 1.0 / (1.0 + 0.01 * i);
        b[i] = cos(0.37 * i);
    }
    __syncthreads();
    if (wave_id() == 0) {
        const long long t0 = __builtin_amdgcn_s_memtime();
        for (int r = 0; r < reps; ++r) {
            Solver<R, ldouble*, kSolveChunk, (CT ? N : 0)> S(H, dinv, n, 0, b);
            S.run(x);
            __builtin_amdgcn_s_waitcnt(0);
        }
        const long long t1 = __builtin_amdgcn_s_memtime();
        if ((threadIdx.x & 63) == 0) cyc[blockIdx.x] = t1 - t0;
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < n; i += 256) xout[i] = x[i];
}
}  // namespace

template <int N, bool CT>
void run(const char* name, int grid, int reps, double* dx, long long* dc, const double* ref) {
    const size_t lds = (size_t)(pad2(roff(N + 1) + 16) + 3 * pad2(N)) * 8;
    auto k = solve_probe<N, CT>;
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, 0, dx, dc, N, reps);
    (void)hipDeviceSynchronize();
    std::vector<long long> c(grid);
    std::vector<double> x(N);
    (void)hipMemcpy(c.data(), dc, grid * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(x.data(), dx, N * 8, hipMemcpyDeviceToHost);
    double mx = 0, err = 0;
    for (int g = 0; g < grid; ++g) mx = c[g] > mx ? c[g] : mx;
    for (int i = 0; i < N; ++i) err = fmax(err, fabs(x[i] - ref[i]));
    printf("%-22s n=%3d grid=%4d: %8.0f cycles/solve (max over WGs), |x - ref| %.1e\n", name, N, grid,
           mx / reps, err);
}

template <int N>
void all(double* dx, long long* dc) {
    // host reference: L unit lower, D^-1 = dinv
    std::vector<double> L(N * N, 0.0), bb(N), y(N), xr(N);
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j < i; ++j) L[i * N + j] = 0.3 * sin(0.7 * i + 1.3 * j) / (1.0 + 0.05 * (i - j));
        bb[i] = cos(0.37 * i);
    }
    for (int i = 0; i < N; ++i) { double s = bb[i]; for (int j = 0; j < i; ++j) s -= L[i * N + j] * y[j]; y[i] = s; }
    for (int i = 0; i < N; ++i) y[i] *= 1.0 / (1.0 + 0.01 * i);
    for (int i = N - 1; i >= 0; --i) { double s = y[i]; for (int j = i + 1; j < N; ++j) s -= L[j * N + i] * xr[j]; xr[i] = s; }
    for (int grid : {1, 768}) {
        run<N, true>("Solver (n compiled in)", grid, N > 100 ? 20 : 50, dx, dc, xr.data());
        run<N, false>("Solver (run-time n)", grid, N > 100 ? 20 : 50, dx, dc, xr.data());
    }
}

int main() {
    double* dx;
    long long* dc;
    (void)hipMalloc(&dx, 512 * 8);
    (void)hipMalloc(&dc, 2048 * 8);
    all<41>(dx, dc);
    all<81>(dx, dc);
    all<121>(dx, dc);
    return 0;
}
