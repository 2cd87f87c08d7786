// scpqp_philox.h — Philox4x32-10 and the normal pair of one right-hand-side
// evaluation (device side of include/scpqp_noise.h, which fixes the key, the
// counter layout and the uniform / Box-Muller mapping).
#ifndef SCPQP_PHILOX_H
#define SCPQP_PHILOX_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace scpqp_noise_dev {

// Salmon et al., SC'11: c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
// the key bumped by (W0, W1) between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
        k0 += W0;
        k1 += W1;
    }
}

// the raw uniforms of one call's four words (include/scpqp_noise.h): u1 in (0, 1],
// u2 in [0, 1)
__device__ __forceinline__ void uniforms(const uint32_t (&c)[4], double& u1, double& u2) {
    const uint64_t a = (((uint64_t)c[0] << 32) | c[1]) >> 11;
    const uint64_t b = (((uint64_t)c[2] << 32) | c[3]) >> 11;
    u1 = (double)(a + 1) * 0x1p-53;
    u2 = (double)b * 0x1p-53;
}

// the stream of one lane: key, (c1, c2, c3) and the running evaluation index c0
struct Stream {
    uint32_t k0, k1, c0, c1, c2, c3;
    double sigma;
};

__device__ __forceinline__ Stream make_stream(uint64_t seed, double sigma, uint32_t epoch,
                                              uint32_t site, uint32_t k, uint32_t v,
                                              uint32_t b_global) {
    return Stream{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, epoch, (site << 24) | (k << 8) | v,
                  b_global, sigma};
}

// the two draws of evaluation s.c0 (sigma z0, sigma z1); advances c0.  The + 0.0
// turns a -0.0 (sigma = 0, z < 0) into the +0.0 the noise-free path adds.
__device__ __forceinline__ void draw(Stream& s, double& n0, double& n1) {
    uint32_t c[4] = {s.c0, s.c1, s.c2, s.c3};
    philox4x32_10(c, s.k0, s.k1);
    ++s.c0;
    const uint64_t a = (((uint64_t)c[0] << 32) | c[1]) >> 11;
    const uint64_t b = (((uint64_t)c[2] << 32) | c[3]) >> 11;
    const double u1 = (double)(a + 1) * 0x1p-53;   // (0, 1]
    const double u2 = (double)b * 0x1p-53;         // [0, 1)
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    n0 = s.sigma * (r * cs) + 0.0;
    n1 = s.sigma * (r * sn) + 0.0;
}

}  // namespace scpqp_noise_dev

#endif  // SCPQP_PHILOX_H
