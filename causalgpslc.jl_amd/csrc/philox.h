// The library's standard normals: Philox4x32-10 + Box-Muller, one definition for the device (the draw kernels' operand
// staging, k_draws.hip) and the host (gpslc_sate_samples, gpslc_curve_samples), restated in oracle/gpslc_oracle.py:philox_normals.
// Element e of stream `stream` under `seed`: counter e >> 1 gives one Box-Muller transform, even e its cos branch, odd e its sin.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

__host__ __device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                                       unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int rd = 0; rd < 10; ++rd) {
        const unsigned long long p0 = 0xD2511F53ull * c0;
        const unsigned long long p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        const unsigned n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        const unsigned n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// radius and angle of the Box-Muller transform of counter `pair`: elements 2 pair and 2 pair + 1 are rad cos(ang) and rad sin(ang)
__host__ __device__ __forceinline__ void philox_box_muller(unsigned long long seed, unsigned long long stream,
                                                           unsigned long long pair, double& rad, double& ang) {
    unsigned w[4];
    philox4x32_10((unsigned)pair, (unsigned)(pair >> 32), (unsigned)stream, (unsigned)(stream >> 32),
                  (unsigned)seed, (unsigned)(seed >> 32), w);
    const unsigned long long A = ((unsigned long long)w[0] << 21) ^ ((unsigned long long)w[1] >> 11);
    const unsigned long long Bq = ((unsigned long long)w[2] << 21) ^ ((unsigned long long)w[3] >> 11);
    const double u1 = ((double)A + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)Bq + 0.5) * (1.0 / 9007199254740992.0);
    rad = sqrt(-2.0 * log(u1));
    ang = 6.283185307179586476925286766559 * u2;
}
__host__ __device__ __forceinline__ double philox_normal(unsigned long long seed, unsigned long long stream,
                                                         unsigned long long e) {
    double rad, ang;
    philox_box_muller(seed, stream, e >> 1, rad, ang);
    return (e & 1ull) ? rad * sin(ang) : rad * cos(ang);
}
