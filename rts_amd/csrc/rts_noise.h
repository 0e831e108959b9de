// rts_noise.h -- receiver noise (include/rts_amd.h: rts_cube_add_noise), evaluated on the host (rts_noise_eval) and in the noise
// kernel (rts_detect.hip: k_cube_noise) by the SAME generator: sample i of seed s is a pure function of (s, i).
//   Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): counter (lo32(i), hi32(i), 0, 0), key (lo32(s), hi32(s))
//   a = (x0 << 32 | x1) >> 11, u1 = (a + 1) 2^-53 in (0, 1];  b = (x2 << 32 | x3) >> 11, u2 = b 2^-53 in [0, 1)
//   Box-Muller: r = sqrt(-2 ln u1), n = sqrt(noise_power / 2) r (cos 2 pi u2, sin 2 pi u2): E|n|^2 = noise_power
// Rules of use (include/rts_amd.h):
//   * noise goes in after the render and before rts_cube_compress -- where thermal noise enters a receiver;
//   * with several GPUs it is added ONCE, on one handle, after rts_cube_reduce or the caller's all-reduce (else it is summed N times).
// Fixed trees of IEEE basic operations, compiled with -ffp-contract=off; log, sin and cos are the platform's (OCML on the device,
// libm on the host), so the two agree to a few ulp, not bit for bit.
// rts_noise_sample4 takes the four counter words as they are: the correlated sources (rts_source.h) draw under counter
// (bin, pulse, patch, 1), which no flat index of the cube reaches (its words 2 and 3 are 0).
// Includes nothing of HIP: the library's units bring rts_device_math.h's RTS_HD first, a host compiler gets the plain form.
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif
#ifndef RTS_PI
#define RTS_PI 3.14159265358979323846
#endif

#define RTS_PHILOX_M0 0xD2511F53u
#define RTS_PHILOX_M1 0xCD9E8D57u
#define RTS_PHILOX_W0 0x9E3779B9u
#define RTS_PHILOX_W1 0xBB67AE85u

// Philox4x32-10 of counter c[4] under key (k0, k1), in place
RTS_HD void rts_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += RTS_PHILOX_W0; k1 += RTS_PHILOX_W1; }
        const uint64_t p0 = (uint64_t)RTS_PHILOX_M0 * c[0], p1 = (uint64_t)RTS_PHILOX_M1 * c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
    }
}

// the complex sample of counter (c0, c1, c2, c3) under seed, scaled by sigma: E|n|^2 = 2 sigma^2
RTS_HD void rts_noise_sample4(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, double sigma, double* re, double* im)
{
    uint32_t c[4] = {c0, c1, c2, c3};
    rts_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t a = (((uint64_t)c[0] << 32) | c[1]) >> 11, b = (((uint64_t)c[2] << 32) | c[3]) >> 11;
    const double u1 = (double)(a + 1) * 0x1p-53, u2 = (double)b * 0x1p-53;
    const double sr = sigma * sqrt(-2.0 * log(u1));
    const double ang = 2.0 * RTS_PI * u2;
    *re = sr * cos(ang); *im = sr * sin(ang);
}

// the complex noise sample of flat index i under seed, scaled by sigma = sqrt(noise_power / 2)
RTS_HD void rts_noise_sample(uint64_t seed, uint64_t i, double sigma, double* re, double* im)
{
    rts_noise_sample4(seed, (uint32_t)i, (uint32_t)(i >> 32), 0u, 0u, sigma, re, im);
}
