// philox.hpp -- the random numbers of the Monte-Carlo closed loop (monte_carlo.hpp): Philox4x32-10 (Salmon et al., "Parallel
// random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) and Box-Muller normals.  Plain C++: the same text serves
// the library's build, a run-time compiled user model (__HIPCC_RTC__) and a host compiler.
//
// THE CONTRACT (a seeded run is repeatable across versions of this library, launch shapes, tiles and chunks):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (sample, problem, step, coordinate / 4)        sample, problem: the indices the CALLER counts from
//             (isls_mc_loop_args.sample0 / problem0 + the index inside the launch); step = 0xffffffff for the initial-state draw,
//             else the step i whose noise w_i enters x_{i+1}
//   the four output words r0..r3 give the normals of coordinates 4q .. 4q+3:
//             u_k = (r_k + 0.5) * 2^-32   (never 0 or 1)
//             z0 = sqrt(-2 ln u_0) cos(2 pi u_1),  z1 = sqrt(-2 ln u_0) sin(2 pi u_1),  z2, z3 likewise from (u_2, u_3)
//   always in fp64; an fp32 entry point rounds what it makes of them (std * z, mean + std * z).
// 32-bit uniforms: u_0 >= 2^-33, so |z| <= sqrt(2 * 33 ln 2) = 6.76: the tails are cut at about 6.8 sigma.
#pragma once

#ifndef __HIPCC_RTC__
#include <math.h>
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define ISLS_PHILOX_FN __host__ __device__ inline
#else
#define ISLS_PHILOX_FN inline
#endif

namespace isls {
namespace philox {

typedef unsigned int u32;
typedef unsigned long long u64;

struct Words {
    u32 v[4];
};

ISLS_PHILOX_FN Words philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1)
{
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n1 = (u32)p1, n2 = (u32)(p0 >> 32) ^ c3 ^ k1, n3 = (u32)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Words w;
    w.v[0] = c0; w.v[1] = c1; w.v[2] = c2; w.v[3] = c3;
    return w;
}

// the four standard normals of (seed, sample, problem, step, q = coordinate / 4)
ISLS_PHILOX_FN void normal4(u64 seed, u32 sample, u32 problem, u32 step, u32 q, double (&z)[4])
{
    const Words w = philox4x32_10(sample, problem, step, q, (u32)seed, (u32)(seed >> 32));
    const double two_m32 = 2.3283064365386963e-10, two_pi = 6.283185307179586476925286766559;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const double u1 = ((double)w.v[2 * h] + 0.5) * two_m32, u2 = ((double)w.v[2 * h + 1] + 0.5) * two_m32;
        const double r = ::sqrt(-2.0 * ::log(u1)), a = two_pi * u2;
        z[2 * h] = r * ::cos(a);
        z[2 * h + 1] = r * ::sin(a);
    }
}

}  // namespace philox
}  // namespace isls
