// Per-sample arithmetic of the simulated links and the noise generator, shared by channel.hip (one TX window
// into one RX window) and vspace.hip (many emissions into a receiver ring).
#pragma once

#include "kernels.hpp"

namespace dnrp::dev {

__device__ __forceinline__ uint64_t ch_mix(uint64_t z) {  // splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// two independent standard normals for counter c (Box-Muller on two 24-bit uniforms)
__device__ __forceinline__ float2 ch_gauss(uint64_t seed, uint64_t c) {
    const uint64_t h = ch_mix(seed ^ ch_mix(c));
    const float u1 = (static_cast<float>(h >> 40) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
    const float u2 = static_cast<float>((h >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * __logf(u1));
    float s, co;
    __sincosf(6.28318530717958647692f * u2, &s, &co);
    return make_float2(r * co, r * s);
}

// acc + one TX stream x through one link, for the RX sample at global time t (Doppler phases) at which
// the TX sample q0 arrives with zero delay; x[q] is zero outside [0, S).
//   awgn:   x[q0]                                      (channel_awgn_t::superimpose)
//   flat:   coef * x[q0]                               (channel_flat_t)
//   doubly: sum_i amp_i x[q0 - d_i] sum_j exp(j 2 pi ((t mod |P_ij|) / P_ij + phi_ij))
//           (link_t::pass_through_link, link.cpp:246-288)
// coef: this link's coefficient, taps [n_taps] / sins [n_taps][n_sin]: this link's delay line
__device__ __forceinline__ float2 ch_link_add(float2 acc, uint32_t kind, const float2* __restrict__ x, int64_t q0,
                                              int64_t S, int64_t t, const float2* __restrict__ coef,
                                              const channel_tap* __restrict__ taps,
                                              const channel_sin* __restrict__ sins, uint32_t n_taps, uint32_t n_sin) {
    if (kind == CH_DOUBLY) {
        for (uint32_t i = 0; i < n_taps; ++i) {
            const int64_t q = q0 - taps[i].delay;
            if (q < 0 || q >= S) continue;
            const float2 xv = x[q];
            float2 g = make_float2(0.f, 0.f);
            const channel_sin* sn = sins + size_t(i) * n_sin;
            for (uint32_t j = 0; j < n_sin; ++j) {
                const int64_t P = sn[j].period;
                const int64_t aP = P < 0 ? -P : P;
                const double rev = static_cast<double>(t % aP) / static_cast<double>(P) + sn[j].phase_rev;
                g = cadd(g, phasor(6.28318530717958647692 * rev));
            }
            acc = cadd(acc, cscale(cmul(xv, g), taps[i].amp));
        }
    } else {
        if (q0 < 0 || q0 >= S) return acc;
        float2 v = x[q0];
        if (kind == CH_FLAT) v = cmul(v, *coef);
        acc = cadd(acc, v);
    }
    return acc;
}

}  // namespace dnrp::dev
