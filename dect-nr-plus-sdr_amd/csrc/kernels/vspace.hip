// Virtual space on the GPU (lib/src/simulation/vspace.cpp:449-513 wchannel_execute, then the simulated
// radio's ADC, lib/src/radio/hw_simulator.cpp:710-733 with simulation/hardware/clip.cpp, quantize.cpp):
// every emission through its link, superimposed into the receiver's per-antenna ring at global time t:
//   s_r(t)  = sum over foreign emissions e, in em order, of g_e link_e(r, x_e, t - t_start_e)
//   s_r(t)  = 0 while an own emission is on the air (the RX path is detached, vspace.cpp:477-479)
//   s_r(t) += the own emissions through their links (TX into RX leakage, vspace.cpp:487)
//   y_r(t)  = s_r(t) + sigma z_r(t)                        (noise after the superposition, 489-498)
//   ring[r][t % ring_len] = adc(y_r(t))                    (clamp, then roundf(y / step) * step)
// One workgroup per (tile of VS_TILE span samples, antenna). The tile's emission list (host-built CSR,
// uniform across the workgroup) is walked per sample; a sample's value depends on its global time
// alone -- which emissions cover it, the Doppler phases, the noise counter (seed, antenna, all 64 bits
// of t) -- never on the tile it fell into, so any split of a span over several launches writes the same
// bits. Each lane owns VS_PAIRS pairs of consecutive samples and stores each sample once: 16-B stores
// where the span start, the ring length and the row base keep pairs contiguous and aligned, 8-B
// otherwise (the choice ring.hip makes for its loads). Nothing is read from the ring; a tile may hold
// the ring's wrap point (the span is at most one ring turn: one wrap).
#include "channel_dev.hpp"

namespace dnrp::dev {

// s + g * (emission m through its N_TX links into antenna r at global time t)
__device__ __forceinline__ float2 vs_add(const vspace_args& A, float2 s, const vspace_em& m, uint32_t r, int64_t t) {
    float2 v = make_float2(0.f, 0.f);
    for (uint32_t tx = 0; tx < A.N_TX; ++tx) {
        const size_t link = (size_t(m.slot) * A.N_RX + r) * A.N_TX + tx;
        v = ch_link_add(v, A.kind, A.tx + (size_t(m.tx_row) * A.N_TX + tx) * A.S_tx, t - m.t_start, m.length, t,
                        A.coef + link, A.taps + link * A.n_taps, A.sins + link * A.n_taps * A.n_sin, A.n_taps, A.n_sin);
    }
    return make_float2(fmaf(m.g, v.x, s.x), fmaf(m.g, v.y, s.y));
}

__device__ __forceinline__ float2 vs_sample(const vspace_args& A, uint32_t r, uint64_t seed_r, int64_t t, uint32_t e0,
                                            uint32_t e1, uint32_t o0, uint32_t o1) {
    float2 s = make_float2(0.f, 0.f);
    for (uint32_t e = e0; e < e1; ++e) {
        const vspace_em& m = A.em[A.em_idx[e]];
        if (!m.own) s = vs_add(A, s, m, r, t);
    }
    bool detached = false;
    for (uint32_t o = o0; o < o1; ++o) {
        const vspace_em& m = A.em[A.own_idx[o]];
        const int64_t q = t - m.t_start;
        detached = detached || (q >= 0 && q < static_cast<int64_t>(m.length));
    }
    if (detached) s = make_float2(0.f, 0.f);
    for (uint32_t e = e0; e < e1; ++e) {
        const vspace_em& m = A.em[A.em_idx[e]];
        if (m.own) s = vs_add(A, s, m, r, t);
    }
    // an emission listed for the tile that does not reach this sample added +0: one sign for a zero sum,
    // whichever emissions the tile listed
    s = make_float2(s.x + 0.0f, s.y + 0.0f);
    if (A.sigma > 0.f) {
        const float2 z = ch_gauss(seed_r, static_cast<uint64_t>(t));
        s = make_float2(fmaf(A.sigma, z.x, s.x), fmaf(A.sigma, z.y, s.y));
    }
    if (A.clip > 0.f) {
        s = make_float2(fminf(fmaxf(s.x, -A.clip), A.clip), fminf(fmaxf(s.y, -A.clip), A.clip));
        // a correctly rounded division, as quantize.cpp's: a reciprocal multiply rounds some quotients the other way
        if (A.step > 0.f) s = make_float2(roundf(__fdiv_rn(s.x, A.step)) * A.step, roundf(__fdiv_rn(s.y, A.step)) * A.step);
    }
    return s;
}

__global__ void __launch_bounds__(VS_THREADS) vspace_kernel(vspace_args A) {
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const uint32_t e0 = A.em_off[tile], e1 = A.em_off[tile + 1], o0 = A.own_off[tile], o1 = A.own_off[tile + 1];
    const uint64_t b0 = static_cast<uint64_t>(A.t_begin) % A.ring_len;
    float2* row = A.ring + size_t(r) * A.ant_stride;
    // span sample i (even) and i + 1 at ring samples b0 + i, b0 + i + 1: adjacent, 16-B aligned, no wrap between
    const bool pairs = ((b0 | A.ring_len) & 1u) == 0 && (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    const uint64_t seed_r = ch_mix(A.seed ^ (0x616E74656E6E6100ull + r));  // "antenna" r: its own noise stream
#pragma unroll
    for (uint32_t j = 0; j < VS_PAIRS; ++j) {
        const uint64_t i = uint64_t(tile) * VS_TILE + 2ull * (j * VS_THREADS + threadIdx.x);
        if (i >= A.n_samples) continue;
        const bool two = i + 1 < A.n_samples;
        const float2 y0 = vs_sample(A, r, seed_r, A.t_begin + static_cast<int64_t>(i), e0, e1, o0, o1);
        float2 y1 = make_float2(0.f, 0.f);
        if (two) y1 = vs_sample(A, r, seed_r, A.t_begin + static_cast<int64_t>(i) + 1, e0, e1, o0, o1);
        uint64_t q0 = b0 + i, q1 = b0 + i + 1;  // < 2 ring_len: b0 < ring_len, i + 1 < n_samples <= ring_len
        if (q0 >= A.ring_len) q0 -= A.ring_len;
        if (q1 >= A.ring_len) q1 -= A.ring_len;
        if (pairs && two) {
            *reinterpret_cast<float4*>(row + q0) = make_float4(y0.x, y0.y, y1.x, y1.y);
        } else {
            row[q0] = y0;
            if (two) row[q1] = y1;
        }
    }
}

hipError_t launch_vspace(const vspace_args& a, uint32_t n_tiles, hipStream_t st) {
    if (n_tiles == 0 || a.N_RX == 0) return hipSuccess;
    if (a.N_RX > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vspace_kernel, dim3(n_tiles, a.N_RX), dim3(VS_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace dnrp::dev
