// Simulated wireless channel on the GPU (lib/src/simulation/wireless: channel_awgn.cpp, channel_flat.cpp,
// channel_doubly.cpp + link.cpp, hardware/noise.cpp): n TX windows (dnrp_tx_batch output) through
// N_TX x N_RX links into RX windows. One thread per RX output sample:
//   y_r[n] = noise_r[n] + g * sum_tx h_{r,tx}(x_tx, n - off)
//   awgn:   h = x[n]                                        (channel_awgn_t::superimpose)
//   flat:   h = c_{r,tx} x[n]                               (channel_flat_t, Rayleigh coefficient)
//   doubly: h = sum_i sqrt(p_i / N_sin) x[n - d_i] sum_j exp(j (2 pi ((t mod |P_ij|) / P_ij) + phi_ij))
//           t = t0 + n (global hw time), tapped delay line with N_sin sinusoids per tap
//           (link_t::pass_through_link, link.cpp:246-288; the rotator's per-block restart folded
//           into the per-sample phase)
// The per-sample link sum and the noise generator are channel_dev.hpp's (shared with vspace.hip).
// Noise: complex Gaussian, standard deviation sigma per component (srsRAN ch_awgn as noise.cpp
// configures it), from a counter-based generator (seed, window, antenna, sample): reproducible and
// independent of the launch geometry.
#include "channel_dev.hpp"

namespace dnrp::dev {

constexpr uint32_t CH_THREADS = 256;

__global__ void __launch_bounds__(CH_THREADS) channel_kernel(channel_args A) {
    const uint32_t row = blockIdx.y, w = row / A.N_RX, r = row % A.N_RX;
    const uint32_t n = blockIdx.x * CH_THREADS + threadIdx.x;
    if (n >= A.S_rx) return;
    const int64_t off = A.offset[w];
    const int64_t t = A.t0[w] + n;
    float2 acc = make_float2(0.f, 0.f);
    for (uint32_t tx = 0; tx < A.N_TX; ++tx) {
        const size_t link = size_t(w) * A.N_RX * A.N_TX + r * A.N_TX + tx;
        acc = ch_link_add(acc, A.kind, A.tx + (size_t(w) * A.N_TX + tx) * A.S_tx, static_cast<int64_t>(n) - off, A.S_tx, t,
                          A.coef + link, A.taps + link * A.n_taps, A.sins + link * A.n_taps * A.n_sin, A.n_taps, A.n_sin);
    }
    acc = cscale(acc, A.large_scale);
    if (A.sigma > 0.f) {
        const float2 z = ch_gauss(A.seed, (uint64_t(row) << 32) | n);
        acc = make_float2(fmaf(A.sigma, z.x, acc.x), fmaf(A.sigma, z.y, acc.y));
    }
    A.rx[size_t(row) * A.S_rx + n] = acc;
}

hipError_t launch_channel(const channel_args& a, uint32_t n, hipStream_t st) {
    const uint64_t rows = uint64_t(n) * a.N_RX;
    if (rows == 0 || a.S_rx == 0) return hipSuccess;
    if (rows > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(channel_kernel, dim3((a.S_rx + CH_THREADS - 1) / CH_THREADS, static_cast<uint32_t>(rows)),
                       dim3(CH_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace dnrp::dev
