// Synchronisation kernels: sync_chunk_t::search() (lib/src/phy/rx/sync/sync_chunk.cpp:143-279)
// for a batch of windows, each window one chunk whose sync resampler starts with zero history.
//
//  sync_steps.hip   sync_steps_kernel and its wave / stream / pipe forms: per (window, antenna) the sync
//                   resampler (M/L polyphase, register blocks), then per step the power sum |x|^2 and
//                   the pattern-lag correlation sum x[n-P] conj(x[n]) over the step's samples
//                   (autocorrelator_detection.cpp:107-128, 152-178). These are the only per-sample
//                   passes over the window; everything after reads them.
//  sync_detect.hip  sync_detect_kernel, one WG per window, the detection / coarse-peak state machine:
//                   detection conditions on moving sums of the step values (RMS limits, front/back
//                   RMS, coarse metric band, streak; autocorrelator_detection.cpp:186-280,
//                   movsum_uw.cpp:55-74), then for every detection the per-sample coarse-peak search
//                   over one STF with the smoothed metric (autocorrelator_peak.cpp:145-264), validity,
//                   metric-weighted coarse peak time (:311-394), skip after the peak. Windowed sums are
//                   exact prefix differences in double (the reference keeps float running sums with
//                   periodic re-summation). sync_peak_kernel: the same search for the split rounds.
//  sync_fine.hip    sync_post_kernel (RMS and fractional CFO at the peak), sync_beta_kernel, sync_icfo_kernel, and
//                   sync_fine_kernel, one WG per report: CFO pre-rotation of the strongest antenna's
//                   hw-rate samples around the coarse peak and cross-correlation with every STF
//                   template (crosscorrelator.cpp:80-251) as one forward FFT plus one inverse FFT per
//                   template, argmax over the search range, N_eff_TX, fine peak.
// This header: what the three units share. Each LDS layout is one function, called by kernel and launcher.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "device_common.hpp"
#include "experiments.hpp"
#include "kernels.hpp"
#include "polyphase.hpp"
#include "taps_gen.hpp"

#ifndef DNRP_STAGE_G
#define DNRP_STAGE_G 11  // span loads in flight per thread: sync_peak's 5200-input span by 512 threads and
                         // sync_post's 2600 by 256 in one round trip (6: two)
#endif

namespace dnrp::dev {

constexpr uint32_t SYNC_THREADS = 256;
constexpr uint32_t SYNC_TILE_STEPS = 64;
constexpr uint32_t SYNC_PAD_PEAK = 32;  // samples before the coarse-peak region (weighted peak can sit left of it)

__device__ __forceinline__ int64_t floordiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// ===================================================================== resampler-class dispatch
// The sync resampler classes the kernels are instantiated for. This is the one place the rule is written.
enum sync_class : uint32_t { SYNC_CLASS_9_10_24, SYNC_CLASS_9_10_4, SYNC_CLASS_1_1, SYNC_CLASS_GENERIC };
inline sync_class sync_class_of(const sync_args& a) {
    if (a.L == 9 && a.M == 10 && a.hl == 24) return SYNC_CLASS_9_10_24;
    if (a.L == 9 && a.M == 10 && a.hl == 4) return SYNC_CLASS_9_10_4;
    if (a.L == 1 && a.M == 1) return SYNC_CLASS_1_1;
    return SYNC_CLASS_GENERIC;
}

// f(LR, MR, HLR, CT) as std::integral_constants of a's class. CT (the compiled-in 9/10 taps,
// sync_args::ct_taps) is true only for 9/10/24 and only where the caller has such a form (CT_FORM):
// without one, f is never instantiated with CT true.
template <bool CT_FORM, class F>
inline void sync_dispatch(const sync_args& a, F&& f) {
    using std::integral_constant;
    constexpr std::false_type no{};
    switch (sync_class_of(a)) {
        case SYNC_CLASS_9_10_24:
            if constexpr (CT_FORM)
                if (a.ct_taps) return f(integral_constant<int, 9>{}, integral_constant<int, 10>{}, integral_constant<int, 24>{}, std::true_type{});
            f(integral_constant<int, 9>{}, integral_constant<int, 10>{}, integral_constant<int, 24>{}, no);
            break;
        case SYNC_CLASS_9_10_4:
            f(integral_constant<int, 9>{}, integral_constant<int, 10>{}, integral_constant<int, 4>{}, no);
            break;
        case SYNC_CLASS_1_1:
            f(integral_constant<int, 1>{}, integral_constant<int, 1>{}, integral_constant<int, 0>{}, no);
            break;
        default:
            f(integral_constant<int, 0>{}, integral_constant<int, 0>{}, integral_constant<int, 0>{}, no);
    }
}

// ===================================================================== LDS layouts
struct sync_shared {  // block scalars, at the start of the dynamic LDS (no static __shared__)
    double red[24];
    int s_min;
    float s_rms, s_metric;
    uint32_t s_ant;
    float s_pk_metric[8];
    uint32_t s_pk_idx[8];
};
constexpr uint32_t SYNC_SHARED_F2 = (sizeof(sync_shared) + 15) / 16 * 2;  // float2 slots, 16-B multiple

// float2 slots of the LDS copy of the block taps (npp floats, 16-B multiple)
__host__ __device__ __forceinline__ uint32_t sync_tap_f2(uint32_t npp) { return (npp + 3) / 4 * 2; }

__host__ __device__ inline uint32_t sync_stage_cap(uint32_t L, uint32_t M, uint32_t hl, uint32_t cnt) {
    if (L <= 1) return 0;
    const uint32_t W = hl + 1 + ((L - 1) * M) / L;
    return M * (cnt / L + 2) + W + M;
}

// sync_detect_kernel's detection staging: per antenna det_c correlations (float2) of a batch of
// SYNC_THREADS steps with the lookback, all antennas' rows, then det_p powers (float) each
struct sync_det_lds {
    uint32_t det_p, det_c;
    __host__ __device__ size_t bytes(uint32_t n_ant) const { return n_ant * (det_c * sizeof(float2) + det_p * sizeof(float)); }
};
__host__ __device__ __forceinline__ sync_det_lds sync_det_layout(uint32_t np, uint32_t nc) {  // np = 4 n_pattern, nc = 4 n_uw
    return {(SYNC_THREADS + np + 3) / 4 * 4, SYNC_THREADS + nc};
}

// the inline peak search's arrays (peak_search), aliasing the resampler stage: n16 double2 correlation
// prefixes, n16 double power prefixes (the 16-sample grid), then D float metrics
__host__ __device__ __forceinline__ uint32_t sync_peak_n16(uint32_t region) { return (region + 15) / 16 + 2; }

// resample_staged's staged inputs for nb polyphase blocks. The kernel has the exact nb of its outputs; the
// launchers size by their bound on nb and a block to spare (sync_peak_ok, sync_post_lds)
template <int LR, int MR, int HLR>
__host__ __device__ constexpr uint32_t sync_staged_n_in(uint32_t nb) { return MR * (nb - 1) + pp_direct<LR, MR, HLR>::W; }

// the fine search's LDS (sync_fine_body) behind its 16-slot header: one buffer of nbuf slots where the
// transform runs in place (radix 8 at 4096 points, radix 4 at the other powers of 4; bank-padded),
// else the two buffers of the Stockham passes. r8: DNRP_FINE_R8 of the caller.
struct sync_fine_lds {
    uint32_t nf;  // points
    bool ip, r8;  // in place by radix 4; by radix 8
    __host__ __device__ __forceinline__ uint32_t nbuf() const { return r8 ? R8_SLOTS : ip ? nf + nf / 32 : nf; }
    __host__ __device__ __forceinline__ uint32_t slots() const { return 16 + (r8 || ip ? nbuf() : 2 * nbuf()); }  // float2 of the launch
};
__host__ __device__ __forceinline__ sync_fine_lds sync_fine_layout(uint32_t log2_fft, bool r8) {
    return {1u << log2_fft, (log2_fft & 1u) == 0, r8 && log2_fft == 12};
}

// ===================================================================== device helpers
// The step sums are computed in tranches [A.s_lo, A.s_hi) (host loop of dnrp_rx_sync_batch), the
// detection running up to the frontier between them. From the second tranche of a call on (A.skip)
// a window whose search has finished (max_reports reached: pend == 2) needs no further step values:
// its waves leave at once. w is wave-uniform (w < n_win checked by the caller), so this is one scalar
// load. The first tranche never reads the state: it is not initialised yet (A.first).
__device__ __forceinline__ bool sync_window_done(const sync_args& A, uint32_t w) {
    return A.skip && A.state[w].pend == 2u;
}

// output y >= 0 of the generic L/M resampler (os_min 4/8) as a direct FIR on x[0, S), zero history, added to acc
__device__ __forceinline__ void sync_fir_generic(const sync_args& A, const float2* __restrict__ x, int64_t y, int64_t S, float2& acc) {
    const uint64_t t = A.delay + static_cast<uint64_t>(y) * A.M;
    const int64_t p = static_cast<int64_t>(t / A.L);
    const uint32_t ph = static_cast<uint32_t>(t % A.L);
    for (uint32_t d = 0; d <= A.hl; ++d) {
        const int64_t q = p - d;
        if (q < 0 || q >= S) continue;
        const float h = A.taps[ph + d * A.L];
        acc.x = fmaf(x[q].x, h, acc.x);
        acc.y = fmaf(x[q].y, h, acc.y);
    }
}

// one polyphase block's outputs mb .. mb + LR - 1 clipped to [y0, y0 + cnt): put(m - y0, value), zero
// for the outputs m < 0 (before the stream)
template <int LR, class PUT>
__device__ __forceinline__ void sync_emit_block(int64_t mb, int64_t y0, uint32_t cnt, const float2 (&y)[LR], const PUT& put) {
#pragma unroll
    for (int k = 0; k < LR; ++k) {
        const int64_t idx = mb + k - y0;
        if (idx >= 0 && idx < static_cast<int64_t>(cnt))
            put(idx, (mb + k >= 0) ? y[k] : make_float2(0.f, 0.f));
    }
}

// step sums of one sample v = x[n] and its pattern lag u = x[n - P]: power, and u conj(v)
__device__ __forceinline__ void ss_power(float2 v, float& pw) { pw = fmaf(v.x, v.x, fmaf(v.y, v.y, pw)); }
__device__ __forceinline__ void ss_corr(float2 u, float2 v, float2& c) {
    c.x = fmaf(u.x, v.x, fmaf(u.y, v.y, c.x));
    c.y = fmaf(u.y, v.x, fmaf(-u.x, v.y, c.y));
}

// sums over the G (2 or 4) adjacent lanes that share a step
template <int G>
__device__ __forceinline__ void ss_group_sum(float& pw, float2& c) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        pw += __shfl_xor(pw, o);
        c.x += __shfl_xor(c.x, o);
        c.y += __shfl_xor(c.y, o);
    }
}

// lb[y] for y in [y0, y0 + cnt) of one antenna (input x[i] valid for i in [0, S_win), zero history)
// into dst[y - y0]. taps: LDS block taps (pp path) or the global natural taps (generic path).
// Whole block participates; ends with a barrier.
template <int LR, int MR, int HLR>
__device__ void sync_resample(const sync_args& A, const float2* __restrict__ x, int64_t y0, uint32_t cnt,
                              float2* stage, float2* dst, const float* taps, uint32_t stage_cap = 0xFFFFFFFFu) {
    const int64_t S = A.S_win;
    if constexpr (LR == 1) {
        stage_span<8>(dst, x, y0, cnt, S, threadIdx.x, blockDim.x);
        __syncthreads();
    } else if constexpr (LR == 0) {  // generic L/M (os_min 4/8): direct FIR per output
        for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
            const int64_t y = y0 + i;
            float2 acc = make_float2(0.f, 0.f);
            if (y >= 0) sync_fir_generic(A, x, y, S, acc);
            dst[i] = acc;
        }
        __syncthreads();
    } else {
        using PB = pp_block<LR, MR, HLR>;
        const int64_t ms = A.m_star;
        const int64_t q0 = floordiv(y0 - ms, LR), q1 = floordiv(y0 + cnt - ms + LR - 1, LR);
        // pieces of nbp blocks whose input span fits the stage (stage_cap float2)
        const int64_t nbp = stage_cap >= static_cast<uint32_t>(PB::W) + MR ? (stage_cap - PB::W) / MR + 1 : 1;
        for (int64_t qa = q0; qa < q1; qa += nbp) {
            const int64_t qe = min(qa + nbp, q1);
            const int64_t in0 = static_cast<int64_t>(A.p_star) + MR * qa - HLR;
            const uint32_t n_in = static_cast<uint32_t>(MR * (qe - 1 - qa) + PB::W);
            stage_span<8>(stage, x, in0, n_in, S, threadIdx.x, blockDim.x);
            __syncthreads();
            for (int64_t q = qa + threadIdx.x; q < qe; q += blockDim.x) {
                float2 yv[LR];
                PB::run(stage + MR * (q - qa), taps, yv);
                sync_emit_block<LR>(ms + LR * q, y0, cnt, yv, [&](int64_t i, float2 v) __attribute__((always_inline)) { dst[i] = v; });
            }
            __syncthreads();
        }
    }
}

// lb[y] for y in [y0, y0 + cnt) of one antenna straight from the window (no LDS staging): each thread
// one polyphase block of L outputs from its W inputs by range-checked buffer loads (zeros outside
// [0, S_win)), put(i, lb[y0 + i]). sync_resample's outputs bit for bit (pp_direct / pp_const sum in
// pp_block's order). CT: the compile-time 9/10 sync taps. No barrier.
template <int LR, int MR, int HLR, bool CT, class PUT>
__device__ __forceinline__ void resample_direct(const sync_args& A, const float2* x, int64_t y0, uint32_t cnt, PUT put) {
    const uint32_t tid = threadIdx.x, T = blockDim.x;
    if constexpr (LR > 1) {
        using PD = pp_direct<LR, MR, HLR>;
        constexpr int W = PD::W;
        const int64_t ms = A.m_star;
        const int64_t q0 = floordiv(y0 - ms, LR), q1 = floordiv(y0 + cnt - ms + LR - 1, LR);
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(x), 0, static_cast<int>(A.S_win * 8u), 0x00020000);
        for (int64_t q = q0 + tid; q < q1; q += T) {
            const int64_t in0 = static_cast<int64_t>(A.p_star) + MR * q - HLR;
            float2 xv[W];
#pragma unroll
            for (int i = 0; i < W; ++i)  // outside [0, S_win): the range check returns zeros
                xv[i] = buffer_load_f2<0>(xr, static_cast<uint32_t>((in0 + i) * 8));
            float2 y[LR];
            if constexpr (CT) {
                static_assert(taps_sync_9_10::L == LR && taps_sync_9_10::M == MR && taps_sync_9_10::HL == HLR, "taps");
                pp_const<taps_sync_9_10>::run(xv, y);
            } else {
                const float* tp = A.taps;
                asm volatile("" : "+s"(tp));
                PD::run(xv, (ctap_ptr)(tp), y);
            }
            sync_emit_block<LR>(ms + LR * q, y0, cnt, y, put);
        }
    } else {
        for (uint32_t i = tid; i < cnt; i += T) {
            const int64_t yy = y0 + i;
            float2 acc = make_float2(0.f, 0.f);
            if constexpr (LR == 1) {
                if (yy >= 0 && yy < static_cast<int64_t>(A.S_win)) acc = x[yy];
            } else if (yy >= 0) {  // generic L/M: sync_resample's direct FIR
                sync_fir_generic(A, x, yy, static_cast<int64_t>(A.S_win), acc);
            }
            put(i, acc);
        }
    }
}

// resample_direct for one workgroup with the window span staged in LDS first: the span's inputs
// [ib0, ib0 + n_in) are read by all threads together (coalesced, range-checked: zeros outside
// [0, S_win)) into stage[], then every thread takes the FIR windows of at most two blocks from LDS
// (its own and one tail block -- 9 region outputs per block, so a region of stf_len + D + pad =
// 4640 outputs is 517 blocks for 512 threads), computes them into registers, and after a barrier
// (every window read: stage[] may alias the outputs' slots) hands the outputs to put. One global
// load latency instead of two (the tail blocks' second round), the same sums as resample_direct.
// Preconditions (host, sync_peak_ok and sync_post_lds): blocks <= 2 T, n_in <= the stage's capacity.
template <int LR, int MR, int HLR, bool IMAJ = false, class PUT>
__device__ __forceinline__ void resample_staged(const sync_args& A, const float2* x, int64_t y0, uint32_t cnt,
                                                float2* stage, PUT put) {
    using PD = pp_direct<LR, MR, HLR>;
    constexpr int W = PD::W;
    const uint32_t tid = threadIdx.x, T = blockDim.x;
    const int64_t ms = A.m_star;
    const int64_t q0 = floordiv(y0 - ms, LR), q1 = floordiv(y0 + cnt - ms + LR - 1, LR);
    const uint32_t nb = static_cast<uint32_t>(q1 - q0);
    const int64_t ib0 = static_cast<int64_t>(A.p_star) + MR * q0 - HLR;
    const uint32_t n_in = sync_staged_n_in<LR, MR, HLR>(nb);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(x), 0, static_cast<int>(A.S_win * 8u), 0x00020000);
    // indices past the stream end read a range-checked zero; a negative start wraps into the
    // descriptor's "outside" range as well (offsets are unsigned)
    constexpr uint32_t G = DNRP_STAGE_G;  // loads in flight per thread and group
    for (uint32_t i0 = 0; i0 < n_in; i0 += G * T) {
        float2 v[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const int64_t q = ib0 + i0 + g * T + tid;
            v[g] = buffer_load_f2<0>(xr, q >= 0 ? static_cast<uint32_t>(q * 8) : 0x80000000u);
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g)
            if (i0 + g * T + tid < n_in) stage[i0 + g * T + tid] = v[g];
    }
    __syncthreads();
    float2 y[LR], y2[LR];
    const uint32_t b2 = tid + T;
    if constexpr (IMAJ) {  // windows input-major from LDS (stage 16-B aligned, MR even)
        if (tid < nb) pp_const<taps_sync_9_10>::run_imaj(stage + MR * tid, y);
        if (b2 < nb) pp_const<taps_sync_9_10>::run_imaj(stage + MR * b2, y2);
    } else {
        if (tid < nb) {
            float2 xv[W];
            PD::template load<false>(stage + MR * tid, xv);
            pp_const<taps_sync_9_10>::run(xv, y);
        }
        if (b2 < nb) {
            float2 xv[W];
            PD::template load<false>(stage + MR * b2, xv);
            pp_const<taps_sync_9_10>::run(xv, y2);
        }
    }
    __syncthreads();  // every window read before the outputs overwrite the stage
    if (tid < nb) sync_emit_block<LR>(ms + LR * (q0 + tid), y0, cnt, y, put);
    if (b2 < nb) sync_emit_block<LR>(ms + LR * (q0 + b2), y0, cnt, y2, put);
}

}  // namespace dnrp::dev
