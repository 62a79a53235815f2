// Coarse-peak post-processing, beta, integer CFO and fine peak of the synchronisation (sync_common.hpp).
#include "sync_common.hpp"

// ---- compile-time knobs (-D), shipped values
#ifndef DNRP_POST_STAGED
#define DNRP_POST_STAGED 1  // sync_post_kernel with compiled-in taps: the STF's input span staged in LDS first
                            // (resample_staged, 8 waves per SIMD; 0: straight from the window)
#endif
#ifndef DNRP_FINE_WPE
#define DNRP_FINE_WPE 1  // waves per SIMD the register budget must allow (1: the compiler's choice; radix 8
                         // at 8: 64 VGPRs + 160 B of spills, 1.55-1.57 ms per C4 chunk against 1.50-1.51
                         // at the compiler's 113 VGPRs)
#endif
#ifndef DNRP_FINE_R8
#define DNRP_FINE_R8 1  // 4096-point transforms by fft_r8_4096 (four radix-8 passes; 0: six radix-4 passes):
                        // sync_fine 1.63-1.65 -> 1.50-1.51 ms per C4 chunk (same box)
#endif
#ifndef DNRP_FINE_BATCH
#define DNRP_FINE_BATCH 8  // spectrum x template loads in flight per thread (1: one per loop iteration)
#endif

namespace dnrp::dev {

// ===================================================================== coarse-peak post-processing
// autocorrelator_peak.cpp:366-394 for one (report, antenna): the STF at the coarse peak resampled
// again, its power and cover-weighted pattern correlation (the same loops and block reduction the
// detection kernel ran, so the same doubles) -> rms[a] into the report and the antenna's CFO term
// m_a atan2(c_a) / P into A.post; sync_fine_kernel sums the terms in antenna order. One workgroup
// per (report, antenna) instead of four serial passes inside the detection workgroup.
template <int LR, int MR, int HLR, bool CT>
__global__ void __launch_bounds__(SYNC_THREADS) __attribute__((amdgpu_waves_per_eu(CT && DNRP_POST_STAGED ? 8 : 1))) sync_post_kernel(sync_args A) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    double* red = reinterpret_cast<double*>(smem);  // [24]
    float2* lbuf = smem + 12;  // 16-B aligned (resample_staged's stage)
    const uint32_t rep = blockIdx.x / A.n_ant, a = blockIdx.x % A.n_ant, w = rep / A.max_reports;
    sync_res* rp = A.res + rep;
    const float m = rp->coarse_metric[a];
    if (!rp->found || !(m > 0.f)) return;  // uniform: the whole workgroup leaves
    const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
    // the STF at the coarse peak (sync_resample's values): compiled-in 9/10 taps -> the span staged in
    // LDS and the FIR input-major from it (DNRP_POST_STAGED, 8 waves per SIMD), else straight from the window
    if constexpr (CT && LR == 9 && DNRP_POST_STAGED)
        resample_staged<LR, MR, HLR, true>(A, x, rp->coarse_local, A.stf_len, lbuf, [&](uint32_t i, float2 v) { lbuf[i] = v; });
    else
        resample_direct<LR, MR, HLR, CT>(A, x, rp->coarse_local, A.stf_len, [&](uint32_t i, float2 v) { lbuf[i] = v; });
    __syncthreads();
    double cr = 0.0, ci = 0.0, pw = 0.0;
    const uint32_t Lw = A.pattern * A.n_uw;
    for (uint32_t i = threadIdx.x; i < A.stf_len; i += blockDim.x) {
        pw += cnorm(lbuf[i]);
        if (i < Lw) {
            const float2 c = cmulc(lbuf[i], lbuf[i + A.pattern]);
            const float u = A.uw[i / A.pattern];
            cr += u * static_cast<double>(c.x);
            ci += u * static_cast<double>(c.y);
        }
    }
    block_sum3(pw, cr, ci, red);
    if (threadIdx.x == 0) {
        rp->rms[a] = sqrtf(static_cast<float>(pw) / static_cast<float>(A.stf_len));
        A.post[size_t(rep) * 8 + a] = m * atan2f(static_cast<float>(ci), static_cast<float>(cr)) / static_cast<float>(A.pattern);
    }
}

// ===================================================================== beta at the coarse peak
// coarse_peak_f_domain_t::process (coarse_peak_f_domain.cpp:70-92) for one (report, antenna), launched
// only with the beta search on: the last N = 64 bos samples of the STF at the coarse peak (the samples
// sync_post_kernel resamples, from N_samples_STF_CP_only_os on; no CFO correction, as the reference),
// their N-point transform in LDS, and after the FFT shift the power of every band the decision can ask
// for: band i = the 32-bin half-bands [b_idx2b[i - 1], b_idx2b[i]) left and right of the centre. Every
// searched antenna, with or without a valid coarse peak (estimate_beta sums all nof_antennas_limited).
// Only the band powers leave; sync_fine_kernel sums them in antenna order and decides.
// SHIFT: the second pass with both searches on (sync_beta_args::shift), a form of its own so that the beta
// search alone runs the code it had.
template <int LR, int MR, int HLR, bool CT, bool SHIFT>
__global__ void __launch_bounds__(SYNC_THREADS) sync_beta_kernel(sync_args A, sync_beta_args B) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    double* red = reinterpret_cast<double*>(smem);  // [24]
    const uint32_t N = B.plan.N;
    float2* xb = smem + 12;
    float2* yb = xb + N;
    const uint32_t rep = blockIdx.x / A.n_ant, a = blockIdx.x % A.n_ant, w = rep / A.max_reports;
    const sync_res* rp = A.res + rep;
    if (!rp->found) return;  // uniform: the whole workgroup leaves
    // second pass (B.shift, launched after sync_icfo_kernel with both searches on): the reports whose decided
    // integer CFO is k != 0 get the band powers of the spectrum moved back by 4 k bins -- the transform of the
    // samples derotated by 4 k subcarriers, exactly -- in place of the first pass's; k = 0: nothing to redo
    int32_t sh = 0;
    if constexpr (SHIFT) {
        sh = 4 * sync_icfo_k(A.icfo + size_t(rep) * 8 * SYNC_ICFO_COLS, A.n_ant);
        if (sh == 0) return;  // uniform
    }
    const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
    resample_direct<LR, MR, HLR, CT>(A, x, static_cast<int64_t>(rp->coarse_local) + B.cp, N, [&](uint32_t i, float2 v) { xb[i] = v; });
    __syncthreads();
    const float2* S = fft_any<-1>(xb, yb, B.tw, B.plan);
    // FFT shift: bin k sits d = k bins right of the centre (k < N / 2) or N - 1 - k bins left of it
    double p[SYNC_BANDS] = {};
    for (uint32_t kb = threadIdx.x; kb < N; kb += blockDim.x) {
        uint32_t k = kb;
        if constexpr (SHIFT) {  // the bin this one is without the integer CFO (|sh| <= 16 < N)
            int32_t ks = static_cast<int32_t>(kb) - sh;
            ks += ks < 0 ? static_cast<int32_t>(N) : ks >= static_cast<int32_t>(N) ? -static_cast<int32_t>(N) : 0;
            k = static_cast<uint32_t>(ks);
        }
        const uint32_t h = (k < N / 2 ? k : N - 1 - k) >> 5;  // 32-bin half-band, 0 at the centre
        const uint32_t band = h < 1 ? 0u : h < 2 ? 1u : h < 4 ? 2u : h < 8 ? 3u : h < 12 ? 4u : h < 16 ? 5u : SYNC_BANDS;
        const double v = static_cast<double>(cnorm(S[kb]));
#pragma unroll
        for (uint32_t i = 0; i < SYNC_BANDS; ++i) p[i] += band == i ? v : 0.0;
    }
    block_sum3(p[0], p[1], p[2], red);
    block_sum3(p[3], p[4], p[5], red);
    if (threadIdx.x == 0) {
        float* o = B.band + (size_t(rep) * 8 + a) * SYNC_BANDS;
#pragma unroll
        for (uint32_t i = 0; i < SYNC_BANDS; ++i) o[i] = static_cast<float>(p[i]);
    }
}

// estimate_beta (coarse_peak_f_domain.cpp:94-193) on the band powers of one report, summed over the
// searched antennas in antenna order: from b = 1 the next b of b_idx2b is taken while the sideband's
// power per bin over the centre band's exceeds the threshold. The loop ends at b_max (the reference's
// runs one step further into its asserts).
__device__ uint32_t sync_beta_decide(const sync_args& A, const float* band) {
    const uint32_t b_idx2b[SYNC_BANDS] = {1, 2, 4, 8, 12, 16};
    float pw[SYNC_BANDS];
    for (uint32_t i = 0; i < SYNC_BANDS; ++i) {
        pw[i] = 0.f;
        for (uint32_t a = 0; a < A.n_ant; ++a) pw[i] += band[a * SYNC_BANDS + i];
    }
    uint32_t b_est = 1;
    float centre = pw[0];
    for (uint32_t i = 1; i < SYNC_BANDS && b_est < A.b; ++i) {
        const uint32_t n_side = (b_idx2b[i] - b_est) * 32;
        const float centre_norm = centre / static_cast<float>(b_est * 64);
        const float side_norm = pw[i] / static_cast<float>(n_side * 2);
        if (!(side_norm / centre_norm > A.beta_thr)) break;
        b_est = b_idx2b[i];
        centre += pw[i];
    }
    return b_est;
}

// fractional CFO of a report: metric-weighted antenna mean of sync_post_kernel's terms, in antenna order
__device__ __forceinline__ float sync_cfo_frac(const sync_args& A, const sync_res* rp, uint32_t rep) {
    float cfo_w = 0.f, msum = 0.f;
    for (uint32_t a = 0; a < A.n_ant; ++a) {
        const float m = rp->coarse_metric[a];
        if (!(m > 0.f)) continue;
        msum += m;
        cfo_w += A.post[size_t(rep) * 8 + a];
    }
    return cfo_w / msum;
}

// ===================================================================== integer CFO at the coarse peak
// The project's own estimator (the reference leaves it unimplemented,
// coarse_peak_f_domain.cpp:195-199), launched only with the search on, after sync_beta_kernel: the samples
// sync_beta_kernel transforms, each multiplied by its pattern's cover-sequence sign (the STF periodic again,
// its spectrum on the 4-subcarrier comb) and by the fractional-CFO correction the fine search applies, their
// N-point transform, and per candidate k the power on the STF cells of the packet's b shifted by 4 k bins:
// the comb bins 4 (i + k), 0 < |i| <= 7 b. One pass over the N / 4 comb bins, every candidate's sum in
// registers. A candidate whose cells would reach N / 2 is not searched. Scores leave as floats, -1 for the
// columns outside the range or not searched; sync_icfo_decide sums them in antenna order.
// Six waves per SIMD asked for: the compiler's own choice is 85 VGPRs and five, with the budget 78, no spills.
template <int LR, int MR, int HLR, bool CT>
__global__ void __launch_bounds__(SYNC_THREADS) __attribute__((amdgpu_waves_per_eu(6))) sync_icfo_kernel(sync_args A, sync_beta_args B) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    static_assert(3 * (SYNC_THREADS / 64) * sizeof(double) <= 12 * sizeof(float2), "block_sum3's area: the 12 slots ahead of xb");
    double* red = reinterpret_cast<double*>(smem);  // [12]: 3 sums x 4 waves (block_sum3)
    const uint32_t N = B.plan.N;
    float2* xb = smem + 12;
    float2* yb = xb + N;
    const uint32_t rep = blockIdx.x / A.n_ant, a = blockIdx.x % A.n_ant, w = rep / A.max_reports;
    const sync_res* rp = A.res + rep;
    if (!rp->found) return;  // uniform: the whole workgroup leaves
    const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
    resample_direct<LR, MR, HLR, CT>(A, x, static_cast<int64_t>(rp->coarse_local) + B.cp, N, [&](uint32_t i, float2 v) { xb[i] = v; });
    __syncthreads();
    const double cfo_frac = static_cast<double>(sync_cfo_frac(A, rp, rep));
    // cover sequence and fractional CFO in a pass of their own: inside the polyphase blocks the phasors'
    // doubles cost 18 VGPRs and a wave per SIMD
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x)
        xb[i] = cscale(cmul(xb[i], phasor(cfo_frac * static_cast<double>(i))), B.cover[i / A.pattern]);
    __syncthreads();
    const float2* S = fft_any<-1>(xb, yb, B.tw, B.plan);
    // the packet's b: the class b, or the beta decision of this report (every thread the same sums)
    const uint32_t b = A.beta_on ? sync_beta_decide(A, A.band + size_t(rep) * 8 * SYNC_BANDS) : A.b;
    const int32_t h = 7 * static_cast<int32_t>(b), nc = static_cast<int32_t>(N / 4);  // cells 4 i, 0 < |i| <= h
    double p[SYNC_ICFO_COLS] = {};
    for (int32_t c = threadIdx.x; c < nc; c += blockDim.x) {
        const int32_t cs = c < nc / 2 ? c : c - nc;  // comb index of bin 4 c, centred
        const double v = static_cast<double>(cnorm(S[4 * c]));
#pragma unroll
        for (int32_t j = 0; j < static_cast<int32_t>(SYNC_ICFO_COLS); ++j) {
            const int32_t i = cs - (j - static_cast<int32_t>(SYNC_ICFO_MAX));
            p[j] += i != 0 && i >= -h && i <= h ? v : 0.0;
        }
    }
    block_sum3(p[0], p[1], p[2], red);
    block_sum3(p[3], p[4], p[5], red);
    block_sum3(p[6], p[7], p[8], red);
    if (threadIdx.x == 0) {
        float* o = A.icfo + (size_t(rep) * 8 + a) * SYNC_ICFO_COLS;
#pragma unroll
        for (int32_t j = 0; j < static_cast<int32_t>(SYNC_ICFO_COLS); ++j) {
            const int32_t ak = abs(j - static_cast<int32_t>(SYNC_ICFO_MAX));
            o[j] = ak <= static_cast<int32_t>(A.icfo_range) && 2 * (h + ak) < nc ? static_cast<float>(p[j]) : -1.f;
        }
    }
}

// The decision of one report (sync_icfo_k, kernels.hpp) as its correction in radians per sample of the class
// rate, the sign of cfo_frac: -k 4 2 pi / N, +0 for k = 0
__device__ float sync_icfo_decide(const sync_args& A, uint32_t rep) {
    const int32_t k = sync_icfo_k(A.icfo + size_t(rep) * 8 * SYNC_ICFO_COLS, A.n_ant);
    return k == 0 ? 0.f : static_cast<float>(static_cast<double>(-k) * 8.0 * 3.14159265358979323846 / static_cast<double>(A.icfo_N));
}

// ===================================================================== fine peak
constexpr uint32_t SYNC_FINE_THREADS = 512;  // 8 waves: the FFT passes' butterflies 2 per thread

// The fine search of one workgroup (crosscorrelator.cpp:122-249), two forms:
//  ALL = false  one workgroup per report: the antenna with the largest coarse-peak metric against every
//               template, N_eff_TX and the fine peak written to the report (the reference without
//               RX_SYNC_PARAM_CROSSCORRELATOR_ALL_ANTENNAS_OR_ONLY_STRONGEST);
//  ALL = true   one workgroup per (report, antenna), blockIdx.x = rep * n_ant + a: antenna a against every
//               template, (metric, index) per template into A.fine_m / A.fine_i [rep][8][4]; workgroups of
//               reports not found and of antennas without a coarse peak leave after writing zeros, the
//               last antenna's workgroup also zeroes the rows n_ant..7. The report is only read here (the
//               CFO and b derived in registers from coarse_metric, post and band, which no workgroup of
//               this launch writes); sync_fine_combine_kernel writes it afterwards.
template <bool ALL>
__device__ __forceinline__ void sync_fine_body(const sync_args& A) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float* s_val = reinterpret_cast<float*>(smem);  // [16]
    uint32_t* s_idx = reinterpret_cast<uint32_t*>(smem + 8);  // [16]
    const uint32_t rep = ALL ? blockIdx.x / A.n_ant : blockIdx.x;
    sync_res* rp = A.res + rep;
    uint32_t best = ALL ? blockIdx.x % A.n_ant : 0u;  // the antenna searched
    float cfo_frac = 0.f;
    if constexpr (!ALL)
        if (!rp->found) return;
    const uint32_t w = rep / A.max_reports;
    if constexpr (ALL) {
        const bool live = rp->found && rp->coarse_metric[best] > 0.f;
        const uint32_t rows = best + 1 == A.n_ant ? 8 - best : 1;  // table rows this workgroup owns
        if (threadIdx.x < 4 * rows && (!live || threadIdx.x >= 4)) {
            A.fine_m[(size_t(rep) * 8 + best) * 4 + threadIdx.x] = 0.f;
            A.fine_i[(size_t(rep) * 8 + best) * 4 + threadIdx.x] = 0u;
        }
        if (!live) return;  // uniform: the whole workgroup leaves
        cfo_frac = sync_cfo_frac(A, rp, rep);
    } else {
        cfo_frac = sync_cfo_frac(A, rp, rep);
        __syncthreads();  // every thread has read the report before thread 0 updates it
        if (threadIdx.x == 0) rp->cfo_frac = cfo_frac;
        __syncthreads();
    }
    const sync_fine_lds fl = sync_fine_layout(A.log2_fft, DNRP_FINE_R8);
    const uint32_t nf = fl.nf;
    // beta search on (kernel argument, uniform): the packet's b from sync_beta_kernel's band powers, every
    // thread the same sums in the same order; the templates below are the row block of that b
    const float2* tmpl = A.tmpl_f;
    if (A.beta_on) {
        const uint32_t b_est = sync_beta_decide(A, A.band + size_t(rep) * 8 * SYNC_BANDS);
        const uint32_t b_idx = b_est <= 2 ? b_est - 1 : b_est / 4 + 1;  // b2b_idx: 1 2 4 8 12 16 -> 0..5
        tmpl += static_cast<size_t>(b_idx) * A.n_templates * nf;
        if constexpr (!ALL)
            if (threadIdx.x == 0) rp->b = b_est;
    }
    // power-of-4 sizes (4096 for C3 / C4): in-place radix-4 DIT on one LDS buffer, the inputs stored
    // at their base-4 digit-reversed positions (ip); otherwise the two-buffer Stockham passes
    const bool ip = fl.ip;
    const bool r8 = fl.r8;  // C3 / C4: radix 8, four passes
    // in place: bank-padded slots (r4pad / r8pad), inputs written at their digit-reversed slots
    auto ix = [&](uint32_t i) { return r8 ? r8pad(rev8(i)) : ip ? r4pad(rev4(i, A.log2_fft)) : i; };
    auto ox = [&](uint32_t i) { return r8 ? r8pad(i) : ip ? r4pad(i) : i; };
    auto fft = [&](auto sign, float2* a, float2* b) -> const float2* {
        constexpr int SG = decltype(sign)::value;
        if (r8) {
            fft_r8_4096<SG>(a, A.tw_fft);
            return a;
        }
        if (ip) {
            if (A.log2_fft == 12)  // C3 / C4
                fft_r4_inplace_ct<SG, 12>(a, A.tw_fft);
            else
                fft_r4_inplace<SG, true>(a, A.tw_fft, A.log2_fft);
            return a;
        }
        return fft_pow2<SG>(a, b, A.tw_fft, A.log2_fft);
    };
    float2* xb = smem + 16;
    float2* yb = xb + fl.nbuf();  // the second buffer (Stockham passes only)
    // the forward spectrum is read once per template: kept in a global scratch row of this workgroup
    // (L2-resident while it runs) instead of a third LDS buffer, for two workgroups per CU
    float2* Sb = A.spec + static_cast<size_t>(blockIdx.x) * nf;
    if constexpr (!ALL) {
        // strongest antenna: first maximum of coarse_peak_array (ant.cpp:104-108)
        for (uint32_t a = 1; a < A.n_ant; ++a)
            if (rp->coarse_metric[a] > rp->coarse_metric[best]) best = a;
        cfo_frac = rp->cfo_frac;
    }
    // integer CFO search on (kernel argument, uniform): the decision on sync_icfo_kernel's scores, every thread
    // the same sums in the same order; off: the report's 0
    const float cfo_int = A.icfo_range ? sync_icfo_decide(A, rep) : rp->cfo_int;
    if constexpr (!ALL)
        if (A.icfo_range && threadIdx.x == 0) rp->cfo_int = cfo_int;
    const float cfo_hw = (cfo_frac + cfo_int) * static_cast<float>(A.Mtx) / static_cast<float>(A.Ltx);
    const int64_t base = rp->coarse_64 - static_cast<int64_t>(A.xc_l);
    const uint32_t stage_len = A.xc_len - 1 + A.tmpl_len;
    const float2* x = A.iq + w * A.win_stride + best * A.ant_stride;
    for (uint32_t i0 = 0; i0 < nf; i0 += 8 * blockDim.x) {  // 8 loads in flight per thread
        float2 v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            const uint32_t i = i0 + u * blockDim.x + threadIdx.x;
            const int64_t q = base + i;
            v[u] = (i < stage_len && q >= 0 && q < static_cast<int64_t>(A.S_win)) ? x[q] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            const uint32_t i = i0 + u * blockDim.x + threadIdx.x;
            if (i < nf) xb[ix(i)] = i < stage_len ? cmul(v[u], phasor(static_cast<double>(cfo_hw) * static_cast<double>(i))) : v[u];
        }
    }
    __syncthreads();
    const float2* S = fft(std::integral_constant<int, -1>{}, xb, yb);
    for (uint32_t i = threadIdx.x; i < nf; i += blockDim.x) Sb[i] = S[ox(i)];
    __syncthreads();  // S's buffer is overwritten below; each thread re-reads only its own Sb[i]
    // per template: its peak metric and index in the header's upper half (s_val / s_idx 8 + k; the
    // wave maxima use 0..7), written by thread 0, the only reader: no registers held across the FFTs
    for (uint32_t k = 0; k < A.n_templates; ++k) {
        const float2* T = tmpl + static_cast<size_t>(k) * nf;
        if constexpr (DNRP_FINE_BATCH > 1) {
            // the spectrum row and the template read DNRP_FINE_BATCH per thread at a time (one L2
            // round trip per batch instead of one per element), then the products stored
            constexpr uint32_t U = DNRP_FINE_BATCH;
            for (uint32_t i0 = 0; i0 < nf; i0 += U * blockDim.x) {
                float2 sv[U], tv[U];
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint32_t i = min(i0 + u * blockDim.x + threadIdx.x, nf - 1);
                    sv[u] = Sb[i];
                    tv[u] = T[i];
                }
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint32_t i = i0 + u * blockDim.x + threadIdx.x;
                    if (i < nf) xb[ix(i)] = cmul(sv[u], tv[u]);
                }
            }
        } else {
            for (uint32_t i = threadIdx.x; i < nf; i += blockDim.x) xb[ix(i)] = cmul(Sb[i], T[i]);
        }
        __syncthreads();
        const float2* R = fft(std::integral_constant<int, 1>{}, xb, yb);
        float bv = -1.f;
        uint32_t bi = 0xFFFFFFFFu;
        for (uint32_t j = threadIdx.x; j < A.xc_len; j += blockDim.x) {
            const float m = cnorm(R[ox(j)]);
            if (m > bv) {  // first maximum (volk_32fc_index_max_32u)
                bv = m;
                bi = j;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const uint32_t oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((threadIdx.x & 63u) == 0) {
            s_val[threadIdx.x >> 6] = bv;
            s_idx[threadIdx.x >> 6] = bi;
        }
        __syncthreads();
        for (uint32_t v = 0; v < blockDim.x / 64; ++v)
            if (s_val[v] > bv || (s_val[v] == bv && s_idx[v] < bi)) {
                bv = s_val[v];
                bi = s_idx[v];
            }
        if (threadIdx.x == 0) {
            s_val[8 + k] = sqrtf(bv);
            s_idx[8 + k] = bi;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float* xm = s_val + 8;
        const uint32_t* xi = s_idx + 8;
        if constexpr (ALL) {
            for (uint32_t k = 0; k < 4; ++k) {
                A.fine_m[(size_t(rep) * 8 + best) * 4 + k] = k < A.n_templates ? xm[k] : 0.f;
                A.fine_i[(size_t(rep) * 8 + best) * 4 + k] = k < A.n_templates ? xi[k] : 0u;
            }
            return;
        }
        uint32_t kbest = 0;
        float msum_max = 0.f;
        for (uint32_t k = 0; k < A.n_templates; ++k)
            if (msum_max < xm[k]) {  // strictly larger (crosscorrelator.cpp:214-226)
                msum_max = xm[k];
                kbest = k;
            }
        for (uint32_t k = 0; k < 4; ++k) {
            rp->xc_metric[k] = k < A.n_templates ? xm[k] : 0.f;
            rp->xc_idx[k] = k < A.n_templates ? xi[k] : 0u;
        }
        rp->N_eff_TX = 1u << kbest;
        const float wi = xm[kbest] * static_cast<float>(xi[kbest]);
        rp->fine_local = static_cast<uint32_t>(roundf(wi / msum_max));
        rp->fine_64 = base + rp->fine_local;
    }
}

__global__ void __launch_bounds__(SYNC_FINE_THREADS) __attribute__((amdgpu_waves_per_eu(DNRP_FINE_WPE))) sync_fine_kernel(sync_args A) {
    sync_fine_body<false>(A);
}

// every antenna with a coarse peak (sync_args::fine_all): grid n * max_reports * n_ant, the LDS of sync_fine_kernel
__global__ void __launch_bounds__(SYNC_FINE_THREADS) __attribute__((amdgpu_waves_per_eu(DNRP_FINE_WPE))) sync_fine_ant_kernel(sync_args A) {
    sync_fine_body<true>(A);
}

// crosscorrelator.cpp:205-248 on sync_fine_ant_kernel's table, one thread per report, its own launch (the
// sums run in ascending antenna order whatever the scheduling of the search workgroups): per template the
// metric sum and the metric-weighted mean index, N_eff_TX of the first largest sum, the fine peak the
// index of that template; and the report's CFO and b, which the one-workgroup form writes in its search.
constexpr uint32_t SYNC_COMBINE_THREADS = 64;
__global__ void __launch_bounds__(SYNC_COMBINE_THREADS) sync_fine_combine_kernel(sync_args A, uint32_t n_rep) {
    const uint32_t rep = blockIdx.x * SYNC_COMBINE_THREADS + threadIdx.x;
    if (rep >= n_rep) return;
    sync_res* rp = A.res + rep;
    if (!rp->found) return;
    rp->cfo_frac = sync_cfo_frac(A, rp, rep);
    if (A.beta_on) rp->b = sync_beta_decide(A, A.band + size_t(rep) * 8 * SYNC_BANDS);
    if (A.icfo_range) rp->cfo_int = sync_icfo_decide(A, rep);
    float ms[4] = {0.f, 0.f, 0.f, 0.f}, wi[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t a = 0; a < A.n_ant; ++a) {
        if (!(rp->coarse_metric[a] > 0.f)) continue;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const float m = A.fine_m[(size_t(rep) * 8 + a) * 4 + k];  // 0 for k >= n_templates
            ms[k] += m;
            wi[k] += m * static_cast<float>(A.fine_i[(size_t(rep) * 8 + a) * 4 + k]);
        }
    }
    uint32_t kbest = 0, ibest = 0;
    float msum_max = 0.f;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t idx = k < A.n_templates && ms[k] > 0.f ? static_cast<uint32_t>(roundf(wi[k] / ms[k])) : 0u;
        rp->xc_metric[k] = k < A.n_templates ? ms[k] : 0.f;
        rp->xc_idx[k] = idx;
        if (k < A.n_templates && msum_max < ms[k]) {  // strictly larger (crosscorrelator.cpp:218-233)
            msum_max = ms[k];
            kbest = k;
            ibest = idx;
        }
    }
    rp->N_eff_TX = 1u << kbest;
    rp->fine_local = ibest;
    rp->fine_64 = rp->coarse_64 - static_cast<int64_t>(A.xc_l) + ibest;
}

bool sync_taps_match(const float* h, size_t n) {  // run-time sync taps == compiled-in taps, bitwise
    if (n != static_cast<size_t>(taps_sync_9_10::N)) return false;
    for (size_t i = 0; i < n; ++i)
        if (__builtin_bit_cast(uint32_t, h[i]) != __builtin_bit_cast(uint32_t, taps_sync_9_10::h[i])) return false;
    return true;
}

// ===================================================================== launchers
// sync_post_kernel's compiled-in-tap form is the staged one (DNRP_POST_STAGED): at most 2 blocks per thread.
// Where the STF is longer, the run-time-tap form reads the windows straight from the stream (the same sums)
static bool sync_post_ct_form(const sync_args& a) { return !DNRP_POST_STAGED || (a.stf_len + 8) / 9 + 2 <= 2 * SYNC_THREADS; }
static bool sync_post_staged(const sync_args& a) {
    return DNRP_POST_STAGED && sync_class_of(a) == SYNC_CLASS_9_10_24 && a.ct_taps && sync_post_ct_form(a);
}
size_t sync_post_lds(const sync_args& a) {  // the staged form's input span (n_in inputs) or the STF
    const uint32_t n_in = sync_staged_n_in<9, 10, 24>((a.stf_len + 8) / 9 + 3);
    return (12 + (std::max(a.stf_len, sync_post_staged(a) ? n_in : 0u) + 1) / 2 * 2) * sizeof(float2);
}

hipError_t launch_sync_post(const sync_args& a, uint32_t n, hipStream_t st) {
    const dim3 g(n * a.max_reports * a.n_ant);
    const size_t lds = sync_post_lds(a);
    if (lds > LDS_BYTES) return hipErrorInvalidValue;
    auto go = [&](auto l, auto m, auto h, auto ct) {
        hipLaunchKernelGGL((sync_post_kernel<decltype(l)::value, decltype(m)::value, decltype(h)::value, decltype(ct)::value>), g,
                           dim3(SYNC_THREADS), lds, st, a);
    };
    sync_post_ct_form(a) ? sync_dispatch<true>(a, go) : sync_dispatch<false>(a, go);
    return hipGetLastError();
}

hipError_t launch_sync_beta(const sync_args& a, const sync_beta_args& ba, uint32_t n, hipStream_t st) {
    const dim3 g(n * a.max_reports * a.n_ant);
    const size_t lds = (12 + 2 * size_t(ba.plan.N)) * sizeof(float2);
    if (lds > LDS_BYTES || ba.cp + ba.plan.N != a.stf_len || (ba.shift && (!a.icfo || !a.icfo_range))) return hipErrorInvalidValue;
    sync_dispatch<true>(a, [&](auto l, auto m, auto h, auto ct) {  // compiled-in 9/10 taps, as sync_post_kernel
        constexpr int LR = decltype(l)::value, MR = decltype(m)::value, HLR = decltype(h)::value;
        constexpr bool CT = decltype(ct)::value;
        if (ba.shift)
            hipLaunchKernelGGL((sync_beta_kernel<LR, MR, HLR, CT, true>), g, dim3(SYNC_THREADS), lds, st, a, ba);
        else
            hipLaunchKernelGGL((sync_beta_kernel<LR, MR, HLR, CT, false>), g, dim3(SYNC_THREADS), lds, st, a, ba);
    });
    return hipGetLastError();
}

// sync_beta_kernel's grid, LDS and class dispatch
hipError_t launch_sync_icfo(const sync_args& a, const sync_beta_args& ba, uint32_t n, hipStream_t st) {
    const dim3 g(n * a.max_reports * a.n_ant);
    const size_t lds = (12 + 2 * size_t(ba.plan.N)) * sizeof(float2);
    if (lds > LDS_BYTES || ba.cp + ba.plan.N != a.stf_len || ba.plan.N != 4 * a.pattern || a.icfo_N != ba.plan.N ||
        a.icfo_range > SYNC_ICFO_MAX || !a.icfo)
        return hipErrorInvalidValue;
    sync_dispatch<true>(a, [&](auto l, auto m, auto h, auto ct) {
        hipLaunchKernelGGL((sync_icfo_kernel<decltype(l)::value, decltype(m)::value, decltype(h)::value, decltype(ct)::value>), g,
                           dim3(SYNC_THREADS), lds, st, a, ba);
    });
    return hipGetLastError();
}

size_t sync_fine_lds(const sync_args& a) { return sync_fine_layout(a.log2_fft, DNRP_FINE_R8).slots() * sizeof(float2); }

// The fine search is offered where two unpadded buffers would fit the LDS. That is an upper bound of
// sync_fine_lds: the in-place forms of a 16384-point search would fit, but no test holds that size to
// the oracle, so it stays declined.
bool sync_fine_ok(const sync_args& a) {
    const size_t two = (16 + 2 * (size_t(1) << a.log2_fft)) * sizeof(float2);
    return std::max(two, sync_fine_lds(a)) <= LDS_BYTES;
}

hipError_t launch_sync_fine(const sync_args& a, uint32_t n, hipStream_t st) {
    const size_t lds = sync_fine_lds(a);
    if (!a.fine_all) {
        hipLaunchKernelGGL(sync_fine_kernel, dim3(n * a.max_reports), dim3(SYNC_FINE_THREADS), lds, st, a);
        return hipGetLastError();
    }
    const uint32_t n_rep = n * a.max_reports;
    hipLaunchKernelGGL(sync_fine_ant_kernel, dim3(n_rep * a.n_ant), dim3(SYNC_FINE_THREADS), lds, st, a);
    hipLaunchKernelGGL(sync_fine_combine_kernel, dim3((n_rep + SYNC_COMBINE_THREADS - 1) / SYNC_COMBINE_THREADS),
                       dim3(SYNC_COMBINE_THREADS), 0, st, a, n_rep);
    return hipGetLastError();
}

}  // namespace dnrp::dev
