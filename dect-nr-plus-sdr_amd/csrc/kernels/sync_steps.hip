// Step sums of the synchronisation (sync_common.hpp): the tile, wave, stream and pipe kernels, and their launcher.
#include "sync_common.hpp"

// ---- compile-time knobs (-D), shipped values
#ifndef SYNC_WB_DEF
#define SYNC_WB_DEF 4  // wave kernel: polyphase blocks per lane
#endif
#ifndef SYNC_WPG_DEF
#define SYNC_WPG_DEF 2  // wave kernel: waves per workgroup
#endif
#ifndef DNRP_SS_SUMG
#define DNRP_SS_SUMG 8  // step-sum samples per group of LDS reads in flight (two halves of 8)
#endif
#ifndef DNRP_SS_IMAJ
#define DNRP_SS_IMAJ 1  // the FIR window input-major from LDS (pp_const::run_imaj): 131 VGPRs against 159, sync_steps
                        // 13.80 -> 13.31 ms per C4 chunk at the same 11 waves per CU (0: window loaded whole)
#endif
#ifndef DNRP_SS_WPE
#define DNRP_SS_WPE 1  // waves per SIMD the register budget must allow (1: the compiler's choice)
#endif
#ifndef DNRP_SS_RING
#define DNRP_SS_RING 1024  // stream kernel's ring: power of two >= 64 * 9 + step + pattern + 9 (host-checked)
#endif
// the pipelined kernel's ring (sync_steps_pipe_kernel), a power of two as well. The measured alternatives
// (a 912-slot ring, the FIR window read lazily, 4-sample step-sum groups: all slower) are recorded in
// docs/DESIGN_LOG.md §6 and DESIGN.md §6.2. Kept: 1024, one load group, two halves of 8.
#ifndef DNRP_SS_PRING
#define DNRP_SS_PRING 1024
#endif
#ifndef DNRP_SS_SEG_CHUNKS
#define DNRP_SS_SEG_CHUNKS 96u  // at most this many chunks of 64 polyphase blocks per sync_steps segment (each
                                // segment re-resamples its lag history first). C4 (1440 steps per window):
                                // 32 -> 5 x 288 steps 12.95 / 12.79 ms, 64 -> 3 x 480 12.71 / 12.74, 96 -> 2 x 720
                                // 12.55 / 12.65, 160 -> 1 x 1440 12.61 / 12.65 (same box)
#endif

namespace dnrp::dev {

template <int LR, int MR, int HLR>
__global__ void __launch_bounds__(SYNC_THREADS) sync_steps_kernel(sync_args A) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const uint32_t ntile = (A.s_hi - A.s_lo + SYNC_TILE_STEPS - 1) / SYNC_TILE_STEPS;  // tiles of the tranche
    const uint32_t tile = blockIdx.x % ntile;
    const uint32_t a = (blockIdx.x / ntile) % A.n_ant;
    const uint32_t w = blockIdx.x / (ntile * A.n_ant);
    if (sync_window_done(A, w)) return;  // uniform over the workgroup, before any barrier
    float* taps = reinterpret_cast<float*>(smem);
    float2* lb = smem + sync_tap_f2(A.npp);
    const uint32_t s0 = A.s_lo + tile * SYNC_TILE_STEPS;
    const uint32_t s1 = min(s0 + SYNC_TILE_STEPS, A.s_hi);
    const int64_t y0 = static_cast<int64_t>(s0) * A.step - A.pattern;
    const uint32_t cnt = (s1 - s0) * A.step + A.pattern;
    float2* stage = lb + (cnt + 1) / 2 * 2;
    if (LR > 1)
        stage_copy<4>(taps, A.taps_pp, A.npp, threadIdx.x, blockDim.x);
    const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
    sync_resample<LR, MR, HLR>(A, x, y0, cnt, stage, lb, taps);
    // step s = s0 + tid/4, quarter tid%4 of its samples; reduce over the 4 lanes
    const uint32_t sl = threadIdx.x >> 2, part = threadIdx.x & 3u;
    const uint32_t s = s0 + sl, seg = A.step >> 2;
    float pw = 0.f;
    float2 c = make_float2(0.f, 0.f);
    if (s < s1) {
        const uint32_t i0 = (s - s0) * A.step + A.pattern + part * seg;  // index of y = s*step + part*seg
        for (uint32_t j = 0; j < seg; ++j) {
            const float2 v = lb[i0 + j];
            ss_power(v, pw);
            if (s >= 4) ss_corr(lb[i0 + j - A.pattern], v, c);  // A = x[n - P], B = x[n]: A conj(B)
        }
    }
    ss_group_sum<4>(pw, c);
    if (s < s1 && part == 0) {
        const size_t o = (static_cast<size_t>(w) * A.n_ant + a) * A.n_steps + s;
        A.P[o] = pw;
        A.Cs[o] = c;
    }
}

// ---- pp resampler path: one wavefront per range of SYNC_WB_STEPS-ish steps, no workgroup barrier
// after the table load. The wave stages its hw-rate input span in its own LDS region, resamples it
// with B polyphase blocks per lane (pp_block::run_multi: one tap-row read serves B blocks, which
// keeps the LDS traffic per FMA under the 128 B/clk/CU the VALU needs), writes the outputs back into
// the region and sums the steps from there.
constexpr int SYNC_WB = SYNC_WB_DEF;    // blocks per lane
constexpr int SYNC_WPG = SYNC_WPG_DEF;  // waves per workgroup

__host__ __device__ inline uint32_t sync_wave_steps(uint32_t L, uint32_t step, uint32_t pattern) {
    return (64u * SYNC_WB * L - pattern - 2 * L) / step;  // steps whose span (+ lookback) fits 64 B blocks
}
__host__ __device__ inline uint32_t sync_wave_region(uint32_t L, uint32_t M, uint32_t hl) {  // float2 per wave
    const uint32_t W = hl + 1 + ((L - 1) * M) / L;
    return (M * (64 * SYNC_WB - 1) + W + 1) / 2 * 2;
}

template <int LR, int MR, int HLR, int WPG>
__global__ void __launch_bounds__(64 * WPG) sync_steps_wave_kernel(sync_args A) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    using PB = pp_block<LR, MR, HLR>;
    float* taps = reinterpret_cast<float*>(smem);
    const uint32_t region = sync_wave_region(LR, MR, HLR);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;  // uniform
    float2* R = smem + sync_tap_f2(A.npp) + wv * region;
    const uint32_t sw = sync_wave_steps(LR, A.step, A.pattern);
    const uint32_t parts = (A.s_hi - A.s_lo + sw - 1) / sw;  // parts of the tranche
    const uint32_t gw = blockIdx.x * WPG + wv;
    const uint32_t part = gw % parts;
    const uint32_t a = (gw / parts) % A.n_ant;
    const uint32_t w = gw / (parts * A.n_ant);
    const uint32_t s0 = A.s_lo + part * sw, s1 = min(s0 + sw, A.s_hi);
    const int64_t y0 = static_cast<int64_t>(s0) * A.step - A.pattern;
    const uint32_t cnt = (s1 - s0) * A.step + A.pattern;
    const int64_t ms = A.m_star;
    const int64_t q0 = floordiv(y0 - ms, LR), q1 = floordiv(y0 + cnt - ms + LR - 1, LR);
    const int64_t in0 = static_cast<int64_t>(A.p_star) + MR * q0 - HLR;
    const uint32_t n_in = static_cast<uint32_t>(MR * (q1 - 1 - q0) + PB::W);
    const bool live = w < A.n_win && !sync_window_done(A, w);  // a finished window's wave still meets the barrier
    if (live) {
        const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
        const int64_t S = A.S_win;
        stage_span<24>(R, x, in0, n_in, S, lane, 64);
    }
    stage_copy<4>(taps, A.taps_pp, A.npp, threadIdx.x, blockDim.x);
    __syncthreads();
    if (!live) return;
    float2 y[SYNC_WB][LR];
    const float2* xw[SYNC_WB];
#pragma unroll
    for (int b = 0; b < SYNC_WB; ++b) xw[b] = R + MR * (lane + 64 * b);
    PB::template run_multi<SYNC_WB>(xw, taps, y);
    __builtin_amdgcn_wave_barrier();
    const int64_t nblk = q1 - q0;
#pragma unroll
    for (int b = 0; b < SYNC_WB; ++b) {
        const int64_t j = lane + 64 * b;
        if (j < nblk) sync_emit_block<LR>(ms + LR * (q0 + j), y0, cnt, y[b], [&](int64_t i, float2 v) __attribute__((always_inline)) { R[i] = v; });
    }
    __builtin_amdgcn_wave_barrier();
    // steps: 32 per round, half of each step's samples per lane (reduced over the lane pair). Each
    // lane walks its half starting at its own rotation (j + lane) mod half, so the 32 lanes of a
    // ds_read_b64 half-wave hit 32 different bank pairs (step starts are 0 mod 64 banks).
    const uint32_t half = A.step >> 1, h = lane & 1u, rot = lane % half;
    for (uint32_t sb = s0; sb < s1; sb += 32) {
        const uint32_t s = sb + (lane >> 1);
        float pw = 0.f;
        float2 c = make_float2(0.f, 0.f);
        if (s < s1) {
            const uint32_t i0 = (s - s0) * A.step + A.pattern + h * half;
            for (uint32_t j = 0; j < half; ++j) {
                uint32_t jj = j + rot;
                if (jj >= half) jj -= half;
                const float2 v = R[i0 + jj];
                ss_power(v, pw);
                if (s >= 4) ss_corr(R[i0 + jj - A.pattern], v, c);
            }
        }
        ss_group_sum<2>(pw, c);
        if (s < s1 && h == 0) {
            const size_t o = (static_cast<size_t>(w) * A.n_ant + a) * A.n_steps + s;
            A.P[o] = pw;
            A.Cs[o] = c;
        }
    }
}

// ---- streaming path (pp resampler, ring fits): one wavefront walks a segment of steps in chunks
// of 64 polyphase blocks (64 L outputs), software-pipelined: the next chunk's M * 64 new inputs are
// loaded into registers (coalesced, 8 B per lane and instruction) while the current chunk is
// resampled, so every wave keeps its own loads in flight instead of waiting on a staging pass.
// Per wave LDS: the chunk's input window (carry W - M + M * 64) and a 1024-sample output ring
// holding the pattern lookback; no workgroup barrier anywhere.
constexpr uint32_t SS_RING = DNRP_SS_RING;
constexpr uint32_t SS_PRING = DNRP_SS_PRING;
static_assert((SS_PRING & (SS_PRING - 1)) == 0 && SS_PRING >= 16, "a power of two: 16-slot step-sum reads stay inside the ring");
__device__ __forceinline__ uint32_t pring(int64_t m) { return static_cast<uint32_t>(m) & (SS_PRING - 1); }  // m mod SS_PRING
constexpr uint32_t SS_WPG = 4;

template <int LR, int MR, int HLR>
__host__ __device__ constexpr uint32_t ss_inbuf() {  // float2 per wave, 16-B multiple
    return ((HLR + 1 + ((LR - 1) * MR) / LR - MR) + 64 * MR + 1) / 2 * 2;
}

// the polyphase blocks of the steps [s_a, s_b): first block qa, nch chunks of 64. The outputs start one
// pattern lag early (m_lo), so a segment warms its lag history up
struct ss_blocks {
    int64_t qa;
    uint32_t nch;
};
template <int LR>
__device__ __forceinline__ ss_blocks ss_blocks_of(const sync_args& A, uint32_t s_a, uint32_t s_b) {
    const int64_t step = A.step, P = A.pattern;
    const int64_t m_lo = max<int64_t>(0, s_a * step - P), m_hi = s_b * step;
    const int64_t ms = A.m_star;
    const int64_t qa = floordiv(m_lo - ms, LR), qb = floordiv(m_hi - 1 - ms, LR);
    return {qa, static_cast<uint32_t>((qb - qa + 64) / 64)};
}

template <int LR, int MR, int HLR, int SQ, int WPG = SS_WPG>
__global__ void __launch_bounds__(64 * SS_WPG) sync_steps_stream_kernel(sync_args A, uint32_t seg_steps, uint32_t n_seg) {
    using PD = pp_direct<LR, MR, HLR>;
    constexpr int W = PD::W, CARRY = W - MR, NEW = 64 * MR;
    constexpr uint32_t INB = ss_inbuf<LR, MR, HLR>();
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;  // uniform
    float2* inb = smem + wv * (INB + SS_RING);
    float2* ring = inb + INB;
    const uint32_t gw = blockIdx.x * WPG + wv;
    const uint32_t seg = gw % n_seg, a = (gw / n_seg) % A.n_ant, w = gw / (n_seg * A.n_ant);
    if (w >= A.n_win) return;  // no barriers below: a retired wave stalls nobody
    if (sync_window_done(A, w)) return;
    const uint32_t s_a = A.s_lo + seg * seg_steps, s_b = min(s_a + seg_steps, A.s_hi);  // segments of the tranche
    if (s_a >= s_b) return;
    const int64_t step = A.step, P = A.pattern, ms = A.m_star;
    const ss_blocks sg = ss_blocks_of<LR>(A, s_a, s_b);
    const int64_t qa = sg.qa;
    const uint32_t nch = sg.nch;
    const float2* __restrict__ x = A.iq + w * A.win_stride + a * A.ant_stride;
    const int64_t S = A.S_win;
    const float* taps_g = A.taps;
    auto ld = [&](int64_t q) { return (q >= 0 && q < S) ? x[q] : make_float2(0.f, 0.f); };
    // chunk c: blocks qa + 64 c + lane, window inputs [ib_c, ib_c + CARRY + NEW), ib_c = p_star + M qc - HL
    const int64_t ib0 = static_cast<int64_t>(A.p_star) + MR * qa - HLR;
    float2 pre[MR];
#pragma unroll
    for (int j = 0; j < MR; ++j) pre[j] = ld(ib0 + CARRY + j * 64 + lane);
    if (lane < CARRY) inb[lane] = ld(ib0 + lane);
    uint32_t s_next = s_a;
    const uint32_t sq = A.step >> 2;  // samples per lane quarter of a step
    for (uint32_t c = 0; c < nch; ++c) {
#pragma unroll
        for (int j = 0; j < MR; ++j) inb[CARRY + j * 64 + lane] = pre[j];
        if (c + 1 < nch) {
            const int64_t ibn = ib0 + static_cast<int64_t>(c + 1) * NEW;
#pragma unroll
            for (int j = 0; j < MR; ++j) pre[j] = ld(ibn + CARRY + j * 64 + lane);
        }
        __builtin_amdgcn_wave_barrier();
        float2 xv[W];
        if constexpr ((MR & 1) == 0) PD::template load<true>(inb + MR * lane, xv);
        else PD::template load<false>(inb + MR * lane, xv);
        float2 y[LR];
        {
            // opaque per chunk: the taps are re-read (scalar loads, K$ hits) instead of being hoisted
            // into more SGPRs than a wave has
            const float* tp = taps_g;
            asm volatile("" : "+s"(tp));
            PD::run(xv, (ctap_ptr)(tp), y);
        }
        const int64_t mb = ms + LR * (qa + 64 * static_cast<int64_t>(c) + lane);
        // unconditional: outputs m < 0 (first block only) land in slots that outputs 1024 - L..1023
        // overwrite before any step reads them, and keeping the stores unconditional keeps the
        // compiler from sinking the FMAs into per-output branches
#pragma unroll
        for (int k = 0; k < LR; ++k) ring[static_cast<uint32_t>(mb + k) & (SS_RING - 1)] = y[k];
        // carry: the last W - M inputs of this window start the next one (disjoint from the reads)
        if (lane < CARRY) inb[lane] = inb[NEW + lane];
        __builtin_amdgcn_wave_barrier();
        // steps complete in the ring: 4 lanes per step, a quarter each, bank-rotated walk
        const int64_t m_end = ms + LR * (qa + 64 * static_cast<int64_t>(c) + 64);
        const uint32_t s_end = static_cast<uint32_t>(min<int64_t>(s_b, m_end >= 0 ? m_end / step : 0));
        for (uint32_t sb = s_next; sb < s_end; sb += 16) {
            const uint32_t s = sb + (lane >> 2), part = lane & 3u;
            const uint32_t rot = (2u * ((lane >> 2) & 7u) + ((part >> 1) & 1u) + (lane >> 5)) % sq;
            float pw = 0.f;
            float2 cc = make_float2(0.f, 0.f);
            if (s < s_end) {
                const uint32_t n0 = s * A.step + part * sq;
                const bool corr = static_cast<int64_t>(s) * step >= P;
                if (SQ > 0) {
                    // quarter of 16 samples: n0 and the pattern lag are multiples of 16, so the
                    // quarter never wraps the ring; all 32 reads issue back to back
                    const float2* rv = ring + (n0 & (SS_RING - 1));
                    const float2* ru = ring + ((n0 - A.pattern) & (SS_RING - 1));
                    float2 v[SQ > 0 ? SQ : 1], u[SQ > 0 ? SQ : 1];
#pragma unroll
                    for (int j = 0; j < SQ; ++j) {
                        const uint32_t jj = (j + rot) & (SQ - 1);
                        v[j] = rv[jj];
                        u[j] = corr ? ru[jj] : make_float2(0.f, 0.f);
                    }
#pragma unroll
                    for (int j = 0; j < SQ; ++j) {
                        ss_power(v[j], pw);
                        ss_corr(u[j], v[j], cc);
                    }
                } else {
                    for (uint32_t j = 0; j < sq; ++j) {
                        uint32_t jj = j + rot;
                        if (jj >= sq) jj -= sq;
                        const uint32_t n = n0 + jj;
                        const float2 v = ring[n & (SS_RING - 1)];
                        ss_power(v, pw);
                        if (corr) ss_corr(ring[(n - A.pattern) & (SS_RING - 1)], v, cc);
                    }
                }
            }
            ss_group_sum<4>(pw, cc);
            if (s < s_end && part == 0) {
                const size_t o = (static_cast<size_t>(w) * A.n_ant + a) * A.n_steps + s;
                A.P[o] = pw;
                A.Cs[o] = cc;
            }
        }
        s_next = max(s_next, s_end);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- the streaming path for 64-sample steps with two chunks of loads in flight per wave
// (sync_steps_stream_kernel<.., 16, 1> restated): the window is read through a range-checked buffer
// descriptor (samples outside [0, S_win) read as zeros, no branches), the P / C step values are
// stored the same way, and a chunk completes at most 10 steps (576 outputs), so every chunk issues
// a fixed number of memory instructions. The waits for a chunk's loads are then counted vmcnt(n)
// with the next chunk's loads still in flight, instead of draining the queue.
template <int LR, int MR, int HLR, bool CT>
__device__ __forceinline__ void ss_pipe_chunk(const sync_args& A, float2* inb, float2* ring, float2 (&pre)[MR],
                                              __amdgpu_buffer_rsrc_t xr, __amdgpu_buffer_rsrc_t pr,
                                              __amdgpu_buffer_rsrc_t cr, int64_t ib0, int64_t qa, uint32_t c,
                                              uint32_t s_b, uint32_t& s_next, uint32_t lane) {
    using PD = pp_direct<LR, MR, HLR>;
    constexpr int W = PD::W, CARRY = W - MR, NEW = 64 * MR;
    const int64_t step = A.step, ms = A.m_star;
#pragma unroll
    for (int j = 0; j < MR; ++j) inb[CARRY + j * 64 + lane] = pre[j];
    {  // the chunk after next (past the segment: harmless reads, range-checked)
        const int64_t ibn = ib0 + static_cast<int64_t>(c + 2) * NEW + CARRY + lane;
#pragma unroll
        for (int j = 0; j < MR; ++j)  // cache policy nt: the window row is streamed once by this wave
            pre[j] = buffer_load_f2<2>(xr, static_cast<uint32_t>((ibn + j * 64) * 8));
    }
    __builtin_amdgcn_wave_barrier();
    float2 y[LR];
    if constexpr (CT && DNRP_SS_IMAJ) {
        pp_const<taps_sync_9_10>::run_imaj(inb + MR * lane, y);  // inb 16-B aligned, MR even
    } else {
        float2 xv[W];
        if constexpr ((MR & 1) == 0) PD::template load<true>(inb + MR * lane, xv);
        else PD::template load<false>(inb + MR * lane, xv);
        if constexpr (CT) {
            pp_const<taps_sync_9_10>::run(xv, y);
        } else {
            const float* tp = A.taps;
            asm volatile("" : "+s"(tp));
            PD::run(xv, (ctap_ptr)(tp), y);
        }
    }
    const int64_t mb = ms + LR * (qa + 64 * static_cast<int64_t>(c) + lane);
#pragma unroll
    for (int k = 0; k < LR; ++k) ring[pring(mb + k)] = y[k];
    if (lane < CARRY) inb[lane] = inb[NEW + lane];
    __builtin_amdgcn_wave_barrier();
    const int64_t m_end = ms + LR * (qa + 64 * static_cast<int64_t>(c) + 64);
    const uint32_t s_end = static_cast<uint32_t>(min<int64_t>(s_b, m_end >= 0 ? m_end / step : 0));
    // one pass of 16 steps covers the chunk's (<= 10) completed steps: 4 lanes per step, a quarter each
    const uint32_t s = s_next + (lane >> 2), part = lane & 3u;
    const uint32_t rot = (2u * ((lane >> 2) & 7u) + ((part >> 1) & 1u) + (lane >> 5)) % 16u;
    const bool live = s < s_end;
    const uint32_t n0 = (live ? s : s_next) * 64u + part * 16u;
    const bool corr = live && static_cast<int64_t>(s) * step >= A.pattern;
    const float2* rv = ring + pring(n0);
    const float2* ru = ring + pring(static_cast<int64_t>(n0) - A.pattern);
    float pw = 0.f;
    float2 cc = make_float2(0.f, 0.f);
    constexpr int SG = DNRP_SS_SUMG;  // samples per group of reads in flight (same summation order)
#pragma unroll
    for (int h = 0; h < 16 / SG; ++h) {
        float2 v[SG], u[SG];
#pragma unroll
        for (int j = 0; j < SG; ++j) {
            const uint32_t jj = (SG * h + j + rot) & 15u;
            v[j] = rv[jj];
            u[j] = ru[jj];
        }
#pragma unroll
        for (int j = 0; j < SG; ++j) {
            ss_power(v[j], pw);
            ss_corr(u[j], v[j], cc);
        }
    }
    // a step before the first full lag has no correlation term: dropped once here, not per sample
    // (the sums of zero products were +0, as the select gives)
    if (!corr) cc = make_float2(0.f, 0.f);
    if (!live) {
        pw = 0.f;
        cc = make_float2(0.f, 0.f);
    }
    ss_group_sum<4>(pw, cc);
    const bool st = live && part == 0;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(pw), pr, st ? s * 4u : 0x80000000u, 0, 0);
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    const u2 cv = {__float_as_uint(cc.x), __float_as_uint(cc.y)};
    __builtin_amdgcn_raw_buffer_store_b64(cv, cr, st ? s * 8u : 0x80000000u, 0, 0);
    s_next = max(s_next, s_end);
    __builtin_amdgcn_wave_barrier();
}

template <int LR, int MR, int HLR, bool CT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DNRP_SS_WPE))) sync_steps_pipe_kernel(sync_args A, uint32_t seg_steps, uint32_t n_seg) {
    using PD = pp_direct<LR, MR, HLR>;
    constexpr int W = PD::W, CARRY = W - MR, NEW = 64 * MR;
    constexpr uint32_t INB = ss_inbuf<LR, MR, HLR>();
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const uint32_t lane = threadIdx.x & 63u;
    float2* inb = smem;
    float2* ring = inb + INB;
    const uint32_t gw = blockIdx.x;
    const uint32_t seg = gw % n_seg, a = (gw / n_seg) % A.n_ant, w = gw / (n_seg * A.n_ant);
    if (w >= A.n_win) return;
    if (sync_window_done(A, w)) return;
    const uint32_t s_a = A.s_lo + seg * seg_steps, s_b = min(s_a + seg_steps, A.s_hi);  // segments of the tranche
    if (s_a >= s_b) return;
    const ss_blocks sg = ss_blocks_of<LR>(A, s_a, s_b);
    const int64_t qa = sg.qa;
    const uint32_t nch = sg.nch;
    // range-checked rows: the window row (zeros outside [0, S_win)) and the step-value rows. The
    // window row's range ends at the segment's last input: the prefetches past the segment (the two
    // chunks after its last) return zeros without a memory request (they were 6 % of the bytes)
    const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
    const size_t orow = (static_cast<size_t>(w) * A.n_ant + a) * A.n_steps;
    const int64_t ib0 = static_cast<int64_t>(A.p_star) + MR * qa - HLR;
    const int64_t in_end = experiment(XS_SYNC_NOCLAMP) ? int64_t(A.S_win)
                                                       : min<int64_t>(A.S_win, max<int64_t>(0, ib0 + int64_t(NEW) * nch + CARRY));
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(x), 0, static_cast<int>(in_end * 8), 0x00020000);
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(A.P + orow, 0, static_cast<int>(A.n_steps * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t cr = __builtin_amdgcn_make_buffer_rsrc(A.Cs + orow, 0, static_cast<int>(A.n_steps * 8u), 0x00020000);
    auto ldb = [&](int64_t q) { return buffer_load_f2<0>(xr, static_cast<uint32_t>(q * 8)); };
    float2 pa[MR], pb[MR];
#pragma unroll
    for (int j = 0; j < MR; ++j) pa[j] = ldb(ib0 + CARRY + j * 64 + lane);
#pragma unroll
    for (int j = 0; j < MR; ++j) pb[j] = ldb(ib0 + NEW + CARRY + j * 64 + lane);
    if (lane < CARRY) inb[lane] = ldb(ib0 + lane);
    uint32_t s_next = s_a;
    for (uint32_t c = 0; c < nch; c += 2) {  // chunk c + 1 >= nch: harmless work, no stores
        ss_pipe_chunk<LR, MR, HLR, CT>(A, inb, ring, pa, xr, pr, cr, ib0, qa, c, s_b, s_next, lane);
        ss_pipe_chunk<LR, MR, HLR, CT>(A, inb, ring, pb, xr, pr, cr, ib0, qa, c + 1, s_b, s_next, lane);
    }
}

// ===================================================================== launcher
// The form a step-sum launch takes and its launch geometry. The streaming forms cut the tranche into
// segments of at most DNRP_SS_SEG_CHUNKS chunks, balanced: ceil(n_rng / max) segments of equal length (a
// short last segment leaves its waves idle at the tail).
enum ss_form : uint32_t { SS_FORM_PIPE, SS_FORM_STREAM16, SS_FORM_STREAM, SS_FORM_WAVE, SS_FORM_TILE };
struct ss_launch {
    ss_form form;
    uint32_t seg_steps, n_seg;  // streaming forms
    uint32_t grid, block;
    size_t lds;
};
static ss_launch ss_form_of(const sync_args& a, uint32_t n, sync_steps_kind kind) {
    const uint32_t n_rng = a.s_hi - a.s_lo;
    const bool c24 = sync_class_of(a) == SYNC_CLASS_9_10_24;
    const uint32_t back = 64u * 9u + a.step + a.pattern + 9u;  // ring slots a chunk's steps look back over
    if (kind != SYNC_STEPS_WAVE && c24 && a.step % 4 == 0 && a.step >= 4 && back <= SS_RING) {
        const uint32_t seg_max = std::max(1u, (DNRP_SS_SEG_CHUNKS * 64u * 9u) / a.step);
        const uint32_t n_seg0 = (n_rng + seg_max - 1) / seg_max;
        const uint32_t seg_steps = std::max(1u, (n_rng + n_seg0 - 1) / n_seg0);
        const uint32_t n_seg = (n_rng + seg_steps - 1) / seg_steps;
        const uint64_t waves = uint64_t(n) * a.n_ant * n_seg;
        const size_t wlds = size_t(ss_inbuf<9, 10, 24>() + SS_RING) * sizeof(float2);  // per wave
        // the pipelined kernel, one wave per workgroup, unless the caller keeps to the single-chunk-prefetch form
        if (a.step == 64 && kind == SYNC_STEPS_PIPE && a.pattern % 16 == 0 && back <= SS_PRING)
            return {SS_FORM_PIPE, seg_steps, n_seg, static_cast<uint32_t>(waves), 64,
                    size_t(ss_inbuf<9, 10, 24>() + SS_PRING) * sizeof(float2)};
        if (a.step == 64) return {SS_FORM_STREAM16, seg_steps, n_seg, static_cast<uint32_t>(waves), 64, wlds};
        return {SS_FORM_STREAM, seg_steps, n_seg, static_cast<uint32_t>((waves + SS_WPG - 1) / SS_WPG), 64 * SS_WPG, SS_WPG * wlds};
    }
    if (c24) {
        const uint32_t sw = sync_wave_steps(9, a.step, a.pattern);
        const uint32_t waves = n * a.n_ant * ((n_rng + sw - 1) / sw);
        return {SS_FORM_WAVE, 0, 0, (waves + SYNC_WPG - 1) / SYNC_WPG, 64 * SYNC_WPG,
                (sync_tap_f2(a.npp) + SYNC_WPG * size_t(sync_wave_region(9, 10, 24))) * sizeof(float2)};
    }
    const uint32_t ntile = (n_rng + SYNC_TILE_STEPS - 1) / SYNC_TILE_STEPS;
    const uint32_t cnt = SYNC_TILE_STEPS * a.step + a.pattern;
    return {SS_FORM_TILE, 0, 0, n * a.n_ant * ntile, SYNC_THREADS,
            (sync_tap_f2(a.npp) + size_t((cnt + 1) / 2 * 2) + sync_stage_cap(a.L, a.M, a.hl, cnt)) * sizeof(float2)};
}

hipError_t launch_sync_steps(const sync_args& a, uint32_t n, hipStream_t st, sync_steps_kind kind) {
    // the tranche [s_lo, s_hi) of the window's steps: only the segments / parts / tiles that cover it
    // are launched (one tranche over all steps: the grids are the whole-window ones)
    if (a.s_lo >= a.s_hi || a.s_hi > a.n_steps) return hipErrorInvalidValue;
    const ss_launch f = ss_form_of(a, n, kind);
    const dim3 g(f.grid), b(f.block);
    switch (f.form) {
        case SS_FORM_PIPE:
            // compile-time sync taps where the run-time taps are the generated ones (neutral, 3.48 ms both;
            // docs/DESIGN_LOG.md §6)
            sync_dispatch<true>(a, [&](auto, auto, auto, auto ct) {
                hipLaunchKernelGGL((sync_steps_pipe_kernel<9, 10, 24, decltype(ct)::value>), g, b, f.lds, st, a, f.seg_steps, f.n_seg);
            });
            break;
        case SS_FORM_STREAM16:
            hipLaunchKernelGGL((sync_steps_stream_kernel<9, 10, 24, 16, 1>), g, b, f.lds, st, a, f.seg_steps, f.n_seg);
            break;
        case SS_FORM_STREAM:
            hipLaunchKernelGGL((sync_steps_stream_kernel<9, 10, 24, 0>), g, b, f.lds, st, a, f.seg_steps, f.n_seg);
            break;
        case SS_FORM_WAVE:
            hipLaunchKernelGGL((sync_steps_wave_kernel<9, 10, 24, SYNC_WPG>), g, b, f.lds, st, a);
            break;
        case SS_FORM_TILE:
            sync_dispatch<false>(a, [&](auto l, auto m, auto h, auto) {
                hipLaunchKernelGGL((sync_steps_kernel<decltype(l)::value, decltype(m)::value, decltype(h)::value>), g, b, f.lds, st, a);
            });
            break;
    }
    return hipGetLastError();
}

}  // namespace dnrp::dev
