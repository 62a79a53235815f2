// RX back end of the synchronised receiver: channel estimation, equalisation, soft demapping.
//
//  rx_snr_kernel    one WG per packet: zero-forcing of every DRS symbol of the phase, SNR
//                   accumulation (estimator_snr.cpp:104-146) and the SNR-driven Wiener LUT profile
//                   pick after each DRS symbol (rx_synced.cpp:863-891). One wavefront per DRS
//                   symbol; the accumulation itself is a short serial prefix.
//  rx_sto_track_kernel  one WG per packet, only with residual STO tracking on: the STO increment after
//                   every DRS symbol of the phase and the per-symbol table the front ends derotate with
//                   (estimator_sto.cpp:64-97, 148-171).
//  rx_cfo_track_kernel  one WG per packet, only with residual CFO tracking on: the mixer increment after
//                   every DRS symbol of the phase, from the rotation between DRS symbols one period apart,
//                   and the per-symbol table the front ends mix with (rx_synced_param.hpp:162-181).
//  rx_cells_kernel  one WG per (packet, epoch): an epoch is a run of cell work over which the
//                   interlaced pilot buffer (channel_antenna.hpp:38-63) does not change. The WG
//                   rebuilds that buffer in LDS from the zero-forced DRS cells of Y, then every
//                   thread takes whole work units (a cell for MRC, an SFBC pair for transmit
//                   diversity): Wiener interpolation of the channel at the unit's subcarriers
//                   (rx_synced.cpp:932-946), MRC (1204-1306) or SFBC combining (1335-1392),
//                   srsRAN-style int16 soft demapping and descrambling (pcc_enc.cpp:297,
//                   pdc_enc.cpp:339-344).
//  rx_mimo_kernel   one wavefront per packet: the MIMO report's codebook search at the packet end.
//  rx_mimo_detail_kernel  one WG per packet, only with a non-default dnrp_ctx_set_rx_mimo_report: the same
//                   search with the chosen metric and start, every score, and the rank / precoder report.
// Y layout: [packet][N_RX][n_sym_total][Nf_pad] float2 (rx_fft_kernel).
#include "device_common.hpp"
#include "experiments.hpp"
#include "kernels.hpp"
#include "rx_eq.hpp"

namespace dnrp::dev {

// ===================================================================== SNR chain
constexpr uint32_t SNR_THREADS = 256, MAX_DOPS = RX_MAX_DOPS;
constexpr int SNR_ROUNDS = 4;  // DRS cells per (symbol, stream) <= 256 (b <= 16: 224)

template <int NRX>
__global__ void __launch_bounds__(SNR_THREADS) rx_snr_kernel(rx_snr_args A) {
    __shared__ double s1s[MAX_DOPS], s2s[MAX_DOPS];
    const uint32_t pkt = rx_slot_of(A.sel, blockIdx.x), nd = A.n_drs;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nw = SNR_THREADS / 64;
    const size_t ast = size_t(A.n_sym_total) * A.Nf_pad;
    const float2* Yp = A.Y + size_t(pkt) * NRX * ast;
    if (A.snr_part) {  // the front end's partial sums of every RX antenna (one lane each)
        for (uint32_t d = wave; d < A.n_dops; d += nw) {
            const uint32_t meta = __builtin_amdgcn_readfirstlane(A.dmeta[d]);
            const uint32_t l = __builtin_amdgcn_readfirstlane(A.dl[d]);
            const uint32_t tf = meta & 0xFFu;
            double s1 = 0.0, s2 = 0.0;
            if (lane < NRX) {
                const double2 p = A.snr_part[((size_t(pkt) * A.n_sym_total + l) * NRX + lane) * 8 + tf];
                s1 = p.x;
                s2 = p.y;
            }
            for (int o = 32; o > 0; o >>= 1) {
                s1 += __shfl_xor(s1, o);
                s2 += __shfl_xor(s2, o);
            }
            if (lane == 0) {
                s1s[d] = s1;
                s2s[d] = s2;
            }
        }
    }
    for (uint32_t d = A.snr_part ? A.n_dops : wave; d < A.n_dops; d += nw) {
        const uint32_t meta = __builtin_amdgcn_readfirstlane(A.dmeta[d]);
        const uint32_t l = __builtin_amdgcn_readfirstlane(A.dl[d]);
        const uint32_t tf = meta & 0xFFu, tl = (meta >> 8) & 0xFFu, par = (meta >> 16) & 0xFFu;
        const float2* rows = Yp + size_t(l) * A.Nf_pad;
        double s1 = 0.0, s2 = 0.0;
        // lanes take 64 consecutive DRS cells of one transmit stream for every RX antenna at once
        // (the subcarrier index and DRS value are shared by the antennas); the right neighbour of
        // the noise difference comes from the next lane, lane 63 fetches its own
        for (uint32_t t = tf; t <= tl; ++t) {
            const uint32_t* __restrict__ kb = A.drs_k + (par * 4 + (t & 3u)) * nd;
            const float* __restrict__ vv = A.drs_v + t * nd;
            // all SNR_ROUNDS rounds' index loads, then all their cells, in flight together
            uint32_t k[SNR_ROUNDS], k1[SNR_ROUNDS];
            float w[SNR_ROUNDS], w1[SNR_ROUNDS];
#pragma unroll
            for (int r = 0; r < SNR_ROUNDS; ++r) {
                const uint32_t i = 64 * r + lane;
                const bool in = i < nd, nx = lane == 63 && i + 1 < nd;
                k[r] = in ? kb[i] : 0u;
                k1[r] = nx ? kb[i + 1] : 0u;
                w[r] = in ? vv[i] : 0.f;
                w1[r] = nx ? vv[i + 1] : 0.f;
            }
            float2 y[SNR_ROUNDS][NRX], y1[SNR_ROUNDS][NRX];
#pragma unroll
            for (int r = 0; r < SNR_ROUNDS; ++r)
#pragma unroll
                for (int a = 0; a < NRX; ++a) {
                    y[r][a] = rows[a * ast + k[r]];
                    y1[r][a] = rows[a * ast + k1[r]];
                }
#pragma unroll
            for (int r = 0; r < SNR_ROUNDS; ++r) {
                const uint32_t i = 64 * r + lane;
                if (64 * r >= nd) break;
                const bool in = i < nd;
#pragma unroll
                for (int a = 0; a < NRX; ++a) {
                    const float2 v = cscale(y[r][a], w[r]);
                    float2 vn = make_float2(__shfl_down(v.x, 1), __shfl_down(v.y, 1));
                    if (lane == 63) vn = cscale(y1[r][a], w1[r]);
                    if (in) s1 += cnorm(v);
                    if (i + 1 < nd) s2 += cnorm(csub(v, vn));
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o);
            s2 += __shfl_xor(s2, o);
        }
        if (lane == 0) {
            s1s[d] = s1;
            s2s[d] = s2;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    rx_pkt_state* st = A.st + pkt;
    double sn = st->snr_SN, nn = st->snr_N;
    uint32_t sn_cnt = st->snr_SN_cnt, nn_cnt = st->snr_N_cnt;
    auto snr_db = [&]() -> float {
        if (sn <= 0.0 || nn <= 0.0) return 0.f;
        const float Sa = static_cast<float>((sn - nn) / sn_cnt), Na = static_cast<float>(nn / nn_cnt);
        return 10.f * log10f(Sa / Na);
    };
    for (uint32_t d = 0; d < A.n_dops; ++d) {
        const uint32_t meta = A.dmeta[d];
        const uint32_t nts = ((meta >> 8) & 0xFFu) - (meta & 0xFFu) + 1;
        sn += s1s[d];
        nn += s2s[d] / 2.0;
        sn_cnt += A.N_RX * nts * nd;
        nn_cnt += A.N_RX * nts * (nd - 1);
        // nearest profile SNR, ties to the later profile (rx_synced.cpp:863-891)
        const float s = snr_db();
        float best = fabsf(s - A.prof_snr[0]);
        uint32_t pick = 0;
        for (uint32_t i = 1; i < 3; ++i) {
            const float dd = fabsf(s - A.prof_snr[i]);
            if (dd <= best) {
                best = dd;
                pick = i;
            }
        }
        A.lut_d[size_t(pkt) * MAX_DOPS + d] = static_cast<uint8_t>(pick);
        // noise variance per RX cell behind the pick (MMSE regularisation of spatial multiplexing)
        A.nv_d[size_t(pkt) * MAX_DOPS + d] = nn > 0.0 ? static_cast<float>(nn / nn_cnt) : 0.f;
    }
    if (A.is_pdc)
        st->snr_pdc = snr_db();
    else
        st->snr_pcc = snr_db();
}

hipError_t launch_rx_snr(const rx_snr_args& a, uint32_t n, hipStream_t st) {
    if (a.n_dops > MAX_DOPS || a.n_drs > 64 * SNR_ROUNDS || (a.snr_part && a.N_RX > 64)) return hipErrorInvalidValue;
    switch (a.N_RX) {
        case 1: hipLaunchKernelGGL(rx_snr_kernel<1>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        case 2: hipLaunchKernelGGL(rx_snr_kernel<2>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        case 4: hipLaunchKernelGGL(rx_snr_kernel<4>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        case 8: hipLaunchKernelGGL(rx_snr_kernel<8>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ===================================================================== residual STO tracking
// The reference's second STO stage (RX_SYNCED_PARAM_STO_RESIDUAL_BASED_ON_DRS, compiled out in its default
// build): after every DRS symbol the slope of the zero-forced pilots over frequency is added to the
// running increment (estimator_sto.cpp:64-97), and every later symbol is derotated with the new value
// (rx_synced.cpp:767-770). Here the DRS rows of the phase are in Y, derotated with the STF increment alone;
// rotating them by exp(j delta (k - N_b_OCC/2)), delta = running - STF increment, gives the pilots the
// reference measures. One wavefront per (RX antenna, transmit stream) of an op: the pilot products in
// float (as rx_drs_partials'), their sums, the angles, the recurrence and the table in double. The
// DC-straddling pair is 5 subcarriers apart and divided by 4 like the others (estimator_sto.cpp:160).
constexpr uint32_t STO_THREADS = 256;
constexpr uint32_t STO_TS_MAX = 8;  // RX_SYNCED_PARAM_STO_RESIDUAL_BASED_ON_DRS_N_TS_MAX

__global__ void __launch_bounds__(STO_THREADS) rx_sto_track_kernel(rx_sto_args A) {
    __shared__ double ang[8 * STO_TS_MAX];  // per (rx, stream) of the op
    const uint32_t pkt = rx_slot_of(A.sel, blockIdx.x), nd = A.n_drs;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nw = STO_THREADS / 64;
    const size_t ast = size_t(A.n_sym_total) * A.Nf_pad;
    const float2* Yp = A.Y + size_t(pkt) * A.N_RX * ast;
    double* tab = A.tab + size_t(pkt) * A.n_sym_total;
    rx_pkt_state* st = A.st + pkt;
    const double inc0 = st->sto_inc, half = static_cast<double>(A.N_occ / 2);
    // the PDC phase continues where the PCC phase stopped (and leaves that state as it is: a second PDC
    // call on the same PCC batch starts from it again); every thread carries the same recurrence
    double run = A.is_pdc ? st->sto_run : inc0;
    uint32_t d = A.is_pdc ? st->sto_ops : 0u, lf = A.sym_first;
    for (; d < A.n_dops; ++d) {
        const uint32_t l = A.dl[d], meta = A.dmeta[d];
        if (l > A.sym_last) break;
        // a DRS symbol itself is derotated with the value from before its own update (run_cp_fft_scale
        // comes before run_drs_chestim_zf)
        for (uint32_t s = lf + threadIdx.x; s <= l; s += STO_THREADS) tab[s] = run;
        lf = max(lf, l + 1);
        const uint32_t tf = meta & 0xFFu, tl = min((meta >> 8) & 0xFFu, STO_TS_MAX - 1), par = (meta >> 16) & 0xFFu;
        const uint32_t nts = tl >= tf ? tl - tf + 1 : 0u, cnt = A.N_RX * nts;
        const double delta = run - inc0;
        const float2* rows = Yp + size_t(l) * A.Nf_pad;
        for (uint32_t p = wave; p < cnt; p += nw) {
            const uint32_t a = p / nts, t = tf + p % nts;
            const uint32_t* __restrict__ kb = A.drs_k + (par * 4 + (t & 3u)) * nd;
            const float* __restrict__ vv = A.drs_v + t * nd;
            double br = 0.0, bi = 0.0;
            for (uint32_t i = lane; i + 1 < nd; i += 64) {
                const uint32_t k0 = kb[i], k1 = kb[i + 1];
                float2 h0 = cscale(rows[a * ast + k0], vv[i]), h1 = cscale(rows[a * ast + k1], vv[i + 1]);
                if (delta != 0.0) {
                    h0 = cmul(h0, phasor(delta * (static_cast<double>(k0) - half)));
                    h1 = cmul(h1, phasor(delta * (static_cast<double>(k1) - half)));
                }
                const float2 c = cmulc(h0, h1);
                br += c.x;
                bi += c.y;
            }
            for (int o = 32; o > 0; o >>= 1) {
                br += __shfl_xor(br, o);
                bi += __shfl_xor(bi, o);
            }
            if (lane == 0) ang[p] = atan2(bi, br) / static_cast<double>(prm::N_STF_CELLS_SPACING);
        }
        __syncthreads();
        if (cnt) {  // cnt = 0: the stream limit leaves nothing to measure, no update (estimator_sto.cpp:86-88)
            double s = 0.0;
            for (uint32_t p = 0; p < cnt; ++p) s += ang[p];
            run += A.gain * (s / static_cast<double>(cnt));
        }
        __syncthreads();
    }
    for (uint32_t s = lf + threadIdx.x; s <= A.sym_last; s += STO_THREADS) tab[s] = run;
    if (!A.is_pdc && threadIdx.x == 0) {
        st->sto_run = run;
        st->sto_ops = d;
    }
}

hipError_t launch_rx_sto_track(const rx_sto_args& a, uint32_t n, hipStream_t st) {
    if (a.N_RX > 8 || a.n_dops > MAX_DOPS || a.sym_last >= a.n_sym_total || a.sym_first > a.sym_last) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_sto_track_kernel, dim3(n), dim3(STO_THREADS), 0, st, a);
    return hipGetLastError();
}

// ===================================================================== residual CFO tracking
// What the reference's RX_SYNCED_PARAM_CFO_RESIDUAL_BASED_ON_DRS header describes (rx_synced_param.hpp:162-181:
// two OFDM symbols with DRS cells are compared, N_step apart) and its stub does not compute
// (estimator_cfo.cpp:65-74 multiplies neighbouring cells of one symbol). DRS op d at symbol l is compared with
// d', the latest earlier op with the same first stream, at symbol l'. Both rows are in Y mixed with the STF
// values alone. Consecutive DRS symbols of a stream are interlaced two subcarriers apart, so pilot i of d is
// paired with the pilots of d' on either side of it: a timing offset turns the two products by opposite
// angles, which cancel to first order in their sum. C sums h_d conj(h_d') over both pairs, the streams
// TS_first..TS_last and the RX antennas as one complex number (estimator_cfo.cpp:41-53): one wavefront per
// (antenna, stream), products in float, sums per lane and across lanes in double, the (antenna, stream) sums
// added in index order by every thread. theta = wrap(atan2(C) + Psi(l) - Psi(l')) is the rotation the table
// has not removed yet, Psi(l) = table phase - STF phase at the centre of symbol l's transform window; the
// running increment loses gain theta / ((l - l') (CP + N_b_DFT_os)) and the phase stays continuous at the
// first CP sample of symbol l + 1 (mixer.cpp adjust_phase_increment leaves the accumulated phase alone).
// The PCC phase's ops leave their pilots in `keep`: the PDC phase's first pairs reach back to them, and by
// then the front end has written those Y rows again with the table.
constexpr uint32_t CFO_THREADS = 256;
constexpr uint32_t CFO_TS = 4;  // streams of one DRS op (drs.cpp:90-127)

__global__ void __launch_bounds__(CFO_THREADS) rx_cfo_track_kernel(rx_cfo_args A) {
    __shared__ double cr[8 * CFO_TS], ci[8 * CFO_TS];  // per (rx, stream) of the op
    __shared__ double psi[MAX_DOPS];                    // Psi at every op's symbol
    const uint32_t pkt = rx_slot_of(A.sel, blockIdx.x), nd = A.n_drs;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nw = CFO_THREADS / 64;
    const size_t ast = size_t(A.n_sym_total) * A.Nf_pad, kst = size_t(A.N_RX) * CFO_TS * nd;
    const float2* Yp = A.Y + size_t(pkt) * A.N_RX * ast;
    float2* keep = A.keep + size_t(pkt) * RX_CFO_KEEP * kst;
    double2* tab = A.tab + size_t(pkt) * A.n_sym_total;
    rx_pkt_state* st = A.st + pkt;
    const double inc1 = st->inc1, a0 = static_cast<double>(A.n_stf) * A.pin[pkt].inc0;
    auto psi_of = [&](uint32_t l, double a, double inc) {
        return (a - a0) + static_cast<double>((l - 1) * A.sym_len + (A.sym_len - A.Nd) + A.Nd / 2) * (inc - inc1);
    };
    // the PDC phase continues where the PCC phase stopped (and leaves that state as it is: a second PDC
    // call on the same PCC batch starts from it again); every thread carries the same recurrence
    double a = A.is_pdc ? st->cfo_a : a0, run = A.is_pdc ? st->cfo_run : inc1;
    const uint32_t d_first = A.is_pdc ? min(st->cfo_ops, A.n_dops) : 0u;
    for (uint32_t e = threadIdx.x; e < d_first; e += CFO_THREADS) {  // the PCC phase's ops from its table entries
        const double2 t = tab[A.dl[e]];
        psi[e] = psi_of(A.dl[e], t.x, t.y);
    }
    __syncthreads();
    uint32_t d = d_first, lf = A.sym_first;
    for (; d < A.n_dops; ++d) {
        const uint32_t l = A.dl[d], meta = A.dmeta[d];
        if (l > A.sym_last) break;
        // a DRS symbol itself is mixed with the entry from before its own update
        for (uint32_t s = lf + threadIdx.x; s <= l; s += CFO_THREADS) tab[s] = make_double2(a, run);
        lf = max(lf, l + 1);
        const uint32_t tf = meta & 0xFFu, tl = min((meta >> 8) & 0xFFu, tf + CFO_TS - 1), par = (meta >> 16) & 0xFFu;
        const uint32_t nts = tl >= tf ? tl - tf + 1 : 0u, cnt = A.N_RX * nts;
        int dp = -1;  // the latest earlier op of the same stream set
        for (uint32_t e = d; e-- > 0;)
            if ((A.dmeta[e] & 0xFFu) == tf) {
                dp = static_cast<int>(e);
                break;
            }
        const bool kept = dp >= 0 && static_cast<uint32_t>(dp) < d_first;  // its pilots come from `keep`
        if (kept && dp >= static_cast<int>(RX_CFO_KEEP)) dp = -1;
        const bool save = !A.is_pdc && d < RX_CFO_KEEP;
        const double psi_d = psi_of(l, a, run);
        if (threadIdx.x == 0) psi[d] = psi_d;
        const uint32_t lp = dp >= 0 ? A.dl[dp] : 0u, parp = dp >= 0 ? (A.dmeta[dp] >> 16) & 0xFFu : 0u;
        const float2* rows = Yp + size_t(l) * A.Nf_pad;
        const float2* rowp = Yp + size_t(lp) * A.Nf_pad;
        for (uint32_t p = wave; p < cnt && (save || dp >= 0); p += nw) {
            const uint32_t ar = p / nts, tt = p % nts, t = tf + tt;
            const uint32_t* __restrict__ kb = A.drs_k + (par * 4 + (t & 3u)) * nd;
            const uint32_t* __restrict__ kp = A.drs_k + (parp * 4 + (t & 3u)) * nd;
            const float* __restrict__ vv = A.drs_v + t * nd;
            // the cell of d' on the other side of cell i: i - 1 where its cell i lies above, i + 1 where below
            const int sh = kp[0] > kb[0] ? -1 : kp[0] < kb[0] ? 1 : 0;
            const float2* kprow = keep + size_t(kept ? dp : 0) * kst + (size_t(ar) * CFO_TS + tt) * nd;
            auto prev = [&](uint32_t i) {
                return kept ? kprow[i] : cscale(rowp[ar * ast + kp[i]], vv[i]);
            };
            double br = 0.0, bi = 0.0;
            for (uint32_t i = lane; i < nd; i += 64) {
                const float2 h = cscale(rows[ar * ast + kb[i]], vv[i]);
                if (save) keep[size_t(d) * kst + (size_t(ar) * CFO_TS + tt) * nd + i] = h;
                if (dp < 0) continue;
                const float2 c0 = cmulc(h, prev(i));
                br += c0.x;
                bi += c0.y;
                const uint32_t j = i + static_cast<uint32_t>(sh);  // wraps below 0: out of range
                if (sh != 0 && j < nd) {
                    const float2 c1 = cmulc(h, prev(j));
                    br += c1.x;
                    bi += c1.y;
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                br += __shfl_xor(br, o);
                bi += __shfl_xor(bi, o);
            }
            if (lane == 0) {
                cr[p] = br;
                ci[p] = bi;
            }
        }
        __syncthreads();
        if (cnt && dp >= 0) {  // no earlier op of the set, or no stream to measure: no update
            double sr = 0.0, si = 0.0;
            for (uint32_t p = 0; p < cnt; ++p) {
                sr += cr[p];
                si += ci[p];
            }
            const double theta = remainder(atan2(si, sr) + psi_d - psi[dp], 6.283185307179586476925);
            const double nxt = run - A.gain * theta / static_cast<double>((l - lp) * A.sym_len);
            a += static_cast<double>(l * A.sym_len) * (run - nxt);  // continuous at the first CP sample of l + 1
            run = nxt;
        }
        __syncthreads();
    }
    for (uint32_t s = lf + threadIdx.x; s <= A.sym_last; s += CFO_THREADS) tab[s] = make_double2(a, run);
    if (!A.is_pdc && threadIdx.x == 0) {
        st->cfo_a = a;
        st->cfo_run = run;
        st->cfo_ops = d;
    }
}

hipError_t launch_rx_cfo_track(const rx_cfo_args& a, uint32_t n, hipStream_t st) {
    if (a.N_RX > 8 || a.n_dops > MAX_DOPS || a.sym_last >= a.n_sym_total || a.sym_first > a.sym_last || a.Nd > a.sym_len ||
        !a.keep)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_cfo_track_kernel, dim3(n), dim3(CFO_THREADS), 0, st, a);
    return hipGetLastError();
}

// ===================================================================== cells
constexpr uint32_t CELL_THREADS = 512;
#ifndef DNRP_CELLS_PILOT_PRE
#define DNRP_CELLS_PILOT_PRE 0  // 1: pilot sources issued before the weight-table staging: neutral (rx_pcc 0.347 /
                                // 0.349 vs 0.345 / 0.349 ms, C4SM rx_pdc 17.58 / 17.66 vs 17.58 / 17.67), off
#endif

template <int NRX, int NT, bool SM = false, int NBPS = 0>
__global__ void __launch_bounds__(CELL_THREADS) rx_cells_kernel(rx_cells_args A) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const uint32_t zst = zfi_stride(A.n_drs);
    float2* zfi = smem;                                                       // [NRX][NT][zst]
    float* wtab = reinterpret_cast<float*>(zfi + NRX * NT * zst);            // slots: mode l, mode lr
    cell_seg* sg = reinterpret_cast<cell_seg*>(wtab + A.wcap[0] + A.wcap[1]);  // CELL_MAX_SEGS
    uint32_t* pairs = reinterpret_cast<uint32_t*>(sg + CELL_MAX_SEGS);       // 12
    // XCD-aware: workgroups are dealt round-robin over the 8 XCDs, so workgroup b runs on XCD b % 8;
    // the epochs of one packet are consecutive on one XCD (b / 8 = packet-of-XCD * n_epochs + epoch)
    // and re-read the packet's DRS cells from that XCD's L2 instead of HBM
    const uint32_t xs = blockIdx.x >> 3;
    const uint32_t pl = (xs / A.n_epochs) * 8 + (blockIdx.x & 7u), ep = xs % A.n_epochs;
    if (pl >= A.n_pkt) return;
    const uint32_t pkt = rx_slot_of(A.sel, pl), row = rx_row_of(A.sel, pl);
    const rx_epoch* E = A.epochs + ep;
    const uint32_t units = E->units, seg0 = E->seg0, nseg = E->seg1 - E->seg0;
    const float2* Yp = A.Y + size_t(pkt) * NRX * A.n_sym_total * A.Nf_pad;
    const uint32_t tid = threadIdx.x;
    // the epoch's segments share one DRS count (host-checked), so one LUT profile: weight table
    // slot m holds the profile's table of mode m (l / lr)
    const uint8_t* lutp = A.lut_d + size_t(pkt) * RX_MAX_DOPS;
    const uint32_t dc = nseg ? A.segs[seg0].drs_cnt : 0u;
    const uint32_t prof = dc ? lutp[dc - 1] : 0u;
    // the pilot buffer's dependent source loads first (pilot_offsets, where 2 n_drs <= threads), so
    // they overlap the weight-table staging instead of following it
    const bool ppre = DNRP_CELLS_PILOT_PRE && 2 * A.n_drs <= CELL_THREADS;  // uniform
    const bool pact = ppre && tid < 2 * A.n_drs;
    uint32_t pyk[NT] = {}, pok = 0;
    float pdv[NT] = {};
    if (pact) pilot_offsets<NT>(A, E, tid, pyk, pdv, pok);
    if (units) {
#pragma unroll
        for (uint32_t m = 0; m < 2; ++m) {
            const rx_lut LT = A.luts[m * 3 + prof];
            for (uint32_t i = tid; i < LT.nw; i += CELL_THREADS) wtab[m * A.wcap[0] + i] = LT.w[i];
        }
        if (tid < nseg) {
            const rx_seg S = A.segs[seg0 + tid];
            const rx_lut LT = A.luts[S.mode * 3 + prof];
            cell_seg c;
            c.u0 = S.u0;
            c.j0 = S.j0;
            c.l = S.l;
            c.info = (S.mode & 1u) | (S.swap & 3u) << 1 | (S.off & 0xFFu) << 4 | LT.n << 12;
            c.pw = LT.pw + size_t(S.rel) * 4 * (A.N_occ + 1);
            c.wbase = (S.mode & 1u) * A.wcap[0];
            c.twin = 0;
            sg[tid] = c;
        }
        if (tid < 12) pairs[tid] = A.pair[tid];
    }
    if constexpr (!experiment(XS_CELLS_SKIP_PRO)) {
        if (ppre)
            pilot_cells<NRX, NT>(A, Yp, zfi, tid, CELL_THREADS, pact, pyk, pdv, pok);
        else
            build_pilots<NRX, NT, cells_ai(NRX, NT)>(A, E, Yp, zfi, tid, CELL_THREADS);
    }
    __syncthreads();
    if constexpr (experiment(XS_CELLS_SKIP_MAIN)) {
        if (tid < units) A.llr[size_t(row) * A.llr_stride + tid] = static_cast<int16_t>(zfi[tid].x);
        return;
    }
    constexpr bool wave_mf = SM && experiment(XS_MMSE_MFMA) && NT == 4;
    if (!wave_mf && tid >= units) return;
    const uint8_t* __restrict__ seq = A.is_pdc ? A.pdc_seq[row] : A.pcc_seq;
    int16_t* __restrict__ llr = A.llr + size_t(row) * A.llr_stride;
    if constexpr (wave_mf) {
        // experiment: MFMA Gram (rx_eq.hpp gram_mfma) needs every lane of the wave, so the wave runs
        // a uniform trip count over clamped units and stores only its real ones
        const float nv = dc ? A.nv_d[size_t(pkt) * RX_MAX_DOPS + dc - 1] : 0.f;
        const uint32_t wf = tid & ~63u;
        if (wf >= units) return;
        const uint32_t nit = (units - wf + CELL_THREADS - 1) / CELL_THREADS;
        float2* scr = reinterpret_cast<float2*>(reinterpret_cast<char*>(smem) +
                                                (cell_lds_bytes(NRX, NT, A.n_drs, A.wcap[0], A.wcap[1]) + 15) / 16 * 16) +
                      (tid >> 6) * NRX * 4 * 24;
        auto cl = [&](uint32_t x) { return min(x, units - 1); };
        uint32_t si = 0;
        unit_a na;
        unit_sm<NRX, NT> cur;
        uint32_t u = tid;
        unit_stage_a(A, sg, nseg, si, cl(u), 1u, na);
        unit_stage_b_sm<NRX, NT>(A, sg, Yp, seq, na, cur);
        if (nit > 1) unit_stage_a(A, sg, nseg, si, cl(u + CELL_THREADS), 1u, na);
        for (uint32_t it = 0; it < nit; ++it, u += CELL_THREADS) {
            unit_sm<NRX, NT> nb;
            const bool m1 = it + 1 < nit, m2 = it + 2 < nit;
            if (m1) unit_stage_b_sm<NRX, NT>(A, sg, Yp, seq, na, nb);
            if (m2) unit_stage_a(A, sg, nseg, si, cl(u + 2 * CELL_THREADS), 1u, na);
            eq_mmse<NRX, NT, NBPS>(A, sg, zfi, wtab, zst, nv, cur, llr, scr, u < units);
            if (m1) cur = nb;
        }
        return;
    }
    if constexpr (SM) {  // spatial multiplexing: unit = one cell carrying NT symbols, MMSE (rx_eq.hpp)
        const float nv = dc ? A.nv_d[size_t(pkt) * RX_MAX_DOPS + dc - 1] : 0.f;
        uint32_t si = 0;
        unit_a na;
        unit_sm<NRX, NT> cur;
        uint32_t u = tid;
        unit_stage_a(A, sg, nseg, si, u, 1u, na);
        unit_stage_b_sm<NRX, NT>(A, sg, Yp, seq, na, cur);
        if (u + CELL_THREADS < units) unit_stage_a(A, sg, nseg, si, u + CELL_THREADS, 1u, na);
        for (; u < units; u += CELL_THREADS) {
            unit_sm<NRX, NT> nb;
            const bool m1 = u + CELL_THREADS < units, m2 = u + 2 * CELL_THREADS < units;
            if (m1) unit_stage_b_sm<NRX, NT>(A, sg, Yp, seq, na, nb);
            if (m2) unit_stage_a(A, sg, nseg, si, u + 2 * CELL_THREADS, 1u, na);
            eq_mmse<NRX, NT, NBPS>(A, sg, zfi, wtab, zst, nv, cur, llr);
            if (m1) cur = nb;
        }
        return;
    }
    constexpr uint32_t per_unit = NT == 1 ? 1u : 2u;
    // stage A two units ahead, stage B one unit ahead of eq_compute (rx_eq.hpp)
    uint32_t si = 0;
    unit_a na;
    unit_b<NRX, NT> cur;
    uint32_t u = tid;
    const __amdgpu_buffer_rsrc_t yr = y_rows(A, Yp);
    unit_stage_a(A, sg, nseg, si, u, per_unit, na);
    unit_stage_b<NRX, NT>(A, sg, pairs, yr, seq, na, cur);
    if (u + CELL_THREADS < units) unit_stage_a(A, sg, nseg, si, u + CELL_THREADS, per_unit, na);
    for (; u < units; u += CELL_THREADS) {
        unit_b<NRX, NT> nb;
        const bool m1 = u + CELL_THREADS < units, m2 = u + 2 * CELL_THREADS < units;
        if (m1) unit_stage_b<NRX, NT>(A, sg, pairs, yr, seq, na, nb);
        if (m2) unit_stage_a(A, sg, nseg, si, u + 2 * CELL_THREADS, per_unit, na);
        eq_compute<NRX, NT, NBPS>(A, sg, zfi, wtab, zst, cur, llr);
        if (m1) cur = nb;
    }
}

hipError_t launch_rx_cells(const rx_cells_args& a, uint32_t n, hipStream_t st) {
    const size_t lds = cell_lds_bytes(a.N_RX, a.NT, a.n_drs, a.wcap[0], a.wcap[1]);
    if (lds > 160 * 1024 || a.n_pkt != n || !y_rows_fit(a)) return hipErrorInvalidValue;
    const dim3 g((n + 7) / 8 * 8 * a.n_epochs), b(CELL_THREADS);
    // 256-QAM (N_bps = 8, the bench's C3 / C4) with the demapper width compiled in
#define DNRP_CELLS(R, T)                                                                 \
    if (a.N_RX == R && a.NT == T) {                                                      \
        if (a.N_bps == 8)                                                                \
            hipLaunchKernelGGL((rx_cells_kernel<R, T, false, 8>), g, b, lds, st, a);     \
        else                                                                             \
            hipLaunchKernelGGL((rx_cells_kernel<R, T>), g, b, lds, st, a);               \
        return hipGetLastError();                                                        \
    }
    DNRP_CELLS(1, 1)
    DNRP_CELLS(2, 1)
    DNRP_CELLS(4, 1)
    DNRP_CELLS(8, 1)
    DNRP_CELLS(2, 2)
    DNRP_CELLS(4, 2)
    DNRP_CELLS(8, 2)
    DNRP_CELLS(4, 4)
    DNRP_CELLS(8, 4)
#undef DNRP_CELLS
    return hipErrorInvalidValue;
}

hipError_t launch_rx_cells_sm(const rx_cells_args& a, uint32_t n, hipStream_t st) {
    size_t lds = cell_lds_bytes(a.N_RX, a.NT, a.n_drs, a.wcap[0], a.wcap[1]);
    if (experiment(XS_MMSE_MFMA) && a.NT == 4) lds = (lds + 15) / 16 * 16 + CELL_THREADS / 64 * a.N_RX * 4 * 24 * sizeof(float2);
    if (lds > 160 * 1024 || a.n_pkt != n) return hipErrorInvalidValue;
    const dim3 g((n + 7) / 8 * 8 * a.n_epochs), b(CELL_THREADS);
    // the demapper width compiled in for 64- and 256-QAM
#define DNRP_CELLS_SM(R, T)                                                              \
    if (a.N_RX == R && a.NT == T) {                                                      \
        if (a.N_bps == 6)                                                                \
            hipLaunchKernelGGL((rx_cells_kernel<R, T, true, 6>), g, b, lds, st, a);      \
        else if (a.N_bps == 8)                                                           \
            hipLaunchKernelGGL((rx_cells_kernel<R, T, true, 8>), g, b, lds, st, a);      \
        else                                                                             \
            hipLaunchKernelGGL((rx_cells_kernel<R, T, true>), g, b, lds, st, a);         \
        return hipGetLastError();                                                        \
    }
    DNRP_CELLS_SM(2, 2)
    DNRP_CELLS_SM(4, 2)
    DNRP_CELLS_SM(8, 2)
    DNRP_CELLS_SM(4, 4)
    DNRP_CELLS_SM(8, 4)
#undef DNRP_CELLS_SM
    return hipErrorInvalidValue;
}

// ===================================================================== MIMO report
// estimator_mimo.cpp:80-222 (mode_single_spatial_stream_3_7, metric HIGHEST_MIN_RX_POWER): lane wm
// scores codebook entry wm (min over the receive side of |sum_tx sum_c H w|, times the entry's
// scaling), the first maximum wins. H: the latest zero-forced DRS value of each (rx, ts) at the 4
// wideband cells (RX_SYNCED_PARAM_MIMO_N_WIDEBAND_CELLS), float sums in the reference's order.
__device__ uint32_t mimo_pick(const float2* H, uint32_t N_TX_virt, uint32_t N_RX_virt, bool transposed, uint32_t N_TS,
                              const float2* W, const float* sc, uint32_t A0, uint32_t ncb, uint32_t lane) {
    float best = -1.0e6f;
    uint32_t bidx = 0xFFFFFFFFu;
    for (uint32_t wm = A0 + lane; wm < ncb; wm += 64) {
        float power_inner = 1.0e6f;
        for (uint32_t rx = 0; rx < N_RX_virt; ++rx) {
            float2 sum = make_float2(0.f, 0.f);
            for (uint32_t tx = 0; tx < N_TX_virt; ++tx) {
                const float2 w = W[wm * N_TX_virt + tx];
                const uint32_t hrx = transposed ? tx : rx, hts = transposed ? rx : tx;
                float2 part = make_float2(0.f, 0.f);
                for (uint32_t c = 0; c < 4; ++c) part = cadd(part, cmul(H[(hrx * N_TS + hts) * 4 + c], w));
                sum = cadd(sum, part);
            }
            const float p = hypotf(sum.x, sum.y);
            if (p < power_inner) power_inner = p;
        }
        power_inner *= sc[wm];
        if (best < power_inner) {
            best = power_inner;
            bidx = wm;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const uint32_t oi = __shfl_xor(bidx, o);
        if (ob > best || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    return bidx;
}

__global__ void __launch_bounds__(64) rx_mimo_kernel(rx_mimo_args A) {
    __shared__ float2 H[8 * 8 * 4];
    const uint32_t pkt = rx_slot_of(A.sel, blockIdx.x), row = rx_row_of(A.sel, blockIdx.x), lane = threadIdx.x;
    const float2* Yp = A.Y + size_t(pkt) * A.N_RX * A.n_sym_total * A.Nf_pad;
    for (uint32_t e = lane; e < A.N_RX * A.N_TS * 4; e += 64) {
        const uint32_t rx = e / (A.N_TS * 4), tc = e % (A.N_TS * 4);
        if (A.zd) {  // the zero-forced pilots of the fused receiver: the same values, sign applied
            const uint32_t zc = A.zcells[tc];
            H[e] = A.zd[(((size_t(pkt) * A.zd_dops + (zc >> 16)) * A.N_RX + rx) * 4 + tc / 4) * A.zd_row + (zc & 0xFFFFu)];
            continue;
        }
        const uint32_t cell = A.cells[tc];
        H[e] = cscale(Yp[(size_t(rx) * A.n_sym_total + (cell >> 16)) * A.Nf_pad + (cell & 0xFFFFu)], A.signs[tc]);
    }
    __syncthreads();
    const uint32_t idx = A.N_TS == 1 ? 0u : mimo_pick(H, A.N_TS, A.N_RX, false, A.N_TS, A.Wtx, A.stx, A.A_tx, A.ncb_tx, lane);
    const uint32_t idr = A.N_RX == 1 ? 0u : mimo_pick(H, A.N_RX, A.N_TS, true, A.N_TS, A.Wrx, A.srx, A.A_rx, A.ncb_rx, lane);
    if (lane == 0) {
        A.out[3 * row] = A.N_TS;
        A.out[3 * row + 1] = idx;
        A.out[3 * row + 2] = idr;
    }
}

hipError_t launch_rx_mimo(const rx_mimo_args& a, uint32_t n, hipStream_t st) {
    if (a.N_RX > 8 || a.N_TS > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_mimo_kernel, dim3(n), dim3(64), 0, st, a);
    return hipGetLastError();
}

// ===================================================================== MIMO report, detailed
// dnrp_ctx_set_rx_mimo_report: estimator_mimo.cpp:162-271 with its two build options as arguments
// (RX_SYNCED_PARAM_MODE_3_7_METRIC, rx_synced_param.hpp:273-283: metric; ..._USE_ALL_W_MATRICES_OR_ONLY_NON_ZERO,
// :286: the search start A0), every candidate's score, and the rank / precoder report for spatial
// multiplexing the reference leaves unset (mimo_report.hpp:51-58). One workgroup of 256 threads per packet on
// the stage rx_mimo_kernel gathers: wave 0 scores the transmit-side codebook, wave 1 the reciprocal one
// (one candidate per lane, mimo_pick's arithmetic and order); then one thread per (rank slot, codebook
// entry, wideband cell) computes the cell's MMSE rate, the entries' rates are their cells' sums in fixed order
// and one thread picks. Every word of the row is written once, by one thread, with plain stores.
constexpr uint32_t MIMO_D_THREADS = 256;
constexpr uint32_t MIMO_D_MAX_ENTRIES = 64;  // codebook entries over the three rank slots: at most 28 + 22 + 5
constexpr uint32_t MIMO_D_UINT_NONE = 0xFFFFFFFFu;

// lane wm scores candidate wm of a single-stream codebook (ncb <= 64); returns the winner, *score_out the
// lane's score times the scaling factor (NaN where the lane has no candidate in [A0, ncb))
__device__ uint32_t mimo_pick_scores(const float2* H, uint32_t N_TX_virt, uint32_t N_RX_virt, bool transposed, uint32_t N_TS,
                                     const float2* W, const float* sc, uint32_t A0, uint32_t ncb, uint32_t metric,
                                     uint32_t lane, float* score_out) {
    const bool smaller = metric == 2;  // MIN_SPREAD_RX_POWER: strictly smaller replaces, from +1e6
    float best = smaller ? 1.0e6f : -1.0e6f;
    uint32_t bidx = MIMO_D_UINT_NONE;
    float score = __builtin_nanf("");
    const uint32_t wm = lane;
    if (wm >= A0 && wm < ncb) {
        float power_inner = metric == 0 ? 1.0e6f : 0.0f, power_max = -1.0e6f, power_min = 1.0e6f;
        for (uint32_t rx = 0; rx < N_RX_virt; ++rx) {
            float2 sum = make_float2(0.f, 0.f);
            for (uint32_t tx = 0; tx < N_TX_virt; ++tx) {
                const float2 w = W[wm * N_TX_virt + tx];
                const uint32_t hrx = transposed ? tx : rx, hts = transposed ? rx : tx;
                float2 part = make_float2(0.f, 0.f);
                for (uint32_t c = 0; c < 4; ++c) part = cadd(part, cmul(H[(hrx * N_TS + hts) * 4 + c], w));
                sum = cadd(sum, part);
            }
            const float p = hypotf(sum.x, sum.y);
            if (metric == 0) {
                if (p < power_inner) power_inner = p;
            } else if (metric == 1) {
                power_inner += p;
            } else {
                power_min = fminf(power_min, p);
                power_max = fmaxf(power_max, p);
                power_inner = power_max - power_min;
            }
        }
        power_inner *= sc[wm];
        score = power_inner;
        if (smaller ? best > power_inner : best < power_inner) {
            best = power_inner;
            bidx = wm;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const uint32_t oi = __shfl_xor(bidx, o);
        if ((smaller ? ob < best : ob > best) || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    *score_out = score;
    return bidx;
}

// sum over the R layers of log2(1 + MMSE SINR) of one wideband cell c through the precoder W [N_TS][R] times sc:
// G = He^H He + nv I by Cholesky, [G^-1]_ii from the inverse of its factor, in float registers
template <int R>
__device__ float mimo_cell_rate(const float2* H, uint32_t N_RX, uint32_t N_TS, uint32_t c, const float2* W, float sc, float nv) {
    float2 G[R][R];  // lower triangle
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) G[i][j] = make_float2(i == j ? nv : 0.f, 0.f);
    for (uint32_t rx = 0; rx < N_RX; ++rx) {
        float2 he[R];
#pragma unroll
        for (int i = 0; i < R; ++i) he[i] = make_float2(0.f, 0.f);
        for (uint32_t ts = 0; ts < N_TS; ++ts) {
            const float2 h = H[(rx * N_TS + ts) * 4 + c];
#pragma unroll
            for (int i = 0; i < R; ++i) he[i] = cadd(he[i], cmul(h, W[ts * R + i]));
        }
#pragma unroll
        for (int i = 0; i < R; ++i) he[i] = cscale(he[i], sc);
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) G[i][j] = cadd(G[i][j], cmulc(he[j], he[i]));  // conj(he_i) he_j
    }
    // G = L L^H in place (lower), the diagonal real
#pragma unroll
    for (int j = 0; j < R; ++j) {
        float d = G[j][j].x;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= cnorm(G[j][k]);
        const float l = sqrtf(d), il = 1.0f / l;
        G[j][j] = make_float2(l, 0.f);
#pragma unroll
        for (int i = j + 1; i < R; ++i) {
            float2 s = G[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = csub(s, cmulc(G[i][k], G[j][k]));
            G[i][j] = cscale(s, il);
        }
    }
    // X = L^-1 (lower); [G^-1]_ii = sum_k |X[k][i]|^2
    float2 X[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float il = 1.0f / G[i][i].x;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (j > i) {
                X[i][j] = make_float2(0.f, 0.f);
                continue;
            }
            float2 s = make_float2(i == j ? 1.f : 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < i; ++k)
                if (k >= j) s = csub(s, cmul(G[i][k], X[k][j]));
            X[i][j] = cscale(s, il);
        }
    }
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        float d = 0.f;
#pragma unroll
        for (int k = i; k < R; ++k) d += cnorm(X[k][i]);
        r += -log2f(nv * d);
    }
    return r;
}

__global__ void __launch_bounds__(MIMO_D_THREADS) rx_mimo_detail_kernel(rx_mimo_detail_args D) {
    __shared__ float2 H[8 * 8 * 4];
    __shared__ float cell_rate[MIMO_D_MAX_ENTRIES * 4], entry_rate[MIMO_D_MAX_ENTRIES];
    __shared__ float nvs[2];
    __shared__ uint32_t picks[2];
    const rx_mimo_args& A = D.M;
    const uint32_t pkt = rx_slot_of(A.sel, blockIdx.x), row = rx_row_of(A.sel, blockIdx.x);
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t N_RX = A.N_RX, N_TS = A.N_TS;
    rx_mimo_detail_row* out = D.rows + row;
    const float2* Yp = A.Y + size_t(pkt) * N_RX * A.n_sym_total * A.Nf_pad;
    for (uint32_t e = tid; e < N_RX * N_TS * 4; e += MIMO_D_THREADS) {
        const uint32_t rx = e / (N_TS * 4), tc = e % (N_TS * 4);
        if (A.zd) {  // the zero-forced pilots of the fused receiver (rx_mimo_kernel)
            const uint32_t zc = A.zcells[tc];
            H[e] = A.zd[(((size_t(pkt) * A.zd_dops + (zc >> 16)) * N_RX + rx) * 4 + tc / 4) * A.zd_row + (zc & 0xFFFFu)];
            continue;
        }
        const uint32_t cell = A.cells[tc];
        H[e] = cscale(Yp[(size_t(rx) * A.n_sym_total + (cell >> 16)) * A.Nf_pad + (cell & 0xFFFFu)], A.signs[tc]);
    }
    __syncthreads();
    // the row's stage [8][8][4], zero beyond N_RX / N_TS
    for (uint32_t e = tid; e < 8 * 8 * 4; e += MIMO_D_THREADS) {
        const uint32_t rx = e >> 5, ts = (e >> 2) & 7u, c = e & 3u;
        const float2 h = rx < N_RX && ts < N_TS ? H[(rx * N_TS + ts) * 4 + c] : make_float2(0.f, 0.f);
        out->H[rx][ts][c][0] = h.x;
        out->H[rx][ts][c][1] = h.y;
    }
    // noise variance: the SNR chain's at the packet end, floored at 2^-14 of the stage's mean power
    if (tid == 0) {
        double p = 0.0;
        const uint32_t cnt = N_RX * N_TS * 4;
        for (uint32_t e = 0; e < cnt; ++e) p += static_cast<double>(cnorm(H[e]));
        const float P = static_cast<float>(p / static_cast<double>(cnt));
        const float nv = D.n_dops ? D.nv_d[size_t(pkt) * RX_MAX_DOPS + D.n_dops - 1] : 0.f;
        nvs[0] = nv;
        nvs[1] = fmaxf(fmaxf(nv, 6.103515625e-05f * P), 1.17549435e-38f);
    }
    // the two single-stream searches, one wave each
    if (wave < 2) {
        const bool rec = wave == 1;
        const uint32_t n_virt = rec ? N_RX : N_TS;
        float score = __builtin_nanf("");
        uint32_t idx = 0u;
        if (n_virt != 1)
            idx = rec ? mimo_pick_scores(H, N_RX, N_TS, true, N_TS, A.Wrx, A.srx, A.A_rx, A.ncb_rx, D.metric, lane, &score)
                      : mimo_pick_scores(H, N_TS, N_RX, false, N_TS, A.Wtx, A.stx, A.A_tx, A.ncb_tx, D.metric, lane, &score);
        if (lane < RX_MIMO_MAX_CB) (rec ? out->score_rx : out->score_tx)[lane] = score;
        if (lane == 0) picks[wave] = idx;
    }
    __syncthreads();
    // spatial multiplexing: one thread per (rank slot, entry, cell), entries in slot order
    const float nv = nvs[1];
    const uint32_t e1 = D.sm_ncb[0], e2 = e1 + D.sm_ncb[1], e3 = e2 + D.sm_ncb[2];
    if (tid < e3 * 4) {
        const uint32_t en = tid >> 2, c = tid & 3u;
        const uint32_t s = en < e1 ? 0u : en < e2 ? 1u : 2u, cb = en - (s == 0 ? 0u : s == 1 ? e1 : e2);
        const uint32_t R = 1u << s;
        const float2* W = D.Wsm + D.sm_woff[s] + cb * N_TS * R;
        const float sc = D.ssm[D.sm_cboff[s] + cb];
        cell_rate[tid] = s == 0   ? mimo_cell_rate<1>(H, N_RX, N_TS, c, W, sc, nv)
                         : s == 1 ? mimo_cell_rate<2>(H, N_RX, N_TS, c, W, sc, nv)
                                  : mimo_cell_rate<4>(H, N_RX, N_TS, c, W, sc, nv);
    }
    __syncthreads();
    if (tid < e3) entry_rate[tid] = (cell_rate[4 * tid] + cell_rate[4 * tid + 1] + cell_rate[4 * tid + 2] + cell_rate[4 * tid + 3]) / 4.0f;
    __syncthreads();
    if (tid < 3 * RX_MIMO_MAX_CB) {
        const uint32_t s = tid / RX_MIMO_MAX_CB, cb = tid % RX_MIMO_MAX_CB;
        const uint32_t base = s == 0 ? 0u : s == 1 ? e1 : e2;
        out->rate_cb[s][cb] = cb < D.sm_ncb[s] ? entry_rate[base + cb] : __builtin_nanf("");
    }
    if (tid != 0) return;
    // the first maximum per rank, then the rank: strictly greater replaces, so ties go to the lower index / rank
    uint32_t RI = 0u, PMI = MIMO_D_UINT_NONE;
    float rate_RI = 0.f;
    for (uint32_t s = 0; s < 3; ++s) {
        const uint32_t base = s == 0 ? 0u : s == 1 ? e1 : e2;
        uint32_t pm = MIMO_D_UINT_NONE;
        float rt = __builtin_nanf("");
        for (uint32_t cb = 0; cb < D.sm_ncb[s]; ++cb) {
            const float r = entry_rate[base + cb];
            if (pm == MIMO_D_UINT_NONE || r > rt) {
                rt = r;
                pm = cb;
            }
        }
        out->pmi[s] = pm;
        out->rate[s] = rt;
        if (pm != MIMO_D_UINT_NONE && (RI == 0u || rt > rate_RI)) {
            RI = 1u << s;
            PMI = pm;
            rate_RI = rt;
        }
    }
    out->N_RX = N_RX;
    out->N_TS = N_TS;
    out->nv = nvs[0];
    out->nv_used = nv;
    out->idx_tx = picks[0];
    out->idx_rx = picks[1];
    out->RI = RI;
    out->PMI = PMI;
    out->sinr_eff_dB = RI ? 10.0f * log10f(exp2f(rate_RI / static_cast<float>(RI)) - 1.0f) : __builtin_nanf("");
    A.out[3 * row] = N_TS;
    A.out[3 * row + 1] = picks[0];
    A.out[3 * row + 2] = picks[1];
}

hipError_t launch_rx_mimo_detail(const rx_mimo_detail_args& a, uint32_t n, hipStream_t st) {
    if (a.M.N_RX > 8 || a.M.N_TS > 8 || a.metric > 2 || a.n_dops > RX_MAX_DOPS || a.M.ncb_tx > RX_MIMO_MAX_CB ||
        a.M.ncb_rx > RX_MIMO_MAX_CB)
        return hipErrorInvalidValue;
    uint32_t entries = 0;
    for (int s = 0; s < 3; ++s) {
        if (a.sm_ncb[s] > RX_MIMO_MAX_CB || (a.sm_ncb[s] && (1u << s) > a.M.N_TS)) return hipErrorInvalidValue;
        entries += a.sm_ncb[s];
    }
    if (entries > MIMO_D_MAX_ENTRIES || entries * 4 > MIMO_D_THREADS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_mimo_detail_kernel, dim3(n), dim3(MIMO_D_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace dnrp::dev
