// RX back end of the synchronised receiver, the kernels that walk a phase's DRS ops once per packet
// (rx_drs_view); the cells kernel is in rx_cells.hip, the MIMO report in rx_mimo.hip.
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
//  rx_aoa_kernel    one WG per packet, only with the angle-of-arrival report on, at the end of the PDC phase:
//                   the spatial covariance of the zero-forced pilots of every DRS op of the packet and its
//                   Bartlett scan (estimator_aoa_t, empty in the reference).
// Y layout: [packet][N_RX][n_sym_total][Nf_pad] float2 (rx_fft_kernel).
#include "device_common.hpp"
#include "kernels.hpp"

namespace dnrp::dev {

constexpr uint32_t MAX_DOPS = RX_MAX_DOPS;

// Transmit stream t of a DRS op with parity par: the subcarrier indices and values of its DRS cells
struct drs_stream {
    const uint32_t* __restrict__ k;
    const float* __restrict__ v;
    __device__ drs_stream(const rx_drs_view& V, uint32_t par, uint32_t t)
        : k(V.drs_k + (par * 4 + (t & 3u)) * V.n_drs), v(V.drs_v + t * V.n_drs) {}
    // the zero-forced pilot w_i y_i of cell i from one antenna's Y row of the op's symbol
    __device__ float2 zf(const float2* row, uint32_t i) const { return cscale(row[k[i]], v[i]); }
};

// ===================================================================== SNR chain
constexpr uint32_t SNR_THREADS = 256;
constexpr int SNR_ROUNDS = 4;  // DRS cells per (symbol, stream) <= 256 (b <= 16: 224)

template <int NRX>
__global__ void __launch_bounds__(SNR_THREADS) rx_snr_kernel(rx_snr_args A) {
    __shared__ double s1s[MAX_DOPS], s2s[MAX_DOPS];
    const rx_drs_view& V = A.V;
    const uint32_t pkt = rx_slot_of(V.sel, blockIdx.x), nd = V.n_drs;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nw = SNR_THREADS / 64;
    const size_t ast = size_t(V.n_sym_total) * V.Nf_pad;
    const float2* Yp = V.Y + size_t(pkt) * NRX * ast;
    if (A.snr_part) {  // the front end's partial sums of every RX antenna (one lane each)
        for (uint32_t d = wave; d < V.n_dops; d += nw) {
            const uint32_t tf = drs_op_of(__builtin_amdgcn_readfirstlane(V.dmeta[d])).tf;
            const uint32_t l = __builtin_amdgcn_readfirstlane(V.dl[d]);
            double s1 = 0.0, s2 = 0.0;
            if (lane < NRX) {
                const double2 p = A.snr_part[((size_t(pkt) * V.n_sym_total + l) * NRX + lane) * 8 + tf];
                s1 = p.x;
                s2 = p.y;
            }
            const double2 s = wave_sum2(s1, s2);
            if (lane == 0) {
                s1s[d] = s.x;
                s2s[d] = s.y;
            }
        }
    }
    for (uint32_t d = A.snr_part ? V.n_dops : wave; d < V.n_dops; d += nw) {
        const drs_op op = drs_op_of(__builtin_amdgcn_readfirstlane(V.dmeta[d]));
        const uint32_t l = __builtin_amdgcn_readfirstlane(V.dl[d]);
        const float2* rows = Yp + size_t(l) * V.Nf_pad;
        double s1 = 0.0, s2 = 0.0;
        // lanes take 64 consecutive DRS cells of one transmit stream for every RX antenna at once
        // (the subcarrier index and DRS value are shared by the antennas); the right neighbour of
        // the noise difference comes from the next lane, lane 63 fetches its own
        for (uint32_t t = op.tf; t <= op.tl; ++t) {
            const drs_stream S(V, op.par, t);
            // all SNR_ROUNDS rounds' index loads, then all their cells, in flight together (so not S.zf)
            uint32_t k[SNR_ROUNDS], k1[SNR_ROUNDS];
            float w[SNR_ROUNDS], w1[SNR_ROUNDS];
#pragma unroll
            for (int r = 0; r < SNR_ROUNDS; ++r) {
                const uint32_t i = 64 * r + lane;
                const bool in = i < nd, nx = lane == 63 && i + 1 < nd;
                k[r] = in ? S.k[i] : 0u;
                k1[r] = nx ? S.k[i + 1] : 0u;
                w[r] = in ? S.v[i] : 0.f;
                w1[r] = nx ? S.v[i + 1] : 0.f;
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
        const double2 s = wave_sum2(s1, s2);
        if (lane == 0) {
            s1s[d] = s.x;
            s2s[d] = s.y;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    rx_pkt_state* st = V.st + pkt;
    double sn = st->snr_SN, nn = st->snr_N;
    uint32_t sn_cnt = st->snr_SN_cnt, nn_cnt = st->snr_N_cnt;
    auto snr_db = [&]() -> float {
        if (sn <= 0.0 || nn <= 0.0) return 0.f;
        const float Sa = static_cast<float>((sn - nn) / sn_cnt), Na = static_cast<float>(nn / nn_cnt);
        return 10.f * log10f(Sa / Na);
    };
    for (uint32_t d = 0; d < V.n_dops; ++d) {
        const drs_op op = drs_op_of(V.dmeta[d]);
        const uint32_t nts = op.tl - op.tf + 1;
        sn += s1s[d];
        nn += s2s[d] / 2.0;
        sn_cnt += V.N_RX * nts * nd;
        nn_cnt += V.N_RX * nts * (nd - 1);
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
    if (V.is_pdc)
        st->snr_pdc = snr_db();
    else
        st->snr_pcc = snr_db();
}

hipError_t launch_rx_snr(const rx_snr_args& a, uint32_t n, hipStream_t st) {
    const rx_drs_view& v = a.V;
    if (v.n_dops > MAX_DOPS || v.n_drs > 64 * SNR_ROUNDS || (a.snr_part && v.N_RX > 64)) return hipErrorInvalidValue;
    switch (v.N_RX) {
        case 1: hipLaunchKernelGGL(rx_snr_kernel<1>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        case 2: hipLaunchKernelGGL(rx_snr_kernel<2>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        case 4: hipLaunchKernelGGL(rx_snr_kernel<4>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        case 8: hipLaunchKernelGGL(rx_snr_kernel<8>, dim3(n), dim3(SNR_THREADS), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ===================================================================== residual trackers, the shared walk
// Both trackers go through the phase's DRS ops in order, every thread carrying the same recurrence: the table
// up to the op's symbol is filled with the running entry (a DRS symbol itself is derotated / mixed with the
// value from before its own update: run_cp_fft_scale comes before run_drs_chestim_zf), the op is measured by
// one wavefront per (RX antenna, stream), the entry is updated between two barriers, and the entries behind
// the last op are filled at the end. The PDC phase continues where the PCC phase stopped and leaves that
// state as it is (a second PDC call on the same PCC batch starts from it again), so only the PCC phase stores.
constexpr uint32_t TRACK_THREADS = 256;

// tab[lf .. l] = e by the workgroup; lf moves behind l
template <class E>
__device__ __forceinline__ void track_fill(E* tab, uint32_t& lf, uint32_t l, E e) {
    for (uint32_t s = lf + threadIdx.x; s <= l; s += TRACK_THREADS) tab[s] = e;
    lf = max(lf, l + 1);
}

// the streams [tf, tl] an op is measured on (the tracker's limit applied to tl) and its (antenna, stream) count
struct track_op {
    uint32_t tf, par, nts, cnt;
    __device__ track_op(const rx_drs_view& V, const drs_op& o, uint32_t tl)
        : tf(o.tf), par(o.par), nts(tl >= o.tf ? tl - o.tf + 1 : 0u), cnt(V.N_RX * nts) {}
};

// one wavefront per pair p = antenna * nts + stream index below cnt: term(p, lane, br, bi) adds the lane's
// share of the pair's complex sum, lane 0 hands the wave's sum to out(p, br, bi)
template <class T, class O>
__device__ __forceinline__ void track_measure(uint32_t cnt, T&& term, O&& out) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t p = wave; p < cnt; p += TRACK_THREADS / 64) {
        double br = 0.0, bi = 0.0;
        term(p, lane, br, bi);
        const double2 b = wave_sum2(br, bi);
        if (lane == 0) out(p, b.x, b.y);
    }
}

static bool track_args_ok(const rx_track_args& a) {
    return a.V.N_RX <= 8 && a.V.n_dops <= MAX_DOPS && a.sym_last < a.V.n_sym_total && a.sym_first <= a.sym_last;
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
constexpr uint32_t STO_TS_MAX = 8;  // RX_SYNCED_PARAM_STO_RESIDUAL_BASED_ON_DRS_N_TS_MAX

__global__ void __launch_bounds__(TRACK_THREADS) rx_sto_track_kernel(rx_sto_args A) {
    __shared__ double ang[8 * STO_TS_MAX];  // per (rx, stream) of the op
    const rx_drs_view& V = A.V;
    const uint32_t pkt = rx_slot_of(V.sel, blockIdx.x), nd = V.n_drs;
    const size_t ast = size_t(V.n_sym_total) * V.Nf_pad;
    const float2* Yp = V.Y + size_t(pkt) * V.N_RX * ast;
    double* tab = A.tab + size_t(pkt) * V.n_sym_total;
    rx_pkt_state* st = V.st + pkt;
    const double inc0 = st->sto_inc, half = static_cast<double>(A.N_occ / 2);
    double run = V.is_pdc ? st->sto_run : inc0;
    uint32_t d = V.is_pdc ? st->sto_ops : 0u, lf = A.sym_first;
    for (; d < V.n_dops; ++d) {
        const uint32_t l = V.dl[d];
        if (l > A.sym_last) break;
        track_fill(tab, lf, l, run);
        const drs_op o = drs_op_of(V.dmeta[d]);
        const track_op op(V, o, min(o.tl, STO_TS_MAX - 1));
        const double delta = run - inc0;
        const float2* rows = Yp + size_t(l) * V.Nf_pad;
        track_measure(
            op.cnt,
            [&](uint32_t p, uint32_t lane, double& br, double& bi) {
                const float2* row = rows + (p / op.nts) * ast;
                const drs_stream S(V, op.par, op.tf + p % op.nts);
                for (uint32_t i = lane; i + 1 < nd; i += 64) {
                    float2 h0 = S.zf(row, i), h1 = S.zf(row, i + 1);
                    if (delta != 0.0) {
                        h0 = cmul(h0, phasor(delta * (static_cast<double>(S.k[i]) - half)));
                        h1 = cmul(h1, phasor(delta * (static_cast<double>(S.k[i + 1]) - half)));
                    }
                    const float2 c = cmulc(h0, h1);
                    br += c.x;
                    bi += c.y;
                }
            },
            [&](uint32_t p, double br, double bi) { ang[p] = atan2(bi, br) / static_cast<double>(prm::N_STF_CELLS_SPACING); });
        __syncthreads();
        if (op.cnt) {  // cnt = 0: the stream limit leaves nothing to measure, no update (estimator_sto.cpp:86-88)
            double s = 0.0;
            for (uint32_t p = 0; p < op.cnt; ++p) s += ang[p];
            run += A.gain * (s / static_cast<double>(op.cnt));
        }
        __syncthreads();
    }
    track_fill(tab, lf, A.sym_last, run);
    if (!V.is_pdc && threadIdx.x == 0) {
        st->sto_run = run;
        st->sto_ops = d;
    }
}

hipError_t launch_rx_sto_track(const rx_sto_args& a, uint32_t n, hipStream_t st) {
    if (!track_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_sto_track_kernel, dim3(n), dim3(TRACK_THREADS), 0, st, a);
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
constexpr uint32_t CFO_TS = 4;  // streams of one DRS op (drs.cpp:90-127)

__global__ void __launch_bounds__(TRACK_THREADS) rx_cfo_track_kernel(rx_cfo_args A) {
    __shared__ double cr[8 * CFO_TS], ci[8 * CFO_TS];  // per (rx, stream) of the op
    __shared__ double psi[MAX_DOPS];                    // Psi at every op's symbol
    const rx_drs_view& V = A.V;
    const uint32_t pkt = rx_slot_of(V.sel, blockIdx.x), nd = V.n_drs;
    const size_t ast = size_t(V.n_sym_total) * V.Nf_pad, kst = size_t(V.N_RX) * CFO_TS * nd;
    const float2* Yp = V.Y + size_t(pkt) * V.N_RX * ast;
    float2* keep = A.keep + size_t(pkt) * RX_CFO_KEEP * kst;
    double2* tab = A.tab + size_t(pkt) * V.n_sym_total;
    rx_pkt_state* st = V.st + pkt;
    const double inc1 = st->inc1, a0 = static_cast<double>(A.n_stf) * A.pin[pkt].inc0;
    auto psi_of = [&](uint32_t l, double a, double inc) {
        return (a - a0) + static_cast<double>((l - 1) * A.sym_len + (A.sym_len - A.Nd) + A.Nd / 2) * (inc - inc1);
    };
    double a = V.is_pdc ? st->cfo_a : a0, run = V.is_pdc ? st->cfo_run : inc1;
    const uint32_t d_first = V.is_pdc ? min(st->cfo_ops, V.n_dops) : 0u;
    for (uint32_t e = threadIdx.x; e < d_first; e += TRACK_THREADS) {  // the PCC phase's ops from its table entries
        const double2 t = tab[V.dl[e]];
        psi[e] = psi_of(V.dl[e], t.x, t.y);
    }
    __syncthreads();
    uint32_t d = d_first, lf = A.sym_first;
    for (; d < V.n_dops; ++d) {
        const uint32_t l = V.dl[d];
        if (l > A.sym_last) break;
        track_fill(tab, lf, l, make_double2(a, run));
        const drs_op o = drs_op_of(V.dmeta[d]);
        const track_op op(V, o, min(o.tl, o.tf + CFO_TS - 1));
        int dp = -1;  // the latest earlier op of the same stream set
        for (uint32_t e = d; e-- > 0;)
            if (drs_op_of(V.dmeta[e]).tf == op.tf) {
                dp = static_cast<int>(e);
                break;
            }
        const bool kept = dp >= 0 && static_cast<uint32_t>(dp) < d_first;  // its pilots come from `keep`
        if (kept && dp >= static_cast<int>(RX_CFO_KEEP)) dp = -1;
        const bool save = !V.is_pdc && d < RX_CFO_KEEP;
        const double psi_d = psi_of(l, a, run);
        if (threadIdx.x == 0) psi[d] = psi_d;
        const uint32_t lp = dp >= 0 ? V.dl[dp] : 0u, parp = dp >= 0 ? drs_op_of(V.dmeta[dp]).par : 0u;
        const float2* rows = Yp + size_t(l) * V.Nf_pad;
        const float2* rowp = Yp + size_t(lp) * V.Nf_pad;
        track_measure(
            save || dp >= 0 ? op.cnt : 0u,
            [&](uint32_t p, uint32_t lane, double& br, double& bi) {
                const uint32_t ar = p / op.nts, tt = p % op.nts;
                const drs_stream S(V, op.par, op.tf + tt), Sp(V, parp, op.tf + tt);
                // the cell of d' on the other side of cell i: i - 1 where its cell i lies above, i + 1 where below
                const int sh = Sp.k[0] > S.k[0] ? -1 : Sp.k[0] < S.k[0] ? 1 : 0;
                const size_t krow = (size_t(ar) * CFO_TS + tt) * nd;
                const float2* kprow = keep + size_t(kept ? dp : 0) * kst + krow;
                auto prev = [&](uint32_t i) { return kept ? kprow[i] : Sp.zf(rowp + ar * ast, i); };
                for (uint32_t i = lane; i < nd; i += 64) {
                    const float2 h = S.zf(rows + ar * ast, i);
                    if (save) keep[size_t(d) * kst + krow + i] = h;
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
            },
            [&](uint32_t p, double br, double bi) {
                cr[p] = br;
                ci[p] = bi;
            });
        __syncthreads();
        if (op.cnt && dp >= 0) {  // no earlier op of the set, or no stream to measure: no update
            double sr = 0.0, si = 0.0;
            for (uint32_t p = 0; p < op.cnt; ++p) {
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
    track_fill(tab, lf, A.sym_last, make_double2(a, run));
    if (!V.is_pdc && threadIdx.x == 0) {
        st->cfo_a = a;
        st->cfo_run = run;
        st->cfo_ops = d;
    }
}

hipError_t launch_rx_cfo_track(const rx_cfo_args& a, uint32_t n, hipStream_t st) {
    if (!track_args_ok(a) || a.Nd > a.sym_len || !a.keep) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_cfo_track_kernel, dim3(n), dim3(TRACK_THREADS), 0, st, a);
    return hipGetLastError();
}

// ===================================================================== angle of arrival
// The project's own estimator (the reference's estimator_aoa_t has empty bodies). R[a][b] sums
// h_a conj(h_b) over every DRS cell of every stream of every op of the PDC plan, h_a the zero-forced pilot of
// antenna a: what is common to the antennas (CFO mixing, STO derotation, the trackers' tables, amp_scale)
// cancels. One wavefront per op, lanes over 64 consecutive cells, every antenna's cell loaded before the first
// product; the upper triangle's products and a lane's sum over its cells of the op in float, the sums across
// lanes and across ops (in index order, by one thread per pair) in double, R rounded to float once and mirrored.
// Then the Bartlett scan of R as stored, in double: lanes over grid points, the argmax by wavefront 0 (the
// lowest index among equal maxima), the parabola and the row by one lane (aoa_finish, shared with the host twin).
constexpr uint32_t AOA_THREADS = 256;

template <int NRX>
__global__ void __launch_bounds__(AOA_THREADS) rx_aoa_kernel(rx_aoa_args A) {
    constexpr int NP = NRX * (NRX + 1) / 2;
    __shared__ double2 part[MAX_DOPS][NP];  // per op and pair (a <= b)
    __shared__ double P[RX_AOA_MAX_GRID];
    __shared__ float Rs[8 * 8 * 2];
    const rx_drs_view& V = A.V;
    const uint32_t pkt = rx_slot_of(V.sel, blockIdx.x), nd = V.n_drs;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nw = AOA_THREADS / 64;
    const size_t ast = size_t(V.n_sym_total) * V.Nf_pad;
    const float2* Yp = V.Y + size_t(pkt) * NRX * ast;
    rx_aoa_row* row = A.rows + rx_row_of(V.sel, blockIdx.x);
    if (threadIdx.x < 8 * 8 * 2) Rs[threadIdx.x] = 0.f;
    for (uint32_t d = wave; d < V.n_dops; d += nw) {
        const drs_op op = drs_op_of(__builtin_amdgcn_readfirstlane(V.dmeta[d]));
        const uint32_t l = __builtin_amdgcn_readfirstlane(V.dl[d]);
        const float2* rows = Yp + size_t(l) * V.Nf_pad;
        float2 acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] = make_float2(0.f, 0.f);
        // one loop over (stream, round of 64 cells): one round's cells in registers beside the running sums
        const uint32_t rounds = (nd + 63) / 64, n_it = (op.tl - op.tf + 1) * rounds;
#pragma unroll 1
        for (uint32_t it = 0; it < n_it; ++it) {
            const drs_stream S(V, op.par, op.tf + it / rounds);
            const uint32_t i = (it % rounds) * 64 + lane;
            const bool in = i < nd;
            const uint32_t k = in ? S.k[i] : 0u;
            const float w = in ? S.v[i] : 0.f;
            float2 h[NRX];
#pragma unroll
            for (int a = 0; a < NRX; ++a) h[a] = rows[a * ast + k];
#pragma unroll
            for (int a = 0; a < NRX; ++a) h[a] = in ? cscale(h[a], w) : make_float2(0.f, 0.f);
            int p = 0;
#pragma unroll
            for (int a = 0; a < NRX; ++a)
#pragma unroll
                for (int b = a; b < NRX; ++b, ++p) {
                    const float2 c = cmulc(h[a], h[b]);
                    acc[p].x += c.x;
                    acc[p].y += c.y;
                }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            // one pair's doubles at a time (the empty statement keeps the conversions in order): all 36 pairs
            // converted ahead of their sums cost 144 registers
            float fx = acc[p].x, fy = acc[p].y;
            asm volatile("" : "+v"(fx), "+v"(fy));
            const double2 s = wave_sum2(static_cast<double>(fx), static_cast<double>(fy));
            if (lane == 0) part[d][p] = s;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    if (threadIdx.x < NP) {
        double sr = 0.0, si = 0.0;
        for (uint32_t d = 0; d < V.n_dops; ++d) {
            sr += part[d][threadIdx.x].x;
            si += part[d][threadIdx.x].y;
        }
        uint32_t a = 0, q = threadIdx.x;  // pair index -> (a, b), a <= b
        while (q >= NRX - a) {
            q -= NRX - a;
            ++a;
        }
        const uint32_t b = a + q;
        const float fr = static_cast<float>(sr), fi = static_cast<float>(si);
        Rs[(a * 8 + b) * 2] = fr;
        if (a != b) {  // the diagonal's imaginary part stays exactly 0, the lower triangle is the exact conjugate
            Rs[(a * 8 + b) * 2 + 1] = fi;
            Rs[(b * 8 + a) * 2] = fr;
            Rs[(b * 8 + a) * 2 + 1] = -fi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 8 * 8 * 2) (&row->R[0][0][0])[threadIdx.x] = Rs[threadIdx.x];
    const double tr = aoa_trace(Rs, NRX);
    for (uint32_t g = threadIdx.x; g < A.n_grid; g += AOA_THREADS)
        P[g] = tr > 0.0 ? aoa_quad(Rs, A.steer + size_t(g) * NRX, NRX) / (static_cast<double>(NRX) * tr) : 0.0;
    __syncthreads();
    if (wave != 0) return;
    double best = -HUGE_VAL;
    uint32_t bi = RX_AOA_NONE;
    for (uint32_t g = lane; g < A.n_grid; g += 64)
        if (P[g] > best) {
            best = P[g];
            bi = g;
        }
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const uint32_t oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
    if (lane != 0) return;
    uint32_t nc = 0;
    for (uint32_t d = 0; d < V.n_dops; ++d) {
        const drs_op op = drs_op_of(V.dmeta[d]);
        nc += (op.tl - op.tf + 1) * nd;
    }
    row->n_cells = nc;
    aoa_finish(Rs, NRX, P, A.n_grid, A.cyclic, A.az0, A.step, tr, bi, row);
}

hipError_t launch_rx_aoa(const rx_aoa_args& a, uint32_t n, hipStream_t st) {
    const rx_drs_view& v = a.V;
    if (v.n_dops > MAX_DOPS || a.n_grid == 0 || a.n_grid > RX_AOA_MAX_GRID || !a.steer || !a.rows) return hipErrorInvalidValue;
    switch (v.N_RX) {
        case 2: hipLaunchKernelGGL(rx_aoa_kernel<2>, dim3(n), dim3(AOA_THREADS), 0, st, a); break;
        case 4: hipLaunchKernelGGL(rx_aoa_kernel<4>, dim3(n), dim3(AOA_THREADS), 0, st, a); break;
        case 8: hipLaunchKernelGGL(rx_aoa_kernel<8>, dim3(n), dim3(AOA_THREADS), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dnrp::dev
