// RX back end of the synchronised receiver: the MIMO report at the packet end.
//
//  rx_mimo_kernel   one wavefront per packet: the MIMO report's codebook search at the packet end.
//  rx_mimo_detail_kernel  one WG per packet, only with a non-default dnrp_ctx_set_rx_mimo_report: the same
//                   search with the chosen metric and start, every score, and the rank / precoder report.
// Y layout: [packet][N_RX][n_sym_total][Nf_pad] float2 (rx_fft_kernel).
#include "device_common.hpp"
#include "kernels.hpp"

namespace dnrp::dev {

// ===================================================================== MIMO report
// estimator_mimo.cpp:80-222 (mode_single_spatial_stream_3_7): codebook entry wm is scored from |sum_tx sum_c H w|
// over the receive side -- its minimum (metric HIGHEST_MIN_RX_POWER, the reference's build), its sum, or its
// spread, rx_synced_param.hpp:273-283 -- times the entry's scaling; the first maximum wins (the first minimum of
// the spread). H: the latest zero-forced DRS value of each (rx, ts) at the 4 wideband cells
// (RX_SYNCED_PARAM_MIMO_N_WIDEBAND_CELLS), float sums in the reference's order.
constexpr uint32_t MIMO_UINT_NONE = 0xFFFFFFFFu;

// the stage H[N_RX][N_TS][4] of slot pkt, filled by the workgroup's nth threads (no barrier)
__device__ void mimo_stage(const rx_mimo_args& A, uint32_t pkt, float2* H, uint32_t tid, uint32_t nth) {
    const float2* Yp = A.Y + size_t(pkt) * A.N_RX * A.n_sym_total * A.Nf_pad;
    for (uint32_t e = tid; e < A.N_RX * A.N_TS * 4; e += nth) {
        const uint32_t rx = e / (A.N_TS * 4), tc = e % (A.N_TS * 4);
        if (A.zd) {  // the zero-forced pilots of the fused receiver: the same values, sign applied
            const uint32_t zc = A.zcells[tc];
            H[e] = A.zd[(((size_t(pkt) * A.zd_dops + (zc >> 16)) * A.N_RX + rx) * 4 + tc / 4) * A.zd_row + (zc & 0xFFFFu)];
            continue;
        }
        const uint32_t cell = A.cells[tc];
        H[e] = cscale(Yp[(size_t(rx) * A.n_sym_total + (cell >> 16)) * A.Nf_pad + (cell & 0xFFFFu)], A.signs[tc]);
    }
}

// One wavefront's search of the single-stream codebook of the transmit side (rec false: (1, N_TS)) or of the
// reciprocal one (rec true: (1, N_RX), the stage transposed) over the entries [A0, ncb); lanes take the entries
// lane, lane + 64, ... Returns the winner, ties to the lower index; *score_out (where given): the score of
// entry `lane`, NaN where that is no entry of the search.
__device__ uint32_t mimo_pick(const rx_mimo_args& A, const float2* H, bool rec, uint32_t metric, uint32_t lane,
                              float* score_out = nullptr) {
    const uint32_t N_TX_virt = rec ? A.N_RX : A.N_TS, N_RX_virt = rec ? A.N_TS : A.N_RX;
    const float2* W = rec ? A.Wrx : A.Wtx;
    const float* sc = rec ? A.srx : A.stx;
    const uint32_t A0 = rec ? A.A_rx : A.A_tx, ncb = rec ? A.ncb_rx : A.ncb_tx;
    const bool smaller = metric == 2;  // MIN_SPREAD_RX_POWER: strictly smaller replaces, from +1e6
    float best = smaller ? 1.0e6f : -1.0e6f, score = __builtin_nanf("");
    uint32_t bidx = MIMO_UINT_NONE;
    for (uint32_t wm = lane; wm < ncb; wm += 64) {
        if (wm < A0) continue;
        float power_inner = metric == 0 ? 1.0e6f : 0.0f, power_max = -1.0e6f, power_min = 1.0e6f;
        for (uint32_t rx = 0; rx < N_RX_virt; ++rx) {
            float2 sum = make_float2(0.f, 0.f);
            for (uint32_t tx = 0; tx < N_TX_virt; ++tx) {
                const float2 w = W[wm * N_TX_virt + tx];
                const uint32_t hrx = rec ? tx : rx, hts = rec ? rx : tx;
                float2 part = make_float2(0.f, 0.f);
                for (uint32_t c = 0; c < 4; ++c) part = cadd(part, cmul(H[(hrx * A.N_TS + hts) * 4 + c], w));
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
        if (wm == lane) score = power_inner;
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
    if (score_out) *score_out = score;
    return bidx;
}

__global__ void __launch_bounds__(64) rx_mimo_kernel(rx_mimo_args A) {
    __shared__ float2 H[8 * 8 * 4];
    const uint32_t pkt = rx_slot_of(A.sel, blockIdx.x), row = rx_row_of(A.sel, blockIdx.x), lane = threadIdx.x;
    mimo_stage(A, pkt, H, lane, 64);
    __syncthreads();
    const uint32_t idx = A.N_TS == 1 ? 0u : mimo_pick(A, H, false, 0, lane);
    const uint32_t idr = A.N_RX == 1 ? 0u : mimo_pick(A, H, true, 0, lane);
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
// (RX_SYNCED_PARAM_MODE_3_7_METRIC: metric; ..._USE_ALL_W_MATRICES_OR_ONLY_NON_ZERO, rx_synced_param.hpp:286:
// the search start A0), every candidate's score, and the rank / precoder report for spatial
// multiplexing the reference leaves unset (mimo_report.hpp:51-58). One workgroup of 256 threads per packet on
// the same stage: wave 0 scores the transmit-side codebook, wave 1 the reciprocal one (mimo_pick, one
// candidate per lane: ncb <= 64); then one thread per (rank slot, codebook entry, wideband cell) computes the
// cell's MMSE rate, the entries' rates are their cells' sums in fixed order and one thread picks. Every word of the row is written once, by one thread, with plain stores.
constexpr uint32_t MIMO_D_THREADS = 256;
constexpr uint32_t MIMO_D_MAX_ENTRIES = 64;  // codebook entries over the three rank slots: at most 28 + 22 + 5

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
    mimo_stage(A, pkt, H, tid, MIMO_D_THREADS);
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
        if (n_virt != 1) idx = mimo_pick(A, H, rec, D.metric, lane, &score);
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
    uint32_t RI = 0u, PMI = MIMO_UINT_NONE;
    float rate_RI = 0.f;
    for (uint32_t s = 0; s < 3; ++s) {
        const uint32_t base = s == 0 ? 0u : s == 1 ? e1 : e2;
        uint32_t pm = MIMO_UINT_NONE;
        float rt = __builtin_nanf("");
        for (uint32_t cb = 0; cb < D.sm_ncb[s]; ++cb) {
            const float r = entry_rate[base + cb];
            if (pm == MIMO_UINT_NONE || r > rt) {
                rt = r;
                pm = cb;
            }
        }
        out->pmi[s] = pm;
        out->rate[s] = rt;
        if (pm != MIMO_UINT_NONE && (RI == 0u || rt > rate_RI)) {
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
