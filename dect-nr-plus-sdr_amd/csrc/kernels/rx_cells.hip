// RX back end of the synchronised receiver: equalisation and soft demapping (the DRS chain is in rx_drs.hip).
//
//  rx_cells_kernel  one WG per (packet, epoch): an epoch is a run of cell work over which the
//                   interlaced pilot buffer (channel_antenna.hpp:38-63) does not change. The WG
//                   rebuilds that buffer in LDS from the zero-forced DRS cells of Y, then every
//                   thread takes whole work units (a cell for MRC, an SFBC pair for transmit
//                   diversity): Wiener interpolation of the channel at the unit's subcarriers
//                   (rx_synced.cpp:932-946), MRC (1204-1306) or SFBC combining (1335-1392),
//                   srsRAN-style int16 soft demapping and descrambling (pcc_enc.cpp:297,
//                   pdc_enc.cpp:339-344).
// Y layout: [packet][N_RX][n_sym_total][Nf_pad] float2 (rx_fft_kernel).
#include "device_common.hpp"
#include "experiments.hpp"
#include "kernels.hpp"
#include "rx_eq.hpp"

namespace dnrp::dev {

constexpr uint32_t CELL_THREADS = 512;

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

// the instantiated (N_RX, N_eff_TX) pairs: MRC / SFBC, and spatial multiplexing (N_RX >= N_SS >= 2)
using cells_pairs = rx_pairs<rx_pair<1, 1>, rx_pair<2, 1>, rx_pair<4, 1>, rx_pair<8, 1>, rx_pair<2, 2>, rx_pair<4, 2>,
                             rx_pair<8, 2>, rx_pair<4, 4>, rx_pair<8, 4>>;
using cells_sm_pairs = rx_pairs<rx_pair<2, 2>, rx_pair<4, 2>, rx_pair<8, 2>, rx_pair<4, 4>, rx_pair<8, 4>>;

bool rx_cells_supported(uint32_t N_RX, uint32_t NT, bool sm) {
    return sm ? rx_pair_in(cells_sm_pairs{}, N_RX, NT) : rx_pair_in(cells_pairs{}, N_RX, NT);
}

hipError_t launch_rx_cells(const rx_cells_args& a, uint32_t n, hipStream_t st) {
    const size_t lds = cell_lds_bytes(a.N_RX, a.NT, a.n_drs, a.wcap[0], a.wcap[1]);
    if (lds > LDS_BYTES || a.n_pkt != n || !y_rows_fit(a)) return hipErrorInvalidValue;
    const dim3 g((n + 7) / 8 * 8 * a.n_epochs), b(CELL_THREADS);
    // 256-QAM (N_bps = 8, the bench's C3 / C4) with the demapper width compiled in
    const bool hit = rx_pair_dispatch(cells_pairs{}, a.N_RX, a.NT, [&](auto r, auto t) {
        constexpr int R = decltype(r)::value, T = decltype(t)::value;
        if (a.N_bps == 8)
            hipLaunchKernelGGL((rx_cells_kernel<R, T, false, 8>), g, b, lds, st, a);
        else
            hipLaunchKernelGGL((rx_cells_kernel<R, T>), g, b, lds, st, a);
    });
    return hit ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_rx_cells_sm(const rx_cells_args& a, uint32_t n, hipStream_t st) {
    size_t lds = cell_lds_bytes(a.N_RX, a.NT, a.n_drs, a.wcap[0], a.wcap[1]);
    if (experiment(XS_MMSE_MFMA) && a.NT == 4) lds = (lds + 15) / 16 * 16 + CELL_THREADS / 64 * a.N_RX * 4 * 24 * sizeof(float2);
    if (lds > LDS_BYTES || a.n_pkt != n) return hipErrorInvalidValue;
    const dim3 g((n + 7) / 8 * 8 * a.n_epochs), b(CELL_THREADS);
    // the demapper width compiled in for 64- and 256-QAM
    const bool hit = rx_pair_dispatch(cells_sm_pairs{}, a.N_RX, a.NT, [&](auto r, auto t) {
        constexpr int R = decltype(r)::value, T = decltype(t)::value;
        if (a.N_bps == 6)
            hipLaunchKernelGGL((rx_cells_kernel<R, T, true, 6>), g, b, lds, st, a);
        else if (a.N_bps == 8)
            hipLaunchKernelGGL((rx_cells_kernel<R, T, true, 8>), g, b, lds, st, a);
        else
            hipLaunchKernelGGL((rx_cells_kernel<R, T, true>), g, b, lds, st, a);
    });
    return hit ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace dnrp::dev
