// ORACLE PINNING HARNESS — TEST INFRASTRUCTURE ONLY.
// Our own driver that links the reference's unmodified cell-map sources (drs.cpp, pcc.cpp, pdc.cpp,
// beamforming_and_antenna_port_mapping.cpp; compiled by oracle/Makefile from the reference tree with
// oracle/ref_standin/ as the only non-reference header, output only into oracle/_ref/) and prints
// what they produce as JSON: the DRS / PCC / PDC cells per OFDM symbol as tx_t walks them
// (tx.cpp:250-262, 944-1005), the packet counts of pdc.cpp / transmission_packet_structure.cpp and
// the beamforming matrices of W_t. tests/golden/make_cells_fixture.py condenses the output into
// tests/golden/ref_cells.json; product and oracle are checked against it in tests/test_cell_pins.py
// and the kernels in tests/test_gpu_cell_grid.py. Never shipped, never on the GPU box.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dectnrp/sections_part3/beamforming_and_antenna_port_mapping.hpp"
#include "dectnrp/sections_part3/drs.hpp"
#include "dectnrp/sections_part3/numerologies.hpp"
#include "dectnrp/sections_part3/pcc.hpp"
#include "dectnrp/sections_part3/pdc.hpp"
#include "dectnrp/sections_part3/transmission_packet_structure.hpp"

using namespace dectnrp;

static constexpr uint32_t L_MAX = 41;  // covers l_limit (6 / 11) and three 10-symbol repetitions

static void print_u32(const std::vector<uint32_t>& v) {
    std::printf("[");
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%u", i ? "," : "", v[i]);
    std::printf("]");
}

static void print_cells() {
    sp3::drs_t drs(16, 8);
    sp3::pcc_t pcc(16, 8);
    sp3::pdc_t pdc(16, 8);
    std::printf("\"L_MAX\": %u,\n\"cells\": [", L_MAX);
    bool first = true;
    for (uint32_t b : {1u, 2u, 4u, 8u, 12u, 16u})
        for (uint32_t N_TS : {1u, 2u, 4u, 8u}) {
            drs.set_configuration(b, N_TS);
            pcc.set_configuration(b, N_TS);
            pdc.set_configuration(b, N_TS);
            std::printf("%s\n{\"b\":%u,\"N_TS\":%u,\"pcc_symbol_idx_max\":%u,", first ? "" : ",", b, N_TS,
                        pcc.get_pcc_symbol_idx_max());
            first = false;
            // one walk over the symbols in tx_t's order: PCC, DRS, PDC (tx.cpp:250-262)
            std::vector<std::vector<uint32_t>> pcc_lk, pdc_k(L_MAX + 1);
            struct drs_row {
                uint32_t l, ts_first, ts_last;
                std::vector<std::vector<uint32_t>> k;
                std::vector<std::vector<cf_t>> y;
            };
            std::vector<drs_row> rows;
            for (uint32_t l = 1; l <= L_MAX; ++l) {
                if (pcc.is_symbol_index(l))
                    for (uint32_t k : pcc.get_k_i_one_symbol()) pcc_lk.push_back({l, k});
                if (drs.is_symbol_index(l)) {
                    // tx_t::run_drs (tx.cpp:977-1002): stream t takes rows t % 4 of k_i and y_DRS_i
                    const auto& k_i = drs.get_k_i();
                    const auto& y = drs.get_y_DRS_i();
                    drs_row r{l, drs.get_ts_idx_first(), 0, {}, {}};
                    r.ts_last = drs.get_ts_idx_last_and_advance();
                    for (uint32_t t = r.ts_first; t <= r.ts_last; ++t) {
                        r.k.push_back(k_i.at(t % 4));
                        r.y.push_back(y.at(t % 4));
                    }
                    rows.push_back(r);
                }
                if (pdc.is_symbol_index(l)) pdc_k[l] = pdc.get_k_i_one_symbol();
            }
            std::printf("\"pcc\":[");
            for (size_t i = 0; i < pcc_lk.size(); ++i)
                std::printf("%s[%u,%u]", i ? "," : "", pcc_lk[i][0], pcc_lk[i][1]);
            std::printf("],\"drs\":[");
            for (size_t i = 0; i < rows.size(); ++i) {
                const auto& r = rows[i];
                std::printf("%s{\"l\":%u,\"ts_first\":%u,\"ts_last\":%u,\"k\":[", i ? "," : "", r.l, r.ts_first,
                            r.ts_last);
                for (size_t t = 0; t < r.k.size(); ++t) {
                    std::printf("%s", t ? "," : "");
                    print_u32(r.k[t]);
                }
                std::printf("],\"y\":[");
                for (size_t t = 0; t < r.y.size(); ++t) {  // values are +-1 + 0j: one character each
                    std::printf("%s\"", t ? "," : "");
                    for (const cf_t v : r.y[t]) {
                        const float re = __real__ v, im = __imag__ v;
                        std::printf("%c", im != 0.0f ? '?' : re == 1.0f ? '+' : re == -1.0f ? '-' : '?');
                    }
                    std::printf("\"");
                }
                std::printf("]}");
            }
            std::printf("],\"pdc\":[");
            for (uint32_t l = 1; l <= L_MAX; ++l) {
                std::printf("%s", l > 1 ? "," : "");
                print_u32(pdc_k[l]);
            }
            std::printf("]}");
        }
    std::printf("],\n");
}

static void print_counts() {
    namespace tps = sp3::transmission_packet_structure;
    // one row per (u, b, PacketLengthType, PacketLength, N_eff_TX): N_PACKET_symb, N_DF_symb,
    // DRS symbols per TS, N_DRS_subc, N_PDC_subc, N_samples_DF. The three DRS-dependent values are -1
    // where pdc_t::get_nof_OFDM_symbols_carrying_DRS_per_TS asserts (pdc.cpp:170-176): the harness
    // is built with ENABLE_ASSERT and must not call it there
    std::printf("\"counts\": [");
    bool first = true;
    for (uint32_t u : {1u, 2u, 4u, 8u})
        for (uint32_t b : {1u, 2u, 4u, 8u, 12u, 16u})
            for (uint32_t plt : {0u, 1u})
                for (uint32_t pl : {1u, 2u, 3u, 4u, 8u, 16u})
                    for (uint32_t n_eff : {1u, 2u, 4u, 8u}) {
                        const auto q = sp3::get_numerologies(u, b);
                        const uint32_t N_P = tps::get_N_PACKET_symb(plt, pl, q);
                        const bool asserts = (n_eff == 4 && N_P < 15) ||
                                             (u == 8 && n_eff == 8 && (N_P < 20 || N_P % 10 != 0));
                        std::printf("%s[%u,%u,%u,%u,%u,%u,%u,", first ? "" : ",", u, b, plt, pl, n_eff, N_P,
                                    sp3::pdc_t::get_N_DF_symb(u, N_P));
                        if (asserts)
                            std::printf("-1,-1,-1,");
                        else
                            std::printf("%u,%u,%u,",
                                        sp3::pdc_t::get_nof_OFDM_symbols_carrying_DRS_per_TS(u, N_P, n_eff),
                                        sp3::pdc_t::get_N_DRS_subc(u, N_P, n_eff, q.N_b_OCC),
                                        sp3::pdc_t::get_N_PDC_subc(N_P, u, n_eff, q.N_b_OCC));
                        std::printf("%u]", tps::get_N_samples_DF(u, b, N_P));
                        first = false;
                    }
    std::printf("],\n");
}

static void print_W() {
    const sp3::W_t W;
    const uint32_t pairs[7][2] = {{1, 1}, {1, 2}, {1, 4}, {2, 2}, {2, 4}, {4, 4}, {8, 8}};  // (N_TS, N_TX)
    std::printf("\"W\": [");
    bool first = true;
    for (const auto& p : pairs) {
        const auto& mats = W.get_W(p[0], p[1]);
        for (uint32_t cb = 0; cb < mats.size(); ++cb) {
            std::printf("%s\n{\"N_TS\":%u,\"N_TX\":%u,\"codebook\":%u,\"index_max\":%u,\"W\":[", first ? "" : ",", p[0],
                        p[1], cb, sp3::W_t::get_codebook_index_max(p[0], p[1]));
            first = false;
            const auto& w = W.get_W(p[0], p[1], cb);
            for (size_t i = 0; i < w.size(); ++i)
                std::printf("%s%.9g,%.9g", i ? "," : "", static_cast<double>(__real__ w[i]),
                            static_cast<double>(__imag__ w[i]));
            std::printf("],\"scaling\":%.9g,\"scaling_optimal_DAC\":%.9g}",
                        static_cast<double>(W.get_scaling_factor(p[0], p[1], cb)),
                        static_cast<double>(W.get_scaling_factor_optimal_DAC(p[0], p[1], cb)));
        }
    }
    std::printf("]\n");
}

int main() {
    std::printf("{\n");
    print_cells();
    print_counts();
    print_W();
    std::printf("}\n");
    return 0;
}
