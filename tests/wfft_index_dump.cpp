// Host program of tests/test_wfft_slots_host.py: prints what csrc/kernels/wfft_index.hpp computes, the header
// the kernels address their LDS with.
//   wfft_index_dump slots                     -> "pattern lane n element closed_form_slot" per access
//   wfft_index_dump blocks STF_CP CP n_sym    -> "m_star l m0 qb0 qb1" and per block "q first_slot"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "wfft_index.hpp"

using namespace dnrp::dev;

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "slots")) {
        printf("xb %u pad %u\n", WFFT_XB, RX_MIX_PAD);
        for (uint32_t lane = 0; lane < 64; ++lane) {
            for (uint32_t k = 0; k < 16; ++k)
                printf("w1 %u %u %u %u\n", lane, k, wfft_w1_base(lane) + wfft_w1_off(k), wfft_pad(wfft_w1_base(lane)) + wfft_off(wfft_w1_off(k)));
            for (uint32_t r = 0; r < 16; ++r)
                printf("r2 %u %u %u %u\n", lane, r, wfft_r2_base(lane) + wfft_r2_off(r), wfft_pad(wfft_r2_base(lane)) + wfft_off(wfft_r2_off(r)));
            for (uint32_t k = 0; k < 16; ++k)
                printf("w2 %u %u %u %u\n", lane, k, wfft_w2_base(lane) + wfft_w2_off(k), wfft_pad(wfft_w2_base(lane)) + wfft_off(wfft_w2_off(k)));
            for (uint32_t b = 0; b < 4; ++b)
                for (uint32_t r = 0; r < 4; ++r)
                    printf("r3 %u %u %u %u\n", lane, 4 * b + r, wfft_r3_base(lane) + wfft_r3_off(b, r), wfft_pad(wfft_r3_base(lane)) + wfft_off(wfft_r3_off(b, r)));
        }
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "blocks")) {
        const uint32_t stf_cp = atoi(argv[2]), cp = atoi(argv[3]), n_sym = atoi(argv[4]);
        const int LR = 9;
        printf("rounds %d\n", rx_block_rounds(LR));
        for (uint32_t m_star = 0; m_star < static_cast<uint32_t>(LR); ++m_star)
            for (uint32_t l = 1; l <= n_sym; ++l) {
                const rx_blocks_t b = rx_blocks(stf_cp, cp, m_star, l, LR);
                printf("sym %u %u %d %d %d\n", m_star, l, b.m0, b.qb0, b.qb1);
                for (int q = b.qb0; q < b.qb1; ++q) printf("blk %d %d\n", q, rx_mix_slot(static_cast<int>(m_star), LR, q, 0, b.m0));
            }
        return 0;
    }
    return 2;
}
