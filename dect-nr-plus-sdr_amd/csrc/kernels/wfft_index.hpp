// Index arithmetic of the one-wavefront FFT's LDS exchanges (device_common.hpp) and of the RX front end's
// polyphase blocks (rx_front.hpp), free of device types so that a host program can include it:
// tests/test_wfft_slots_host.py compiles one and walks every lane, offset, symbol and block.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DNRP_HD __host__ __device__
#else
#define DNRP_HD
#endif

namespace dnrp::dev {

constexpr uint32_t WFFT_XB = 1024 + 64;  // float2 slots of the exchange buffer

// exchange slot of element i: padded i + i / 16 (conflict-free b64 writes of pass 1 and 2, 2-way
// ds_read_b64 conflicts in passes 2 and 3 -- slots 0 and 32 of a half-wave share a bank)
DNRP_HD constexpr uint32_t wfft_pad(uint32_t i) { return i + (i >> 4); }

// Slot of element i0 + c relative to the slot of i0, where c adds into i0 without a carry out of the low
// four bits (c a multiple of 16, or i0 one and c < 16): wfft_pad(i0 + c) = wfft_pad(i0) + wfft_off(c). An
// exchange then costs one padded lane base and immediate offsets; from wfft_pad(i0 + c) itself the
// compiler cannot prove the no-carry property and pays a shift and two adds per element.
DNRP_HD constexpr uint32_t wfft_off(uint32_t c) { return c + (c >> 4); }

// The four access patterns of the transform as (lane base i0, offset c):
// pass-1 writes y[16 lane + k], pass-2 reads y[lane + 64 r], pass-2 writes z[(lane / 16) 256 + lane % 16 + 16 k],
// pass-3 reads z[lane + 64 b + 256 r] (butterfly b of the lane, input r)
DNRP_HD constexpr uint32_t wfft_w1_base(uint32_t lane) { return 16 * lane; }
DNRP_HD constexpr uint32_t wfft_w1_off(uint32_t k) { return k; }
DNRP_HD constexpr uint32_t wfft_r2_base(uint32_t lane) { return lane; }
DNRP_HD constexpr uint32_t wfft_r2_off(uint32_t r) { return 64 * r; }
DNRP_HD constexpr uint32_t wfft_w2_base(uint32_t lane) { return (lane >> 4) * 256 + (lane & 15u); }
DNRP_HD constexpr uint32_t wfft_w2_off(uint32_t k) { return 16 * k; }
DNRP_HD constexpr uint32_t wfft_r3_base(uint32_t lane) { return lane; }
DNRP_HD constexpr uint32_t wfft_r3_off(uint32_t b, uint32_t r) { return 64 * b + 256 * r; }

// Polyphase blocks of data symbol l (1-based) of the L/M = LR/MR front end: the symbol's first DECT-rate
// output m0 and the blocks q in [qb0, qb1) that cover m0 .. m0 + 1023, block q holding the outputs
// m_star + LR q + k, k < LR (m0 >= m_star)
struct rx_blocks_t {
    int m0, qb0, qb1;
};
DNRP_HD constexpr rx_blocks_t rx_blocks(uint32_t STF_CP, uint32_t CP, uint32_t m_star, uint32_t l, int LR) {
    const int m0 = static_cast<int>(STF_CP + 1024 + (l - 1) * (CP + 1024) + CP);
    return {m0, (m0 - static_cast<int>(m_star)) / LR, (m0 + 1024 - static_cast<int>(m_star) + LR - 1) / LR};
}
// block rounds per lane (64 blocks per round); a symbol has at most (1024 + 2 LR - 2) / LR + 1 blocks
DNRP_HD constexpr int rx_block_rounds(int LR) { return (1024 + 2 * LR) / LR / 64 + 1; }

// rx_resample_ct stores output j of the symbol (j = m - m0) at slot RX_MIX_PAD + j of the wave's region: the
// first block of a symbol holds up to LR - 1 outputs before m0 and the last one up to LR - 1 past
// m0 + 1023, no other block holds any; they land in the pad slots on either side, which nothing reads, so
// no store of the mixer needs a range test.
constexpr uint32_t RX_MIX_PAD = 8;
DNRP_HD constexpr int rx_mix_slot(int m_star, int LR, int q, int k, int m0) {
    return m_star + LR * q + k - m0 + static_cast<int>(RX_MIX_PAD);
}

}  // namespace dnrp::dev
