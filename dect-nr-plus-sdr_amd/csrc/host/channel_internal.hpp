// Link realisations and noise level of the simulated channel (channel.cpp), shared with the virtual
// space (vspace.cpp). Not part of the public interface.
#pragma once

#include <cstdint>
#include <vector>

#include "ctx_internal.hpp"

namespace dnrp::host {

constexpr uint32_t CH_N_SIN = 40;  // WIRELESS_CHANNEL_DOUBLY_NOF_SINUSOIDS

// a configuration dnrp_channel_batch accepts
bool channel_cfg_ok(const dnrp_channel_cfg* c);
// link_t::set_pdp (link.cpp:66-120): the taps of the configured power delay profile
void set_pdp(const dnrp_channel_cfg& c, std::vector<dev::channel_tap>& taps);
// realisation of index w (a window of dnrp_channel_batch, a link of dnrp_vspace_mix): flat coefficients
// [N_RX][N_TX] or per link the taps [pdp.size()] and CH_N_SIN sinusoids per tap
void realise(const dnrp_channel_cfg& c, uint32_t w, uint32_t N_TX, uint32_t N_RX, const std::vector<dev::channel_tap>& pdp,
             float2* coef, dev::channel_tap* taps, dev::channel_sin* sins);
// standard deviation per noise component (noise.cpp:30-42), 0: noiseless
float noise_sigma(const dnrp_channel_cfg& c);
uint64_t mix64(uint64_t z);  // splitmix64 finaliser
// seed of the device noise generator: independent of the link draws
inline uint64_t noise_seed(const dnrp_channel_cfg& c) { return mix64(c.seed ^ 0x6E6F697365ull); }


// vspace.cpp: which emissions each tile of a span has to walk (CSR rows per tile, emission order kept)
struct vspace_plan {
    std::vector<uint32_t> em_off, em_idx;    // on the air in the tile, the delay line's tail included
    std::vector<uint32_t> own_off, own_idx;  // own emissions whose [t_start, t_start + length) meets the tile
};
bool vspace_tile_plan(const dnrp_vspace_emission* em, uint32_t n_em, uint32_t max_delay, int64_t t_begin,
                      uint64_t n_samples, uint32_t tile, vspace_plan& p);

}  // namespace dnrp::host
