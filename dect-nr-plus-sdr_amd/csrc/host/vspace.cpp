// C-ABI of the virtual space (include/dnrp.h dnrp_vspace_mix), the GPU counterpart of
// vspace_t::wchannel_execute (lib/src/simulation/vspace.cpp:449-513) and the simulated radio's ADC
// (lib/src/radio/hw_simulator.cpp:686-733): argument checks, one link realisation per distinct link
// index (channel.cpp's draws), the tile plan, and the launch of kernels/vspace.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "channel_internal.hpp"

using namespace dnrp;
using namespace dnrp::host;

namespace dnrp::host {

// Tile plan of a span [t_begin, t_begin + n_samples) cut into tiles of `tile` samples: per tile, in CSR
// form and in em order, the emissions on the air in it -- [t_start, t_start + length + max_delay), the
// delay line's tail included -- and the own emissions whose detached interval [t_start, t_start +
// length) meets it. A pure function of its arguments. Returns false if an index list would not fit
// 32-bit offsets.
bool vspace_tile_plan(const dnrp_vspace_emission* em, uint32_t n_em, uint32_t max_delay, int64_t t_begin,
                      uint64_t n_samples, uint32_t tile, vspace_plan& p) {
    const uint64_t n_tiles = (n_samples + tile - 1) / tile;
    p.em_off.assign(n_tiles + 1, 0);
    p.own_off.assign(n_tiles + 1, 0);
    p.em_idx.clear();
    p.own_idx.clear();
    // tiles [first, last] that global times [a, a + len) meet, false: none
    auto tiles_of = [&](int64_t a, uint64_t len, uint64_t& first, uint64_t& last) {
        if (len == 0 || n_samples == 0) return false;
        // span-relative [lo, hi): times are >= 0, so the differences fit uint64_t
        if (a >= t_begin && static_cast<uint64_t>(a - t_begin) >= n_samples) return false;
        const uint64_t lo = a > t_begin ? static_cast<uint64_t>(a - t_begin) : 0;
        uint64_t hi;  // exclusive
        if (a >= t_begin) {
            hi = std::min<uint64_t>(n_samples, static_cast<uint64_t>(a - t_begin) + len);
        } else {
            const uint64_t before = static_cast<uint64_t>(t_begin - a);
            if (len <= before) return false;
            hi = std::min<uint64_t>(n_samples, len - before);
        }
        first = lo / tile;
        last = (hi - 1) / tile;
        return true;
    };
    uint64_t total[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {  // count, then fill: emission order within every tile
        std::vector<uint32_t> at_em, at_own;
        if (pass == 1) {
            if (total[0] > 0x7FFFFFFFull || total[1] > 0x7FFFFFFFull) return false;
            for (uint64_t k = 0; k < n_tiles; ++k) {
                p.em_off[k + 1] += p.em_off[k];
                p.own_off[k + 1] += p.own_off[k];
            }
            p.em_idx.resize(total[0]);
            p.own_idx.resize(total[1]);
            at_em.assign(p.em_off.begin(), p.em_off.end() - 1);
            at_own.assign(p.own_off.begin(), p.own_off.end() - 1);
        }
        for (uint32_t e = 0; e < n_em; ++e) {
            uint64_t f, l;
            if (tiles_of(em[e].t_start, uint64_t(em[e].length) + max_delay, f, l)) {
                for (uint64_t k = f; k <= l; ++k) {
                    if (pass == 0) ++p.em_off[k + 1];
                    else p.em_idx[at_em[k]++] = e;
                }
                if (pass == 0) total[0] += l - f + 1;
            }
            if (em[e].own && tiles_of(em[e].t_start, em[e].length, f, l)) {
                for (uint64_t k = f; k <= l; ++k) {
                    if (pass == 0) ++p.own_off[k + 1];
                    else p.own_idx[at_own[k]++] = e;
                }
                if (pass == 0) total[1] += l - f + 1;
            }
        }
    }
    return true;
}

}  // namespace dnrp::host

extern "C" {

int dnrp_vspace_mix(dnrp_ctx* ctx, const dnrp_channel_cfg* ch, const dnrp_adc_cfg* adc, uint32_t n_em,
                    const dnrp_vspace_emission* em, uint32_t N_TX, const float* tx, uint32_t n_rows, uint32_t S_tx,
                    uint32_t N_RX, float* ring, uint64_t ring_len, uint64_t ant_stride, int64_t t_begin, uint64_t n_samples,
                    void* stream) {
    if (!ctx || !channel_cfg_ok(ch) || !ring || (n_em > 0 && (!em || !tx))) return DNRP_EINVAL;
    if (N_TX == 0 || N_RX == 0 || N_TX > 8 || N_RX > 8) return DNRP_EINVAL;
    if (ring_len == 0 || ant_stride < ring_len || n_samples > ring_len || t_begin < 0) return DNRP_EINVAL;
    if (static_cast<uint64_t>(std::numeric_limits<int64_t>::max() - t_begin) < n_samples) return DNRP_EINVAL;
    if (adc && (!(adc->clip_limit >= 0.0f) || !std::isfinite(adc->clip_limit) || adc->n_bits > 24)) return DNRP_EINVAL;
    for (uint32_t e = 0; e < n_em; ++e) {
        const auto& m = em[e];
        if (m.t_start < 0 || m.length == 0 || m.length > S_tx || m.tx_row >= n_rows || !(m.gain >= 0.0f) ||
            !std::isfinite(m.gain) || m.reserved != 0)
            return DNRP_EINVAL;
    }
    if (n_samples == 0) return DNRP_OK;
    const uint64_t n_tiles = (n_samples + dev::VS_TILE - 1) / dev::VS_TILE;
    if (n_tiles > 0x7FFFFFFFull) return DNRP_ENOMEM;
    (void)hipSetDevice(ctx->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);

    std::vector<dev::channel_tap> pdp;
    if (ch->kind == DNRP_CH_DOUBLY) set_pdp(*ch, pdp);
    uint32_t max_delay = 0;
    for (const auto& t : pdp) max_delay = std::max(max_delay, static_cast<uint32_t>(t.delay));
    // one realisation per distinct link index (the edge of vspace.cpp:463-468), slots in order of first use
    std::vector<uint32_t> links, slot_of(n_em);
    for (uint32_t e = 0; e < n_em; ++e) {
        const auto it = std::find(links.begin(), links.end(), em[e].link);
        slot_of[e] = static_cast<uint32_t>(it - links.begin());
        if (it == links.end()) links.push_back(em[e].link);
    }
    vspace_plan plan;
    if (!vspace_tile_plan(em, n_em, max_delay, t_begin, n_samples, dev::VS_TILE, plan)) return DNRP_ENOMEM;

    const uint32_t nl = N_RX * N_TX, nt = static_cast<uint32_t>(pdp.size());
    const size_t n_slots = links.size();
    const size_t b_em = sizeof(dev::vspace_em) * n_em, b_sins = sizeof(dev::channel_sin) * nl * nt * CH_N_SIN * n_slots,
                 b_coef = sizeof(float2) * nl * n_slots, b_taps = sizeof(dev::channel_tap) * nl * nt * n_slots,
                 b_off = sizeof(uint32_t) * (n_tiles + 1), b_ei = sizeof(uint32_t) * plan.em_idx.size(),
                 b_oi = sizeof(uint32_t) * plan.own_idx.size();
    const size_t o_sins = b_em, o_coef = o_sins + b_sins, o_taps = o_coef + b_coef, o_eoff = o_taps + b_taps,
                 o_eidx = o_eoff + b_off, o_ooff = o_eidx + b_ei, o_oidx = o_ooff + b_off, bytes = o_oidx + b_oi;
    auto* h = static_cast<char*>(ctx->st_vs.get(bytes));
    if (!h || !ctx->vs_tab.ensure(bytes)) return DNRP_ENOMEM;
    auto* hem = reinterpret_cast<dev::vspace_em*>(h);
    for (uint32_t e = 0; e < n_em; ++e)
        hem[e] = {em[e].t_start, em[e].tx_row, em[e].length, slot_of[e], em[e].own ? 1u : 0u, em[e].gain * ch->large_scale, 0u};
    for (size_t s = 0; s < n_slots; ++s)
        realise(*ch, links[s], N_TX, N_RX, pdp, reinterpret_cast<float2*>(h + o_coef) + s * nl,
                reinterpret_cast<dev::channel_tap*>(h + o_taps) + s * nl * nt,
                reinterpret_cast<dev::channel_sin*>(h + o_sins) + s * nl * nt * CH_N_SIN);
    std::memcpy(h + o_eoff, plan.em_off.data(), b_off);
    if (b_ei) std::memcpy(h + o_eidx, plan.em_idx.data(), b_ei);
    std::memcpy(h + o_ooff, plan.own_off.data(), b_off);
    if (b_oi) std::memcpy(h + o_oidx, plan.own_idx.data(), b_oi);
    HIPCHK(ctx->vs_tab.wait_idle(st));
    HIPCHK(hipMemcpyAsync(ctx->vs_tab.p, h, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->st_vs.ev, st));

    char* d = static_cast<char*>(ctx->vs_tab.p);
    dev::vspace_args a{};
    a.kind = ch->kind;
    a.N_TX = N_TX;
    a.N_RX = N_RX;
    a.S_tx = S_tx;
    a.n_taps = nt;
    a.n_sin = CH_N_SIN;
    a.tx = reinterpret_cast<const float2*>(tx);
    a.ring = reinterpret_cast<float2*>(ring);
    a.ring_len = ring_len;
    a.ant_stride = ant_stride;
    a.t_begin = t_begin;
    a.n_samples = n_samples;
    a.em = reinterpret_cast<const dev::vspace_em*>(d);
    a.em_off = reinterpret_cast<const uint32_t*>(d + o_eoff);
    a.em_idx = reinterpret_cast<const uint32_t*>(d + o_eidx);
    a.own_off = reinterpret_cast<const uint32_t*>(d + o_ooff);
    a.own_idx = reinterpret_cast<const uint32_t*>(d + o_oidx);
    a.coef = reinterpret_cast<const float2*>(d + o_coef);
    a.taps = reinterpret_cast<const dev::channel_tap*>(d + o_taps);
    a.sins = reinterpret_cast<const dev::channel_sin*>(d + o_sins);
    a.sigma = noise_sigma(*ch);
    a.seed = noise_seed(*ch);
    if (adc && adc->clip_limit > 0.0f) {
        a.clip = adc->clip_limit;
        // bit width in float, as hw_simulator.cpp:725
        if (adc->n_bits > 0) a.step = 2.0f * adc->clip_limit / std::pow(2.0f, static_cast<float>(adc->n_bits));
    }
    ctx->tic("vspace_mix", st);
    const hipError_t le = dev::launch_vspace(a, static_cast<uint32_t>(n_tiles), st);
    ctx->toc("vspace_mix", st);
    if (le != hipSuccess) return DNRP_EDEVICE;
    return ctx->vs_tab.mark_busy(st) == hipSuccess ? DNRP_OK : DNRP_EDEVICE;
}

}  // extern "C"
