// C-ABI implementation (include/dnrp.h): context, network-ID scrambling sequences, packet sizes,
// the timing API, and the small table helpers the per-configuration tables share (tables.cpp; the
// batched TX / RX phase launches are in tx.cpp and rx.cpp).
#include "ctx_internal.hpp"

using namespace dnrp;
using namespace dnrp::host;

namespace dnrp::host {

dev::fft_plan make_plan(uint32_t N) {
    dev::fft_plan p{};
    p.N = N;
    uint32_t r = N;
    while (r % 4 == 0 && r > 1) {
        p.radix[p.nr++] = 4;
        r /= 4;
    }
    while (r % 2 == 0) {
        p.radix[p.nr++] = 2;
        r /= 2;
    }
    while (r % 3 == 0) {
        p.radix[p.nr++] = 3;
        r /= 3;
    }
    return p;  // r must be 1 (sizes 64..16384 of tx_rx.hpp:67-69)
}

std::vector<float2> twiddles(uint32_t N) {
    std::vector<float2> t(N);
    for (uint32_t j = 0; j < N; ++j) {
        const double a = -2.0 * M_PI * static_cast<double>(j) / static_cast<double>(N);
        t[j] = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
    }
    return t;
}

std::vector<float2> constellation(uint32_t N_bps) {  // 3GPP TS 36.211 §7.1, index bits MSB first
    const uint32_t n = 1u << N_bps;
    std::vector<float2> t(n);
    auto bit = [&](uint32_t i, uint32_t k) { return static_cast<int>((i >> (N_bps - 1 - k)) & 1u); };
    for (uint32_t i = 0; i < n; ++i) {
        double re = 0, im = 0, nrm = 1;
        switch (N_bps) {
            case 1:
                re = im = 1 - 2 * bit(i, 0);
                nrm = std::sqrt(2.0);
                break;
            case 2:
                re = 1 - 2 * bit(i, 0);
                im = 1 - 2 * bit(i, 1);
                nrm = std::sqrt(2.0);
                break;
            case 4:
                re = (1 - 2 * bit(i, 0)) * (2 - (1 - 2 * bit(i, 2)));
                im = (1 - 2 * bit(i, 1)) * (2 - (1 - 2 * bit(i, 3)));
                nrm = std::sqrt(10.0);
                break;
            case 6:
                re = (1 - 2 * bit(i, 0)) * (4 - (1 - 2 * bit(i, 2)) * (2 - (1 - 2 * bit(i, 4))));
                im = (1 - 2 * bit(i, 1)) * (4 - (1 - 2 * bit(i, 3)) * (2 - (1 - 2 * bit(i, 5))));
                nrm = std::sqrt(42.0);
                break;
            default:
                re = (1 - 2 * bit(i, 0)) * (8 - (1 - 2 * bit(i, 2)) * (4 - (1 - 2 * bit(i, 4)) * (2 - (1 - 2 * bit(i, 6)))));
                im = (1 - 2 * bit(i, 1)) * (8 - (1 - 2 * bit(i, 3)) * (4 - (1 - 2 * bit(i, 5)) * (2 - (1 - 2 * bit(i, 7)))));
                nrm = std::sqrt(170.0);
                break;
        }
        t[i] = make_float2(static_cast<float>(re / nrm), static_cast<float>(im / nrm));
    }
    return t;
}

// input-major block taps for the register-blocked resampler (polyphase.hpp): rows i = 0..W-1 of
// LP = 4*ceil(L/4) floats, g[i][k] = h[ph_k + (hl + o_k - i) * L] inside output k's FIR span
std::vector<float> taps_polyphase(const geo::resampler_t& rs, uint32_t* count) {
    const uint32_t L = rs.L, M = rs.M, hl = rs.hl;
    const uint32_t W = hl + 1 + ((L - 1) * M) / L, lp = (L + 3) / 4 * 4;
    std::vector<float> g(size_t(W) * lp, 0.0f);
    for (uint32_t i = 0; i < W; ++i)
        for (uint32_t k = 0; k < L; ++k) {
            const int d = static_cast<int>(hl + (k * M) / L) - static_cast<int>(i);
            if (d >= 0 && d <= static_cast<int>(hl)) g[i * lp + k] = rs.h[(k * M) % L + d * L];
        }
    *count = static_cast<uint32_t>(g.size());
    return g;
}

double phasor_arg(double rad) {  // mixer_t::set_phase* builds float phasors (mixer.cpp:27-33)
    const float c = std::cos(static_cast<float>(rad)), s = std::sin(static_cast<float>(rad));
    return std::atan2(static_cast<double>(s), static_cast<double>(c));
}

void fill_pairs(uint32_t N_TS, uint32_t* pair, uint32_t& mod) {  // transmit_diversity_precoding.cpp:48-75
    std::memset(pair, 0, 12 * sizeof(uint32_t));
    mod = 1;
    if (N_TS <= 1) return;
    mod = geo::txdiv_modulo(N_TS);
    for (uint32_t i = 0; i < mod; ++i) {
        uint32_t A, B;
        geo::txdiv_pair(N_TS, i, A, B);
        pair[i] = A | (B << 4);
    }
}

static uint32_t G_cap_default(const dnrp_cfg& c) {
    // scrambling sequences cover at least one PacketLength=2 slot packet of the device class
    dnrp_psdef d{c.u_max, c.b_max, 1, 2, 0, 9, 6144};
    dnrp_packet_sizes q;
    if (geo::packet_sizes(d, q)) return q.G;
    return 1u << 20;
}

int ensure_seq(dnrp_ctx* ctx, netid_seq& s, uint32_t nid, uint32_t nbits) {
    if (s.nbits >= nbits) return DNRP_OK;
    const uint32_t len = std::max(nbits, G_cap_default(ctx->cfg));
    // scrambling_pdc.cpp:41-48: type 1 c_init = id & 0xFF, type 2 c_init = id >> 8
    if (!s.t1.upload(geo::gold_bits_packed(nid & 0xFFu, len))) return DNRP_ENOMEM;
    if (!s.t2.upload(geo::gold_bits_packed(nid >> 8, len))) return DNRP_ENOMEM;
    s.nbits = len;
    return DNRP_OK;
}

}  // namespace dnrp::host

extern "C" {

const char* dnrp_strerror(int code) {
    switch (code) {
        case DNRP_OK: return "ok";
        case DNRP_EINVAL: return "invalid argument";
        case DNRP_ECONFIG: return "invalid packet configuration";
        case DNRP_EUNSUPPORTED: return "configuration not supported by the reference receiver";
        case DNRP_ENOMEM: return "device memory allocation failed or batch too large";
        case DNRP_EDEVICE: return "HIP runtime error";
        case DNRP_ENETID: return "network ID not registered";
        case DNRP_ESTATE: return "no preceding dnrp_rx_pcc_batch";
        default: return "unknown error";
    }
}

int dnrp_ctx_create(const dnrp_cfg* cfg, dnrp_ctx** out) {
    if (!cfg || !out) return DNRP_EINVAL;
    *out = nullptr;
    const auto& c = *cfg;
    const bool uok = c.u_max == 1 || c.u_max == 2 || c.u_max == 4 || c.u_max == 8;
    const bool bok = c.b_max == 1 || c.b_max == 2 || c.b_max == 4 || c.b_max == 8 || c.b_max == 12 || c.b_max == 16;
    const bool nok = c.N_TX_max == 1 || c.N_TX_max == 2 || c.N_TX_max == 4 || c.N_TX_max == 8;
    const bool ook = c.os_min == 1 || c.os_min == 2 || c.os_min == 4 || c.os_min == 8;
    if (!uok || !bok || !nok || !ook || c.L == 0 || c.M == 0 || c.max_batch == 0) return DNRP_EINVAL;
    if (!((c.L == 1 && c.M == 1) || c.L > c.M)) return DNRP_EINVAL;  // TX up-samples (rx_pacer.cpp:50-52)
    if (hipSetDevice(c.device) != hipSuccess) return DNRP_EDEVICE;
    auto ctx = std::make_unique<dnrp_ctx>();
    ctx->cfg = c;
    if (ctx->cfg.chestim_lr_stride == 0) ctx->cfg.chestim_lr_stride = 1;
    read_create(ctx->sw);
    if (!ctx->pcc_seq.upload(geo::gold_bits_packed(0x44454354u, 200))) return DNRP_ENOMEM;  // pcc_enc.cpp:46,104
    *out = ctx.release();
    return DNRP_OK;
}

int dnrp_ctx_destroy(dnrp_ctx* ctx) {
    if (!ctx) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    (void)hipDeviceSynchronize();
    delete ctx;
    return DNRP_OK;
}

int dnrp_add_network_id(dnrp_ctx* ctx, uint32_t network_id) {
    if (!ctx) return DNRP_EINVAL;
    auto& s = ctx->netid[network_id];
    if (!s) s = std::make_unique<netid_seq>();
    return ensure_seq(ctx, *s, network_id, G_cap_default(ctx->cfg));
}

int dnrp_get_packet_sizes(const dnrp_ctx* ctx, const dnrp_psdef* d, dnrp_packet_sizes* out) {
    if (!ctx || !d || !out) return DNRP_EINVAL;
    dnrp_packet_sizes q;
    if (!geo::packet_sizes(*d, q)) return DNRP_ECONFIG;
    if (d->u > ctx->cfg.u_max || d->b > ctx->cfg.b_max) return DNRP_EUNSUPPORTED;
    const auto dm = geo::make_dims(ctx->cfg, *d, q);
    q.N_b_DFT_os = dm.Nd;
    q.N_samples_packet_no_GI_os_rs = dm.N_no_GI_rs;
    q.N_samples_packet_os_rs = dm.N_packet_rs;
    *out = q;
    return DNRP_OK;
}

int dnrp_compute_packet_sizes(const dnrp_cfg* cfg, const dnrp_psdef* d, dnrp_packet_sizes* out) {
    if (!d || !out) return DNRP_EINVAL;
    dnrp_packet_sizes q;
    if (!geo::packet_sizes(*d, q)) return DNRP_ECONFIG;
    q.N_b_DFT_os = q.N_samples_packet_no_GI_os_rs = q.N_samples_packet_os_rs = 0;
    if (cfg) {
        if (cfg->L == 0 || cfg->M == 0 || cfg->os_min == 0 || d->u > cfg->u_max || d->b > cfg->b_max)
            return DNRP_EINVAL;
        const auto dm = geo::make_dims(*cfg, *d, q);
        q.N_b_DFT_os = dm.Nd;
        q.N_samples_packet_no_GI_os_rs = dm.N_no_GI_rs;
        q.N_samples_packet_os_rs = dm.N_packet_rs;
    }
    *out = q;
    return DNRP_OK;
}

int dnrp_ctx_set_rx_mode(dnrp_ctx* ctx, uint32_t flags) {
    if (!ctx || (flags & ~uint32_t(DNRP_RX_MODE_SM_MMSE))) return DNRP_EINVAL;
    if (flags != ctx->rx_mode) ctx->rx2t.clear();  // PDC tables depend on the mode
    ctx->rx_mode = flags;
    ctx->rx_valid = false;
    return DNRP_OK;
}

int dnrp_sync(dnrp_ctx* ctx, void* stream) {
    if (!ctx) return DNRP_EINVAL;
    return hipStreamSynchronize(static_cast<hipStream_t>(stream)) == hipSuccess ? DNRP_OK : DNRP_EDEVICE;
}

int dnrp_last_kernel_ms(const dnrp_ctx* ctx, const char* name, float* ms) {
    if (!ctx || !name || !ms) return DNRP_EINVAL;
    auto it = ctx->ev.find(name);
    if (it == ctx->ev.end() || it->second.used == 0) return DNRP_EINVAL;
    const auto& p = it->second.ev[it->second.used - 1];
    if (hipEventSynchronize(p.second) != hipSuccess) return DNRP_EDEVICE;
    return hipEventElapsedTime(ms, p.first, p.second) == hipSuccess ? DNRP_OK : DNRP_EDEVICE;
}

int dnrp_kernel_time_total(dnrp_ctx* ctx, const char* name, float* total_ms, uint32_t* count, int reset) {
    if (!ctx || !name || !total_ms || !count) return DNRP_EINVAL;
    *total_ms = 0.0f;
    *count = 0;
    auto it = ctx->ev.find(name);
    if (it == ctx->ev.end()) return DNRP_OK;
    auto& pool = it->second;
    for (size_t i = 0; i < pool.used; ++i) {
        float ms = 0.0f;
        if (hipEventSynchronize(pool.ev[i].second) != hipSuccess) return DNRP_EDEVICE;
        if (hipEventElapsedTime(&ms, pool.ev[i].first, pool.ev[i].second) != hipSuccess) return DNRP_EDEVICE;
        *total_ms += ms;
    }
    *count = static_cast<uint32_t>(pool.used);
    if (reset) pool.used = 0;
    return DNRP_OK;
}

}  // extern "C"
