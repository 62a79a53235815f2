// C-ABI synchronisation entry point (include/dnrp.h dnrp_rx_sync_batch): per-(u, b) tables built
// as the sync_chunk_t / crosscorrelator_t / stf_template_t constructors do
// (sync_chunk.cpp:32-123, crosscorrelator.cpp:22-59, stf_template.cpp:22-206), then three launches
// (kernels/sync_steps.hip, sync_detect.hip, sync_fine.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstring>
#include <memory>
#include <vector>

#include <cstdio>
#include <cstdlib>

#include "ctx_internal.hpp"

using namespace dnrp;
using namespace dnrp::host;

namespace {

using cd = std::complex<double>;

const float* const COVER = prm::STF_COVER;  // stf.hpp:146-151 (cover sequence active)

// unnormalised DFT of any length: the STF IFFT is 64 b os points (768 / 1536 / 3072 for b = 12),
// the template spectra are powers of two. Init-time only.
void dft_direct(std::vector<cd>& x, int sign) {
    const size_t n = x.size();
    std::vector<cd> y(n, cd(0, 0));
    for (size_t k = 0; k < n; ++k) {
        cd acc(0, 0);
        for (size_t i = 0; i < n; ++i) {
            const double a = sign * 2.0 * M_PI * static_cast<double>((k * i) % n) / static_cast<double>(n);
            acc += x[i] * cd(std::cos(a), std::sin(a));
        }
        y[k] = acc;
    }
    x.swap(y);
}

void fft_host(std::vector<cd>& x, int sign) {  // iterative radix-2 for powers of two, unnormalised
    const size_t n = x.size();
    if (n == 0 || (n & (n - 1))) return dft_direct(x, sign);
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(x[i], x[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double a = sign * 2.0 * M_PI / static_cast<double>(len);
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const cd w(std::cos(a * k), std::sin(a * k));
                const cd u = x[i + k], v = x[i + k + len / 2] * w;
                x[i + k] = u + v;
                x[i + k + len / 2] = u - v;
            }
    }
}

// stf_template_t::generate_stf_time_domain (stf_template.cpp:81-206): the STF of (b, N_eff_TX) at the
// class rate N_b_DFT_os = 64 b_max os for every b <= b_max (insert offset (N_b_DFT_os - 64 b) / 2 +
// guards_bottom(b) before the mirror), IFFT + CP, 1/sqrt(N_b_OCC(b)/4), cover sequence over patterns
// of 16 b_max os samples, TX resampler L/M with the final flush, truncated to stf_len * L / M hw samples
std::vector<cd> stf_template(uint32_t u, uint32_t b_max, uint32_t os, const geo::resampler_t& rs_tx, uint32_t b,
                             uint32_t N_eff_TX) {
    const uint32_t N = 56 * b, Nd = 64 * b_max * os;
    const uint32_t off_lower = Nd - N / 2;  // insert offset + mirror (tx_rx.cpp:197-240)
    const uint32_t cp = (Nd / 4) * (u == 1 ? 3 : 5), len = cp + Nd;
    const auto stf = geo::stf_values(b, N_eff_TX);
    const double scale = 1.0 / std::sqrt(static_cast<double>(static_cast<float>(N / 4)));
    std::vector<cd> bins(Nd, cd(0, 0));
    for (uint32_t k = 0; k <= N; ++k)
        bins[(k >= N / 2) ? (k - N / 2) : (off_lower + k)] = cd(stf[k].real(), stf[k].imag()) * scale;
    fft_host(bins, +1);  // FFTW backward = unnormalised inverse
    const uint32_t pat = 16 * b_max * os, n_pat = u == 1 ? 7 : 9;
    std::vector<cd> x(len);
    for (uint32_t i = 0; i < len; ++i) {
        x[i] = bins[(i + Nd - (cp % Nd)) % Nd];
        if (i / pat < n_pat) x[i] *= static_cast<double>(COVER[i / pat]);
    }
    const uint32_t L = rs_tx.L, M = rs_tx.M, out_len = len * L / M;
    std::vector<cd> y(out_len, cd(0, 0));
    for (uint32_t m = 0; m < out_len; ++m) {
        if (L == 1 && M == 1) {
            y[m] = x[m];
            continue;
        }
        const uint64_t t = rs_tx.delay + static_cast<uint64_t>(m) * M;
        const int64_t p = static_cast<int64_t>(t / L);
        const uint32_t ph = static_cast<uint32_t>(t % L);
        cd acc(0, 0);
        for (uint32_t d = 0; d <= rs_tx.hl; ++d) {
            const int64_t q = p - d;
            if (q < 0 || q >= static_cast<int64_t>(len)) continue;
            acc += x[q] * static_cast<double>(rs_tx.h[ph + d * L]);
        }
        y[m] = acc;
    }
    return y;
}

// one row of sync_args::tmpl_f: conj(DFT(template)) / n_fft of the (b, N_eff_TX) template in a b_max stream
void template_spectrum(uint32_t u, uint32_t b_max, uint32_t os, const geo::resampler_t& rs_tx, uint32_t b, uint32_t N_eff_TX,
                       uint32_t nf, float2* out) {
    auto tm = stf_template(u, b_max, os, rs_tx, b, N_eff_TX);
    tm.resize(nf, cd(0, 0));
    fft_host(tm, -1);
    for (uint32_t i = 0; i < nf; ++i) {
        const cd v = std::conj(tm[i]) / static_cast<double>(nf);
        out[i] = make_float2(static_cast<float>(v.real()), static_cast<float>(v.imag()));
    }
}

// b_idx2b (physical_resources.hpp): the packet bandwidths, ascending
constexpr uint32_t B_IDX2B[6] = {1, 2, 4, 8, 12, 16};

// the N_b_DFT_os-point transform at the coarse peak (coarse_peak_f_domain.cpp:55), first use for this
// (u, b_max) by the beta search or the integer CFO search: plan and twiddles
bool ensure_coarse_fft(sync_tables* t) {
    if (t->coarse_fft_ready) return true;
    const uint32_t N = prm::N_SAMPLES_STF_PATTERN * 4 * t->bos;  // 64 b_max os
    t->beta_plan = make_plan(N);
    if (!t->tw_beta.upload(twiddles(N))) return false;
    t->coarse_fft_ready = true;
    return true;
}

// beta search (dnrp_ctx_set_sync_beta_search), first use for this (u, b_max): the template spectra of
// every b <= b_max (stf_template.cpp:137-199; row block b_idx, the last one equal to tmpl_f) and the
// transform at the coarse peak
bool ensure_beta(const dnrp_cfg& c, sync_tables* t) {
    if (t->beta_ready) return true;
    if (!ensure_coarse_fft(t)) return false;
    const uint32_t nf = 1u << t->log2_fft;
    const auto rs_tx = geo::make_resampler(c.L, c.M, c.os_min, prm::RS_TX);
    uint32_t nb = 0;
    while (nb < 6 && B_IDX2B[nb] <= t->b) ++nb;
    std::vector<float2> tf(size_t(nb) * t->n_templates * nf);
    for (uint32_t bi = 0; bi < nb; ++bi)
        for (uint32_t k = 0; k < t->n_templates; ++k)
            template_spectrum(t->u, t->b, c.os_min, rs_tx, B_IDX2B[bi], 1u << k, nf, &tf[(size_t(bi) * t->n_templates + k) * nf]);
    if (!t->tmpl_fb.upload(tf)) return false;
    t->beta_ready = true;
    return true;
}

sync_tables* get_sync(dnrp_ctx* ctx, uint32_t u, uint32_t b, int* err) {
    auto& slot = ctx->synct[{u, b}];
    if (slot) return slot.get();
    const auto& c = ctx->cfg;
    auto t = std::make_unique<sync_tables>();
    t->u = u;
    t->b = b;
    t->n_pattern = u == 1 ? prm::N_STF_PATTERN_U1 : prm::N_STF_PATTERN_U248;  // stf.hpp:91-97
    t->bos = b * c.os_min;
    t->stf_len = prm::N_SAMPLES_STF_PATTERN * t->n_pattern * t->bos;
    t->pattern = prm::N_SAMPLES_STF_PATTERN * t->bos;
    t->step = t->pattern / prm::SYNC_STEP_DIVIDER;  // autocorrelator_detection.cpp:49
    t->D = static_cast<uint32_t>(prm::SYNC_PEAK_MAX_SEARCH_STFS * t->stf_len);  // sync_chunk.cpp:68
    t->rms_min = static_cast<float>(prm::SYNC_RMS_MIN * std::sqrt(static_cast<double>(u) * b * prm::SAMP_RATE_MIN_U_B /
                                                                  prm::SYNC_RMS_MIN_REF_RATE));
    t->xc_l = prm::SYNC_XC_SEARCH_LEFT * b * c.os_min * c.L / c.M;  // crosscorrelator.cpp:53-56
    t->xc_len = t->xc_l + prm::SYNC_XC_SEARCH_RIGHT * b * c.os_min * c.L / c.M + 1;
    t->tmpl_len = t->stf_len * c.L / c.M;
    t->n_templates = c.N_TX_max >= 8 ? 4 : c.N_TX_max >= 4 ? 3 : c.N_TX_max >= 2 ? 2 : 1;  // physical_resources.hpp:44
    uint32_t lg = 0;
    while ((1u << lg) < t->xc_len - 1 + t->tmpl_len) ++lg;
    t->log2_fft = lg;
    const uint32_t nf = 1u << lg;
    // sync resampler: RX direction, L and M swapped (sync_chunk.cpp:40-48)
    t->rs = geo::make_resampler(c.M, c.L, c.os_min, prm::RS_SYNC);
    if (!(c.L == 1 && c.M == 1)) {
        const auto al = geo::resampler_align(t->rs);
        t->m_star = al.m_star;
        t->p_star = al.p_star;
    }
    const auto rs_tx = geo::make_resampler(c.L, c.M, c.os_min, prm::RS_TX);  // stf_template.cpp: TX filter
    std::vector<float2> tf(size_t(t->n_templates) * nf);
    for (uint32_t k = 0; k < t->n_templates; ++k) template_spectrum(u, b, c.os_min, rs_tx, b, 1u << k, nf, &tf[size_t(k) * nf]);
    std::vector<float> pp = (c.L == 1 && c.M == 1) ? std::vector<float>{0.f} : taps_polyphase(t->rs, &t->npp);
    if (c.L == 1 && c.M == 1) t->npp = 0;
    if (!t->taps.upload(t->rs.h) || !t->taps_pp.upload(pp) || !t->tmpl_f.upload(tf) || !t->tw_fft.upload(twiddles(nf))) {
        *err = DNRP_ENOMEM;
        return nullptr;
    }
    slot = std::move(t);
    return slot.get();
}

// common::adt::db2mag of the threshold: the reference compares a power ratio against this magnitude
// conversion (coarse_peak_f_domain.cpp:143-144,177); kept as it is there
float beta_linear(float db) { return std::pow(10.0f, db / 20.0f); }

}  // namespace

extern "C" int dnrp_ctx_set_sync_beta_search(dnrp_ctx* ctx, uint32_t on, float threshold_db) {
    if (!ctx || on > 1 || !std::isfinite(threshold_db)) return DNRP_EINVAL;
    ctx->sync_beta_on = on;
    ctx->sync_beta_db = threshold_db;
    return DNRP_OK;
}

extern "C" int dnrp_ctx_get_sync_beta_search(const dnrp_ctx* ctx, uint32_t* on, float* threshold_db, float* threshold_linear) {
    if (!ctx) return DNRP_EINVAL;
    if (on) *on = ctx->sync_beta_on;
    if (threshold_db) *threshold_db = ctx->sync_beta_db;
    if (threshold_linear) *threshold_linear = beta_linear(ctx->sync_beta_db);
    return DNRP_OK;
}

extern "C" int dnrp_ctx_set_sync_icfo_search(dnrp_ctx* ctx, uint32_t range) {
    if (!ctx || range > dev::SYNC_ICFO_MAX) return DNRP_EINVAL;
    ctx->sync_icfo_range = range;
    return DNRP_OK;
}

extern "C" int dnrp_ctx_get_sync_icfo_search(const dnrp_ctx* ctx, uint32_t* range) {
    if (!ctx) return DNRP_EINVAL;
    if (range) *range = ctx->sync_icfo_range;
    return DNRP_OK;
}

extern "C" int dnrp_rx_sync_icfo_scores(dnrp_ctx* ctx, uint32_t n_reports, float* score, int32_t* k, void* stream) {
    if (!ctx || !score || !k) return DNRP_EINVAL;
    if (ctx->sync_icfo_reports == 0) return DNRP_ESTATE;
    if (n_reports != ctx->sync_icfo_reports) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t row = 8 * dev::SYNC_ICFO_COLS;
    HIPCHK(hipMemcpyAsync(score, ctx->sy_icfo.p, size_t(n_reports) * row * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // k is decided here, on the copy, by the device's function
    for (uint32_t r = 0; r < n_reports; ++r) k[r] = dev::sync_icfo_k(score + size_t(r) * row, ctx->sync_icfo_ant);
    return DNRP_OK;
}

extern "C" int dnrp_ctx_set_sync_fine_all_antennas(dnrp_ctx* ctx, uint32_t on) {
    if (!ctx || on > 1) return DNRP_EINVAL;
    ctx->sync_fine_all = on;
    return DNRP_OK;
}

extern "C" int dnrp_ctx_get_sync_fine_all_antennas(const dnrp_ctx* ctx, uint32_t* on) {
    if (!ctx) return DNRP_EINVAL;
    if (on) *on = ctx->sync_fine_all;
    return DNRP_OK;
}

extern "C" int dnrp_rx_sync_fine_peaks(dnrp_ctx* ctx, uint32_t n_reports, float* metric, uint32_t* index, void* stream) {
    if (!ctx || !metric || !index) return DNRP_EINVAL;
    if (ctx->sync_fine_reports == 0) return DNRP_ESTATE;
    if (n_reports != ctx->sync_fine_reports) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipMemcpyAsync(metric, ctx->sy_fine_m.p, size_t(n_reports) * 32 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(index, ctx->sy_fine_i.p, size_t(n_reports) * 32 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return DNRP_OK;
}

// dnrp_query_table "sync_template": the time-domain STF template of a b packet in a (u, b_max, os_min,
// L, M) stream, tmpl_len hw samples (the row get_sync / ensure_beta transform for sync_fine_kernel)
std::vector<std::complex<double>> dnrp::geo::sync_template(uint32_t u, uint32_t b_max, uint32_t os_min, uint32_t L, uint32_t M,
                                                           uint32_t b, uint32_t N_eff_TX) {
    return stf_template(u, b_max, os_min, geo::make_resampler(L, M, os_min, prm::RS_TX), b, N_eff_TX);
}

// Tranche schedule of one call: the frontiers (exclusive step ends, ascending, the last n_steps) at
// which the detection runs on the step sums computed so far. sync_chunk_t::search() resamples and
// correlates only as far as its next step needs and returns at the first packet
// (sync_chunk.cpp:159-166, 259); computing every step of every window before the first detection
// spends most of the step-sum work behind the last requested report. A function of the sync
// geometry and the launch geometry only, never of where a packet is expected:
//  - first tranche 4 STFs of steps, then doubling sizes, at most 4 tranches, a remainder shorter
//    than the first tranche joined to the one before it;
//  - one tranche (every step, then the detection) where the search is shorter than 6 first tranches
//    or the call's step sums are under 2^28 DECT samples (~0.6 ms of sync_steps on MI355X): there
//    the added launches per tranche (step sums, split rounds, inline detection) are not paid back
//    (C2: 4-sample steps, launch-latency bound).
// forced (switches::sync_tranche, DNRP_SYNC_TRANCHE): explicit tranche sizes instead.
// (dnrp_query_table "sync_tranches" reports it.)
std::vector<uint32_t> dnrp::geo::sync_tranches(uint32_t n_steps, uint32_t step, uint32_t stf_len, uint32_t n, uint32_t n_ant,
                                               const std::vector<uint64_t>* forced) {
    std::vector<uint32_t> fr;
    if (forced) {
        uint32_t at = 0;
        for (const uint64_t v : *forced)
            if (v > 0 && v < n_steps - at) fr.push_back(at += static_cast<uint32_t>(v));
        fr.push_back(n_steps);
        return fr;
    }
    const uint32_t t0 = std::max(1u, 4 * stf_len / step);
    const uint64_t samples = uint64_t(n) * n_ant * n_steps * step;
    if (n_steps >= 6 * t0 && samples >= (uint64_t(1) << 28))
        for (uint32_t at = 0, sz = t0; fr.size() < 3 && n_steps - at >= sz + t0; sz *= 2) fr.push_back(at += sz);
    fr.push_back(n_steps);
    return fr;
}

extern "C" int dnrp_rx_sync_batch(dnrp_ctx* ctx, const dnrp_sync_cfg* sc, uint32_t n, const float* iq,
                                  uint64_t win_stride, uint64_t ant_stride, uint32_t S_win, dnrp_sync_result* res,
                                  uint32_t* n_found, void* stream) {
    static_assert(sizeof(dnrp_sync_result) == sizeof(dev::sync_res), "dnrp_sync_result layout");
    if (!ctx || !sc || (n > 0 && (!iq || !res))) return DNRP_EINVAL;
    if (n == 0) return DNRP_OK;
    if (n > ctx->cfg.max_batch) return DNRP_ENOMEM;
    const bool uok = sc->u == 1 || sc->u == 2 || sc->u == 4 || sc->u == 8;
    const bool bok = sc->b == 1 || sc->b == 2 || sc->b == 4 || sc->b == 8 || sc->b == 12 || sc->b == 16;
    if (!uok || !bok || sc->u > ctx->cfg.u_max || sc->b > ctx->cfg.b_max) return DNRP_EINVAL;
    if (sc->N_ant_limited == 0 || sc->N_ant_limited > ctx->cfg.N_TX_max || sc->N_ant_limited > prm::SYNC_ANTENNA_LIMIT)
        return DNRP_EINVAL;
    if (sc->max_reports == 0 || S_win == 0 || sc->chunk_len < ctx->cfg.L) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    ctx->sync_fine_reports = 0;  // dnrp_rx_sync_fine_peaks: the table of this call, once it has run with the setting on
    ctx->sync_icfo_reports = 0;  // dnrp_rx_sync_icfo_scores: likewise
    int err = DNRP_OK;
    sync_tables* t = get_sync(ctx, sc->u, sc->b, &err);
    if (!t) return err;
    const auto& c = ctx->cfg;
    dev::sync_args a{};
    a.n_ant = sc->N_ant_limited;
    a.n_pattern = t->n_pattern;
    a.stf_len = t->stf_len;
    a.pattern = t->pattern;
    a.step = t->step;
    const uint64_t A_len = uint64_t(sc->chunk_len) / c.L * c.M;  // sync_chunk.cpp:63-64
    const uint64_t search = A_len + static_cast<uint32_t>(prm::SYNC_OVERLAP_STFS * t->stf_len);
    if (search > (1u << 30)) return DNRP_EINVAL;
    a.search_len = static_cast<uint32_t>(search);
    a.D = t->D;
    a.bos = t->bos;
    a.n_steps = (a.search_len + a.step - 1) / a.step;
    a.L = t->rs.L;
    a.M = t->rs.M;
    a.delay = t->rs.delay;
    a.hl = t->rs.hl;
    a.ct_taps = dev::sync_taps_match(t->rs.h.data(), t->rs.h.size()) ? 1u : 0u;
    a.m_star = t->m_star;
    a.p_star = t->p_star;
    a.npp = t->npp;
    a.taps = t->taps.as<float>();
    a.taps_pp = t->taps_pp.as<float>();
    a.rms_min = t->rms_min;
    a.prefactor = static_cast<float>(t->n_pattern) / static_cast<float>(t->n_pattern - 1);
    a.n_uw = t->n_pattern - 1;
    for (uint32_t i = 0; i < a.n_uw; ++i) a.uw[i] = COVER[i] * COVER[i + 1];  // stf.cpp:140-159
    a.iq = reinterpret_cast<const float2*>(iq);
    a.win_stride = win_stride;
    a.ant_stride = ant_stride;
    a.S_win = S_win;
    a.n_win = n;
    a.max_reports = sc->max_reports;
    a.Ltx = c.L;
    a.Mtx = c.M;
    a.xc_l = t->xc_l;
    a.xc_len = t->xc_len;
    a.tmpl_len = t->tmpl_len;
    a.n_templates = t->n_templates;
    a.log2_fft = t->log2_fft;
    a.tmpl_f = t->tmpl_f.as<float2>();
    a.tw_fft = t->tw_fft.as<float2>();
    a.u = sc->u;
    a.b = sc->b;
    if (ctx->sync_beta_on && sc->b > 1) {  // b_max == 1: nothing to estimate (coarse_peak_f_domain.cpp:97-99)
        if (!ensure_beta(c, t) ||
            !ctx->sy_band.ensure(size_t(n) * sc->max_reports * 8 * dev::SYNC_BANDS * sizeof(float)))
            return DNRP_ENOMEM;
        a.beta_on = 1;
        a.beta_thr = beta_linear(ctx->sync_beta_db);
        a.band = ctx->sy_band.as<float>();
        a.tmpl_f = t->tmpl_fb.as<float2>();
    }
    if (ctx->sync_icfo_range) {
        if (!ensure_coarse_fft(t) ||
            !ctx->sy_icfo.ensure(size_t(n) * sc->max_reports * 8 * dev::SYNC_ICFO_COLS * sizeof(float)))
            return DNRP_ENOMEM;
        a.icfo_range = ctx->sync_icfo_range;
        a.icfo_N = t->beta_plan.N;
        a.icfo = ctx->sy_icfo.as<float>();
    }
    a.fine_all = ctx->sync_fine_all;
    a.det_stage = dev::sync_detect_stage(a);
    if (dev::sync_detect_lds(a) > dev::LDS_BYTES || !dev::sync_fine_ok(a))
        return DNRP_EUNSUPPORTED;
    const size_t nsa = size_t(n) * a.n_ant * a.n_steps;
    if (!ctx->sy_P.ensure(nsa * sizeof(float)) || !ctx->sy_C.ensure(nsa * sizeof(float2)) ||
        !ctx->sy_res.ensure(size_t(n) * a.max_reports * sizeof(dev::sync_res)) || !ctx->sy_cnt.ensure(size_t(n) * 4) ||
        !ctx->sy_spec.ensure(size_t(n) * a.max_reports * (a.fine_all ? a.n_ant : 1u) * (size_t(1) << a.log2_fft) * sizeof(float2)) ||
        !ctx->sy_post.ensure(size_t(n) * a.max_reports * 8 * sizeof(float)) ||
        !ctx->sy_state.ensure(size_t(n) * sizeof(dev::sync_state)) || !ctx->sy_pk.ensure(size_t(n) * 8 * sizeof(float2)))
        return DNRP_ENOMEM;
    if (a.fine_all) {
        if (!ctx->sy_fine_m.ensure(size_t(n) * a.max_reports * 32 * sizeof(float)) ||
            !ctx->sy_fine_i.ensure(size_t(n) * a.max_reports * 32 * sizeof(uint32_t)))
            return DNRP_ENOMEM;
        a.fine_m = ctx->sy_fine_m.as<float>();
        a.fine_i = ctx->sy_fine_i.as<uint32_t>();
    }
    a.state = ctx->sy_state.as<dev::sync_state>();
    a.pk = ctx->sy_pk.as<float2>();
    a.spec = ctx->sy_spec.as<float2>();
    a.post = ctx->sy_post.as<float>();
    a.P = ctx->sy_P.as<float>();
    a.Cs = ctx->sy_C.as<float2>();
    a.res = ctx->sy_res.as<dev::sync_res>();
    a.n_found = ctx->sy_cnt.as<uint32_t>();
    hipStream_t st = static_cast<hipStream_t>(stream);
#ifdef DNRP_SYNC_PROFILE
    // phase clocks of sync_detect per window (tools/sync_profile.py): averages to stderr
    static dbuf prof;
    const bool do_prof = std::getenv("DNRP_SYNC_PROFILE") && prof.ensure(size_t(n) * 32 * 8);
    a.prof = do_prof ? prof.as<unsigned long long>() : nullptr;
    if (do_prof) HIPCHK(hipMemsetAsync(prof.p, 0, size_t(n) * 32 * 8, st));
#endif
    switches& sw = ctx->sw;
    read_sync(sw);  // per call: tests switch them at run time
    // detection + coarse peak: `rounds` split rounds (detection-only workgroups, then one coarse-peak
    // workgroup per (window, antenna) of every pending detection), then the inline form finishes what
    // is left (windows with more detections than rounds); default sw.sync_rounds
    const int rounds = !dev::sync_peak_ok(a) ? 0 : sw.sync_rounds >= 0 ? sw.sync_rounds : (a.n_ant > 1 ? 2 : 0);
    // Step sums in tranches (sync_tranches above): per tranche the step-sum launch over its steps,
    // then the detection launches up to that frontier. A window that reaches max_reports is finished
    // (pend = 2) and the later tranches' step-sum waves of it leave at once; a window whose scan
    // reaches the frontier saves its loop registers and goes on in the next tranche. Stream-ordered
    // throughout; the timer names accumulate over the tranches.
    const std::vector<uint32_t> frontier =
        geo::sync_tranches(a.n_steps, a.step, a.stf_len, n, a.n_ant, sw.sync_tranche_set ? &sw.sync_tranche : nullptr);
    a.first = 1;
    a.rounds = static_cast<uint32_t>(rounds);  // the first `rounds` detections of a window go to sync_peak, in any tranche
    for (size_t k = 0; k < frontier.size(); ++k) {
        a.s_lo = k ? frontier[k - 1] : 0u;
        a.s_hi = frontier[k];
        a.skip = k ? 1u : 0u;  // the first tranche must not read the state: not initialised yet
        ctx->tic("sync_steps", st);
        if (dev::launch_sync_steps(a, n, st, sw.sync_steps) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("sync_steps", st);
        for (int r = 0; r < rounds; ++r) {
            ctx->tic("sync_detect", st);
            if (dev::launch_sync_detect_split(a, n, st) != hipSuccess) return DNRP_EDEVICE;
            ctx->toc("sync_detect", st);
            a.first = 0;
            ctx->tic("sync_peak", st);
            if (dev::launch_sync_peak(a, n, st) != hipSuccess) return DNRP_EDEVICE;
            ctx->toc("sync_peak", st);
        }
        ctx->tic("sync_detect", st);
        if (dev::launch_sync_detect(a, n, st) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("sync_detect", st);
        a.first = 0;
    }
#ifdef DNRP_SYNC_PROFILE
    if (do_prof) {
        std::vector<unsigned long long> h(size_t(n) * 32);
        HIPCHK(hipMemcpyAsync(h.data(), prof.p, h.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double acc[16] = {};
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const unsigned long long* r = &h[size_t(i) * 32];
            if (!r[0] || !r[11]) continue;
            ++cnt;
            unsigned long long prev = r[0];
            for (int k = 1; k < 12; ++k)
                if (r[k]) {
                    acc[k] += double(r[k] - prev);
                    prev = r[k];
                }
        }
        std::fprintf(stderr, "sync_detect phases (wall_clock64 ticks, mean over %u windows):", cnt);
        for (int k = 1; k < 12; ++k) std::fprintf(stderr, " p%d=%.0f", k, cnt ? acc[k] / cnt : 0.0);
        double q[4] = {};
        for (uint32_t i = 0; i < n; ++i) {
            const unsigned long long* r = &h[size_t(i) * 32];
            if (!r[8] || !r[12] || !r[13] || !r[14]) continue;
            q[0] += double(r[12] - r[8]);
            q[1] += double(r[13] - r[12]);
            q[2] += double(r[14] - r[13]);
            q[3] += double(r[9] - r[14]);
        }
        std::fprintf(stderr, " | last peak search: sums %.0f scans %.0f metric %.0f smooth+argmax %.0f\n",
                     cnt ? q[0] / cnt : 0.0, cnt ? q[1] / cnt : 0.0, cnt ? q[2] / cnt : 0.0, cnt ? q[3] / cnt : 0.0);
        double pq[6] = {};
        uint32_t pc = 0;
        for (uint32_t i = 0; i < n; ++i) {  // sync_peak_kernel of antenna 0 (split rounds)
            const unsigned long long* r = &h[size_t(i) * 32 + 16];
            if (!r[0] || !r[6]) continue;
            ++pc;
            for (int k = 0; k < 6; ++k) pq[k] += double(r[k + 1] - r[k]);
        }
        std::fprintf(stderr, "sync_peak phases (%u windows): resample %.0f sums %.0f scans %.0f metric %.0f met %.0f smooth+argmax %.0f\n",
                     pc, pc ? pq[0] / pc : 0.0, pc ? pq[1] / pc : 0.0, pc ? pq[2] / pc : 0.0, pc ? pq[3] / pc : 0.0,
                     pc ? pq[4] / pc : 0.0, pc ? pq[5] / pc : 0.0);
    }
#endif
    ctx->tic("sync_post", st);
    if (dev::launch_sync_post(a, n, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("sync_post", st);
    dev::sync_beta_args ba{};
    if (a.beta_on || a.icfo_range) {
        ba.plan = t->beta_plan;
        ba.tw = t->tw_beta.as<float2>();
        ba.band = ctx->sy_band.as<float>();
        ba.cp = a.stf_len - ba.plan.N;
        for (uint32_t i = 0; i < 4; ++i) ba.cover[i] = COVER[t->n_pattern - 4 + i];
    }
    if (a.beta_on) {  // the band powers sync_fine decides b from; off: no launch, no report field written
        ctx->tic("sync_beta", st);
        if (dev::launch_sync_beta(a, ba, n, st) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("sync_beta", st);
    }
    if (a.icfo_range) {  // the candidate scores sync_fine decides cfo_int from; off: no launch, cfo_int stays 0
        ctx->tic("sync_icfo", st);  // the fill counts as the search's time
        // every row -1: reports not found and the antennas past n_ant are not visited by the kernel
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.icfo), 0xBF800000u,
                                 size_t(n) * a.max_reports * 8 * dev::SYNC_ICFO_COLS, st));
        if (dev::launch_sync_icfo(a, ba, n, st) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("sync_icfo", st);
        if (a.beta_on) {
            // both searches: the first beta decision read the spectrum with the integer CFO in it, and a packet
            // moved across a band edge looks wider than it is. The reports whose decided k is not 0 get their
            // band powers again on the spectrum moved back by 4 k bins; sync_fine then decides b from those
            // (sync_icfo_kernel's scores keep the first decision's cells)
            ba.shift = 1;
            ctx->tic("sync_beta", st);
            if (dev::launch_sync_beta(a, ba, n, st) != hipSuccess) return DNRP_EDEVICE;
            ctx->toc("sync_beta", st);
        }
    }
    ctx->tic("sync_fine", st);
    if (dev::launch_sync_fine(a, n, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("sync_fine", st);
    if (a.fine_all) ctx->sync_fine_reports = n * a.max_reports;
    if (a.icfo_range) {
        ctx->sync_icfo_reports = n * a.max_reports;
        ctx->sync_icfo_ant = a.n_ant;
    }
    HIPCHK(hipMemcpyAsync(res, a.res, size_t(n) * a.max_reports * sizeof(dev::sync_res), hipMemcpyDeviceToHost, st));
    if (n_found) HIPCHK(hipMemcpyAsync(n_found, a.n_found, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    return DNRP_OK;
}
