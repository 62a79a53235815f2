// Detection and coarse peak of the synchronisation (sync_common.hpp): the detection state machine with
// the inline coarse-peak search, the split rounds' coarse-peak kernel, and their launchers.
#include "sync_common.hpp"

// ---- compile-time knobs (-D), shipped values
// sync_detect_kernel: three waves per SIMD (<= 168 VGPRs, a few spills in the post-processing): with three workgroups'
// LDS per CU this beats the 2-wave default in the pipelined bench (A/B on MI355X: 181.4k vs 184.9k
// slot-pairs/s)
#ifndef SYNC_DETECT_ATTR
#define SYNC_DETECT_ATTR __attribute__((amdgpu_waves_per_eu(SPLIT ? DNRP_DET_SPLIT_WPE : 3)))
#endif
// the split form (detection conditions only, no resampling, small LDS): its own register budget
#ifndef DNRP_DET_SPLIT_WPE
#define DNRP_DET_SPLIT_WPE 6  // 69 VGPRs, 7 waves per SIMD (3: the non-split budget, 129 VGPRs)
#endif
// sync_peak_kernel
#ifndef DNRP_PEAK_STAGED
#define DNRP_PEAK_STAGED 1  // 1: the STF region's input span staged in LDS first (resample_staged): at 4 waves
                            // per SIMD neutral (2.75 vs 2.72 ms per chunk); what lets the window loads leave
                            // the registers for 6 waves per SIMD below
#endif
#ifndef DNRP_PEAK_IMAJ
#define DNRP_PEAK_IMAJ 1  // the staged windows input-major (pp_const::run_imaj)
#endif
#ifndef DNRP_PEAK_WPE
#define DNRP_PEAK_WPE 6  // 6 waves per SIMD = 3 workgroups per CU (80 VGPRs; the metric's double divisions
                         // spill ~100 B per lane at NUW 8):
                         // 2.76 -> 2.31-2.36 ms per C4 chunk against 4 (104 VGPRs, 2 workgroups per CU)
#endif

namespace dnrp::dev {

// ===================================================================== detection + coarse peak
struct det_eval {
    float rms, metric;
};

// autocorrelator_detection.cpp:186-280 at the step whose B block starts at s*step (movsums after
// the push: power over the last 4*n_pattern step values, correlation over the last 4*(n_pattern-1)
// with the cover pairwise products per group of 4; front = newest + oldest register, back = the
// two after the oldest: movsum.hpp get_sum_front/get_sum_back with ptr at the oldest element)
// P[i], Cs[i]: step values of step index i (global, or LDS copies addressed through offset pointers)
__device__ __forceinline__ bool detect_eval(const sync_args& A, const float* __restrict__ P, const float2* __restrict__ Cs,
                                            uint32_t s, det_eval& out) {
    const uint32_t np = 4 * A.n_pattern, nc = 4 * A.n_uw;
    // unrolled so each batch of loads is in flight together; the sums keep the reference's order
    double pw = 0.0;
#pragma unroll 8
    for (uint32_t i = 0; i < np; ++i) pw += P[s - (np - 1) + i];
    const double rms = sqrt(pw / static_cast<double>(A.stf_len));
    static_assert(prm::SYNC_RMS_FRONT_STEPS == 2 && prm::SYNC_RMS_BACK_STEPS == 2, "front/back register pairs");
    if (rms < static_cast<double>(A.rms_min) || static_cast<double>(prm::SYNC_RMS_MAX) < rms) return false;
    const double back = static_cast<double>(P[s - (np - 2)]) + P[s - (np - 3)];
    const double front = static_cast<double>(P[s - (np - 1)]) + P[s];
    if (sqrt(back) * prm::SYNC_RMS_FRONT_TO_BACK_RATIO >= sqrt(front)) return false;
    double cr = 0.0, ci = 0.0;
#pragma unroll 4
    for (uint32_t g = 0; g < A.n_uw; ++g) {
        double gr = 0.0, gi = 0.0;
        for (uint32_t j = 0; j < 4; ++j) {
            const float2 v = Cs[s - (nc - 1) + 4 * g + j];
            gr += v.x;
            gi += v.y;
        }
        cr += A.uw[g] * gr;
        ci += A.uw[g] * gi;
    }
    const double q = static_cast<double>(A.prefactor) * sqrt(cr * cr + ci * ci) / pw;
    const double metric = q * q;
    static_assert(prm::SYNC_METRIC_STREAK == 1 && prm::SYNC_METRIC_STREAK_GAIN == 0.0f, "single-step streak");
    if (metric < static_cast<double>(prm::SYNC_METRIC_MIN) || static_cast<double>(prm::SYNC_METRIC_MAX) < metric)
        return false;
    if (!(static_cast<double>(prm::SYNC_METRIC_MIN) < metric)) return false;  // streak_t(0.18, 0, 1)::check
    out.rms = static_cast<float>(rms);
    out.metric = static_cast<float>(metric);
    return true;
}

// exclusive prefix of n double2 values in v[] (in place), one wavefront; v[n] = total
__device__ void wave_scan_d2(double2* v, uint32_t n, uint32_t lane) {
    const uint32_t per = (n + 63) / 64;
    const uint32_t b = lane * per, e = min(b + per, n);
    double sx = 0.0, sy = 0.0;
    for (uint32_t i = b; i < e; ++i) {
        sx += v[i].x;
        sy += v[i].y;
    }
    double ix = sx, iy = sy;  // inclusive scan over lanes
    for (int o = 1; o < 64; o <<= 1) {
        const double tx = __shfl_up(ix, o), ty = __shfl_up(iy, o);
        if (static_cast<int>(lane) >= o) {
            ix += tx;
            iy += ty;
        }
    }
    double rx = ix - sx, ry = iy - sy;
    for (uint32_t i = b; i < e; ++i) {
        const double2 t = v[i];
        v[i] = make_double2(rx, ry);
        rx += t.x;
        ry += t.y;
    }
    if (lane == 63) v[n] = make_double2(ix, iy);
}

#ifdef DNRP_SYNC_PROFILE
#define SYNC_STAMP(i) \
    if (threadIdx.x == 0 && A.prof) A.prof[size_t(w) * 32 + (i)] = wall_clock64()
#else
#define SYNC_STAMP(i)
#endif

struct peak_lds {
    double2* ckc;  // correlation prefix at every 16th product
    double* ckp;   // power prefix at every 16th sample
    float* met;    // metric per position of the peak search (float, as the reference's movsum stages)
};

// autocorrelator_peak.cpp:145-264 for one antenna: per-sample metric over [r0, r0 + D), smoothed
// by the (2 bos + 1)-long moving mean (zero-initialised), last maximum wins (update on >=).
// lbuf[i] = lb[yb + i], yb = r0 - stf_len - SYNC_PAD_PEAK.
__device__ void peak_search(const sync_args& A, const float2* lbuf, uint32_t region, const peak_lds& L, uint32_t r0,
                            double* red, float& pk_metric, uint32_t& pk_idx) {
    const uint32_t P = A.pattern, yoff = A.stf_len + SYNC_PAD_PEAK;  // lbuf index of r0
    const uint32_t nprod = region - P, nsc = (nprod + 15) / 16, nsp = (region + 15) / 16;
    // segment sums: products prod(y) = lb[y-P] conj(lb[y]) indexed from lbuf index P; powers from 0
    // (each thread starts its 16-sample segment at its own rotation: segment starts are 32 banks
    // apart, so an unrotated walk would put a half-wave on two bank pairs)
    for (uint32_t g = threadIdx.x; g < nsc + nsp; g += blockDim.x) {
        if (g < nsc) {
            double sx = 0.0, sy = 0.0;
            for (uint32_t t = 0; t < 16; ++t) {
                const uint32_t j = 16 * g + ((t + g) & 15u);
                if (j >= nprod) continue;
                const float2 c = cmulc(lbuf[j], lbuf[j + P]);
                sx += c.x;
                sy += c.y;
            }
            L.ckc[g] = make_double2(sx, sy);
        } else {
            const uint32_t h = g - nsc;
            double sp = 0.0;
            for (uint32_t t = 0; t < 16; ++t) {
                const uint32_t j = 16 * h + ((t + h) & 15u);
                if (j < region) sp += cnorm(lbuf[j]);
            }
            L.ckp[h] = sp;
        }
    }
    __syncthreads();
#ifdef DNRP_SYNC_PROFILE
    const uint32_t w = blockIdx.x;
#endif
    SYNC_STAMP(12);
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (wv == 0) wave_scan_d2(L.ckc, nsc, lane);
    if (wv == 1) {  // power prefix: scan as double2 with zero imaginary parts via a temporary view
        const uint32_t per = (nsp + 63) / 64;
        const uint32_t b = lane * per, e = min(b + per, nsp);
        double s = 0.0;
        for (uint32_t i = b; i < e; ++i) s += L.ckp[i];
        double inc = s;
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_up(inc, o);
            if (static_cast<int>(lane) >= o) inc += t;
        }
        double r = inc - s;
        for (uint32_t i = b; i < e; ++i) {
            const double t = L.ckp[i];
            L.ckp[i] = r;
            r += t;
        }
        if (lane == 63) L.ckp[nsp] = inc;
    }
    __syncthreads();
    SYNC_STAMP(13);
    // prefix helpers: PC(z) = sum of prod with product index < z; PP(z) = sum of power index < z
    auto PC = [&](uint32_t z, double& rx, double& ry) {
        const uint32_t g = z >> 4;
        double2 c = L.ckc[g];
        for (uint32_t j = 16 * g; j < z; ++j) {
            const float2 v = cmulc(lbuf[j], lbuf[j + P]);
            c.x += v.x;
            c.y += v.y;
        }
        rx = c.x;
        ry = c.y;
    };
    auto PP = [&](uint32_t z) {
        const uint32_t g = z >> 4;
        double p = L.ckp[g];
        for (uint32_t j = 16 * g; j < z; ++j) p += cnorm(lbuf[j]);
        return p;
    };
    const uint32_t D = A.D, per = (D + blockDim.x - 1) / blockDim.x;
    const uint32_t xb = threadIdx.x * per, xe = min(xb + per, D);
    const uint32_t Lw = P * A.n_uw;  // correlation window (products)
    // metric(x), x = r0 + i: corr over products y in [x - Lw + 1, x]; product index of y = (y - yb) - P
    if (xb < xe) {
        const uint32_t pi_end = yoff + xb - P + 1;  // product index just past y = x
        double cr = 0.0, ci = 0.0;
        for (uint32_t k = 0; k <= A.n_uw; ++k) {
            const float ck = (k > 0 ? A.uw[k - 1] : 0.f) - (k < A.n_uw ? A.uw[k] : 0.f);
            if (ck == 0.f) continue;
            double rx, ry;
            PC(pi_end - Lw + P * k, rx, ry);
            cr += ck * rx;
            ci += ck * ry;
        }
        double pw = PP(yoff + xb + 1) - PP(yoff + xb + 1 - A.stf_len);
        for (uint32_t i = xb; i < xe; ++i) {
            if (i > xb) {  // slide by one sample: every prefix point advances by one product / sample
                const uint32_t pe = yoff + i - P;  // product index entering (y = x)
                for (uint32_t k = 0; k <= A.n_uw; ++k) {
                    const float ck = (k > 0 ? A.uw[k - 1] : 0.f) - (k < A.n_uw ? A.uw[k] : 0.f);
                    if (ck == 0.f) continue;
                    const float2 v = cmulc(lbuf[pe - Lw + P * k], lbuf[pe - Lw + P * k + P]);
                    cr += ck * static_cast<double>(v.x);
                    ci += ck * static_cast<double>(v.y);
                }
                pw += static_cast<double>(cnorm(lbuf[yoff + i])) - static_cast<double>(cnorm(lbuf[yoff + i - A.stf_len]));
            }
            // (prefactor |c| / pw)^2 without the square root (equal to double rounding, stored as float)
            const double pf = static_cast<double>(A.prefactor);
            L.met[i] = static_cast<float>(pf * pf * (cr * cr + ci * ci) / (pw * pw));
        }
    }
    __syncthreads();
    SYNC_STAMP(14);
    // smoother (length 2 bos + 1, zero history) and last-maximum argmax
    const uint32_t ns = (prm::SYNC_PEAK_SMOOTH_LEFT + prm::SYNC_PEAK_SMOOTH_RIGHT) * A.bos + 1;
    double best = -1.0;
    uint32_t bidx = 0;
    if (xb < xe) {
        double sm = 0.0;
        for (uint32_t j = 0; j < ns; ++j)
            if (xb >= j) sm += L.met[xb - j];
        for (uint32_t i = xb; i < xe; ++i) {
            if (i > xb) {
                sm += L.met[i];
                if (i >= ns) sm -= L.met[i - ns];
            }
            const double mean = sm / static_cast<double>(ns);
            if (mean >= best) {
                best = mean;
                bidx = i;
            }
        }
    }
    // block argmax: largest value, latest index among equal values
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const uint32_t oi = __shfl_xor(bidx, o);
        if (ob > best || (ob == best && oi > bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    __syncthreads();
    if (lane == 0) {
        red[2 * wv] = best;
        reinterpret_cast<uint32_t*>(red + 16)[wv] = bidx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t v = 1; v < (blockDim.x >> 6); ++v) {
            const double ob = red[2 * v];
            const uint32_t oi = reinterpret_cast<uint32_t*>(red + 16)[v];
            if (ob > best || (ob == best && oi > bidx)) {
                best = ob;
                bidx = oi;
            }
        }
        pk_metric = static_cast<float>(best);
        pk_idx = r0 + bidx - prm::SYNC_PEAK_SMOOTH_RIGHT * A.bos;  // metric_smoother_bos_offset_to_center_samples
    }
    __syncthreads();
}

// The detection / coarse-peak state machine of one window. Two forms of the same loop:
//  SPLIT = false  (sync_detect_kernel): the whole loop in the workgroup, the per-antenna coarse-peak
//                 search inline (resampled STF region in LDS, 3 workgroups per CU);
//  SPLIT = true   (the split rounds): the workgroup runs the detection conditions only and leaves at
//                 the first detection with its state saved (pend = 1); sync_peak_kernel then runs the
//                 coarse-peak search of that detection with one workgroup per (window, antenna), and
//                 the next split launch resumes from the saved state with the peak results. Small
//                 LDS (detection staging only), so many workgroups per CU; the inline form finishes
//                 whatever the split rounds left (several detections or false alarms in one window).
// The split form's coarse-peak search (sync_peak_kernel) evaluates the same metric expression with its
// double sums grouped differently (prefixes on an 8-sample grid): the coarse peaks of the two forms
// agree to double rounding; both are held to the oracle by the same GPU tests (DNRP_SYNC_ROUNDS).
template <int LR, int MR, int HLR, bool SPLIT>
__global__ void __launch_bounds__(SYNC_THREADS) SYNC_DETECT_ATTR sync_detect_kernel(sync_args A) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    sync_shared& sh = *reinterpret_cast<sync_shared*>(smem);
    double* red = sh.red;
    int& s_min = sh.s_min;
    float& s_rms = sh.s_rms;
    float& s_metric = sh.s_metric;
    uint32_t& s_ant = sh.s_ant;
    float* s_pk_metric = sh.s_pk_metric;
    uint32_t* s_pk_idx = sh.s_pk_idx;
    const uint32_t w = blockIdx.x;
    float* taps = reinterpret_cast<float*>(smem + SYNC_SHARED_F2);
    const uint32_t tap_f2 = SPLIT ? 0u : sync_tap_f2(A.npp);
    const uint32_t region = A.stf_len + A.D + SYNC_PAD_PEAK;
    float2* lbuf = smem + SYNC_SHARED_F2 + tap_f2;
    float2* stage = SPLIT ? lbuf : lbuf + (region + 1) / 2 * 2;
    peak_lds pl;  // aliases the staging area (dead once the resampler has run)
    pl.ckc = reinterpret_cast<double2*>(stage);
    pl.ckp = reinterpret_cast<double*>(pl.ckc + sync_peak_n16(region));
    pl.met = reinterpret_cast<float*>(pl.ckp + sync_peak_n16(region));
    // loop registers: the initial state, or the state a split launch saved
    sync_state S0{4u, A.stf_len + A.pattern, 0u, 0u, 0u, 0u, 0.f, 0.f, 0u};
    if (!A.first) S0 = A.state[w];
    if (S0.pend == 2) return;  // uniform: finished in an earlier launch
    if (!SPLIT && LR > 1) stage_copy<4>(taps, A.taps_pp, A.npp, threadIdx.x, blockDim.x);
    __syncthreads();
    const float* Pw = A.P + static_cast<size_t>(w) * A.n_ant * A.n_steps;
    const float2* Cw = A.Cs + static_cast<size_t>(w) * A.n_ant * A.n_steps;
    sync_res* out = A.res + static_cast<size_t>(w) * A.max_reports;
    // detection staging (aliases the resampler stage, dead during detection): per antenna det_p
    // powers and det_c correlations
    const uint32_t np = 4 * A.n_pattern, nc = 4 * A.n_uw;
    const sync_det_lds dl = sync_det_layout(np, nc);
    const uint32_t det_p = dl.det_p, det_c = dl.det_c;
    float2* dc = stage;
    float* dp = reinterpret_cast<float*>(dc + A.n_ant * det_c);
    uint32_t nrep = S0.nrep, s_cur = S0.s_cur, ignore = S0.ignore, ndet = S0.ndet;
    bool resume = S0.pend == 1;  // a saved detection whose coarse peaks sync_peak_kernel has searched
    SYNC_STAMP(0);
    while (nrep < A.max_reports) {
        int sd;
        if (resume) {
            sd = static_cast<int>(S0.sd);
            if (threadIdx.x == 0) {
                s_ant = S0.s_ant;
                s_rms = S0.s_rms;
                s_metric = S0.s_metric;
            }
            if (threadIdx.x < A.n_ant) {
                const float2 r = A.pk[size_t(w) * 8 + threadIdx.x];
                s_pk_metric[threadIdx.x] = r.x;
                s_pk_idx[threadIdx.x] = __float_as_uint(r.y);
            }
            __syncthreads();
        } else {
            // ---------------- detection: first step at or after s_cur meeting the conditions
            if (threadIdx.x == 0) s_min = 0x7FFFFFFF;
            __syncthreads();
            // only steps below the frontier s_lim = A.s_hi exist (the step sums computed so far in this
            // call); the staging below never reads past it: what lies there is stale from earlier calls
            const uint32_t s_lim = A.s_hi;
            for (uint32_t base = s_cur; base < s_lim; base += blockDim.x) {
                // the batch's step values of every antenna in LDS (one coalesced round trip); steps a
                // detection can evaluate have s - (np - 1) >= 0 (ignore >= stf_len + pattern)
                const uint32_t nb = min(blockDim.x, s_lim - base);
                const uint32_t lo_p = base >= np - 1 ? base - (np - 1) : 0u, lo_c = base >= nc - 1 ? base - (nc - 1) : 0u;
                const uint32_t len_p = base + nb - lo_p, len_c = base + nb - lo_c;
                for (uint32_t a = 0; a < A.n_ant; ++a) {
                    for (uint32_t i = threadIdx.x; i < len_p; i += blockDim.x) dp[a * det_p + i] = Pw[a * A.n_steps + lo_p + i];
                    for (uint32_t i = threadIdx.x; i < len_c; i += blockDim.x) dc[a * det_c + i] = Cw[a * A.n_steps + lo_c + i];
                }
                __syncthreads();
                const uint32_t s = base + threadIdx.x;
                if (s < s_lim && (s + 1) * A.step >= ignore) {
                    for (uint32_t a = 0; a < A.n_ant; ++a) {
                        det_eval e;
                        if (detect_eval(A, dp + a * det_p - lo_p, dc + a * det_c - lo_c, s, e)) {
                            atomicMin(&s_min, static_cast<int>(s));
                            break;
                        }
                    }
                }
                __syncthreads();
                const int found = s_min;
                __syncthreads();
                if (found != 0x7FFFFFFF) break;
            }
            sd = s_min;
            __syncthreads();
            if (sd == 0x7FFFFFFF) {
                if (s_lim < A.n_steps) {
                    // the scan reached the frontier with reports still to find: the window is not
                    // finished. The loop registers wait for the next tranche (every step below s_lim
                    // is evaluated or ignored; the reports found so far stay in res)
                    if (threadIdx.x == 0) A.state[w] = sync_state{max(s_cur, s_lim), ignore, nrep, 0u, 0u, 0u, 0.f, 0.f, ndet};
                    return;
                }
                break;
            }
            if (threadIdx.x == 0) {
                for (uint32_t a = 0; a < A.n_ant; ++a) {
                    det_eval e;
                    if (detect_eval(A, Pw + a * A.n_steps, Cw + a * A.n_steps, static_cast<uint32_t>(sd), e)) {
                        s_ant = a;
                        s_rms = e.rms;
                        s_metric = e.metric;
                        break;
                    }
                }
            }
            __syncthreads();
            if constexpr (SPLIT) {  // leave with the detection pending: sync_peak_kernel searches its peaks
                // a window's first A.rounds detections only, as with one tranche (one per split round):
                // a later one is left where it is for the inline form, which finds it again from s_cur
                if (threadIdx.x == 0)
                    A.state[w] = ndet < A.rounds ? sync_state{s_cur, ignore, nrep, 1u, static_cast<uint32_t>(sd), s_ant, s_rms, s_metric, ndet + 1}
                                                 : sync_state{s_cur, ignore, nrep, 0u, 0u, 0u, 0.f, 0.f, ndet};
                return;
            }
            ++ndet;
        }
        SYNC_STAMP(1);
        s_cur = static_cast<uint32_t>(sd) + 1;
        const uint32_t det_time = s_cur * A.step, r0 = det_time - prm::SYNC_JUMP_BACK_PATTERNS * A.pattern;
        const float det_metric = s_metric;
        if (!SPLIT && !resume) {
            // ---------------- coarse peak search over one STF on every antenna
            const int64_t yb = static_cast<int64_t>(r0) - A.stf_len - SYNC_PAD_PEAK;
            for (uint32_t a = 0; a < A.n_ant; ++a) {
                const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
                sync_resample<LR, MR, HLR>(A, x, yb, region, stage, lbuf, taps, A.det_stage);
                SYNC_STAMP(2 + 2 * min(a, 3u));
                peak_search(A, lbuf, region, pl, r0, red, s_pk_metric[a], s_pk_idx[a]);
                SYNC_STAMP(3 + 2 * min(a, 3u));
            }
        }
        resume = false;
        // post_processing_validity (autocorrelator_peak.cpp:311-364), float as in the reference
        float cm[8];
        float wsum = 0.f, msum = 0.f;
        uint32_t nvalid = 0;
        for (uint32_t a = 0; a < A.n_ant; ++a) {
            cm[a] = 0.f;
            const float m = s_pk_metric[a];
            if (det_metric + prm::SYNC_PEAK_ABOVE_DETECTION >= m) continue;
            if (static_cast<int64_t>(det_time) +
                    static_cast<int64_t>(prm::SYNC_PEAK_DETECTION2PEAK_STFS * static_cast<double>(A.stf_len)) >=
                static_cast<int64_t>(s_pk_idx[a]))
                continue;
            cm[a] = m;
            wsum += m * static_cast<float>(s_pk_idx[a]);
            ++nvalid;
        }
        for (uint32_t a = 0; a < A.n_ant; ++a) msum += cm[a];
        __syncthreads();  // every thread has read the peak results before the next detection overwrites them
        if (nvalid == 0) continue;  // false alarm: detection resumes after this step
        const uint32_t wpk = static_cast<uint32_t>(roundf(wsum / msum));
        if (wpk < A.stf_len - 1) continue;  // STF would start before the chunk (asserted in the reference)
        const uint32_t cpl = wpk - (A.stf_len - 1);
        // post_processing_at_coarse_peak (:366-394, RMS and fractional CFO over the STF at the peak)
        // runs per (report, antenna) in sync_post_kernel, the CFO's antenna sum in sync_fine_kernel:
        // nothing in the detection loop depends on them
        SYNC_STAMP(10);
        if (threadIdx.x == 0) {
            sync_res r{};
            r.found = 1;
            r.det_ant = s_ant;
            r.det_rms = s_rms;
            r.det_metric = det_metric;
            r.det_time = det_time;
            r.det_time_jb = r0;
            r.coarse_local = cpl;
            double g = static_cast<double>(cpl);  // rx_pacer.cpp:306-313
            g *= static_cast<double>(A.M);
            g /= static_cast<double>(A.L);
            r.coarse_64 = static_cast<int64_t>(static_cast<uint32_t>(round(g)));
            for (uint32_t a = 0; a < 8; ++a) {
                r.coarse_metric[a] = a < A.n_ant ? cm[a] : 0.f;
                r.rms[a] = 0.f;  // sync_post_kernel
            }
            r.cfo_frac = 0.f;  // sync_fine_kernel (antenna sum of sync_post_kernel's terms)
            r.cfo_int = 0.f;  // coarse_peak_f_domain.cpp:195-199
            r.u = A.u;
            r.b = A.b;  // coarse_peak_f_domain.cpp:75-120: b of the radio device class
            out[nrep] = r;
        }
        ignore = cpl + static_cast<uint32_t>(prm::SYNC_SKIP_AFTER_PEAK_STFS * static_cast<double>(A.stf_len));  // skip_after_peak
        ++nrep;
        __syncthreads();
    }
    SYNC_STAMP(11);
    if (threadIdx.x == 0) {
        A.n_found[w] = nrep;
        for (uint32_t k = nrep; k < A.max_reports; ++k) out[k].found = 0;
        if (A.state) A.state[w].pend = 2u;
    }
}

// ---- coarse-peak search of the split rounds (sync_peak_kernel)
// autocorrelator_peak.cpp:145-264 for the pending detection of one (window, antenna), one workgroup
// each. The per-sample metric is the same expression as peak_search's (exact prefix differences in
// double, sliding by one sample), laid out for parallel latency:
//  - the STF region is resampled straight from the window (pp_direct: each thread one polyphase block
//    of L outputs from its W inputs by range-checked buffer loads; no staging round trips);
//  - thread v owns the 8 positions [8v, 8v + 8): every prefix its first position needs sits on the
//    grid z = 8g + 1 (P, the window Lw = P n_uw and stf_len are multiples of 16), so its initial sums
//    are single LDS reads of the inclusive prefixes Q (products) and R (powers) at grid points;
//  - the region buffer is padded by one slot per 32 samples (pidx) and the metric row by one per 8
//    (midx), so the stride-8 accesses of a wave hit distinct banks;
//  - the smoother's initial window sums whole 8-position blocks (blk) instead of 2 bos + 1 samples.
// Double sums in a different order than peak_search: the metric and the smoothed maxima agree to
// double rounding, the argmax to the same tie rules.
__device__ __forceinline__ uint32_t pidx(uint32_t j) { return j + (j >> 5); }
__device__ __forceinline__ uint32_t midx(uint32_t i) { return i + (i >> 3); }

__host__ __device__ inline uint32_t peak8_lbuf(uint32_t region) { return (region + region / 32 + 2) / 2 * 2; }
__host__ __device__ inline uint32_t peak8_nq(uint32_t region, uint32_t P) { return (region - P) / 8 + 2; }
__host__ __device__ inline uint32_t peak8_nr(uint32_t region) { return region / 8 + 2; }
__host__ __device__ inline size_t peak8_alias(uint32_t region, uint32_t P, uint32_t D) {
    const size_t qr = size_t(peak8_nq(region, P)) * 16 + size_t(peak8_nr(region)) * 8;
    const size_t mb = (size_t(D) + D / 8 + 2) / 2 * 2 * 4 + size_t(D / 8) * 8;
    return qr > mb ? qr : mb;
}

// CT: the 9/10 sync resampler's taps compiled in (pp_const<taps_sync_9_10>, host-checked bit for
// bit): immediates next to their FMAs instead of 225 run-time taps held in SGPRs (which spill)
template <int LR, int MR, int HLR, bool CT, int NUW>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(DNRP_PEAK_WPE))) sync_peak_kernel(sync_args A) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    sync_shared& sh = *reinterpret_cast<sync_shared*>(smem);
    double* red = sh.red;
    const uint32_t w = blockIdx.x / A.n_ant, a = blockIdx.x % A.n_ant;
    const sync_state S0 = A.state[w];
    if (S0.pend != 1) return;  // uniform: no detection pending in this window
#ifdef DNRP_SYNC_PROFILE
#define PEAK_STAMP(i) \
    if (threadIdx.x == 0 && a == 0 && A.prof) A.prof[size_t(w) * 32 + 16 + (i)] = wall_clock64()
#else
#define PEAK_STAMP(i)
#endif
    PEAK_STAMP(0);
    const uint32_t P = A.pattern, D = A.D, yoff = A.stf_len + SYNC_PAD_PEAK;
    const uint32_t region = A.stf_len + D + SYNC_PAD_PEAK, nprod = region - P;
    float2* lbuf = smem + SYNC_SHARED_F2;
    double2* Q = reinterpret_cast<double2*>(lbuf + peak8_lbuf(region));
    double* R = reinterpret_cast<double*>(Q + peak8_nq(region, P));
    float* met = reinterpret_cast<float*>(Q);  // after the metric pass (Q, R dead)
    double* blk = reinterpret_cast<double*>(met + (D + D / 8 + 2) / 2 * 2);
    const uint32_t tid = threadIdx.x, T = blockDim.x;
    const uint32_t det_time = (S0.sd + 1) * A.step, r0 = det_time - prm::SYNC_JUMP_BACK_PATTERNS * A.pattern;
    const int64_t yb = static_cast<int64_t>(r0) - A.stf_len - SYNC_PAD_PEAK;
    const float2* x = A.iq + w * A.win_stride + a * A.ant_stride;
    // ---- resampled region lb[yb + i] -> lbuf[pidx(i)] (sync_resample's outputs, bit for bit)
    if constexpr (CT && LR == 9 && DNRP_PEAK_STAGED)
        resample_staged<LR, MR, HLR, DNRP_PEAK_IMAJ>(A, x, yb, region, lbuf, [&](uint32_t i, float2 v) { lbuf[pidx(i)] = v; });
    else
        resample_direct<LR, MR, HLR, CT>(A, x, yb, region, [&](uint32_t i, float2 v) { lbuf[pidx(i)] = v; });
    __syncthreads();
    PEAK_STAMP(1);
    // ---- 8-sample segment sums: products prod[j] = lb[j] conj(lb[j + P]), powers |lb[j]|^2; segment
    // g >= 1 holds j in [8g - 7, 8g], segment 0 j = 0, so the inclusive scan at g is the prefix < 8g + 1
    const uint32_t nq = peak8_nq(region, P) - 1, nr = peak8_nr(region) - 1;
    // all 8 loads of a segment issued together (out-of-range terms read a valid slot and are masked)
    for (uint32_t h = tid; h < nq; h += T) {
        const uint32_t j0 = h == 0 ? 0u : 8 * h - 7, cnt = h == 0 ? 1u : 8u;
        float2 c[8];
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) {
            const uint32_t j = min(j0 + t, nprod - 1);
            c[t] = cmulc(lbuf[pidx(j)], lbuf[pidx(j + P)]);
        }
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t)
            if (t < cnt && j0 + t < nprod) {
                sx += c[t].x;
                sy += c[t].y;
            }
        Q[h] = make_double2(sx, sy);
    }
    for (uint32_t h = tid; h < nr; h += T) {
        const uint32_t j0 = h == 0 ? 0u : 8 * h - 7, cnt = h == 0 ? 1u : 8u;
        float p[8];
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) p[t] = cnorm(lbuf[pidx(min(j0 + t, region - 1))]);
        double sp = 0.0;
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t)
            if (t < cnt && j0 + t < region) sp += p[t];
        R[h] = sp;
    }
    __syncthreads();
    PEAK_STAMP(2);
    const uint32_t wv = tid >> 6, lane = tid & 63u;
    if (wv == 0) wave_scan_d2(Q, nq, lane);  // exclusive: Q[g + 1] = prefix < 8g + 1
    if (wv == 1) {
        const uint32_t per = (nr + 63) / 64;
        const uint32_t b = lane * per, e = min(b + per, nr);
        double sp = 0.0;
        for (uint32_t i = b; i < e; ++i) sp += R[i];
        double inc = sp;
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_up(inc, o);
            if (static_cast<int>(lane) >= o) inc += t;
        }
        double rr = inc - sp;
        for (uint32_t i = b; i < e; ++i) {
            const double t = R[i];
            R[i] = rr;
            rr += t;
        }
        if (lane == 63) R[nr] = inc;
    }
    __syncthreads();
    PEAK_STAMP(3);
    // ---- metric of the thread's 8 positions (registers)
    const uint32_t Lw = P * A.n_uw, nv = D / 8;
    const double pf = static_cast<double>(A.prefactor);
    float m8[8];
    if (tid < nv) {
        // cover weights ck of the NUW + 1 prefix points (uniform); a zero weight adds an exact zero
        float ck[NUW + 1];
#pragma unroll
        for (int k = 0; k <= NUW; ++k) ck[k] = (k > 0 ? A.uw[k - 1] : 0.f) - (k < NUW ? A.uw[k] : 0.f);
        const uint32_t xb = 8 * tid;
        const uint32_t zb = yoff + xb - P + 1 - Lw;  // = 8g + 1
        double cr = 0.0, ci = 0.0;
        double2 q[NUW + 1];
#pragma unroll
        for (int k = 0; k <= NUW; ++k) q[k] = Q[(zb + P * k - 1) / 8 + 1];
#pragma unroll
        for (int k = 0; k <= NUW; ++k) {
            cr += ck[k] * q[k].x;
            ci += ck[k] * q[k].y;
        }
        double pw = R[(yoff + xb) / 8 + 1] - R[(yoff + xb - A.stf_len) / 8 + 1];
        m8[0] = static_cast<float>(pf * pf * (cr * cr + ci * ci) / (pw * pw));
#pragma unroll
        for (uint32_t ii = 1; ii < 8; ++ii) {
            const uint32_t i = xb + ii;
            const uint32_t pe = yoff + i - P - Lw;  // product index entering (y = x) for k = 0
            float2 u[NUW + 2];
#pragma unroll
            for (int k = 0; k <= NUW + 1; ++k) u[k] = lbuf[pidx(pe + P * k)];
            const float2 s1 = lbuf[pidx(yoff + i)], s0 = lbuf[pidx(yoff + i - A.stf_len)];
#pragma unroll
            for (int k = 0; k <= NUW; ++k) {
                const float2 v = cmulc(u[k], u[k + 1]);
                cr += ck[k] * static_cast<double>(v.x);
                ci += ck[k] * static_cast<double>(v.y);
            }
            pw += static_cast<double>(cnorm(s1)) - static_cast<double>(cnorm(s0));
            m8[ii] = static_cast<float>(pf * pf * (cr * cr + ci * ci) / (pw * pw));
            if (ii & 1) asm volatile("" ::: "memory");  // two slides' loads in flight, not seven (VGPRs)
        }
    }
    __syncthreads();  // Q, R read by every thread: the metric row may overwrite them
    PEAK_STAMP(4);
    if (tid < nv) {
        double bs = 0.0;
#pragma unroll
        for (uint32_t ii = 0; ii < 8; ++ii) {
            met[midx(8 * tid + ii)] = m8[ii];
            bs += m8[ii];
        }
        blk[tid] = bs;
    }
    __syncthreads();
    PEAK_STAMP(5);
    // ---- smoother (length ns = 2 bos + 1, zero history) and last-maximum argmax
    const uint32_t ns = (prm::SYNC_PEAK_SMOOTH_LEFT + prm::SYNC_PEAK_SMOOTH_RIGHT) * A.bos + 1;
    double best = -1.0;
    uint32_t bidx = 0;
    if (tid < nv) {
        const uint32_t xb = 8 * tid, F = (ns - 1) / 8;
        double sm = m8[0];
        for (uint32_t u = 1; u <= F && u <= tid; ++u) sm += blk[tid - u];
        for (uint32_t j = 8 * F + 1; j < ns && j <= xb; ++j) sm += met[midx(xb - j)];
#pragma unroll
        for (uint32_t ii = 0; ii < 8; ++ii) {
            const uint32_t i = xb + ii;
            if (ii > 0) {
                sm += m8[ii];
                if (i >= ns) sm -= met[midx(i - ns)];
            }
            const double mean = sm / static_cast<double>(ns);
            if (mean >= best) {
                best = mean;
                bidx = i;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const uint32_t oi = __shfl_xor(bidx, o);
        if (ob > best || (ob == best && oi > bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    if (lane == 0) {
        red[wv] = best;  // up to 16 waves: best in red[0, 16), indices in red[16, 24)
        reinterpret_cast<uint32_t*>(red + 16)[wv] = bidx;
    }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t v = 1; v < (T >> 6); ++v) {
            const double ob = red[v];
            const uint32_t oi = reinterpret_cast<uint32_t*>(red + 16)[v];
            if (ob > best || (ob == best && oi > bidx)) {
                best = ob;
                bidx = oi;
            }
        }
        const uint32_t pk_idx = r0 + bidx - prm::SYNC_PEAK_SMOOTH_RIGHT * A.bos;  // metric_smoother_bos_offset_to_center_samples
        A.pk[size_t(w) * 8 + a] = make_float2(static_cast<float>(best), __uint_as_float(pk_idx));
    }
    PEAK_STAMP(6);
}

// ===================================================================== launchers
// bytes that alias sync_detect's stage area: the peak-search arrays and the detection staging
static size_t sync_detect_alias(const sync_args& a) {
    const uint32_t region = a.stf_len + a.D + SYNC_PAD_PEAK;
    const size_t alias = sync_peak_n16(region) * (sizeof(double2) + sizeof(double)) + a.D * sizeof(float);
    return std::max(alias, sync_det_layout(4 * a.n_pattern, 4 * a.n_uw).bytes(a.n_ant));
}

// float2 slots of sync_detect's stage area: what aliases it, and the resampler runs in pieces whose
// input span fits it (at least 64 blocks per piece)
uint32_t sync_detect_stage(const sync_args& a) {
    const uint32_t region = a.stf_len + a.D + SYNC_PAD_PEAK;
    const size_t full = sync_stage_cap(a.L, a.M, a.hl, region);
    const size_t piece = a.L > 1 ? a.hl + 1 + ((a.L - 1) * a.M) / a.L + 64 * a.M : 0;
    const size_t need = std::max((sync_detect_alias(a) + sizeof(float2) - 1) / sizeof(float2), piece);
    return static_cast<uint32_t>((std::min(full, need) + 1) / 2 * 2);
}

size_t sync_detect_lds(const sync_args& a) {
    const uint32_t region = a.stf_len + a.D + SYNC_PAD_PEAK;
    const size_t lb = (region + 1) / 2 * 2 * sizeof(float2);
    const size_t stage = size_t(sync_detect_stage(a)) * sizeof(float2);
    return (SYNC_SHARED_F2 + sync_tap_f2(a.npp)) * sizeof(float2) + lb + std::max(stage, sync_detect_alias(a));
}

// the inline form (split = false), or a split round: detection conditions only (LDS: the block scalars
// and the detection staging)
static hipError_t launch_detect(const sync_args& a, uint32_t n, hipStream_t st, bool split) {
    const size_t lds = split ? SYNC_SHARED_F2 * sizeof(float2) + sync_det_layout(4 * a.n_pattern, 4 * a.n_uw).bytes(a.n_ant) : sync_detect_lds(a);
    sync_dispatch<false>(a, [&](auto l, auto m, auto h, auto) {
        constexpr int LR = decltype(l)::value, MR = decltype(m)::value, HLR = decltype(h)::value;
        if (split)
            hipLaunchKernelGGL((sync_detect_kernel<LR, MR, HLR, true>), dim3(n), dim3(SYNC_THREADS), lds, st, a);
        else
            hipLaunchKernelGGL((sync_detect_kernel<LR, MR, HLR, false>), dim3(n), dim3(SYNC_THREADS), lds, st, a);
    });
    return hipGetLastError();
}
hipError_t launch_sync_detect(const sync_args& a, uint32_t n, hipStream_t st) { return launch_detect(a, n, st, false); }
hipError_t launch_sync_detect_split(const sync_args& a, uint32_t n, hipStream_t st) { return launch_detect(a, n, st, true); }

// split round: coarse-peak search of the pending detections, one workgroup per (window, antenna)
// one thread per 8 metric positions and, up to 512 threads, one per polyphase block of the region
// (the resampling is one load round trip per block: thread-count sweep on MI355X, C4 per 4096
// windows: 320 threads 0.98 ms, 384 0.93, 512 0.85, 576 1.20)
uint32_t sync_peak_threads(const sync_args& a) {
    const uint32_t region = a.stf_len + a.D + SYNC_PAD_PEAK, nblk = a.L > 1 ? region / a.L + 2 : 0u;
    return std::max({128u, (a.D / 8 + 63) / 64 * 64, std::min(512u, (nblk + 63) / 64 * 64)});
}

size_t sync_peak_lds(const sync_args& a) {
    const uint32_t region = a.stf_len + a.D + SYNC_PAD_PEAK;
    return SYNC_SHARED_F2 * sizeof(float2) + size_t(peak8_lbuf(region)) * sizeof(float2) + peak8_alias(region, a.pattern, a.D);
}

bool sync_peak_ok(const sync_args& a) {  // the grid layout's preconditions (every DECT geometry meets them)
    const uint32_t region = a.stf_len + a.D + SYNC_PAD_PEAK;
    // resample_staged (9/10): at most 2 blocks per thread, the span inside lbuf + the alias area
    const uint32_t nb = region / 9 + 2, n_in = sync_staged_n_in<9, 10, 24>(nb + 1);
    const bool staged_ok = sync_class_of(a) != SYNC_CLASS_9_10_24 ||
                           (nb <= 2 * 512 && size_t(n_in) * sizeof(float2) <= sync_peak_lds(a) - SYNC_SHARED_F2 * sizeof(float2));
    return a.D % 8 == 0 && a.pattern % 8 == 0 && (a.stf_len + SYNC_PAD_PEAK) % 8 == 0 && a.D / 8 <= 512 &&
           (a.n_uw == 6 || a.n_uw == 8) && sync_peak_lds(a) <= LDS_BYTES && staged_ok;
}

hipError_t launch_sync_peak(const sync_args& a, uint32_t n, hipStream_t st) {
    const dim3 g(n * a.n_ant), b(sync_peak_threads(a));
    const size_t lds = sync_peak_lds(a);
    sync_dispatch<true>(a, [&](auto l, auto m, auto h, auto ct) {
        constexpr int LR = decltype(l)::value, MR = decltype(m)::value, HLR = decltype(h)::value;
        constexpr bool CT = decltype(ct)::value;
        if (a.n_uw == 6)  // n_pattern 7 (u = 1)
            hipLaunchKernelGGL((sync_peak_kernel<LR, MR, HLR, CT, 6>), g, b, lds, st, a);
        else  // n_pattern 9
            hipLaunchKernelGGL((sync_peak_kernel<LR, MR, HLR, CT, 8>), g, b, lds, st, a);
    });
    return hipGetLastError();
}

}  // namespace dnrp::dev
