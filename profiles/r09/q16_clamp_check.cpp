// Host model of q16_pair's int16 conversion (csrc/kernels/rx_eq.hpp) over all 2^32 float bit patterns:
// does the explicit clamp between the rounding and the two saturating conversions change any result?
//   with clamp:  rint -> min(32767, max(-32768, .)) -> v_cvt_i32_f32 -> v_cvt_pk_i16_i32
//   without:     rint ->                               v_cvt_i32_f32 -> v_cvt_pk_i16_i32
//   max only:    rint ->             max(-32768, .) -> v_cvt_i32_f32 -> v_cvt_pk_i16_i32
// v_cvt_i32_f32 truncates, saturates at INT32_MIN / INT32_MAX and maps NaN to 0; v_cvt_pk_i16_i32
// saturates to [-32768, 32767]; fmaxf / fminf return the operand that is not NaN (v_max_f32 / v_min_f32
// in IEEE mode, and v_med3_f32 as the compiler emits it for this pair).
// Build and run: g++ -O2 -fopenmp q16_clamp_check.cpp -o q16_clamp_check && ./q16_clamp_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static int32_t cvt_i32_f32(float x) {
    if (std::isnan(x)) return 0;
    if (x >= 2147483648.f) return INT32_MAX;
    if (x <= -2147483648.f) return INT32_MIN;
    return static_cast<int32_t>(x);
}
static int16_t cvt_pk_i16_i32(int32_t v) { return static_cast<int16_t>(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

int main() {
    uint64_t diff_plain = 0, diff_plain_nan = 0, diff_max = 0;
#pragma omp parallel for reduction(+ : diff_plain, diff_plain_nan, diff_max) schedule(static)
    for (int64_t i = 0; i < (int64_t(1) << 32); ++i) {
        const uint32_t u = static_cast<uint32_t>(i);
        float x;
        std::memcpy(&x, &u, 4);
        const float r = std::nearbyintf(x);  // round to nearest even (v_rndne_f32)
        const int16_t with = cvt_pk_i16_i32(cvt_i32_f32(std::fmin(32767.f, std::fmax(-32768.f, r))));
        const int16_t plain = cvt_pk_i16_i32(cvt_i32_f32(r));
        const int16_t mx = cvt_pk_i16_i32(cvt_i32_f32(std::fmax(-32768.f, r)));
        if (with != plain) {
            ++diff_plain;
            if (std::isnan(x)) ++diff_plain_nan;
        }
        if (with != mx) ++diff_max;
    }
    std::printf("patterns 4294967296\nwithout clamp: %llu differ, %llu of them NaN inputs\nmax only: %llu differ\n",
                (unsigned long long)diff_plain, (unsigned long long)diff_plain_nan, (unsigned long long)diff_max);
    return 0;
}
