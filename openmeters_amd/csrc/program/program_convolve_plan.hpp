// The host-only half of the programme bank's convolve stage (include/omx/program_convolve.h): plan, streaming formula, check, design
// and response.  Plain C++ doubles, no device and no HIP: program_convolve.cpp wraps these for the C ABI,
// tools/convolve_design_check.cpp drives them under the sanitizers.  Every function returns an OMX_* code and, refusing, the reason in
// *why; a refusal writes nothing.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/omx/program_convolve.h"
#include "../../../include/omx/program_resample.h"  // OMX_RESAMPLE_I0_TERMS: the design shares the resampler's I0 series
#include "program_carried.hpp"

namespace omx {

constexpr uint32_t kCvThreads = 256;          // threads per workgroup of the main kernel: four wavefronts
constexpr uint32_t kCvFramesPerThread = 8;    // R: consecutive output frames of one channel a thread keeps in registers
constexpr uint32_t kCvTapBlock = 256;         // KB: taps per staging of the input span; a multiple of R
constexpr double kCvPi = 3.14159265358979323846;

// Threads per channel (each takes R frames): a multiple of 64, so that every wavefront works on one channel and its taps are uniform.
// One and two channels take more frames per tile so that all four wavefronts have work.
constexpr uint32_t cv_groups(uint32_t channels) { return channels == 1 ? 256u : (channels == 2 ? 128u : 64u); }
constexpr uint32_t cv_tile(uint32_t channels) { return cv_groups(channels) * kCvFramesPerThread; }

inline int cv_fail(const char** why, const char* text) {
    if (why) *why = text;
    return OMX_ERR_INVALID;
}

inline int cv_plan(uint32_t channels, uint32_t max_taps, omx_program_convolve_info* info, const char** why) {
    if (!info) return cv_fail(why, "null info");
    if (channels < 1 || channels > OMX_MAX_CHANNELS) return cv_fail(why, "channels outside 1 .. 8");
    if (max_taps < 1 || max_taps > OMX_CONVOLVE_MAX_TAPS) return cv_fail(why, "max_taps 0 or above OMX_CONVOLVE_MAX_TAPS");
    *info = omx_program_convolve_info{cv_tile(channels), kCvFramesPerThread, kCvTapBlock, channels};
    return OMX_NONE;
}

inline int cv_frames(uint32_t delay, uint64_t n_before, uint64_t e_before, uint64_t frames, uint32_t flush, uint64_t* frames_out,
                     const char** why) {
    if (!frames_out) return cv_fail(why, "null frames_out");
    if (delay > OMX_CONVOLVE_MAX_TAPS - 1) return cv_fail(why, "delay above OMX_CONVOLVE_MAX_TAPS - 1");
    if (n_before > (1ull << 63) || frames > (1ull << 63) - n_before) return cv_fail(why, "frames_in_before + frames beyond 2^63");
    if (e_before > n_before) return cv_fail(why, "frames_out_before above frames_in_before");
    *frames_out = carry_emitted(delay, n_before + frames, e_before, flush != 0) - e_before;
    return OMX_NONE;
}

inline int cv_check(const omx_program_fir* fir, const char** why) {
    if (!fir) return cv_fail(why, "null fir");
    if (!fir->taps) return cv_fail(why, "null taps");
    if (fir->n_taps < 1 || fir->n_taps > OMX_CONVOLVE_MAX_TAPS) return cv_fail(why, "n_taps 0 or above OMX_CONVOLVE_MAX_TAPS");
    if (fir->flags != 0) return cv_fail(why, "a flag set");
    for (uint32_t k = 0; k < fir->n_taps; ++k)
        if (!std::isfinite(fir->taps[k])) return cv_fail(why, "a tap that is not finite");
    return OMX_NONE;
}

inline double cv_i0(double v) {  // the resampler's power series, OMX_RESAMPLE_I0_TERMS terms behind the leading 1
    const double y = v * 0.5;
    double t = 1.0, s = 1.0;
    for (uint32_t i = 1; i <= OMX_RESAMPLE_I0_TERMS; ++i) {
        t = t * (y / (double)i);
        s = s + t * t;
    }
    return s;
}

// lp(fc): the Kaiser-windowed sinc with unit DC gain, in f64 (the header's DESIGN FORMULAS)
inline void cv_lowpass(double fc, double fs, double beta, uint32_t T, std::vector<double>& lp) {
    const uint32_t M = (T - 1) / 2;
    const double c = 2.0 * fc / fs, i0_beta = cv_i0(beta);
    lp.assign(T, 0.0);
    for (uint32_t k = 0; k <= M; ++k) {
        const double d = (double)k - (double)M;
        const double r = d / (double)M;
        const double u = c * d;
        const double a = kCvPi * u;
        const double sinc = u == 0.0 ? 1.0 : std::sin(a) / a;
        lp[k] = c * sinc * cv_i0(beta * std::sqrt(1.0 - r * r)) / i0_beta;
        lp[T - 1 - k] = lp[k];
    }
    double sum = 0.0;
    for (uint32_t k = 0; k < T; ++k) sum = sum + lp[k];
    for (uint32_t k = 0; k < T; ++k) lp[k] = lp[k] / sum;
}

inline int cv_design(const omx_program_convolve_spec* spec, double fs, float* taps_out, uint32_t n_floats, const char** why) {
    if (!spec || !taps_out) return cv_fail(why, "null pointer");
    if (spec->kind > OMX_CONVOLVE_BANDSTOP) return cv_fail(why, "unknown kind");
    const uint32_t T = spec->n_taps;
    if (T < 3 || T > OMX_CONVOLVE_MAX_TAPS - 1 || (T & 1u) == 0) return cv_fail(why, "n_taps even or outside 3 .. 4095");
    if (!std::isfinite(fs) || !(fs > 0.0)) return cv_fail(why, "a sample rate that is not finite or not positive");
    const bool uses_lo = spec->kind != OMX_CONVOLVE_LOWPASS, uses_hi = spec->kind != OMX_CONVOLVE_HIGHPASS;
    const auto bad = [&](double f) { return !std::isfinite(f) || !(f > 0.0) || !(f < fs / 2.0); };
    if ((uses_lo && bad(spec->f_lo_hz)) || (uses_hi && bad(spec->f_hi_hz)))
        return cv_fail(why, "a frequency that is not finite, not positive or at or above half the sample rate");
    if (uses_lo && uses_hi && !(spec->f_lo_hz < spec->f_hi_hz)) return cv_fail(why, "f_lo_hz >= f_hi_hz");
    if (!std::isfinite(spec->beta) || spec->beta < 0.0 || spec->beta > 20.0) return cv_fail(why, "beta not finite or outside [0, 20]");
    if (n_floats != T) return cv_fail(why, "n_floats != n_taps");
    const uint32_t M = (T - 1) / 2;
    std::vector<double> hi, lo;
    if (uses_hi) cv_lowpass(spec->f_hi_hz, fs, spec->beta, T, hi);
    if (uses_lo) cv_lowpass(spec->f_lo_hz, fs, spec->beta, T, lo);
    for (uint32_t k = 0; k <= M; ++k) {
        const double delta = k == M ? 1.0 : 0.0;
        double h;
        switch (spec->kind) {
            case OMX_CONVOLVE_LOWPASS: h = hi[k]; break;
            case OMX_CONVOLVE_HIGHPASS: h = delta - lo[k]; break;
            case OMX_CONVOLVE_BANDPASS: h = hi[k] - lo[k]; break;
            default: h = delta - (hi[k] - lo[k]); break;
        }
        taps_out[k] = (float)h;
        taps_out[T - 1 - k] = taps_out[k];
    }
    return OMX_NONE;
}

inline int cv_response(const omx_program_fir* fir, double fs, double hz, double* magnitude_db, double* phase_rad, const char** why) {
    const int rc = cv_check(fir, why);
    if (rc != OMX_NONE) return rc;
    if (!std::isfinite(fs) || !(fs > 0.0) || !std::isfinite(hz) || hz < 0.0)
        return cv_fail(why, "a rate or frequency that is not finite, a rate that is not positive, a negative frequency");
    const double w = 2.0 * kCvPi * hz / fs;
    double re = 0.0, im = 0.0;
    for (uint32_t k = 0; k < fir->n_taps; ++k) {
        const double ph = w * (double)k, h = (double)fir->taps[k];
        re = re + h * std::cos(ph);
        im = im - h * std::sin(ph);
    }
    if (magnitude_db) *magnitude_db = 20.0 * std::log10(std::sqrt(re * re + im * im));
    if (phase_rad) *phase_rad = std::atan2(im, re);
    return OMX_NONE;
}

}  // namespace omx
