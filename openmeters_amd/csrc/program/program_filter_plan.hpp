// The host-only half of the programme bank's filter stage (include/omx/program_filter.h): design, cascade, check, response, plan,
// the tables of the time-parallel form and the rule that says whether a filter may run in it.  Plain C++ doubles, no device and no
// HIP: program_filter.cpp wraps these for the C ABI, tools/filter_design_check.cpp drives them under the sanitizers.  Every function
// returns an OMX_* code and, refusing, the reason in *why.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/omx/program_filter.h"

namespace omx {

constexpr uint32_t kFlTile = 32;            // frames per LDS tile of the filter pass
constexpr uint32_t kFlChunkFrames = 1024;   // frames per work item of the time-parallel form
constexpr double kFlPi = 3.14159265358979323846;

inline int fl_fail(const char** why, const char* text, int code = OMX_ERR_INVALID) {
    if (why) *why = text;
    return code;
}

inline int fl_check(const omx_program_filter* f, const char** why) {
    if (!f) return fl_fail(why, "null filter");
    if (f->n_sections < 1 || f->n_sections > OMX_FILTER_MAX_SECTIONS) return fl_fail(why, "n_sections outside 1 .. 2");
    for (uint32_t k = 0; k < f->n_sections; ++k) {
        const omx_program_filter_section& s = f->section[k];
        if (!std::isfinite(s.b0) || !std::isfinite(s.b1) || !std::isfinite(s.b2) || !std::isfinite(s.a1) || !std::isfinite(s.a2))
            return fl_fail(why, "a coefficient that is not finite");
    }
    for (uint32_t k = 0; k < f->n_sections; ++k) {
        const omx_program_filter_section& s = f->section[k];
        if (!(std::fabs(s.a2) < 1.0 && std::fabs(s.a1) < 1.0 + s.a2))
            return fl_fail(why, "a section that is not strictly stable (|a2| < 1 && |a1| < 1 + a2)", OMX_ERR_UNSUPPORTED);
    }
    return OMX_NONE;
}

inline omx_program_filter_section fl_rbj(double b0, double b1, double b2, double a0, double a1, double a2) {
    return omx_program_filter_section{b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0};
}

inline omx_program_filter_section fl_pass2(bool high, double w0, double q) {
    const double cs = std::cos(w0), al = std::sin(w0) / (2.0 * q);
    if (high) return fl_rbj((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0, 1.0 + al, -2.0 * cs, 1.0 - al);
    return fl_rbj((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0, 1.0 + al, -2.0 * cs, 1.0 - al);
}

inline int fl_design(const omx_program_filter_spec* spec, double fs, omx_program_filter* filter, const char** why) {
    if (!spec || !filter) return fl_fail(why, "null pointer");
    if (!std::isfinite(fs) || !(fs > 0.0)) return fl_fail(why, "a sample rate that is not finite or not positive");
    const uint32_t kind = spec->kind;
    if (kind > OMX_FILTER_PREEMPHASIS) return fl_fail(why, "unknown kind");
    const bool pass = kind == OMX_FILTER_HIGHPASS || kind == OMX_FILTER_LOWPASS;
    const bool emphasis = kind == OMX_FILTER_DEEMPHASIS || kind == OMX_FILTER_PREEMPHASIS;
    const bool first_order = kind == OMX_FILTER_DC_BLOCK || emphasis;
    if (pass ? (spec->order != 1 && spec->order != 2 && spec->order != 4) : (spec->order != 0 && spec->order != (first_order ? 1u : 2u)))
        return fl_fail(why, "an order the kind does not have");
    const double f = spec->frequency_hz;
    if (!emphasis && (!std::isfinite(f) || !(f > 0.0) || !(f < fs / 2.0)))
        return fl_fail(why, "a frequency that is not finite, not positive or at or above half the sample rate");
    const bool uses_q = (pass && spec->order == 2) || (!pass && !first_order);
    if (uses_q && (!std::isfinite(spec->q) || spec->q < 0.0)) return fl_fail(why, "a q that is not finite or negative");
    const bool uses_gain = kind == OMX_FILTER_LOW_SHELF || kind == OMX_FILTER_HIGH_SHELF || kind == OMX_FILTER_PEAKING;
    if (uses_gain && !std::isfinite(spec->gain_db)) return fl_fail(why, "a gain that is not finite");
    if (emphasis) {
        const double t1 = spec->time_constant_us, t2 = spec->time_constant_zero_us;
        if (!std::isfinite(t1) || !(t1 > 0.0)) return fl_fail(why, "a time constant that is not finite or not positive");
        if (!std::isfinite(t2) || t2 < 0.0 || !(t2 < t1)) return fl_fail(why, "a zero time constant that is not finite, negative or not below the other");
    }
    const double q = spec->q == 0.0 ? 1.0 / std::sqrt(2.0) : spec->q;
    const double w0 = 2.0 * kFlPi * f / fs, cs = std::cos(w0), al = std::sin(w0) / (2.0 * q);
    omx_program_filter out{};
    out.n_sections = 1;
    omx_program_filter_section& s = out.section[0];
    switch (kind) {
        case OMX_FILTER_HIGHPASS:
        case OMX_FILTER_LOWPASS: {
            const bool high = kind == OMX_FILTER_HIGHPASS;
            if (spec->order == 1) {
                const double K = std::tan(kFlPi * f / fs);
                if (high) s = {1.0 / (1.0 + K), -(1.0 / (1.0 + K)), 0.0, (K - 1.0) / (K + 1.0), 0.0};
                else s = {K / (1.0 + K), K / (1.0 + K), 0.0, (K - 1.0) / (K + 1.0), 0.0};
            } else if (spec->order == 2) {
                s = fl_pass2(high, w0, q);
            } else {
                out.n_sections = 2;
                out.section[0] = fl_pass2(high, w0, 1.0 / std::sqrt(2.0 + std::sqrt(2.0)));
                out.section[1] = fl_pass2(high, w0, 1.0 / std::sqrt(2.0 - std::sqrt(2.0)));
            }
            break;
        }
        case OMX_FILTER_LOW_SHELF:
        case OMX_FILTER_HIGH_SHELF: {
            const double A = std::pow(10.0, spec->gain_db / 40.0), r = 2.0 * std::sqrt(A) * al;
            if (kind == OMX_FILTER_LOW_SHELF)
                s = fl_rbj(A * ((A + 1.0) - (A - 1.0) * cs + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), A * ((A + 1.0) - (A - 1.0) * cs - r),
                           (A + 1.0) + (A - 1.0) * cs + r, -2.0 * ((A - 1.0) + (A + 1.0) * cs), (A + 1.0) + (A - 1.0) * cs - r);
            else
                s = fl_rbj(A * ((A + 1.0) + (A - 1.0) * cs + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), A * ((A + 1.0) + (A - 1.0) * cs - r),
                           (A + 1.0) - (A - 1.0) * cs + r, 2.0 * ((A - 1.0) - (A + 1.0) * cs), (A + 1.0) - (A - 1.0) * cs - r);
            break;
        }
        case OMX_FILTER_PEAKING: {
            const double A = std::pow(10.0, spec->gain_db / 40.0);
            s = fl_rbj(1.0 + al * A, -2.0 * cs, 1.0 - al * A, 1.0 + al / A, -2.0 * cs, 1.0 - al / A);
            break;
        }
        case OMX_FILTER_NOTCH: s = fl_rbj(1.0, -2.0 * cs, 1.0, 1.0 + al, -2.0 * cs, 1.0 - al); break;
        case OMX_FILTER_DC_BLOCK: s = {1.0, -1.0, 0.0, -(1.0 - w0), 0.0}; break;
        default: {  // the emphasis kinds
            const double k1 = 2.0 * fs * (spec->time_constant_us * 1.0e-6), k2 = 2.0 * fs * (spec->time_constant_zero_us * 1.0e-6);
            if (kind == OMX_FILTER_DEEMPHASIS) s = {(1.0 + k2) / (1.0 + k1), (1.0 - k2) / (1.0 + k1), 0.0, (1.0 - k1) / (1.0 + k1), 0.0};
            else s = {(1.0 + k1) / (1.0 + k2), (1.0 - k1) / (1.0 + k2), 0.0, (1.0 - k2) / (1.0 + k2), 0.0};
            break;
        }
    }
    const int rc = fl_check(&out, why);
    if (rc != OMX_NONE) return rc;
    *filter = out;
    return OMX_NONE;
}

inline int fl_cascade(const omx_program_filter* a, const omx_program_filter* b, omx_program_filter* out, const char** why) {
    if (!a || !b || !out) return fl_fail(why, "null pointer");
    if (a->n_sections < 1 || a->n_sections > OMX_FILTER_MAX_SECTIONS || b->n_sections < 1 || b->n_sections > OMX_FILTER_MAX_SECTIONS)
        return fl_fail(why, "n_sections outside 1 .. 2");
    if (a->n_sections + b->n_sections > OMX_FILTER_MAX_SECTIONS) return fl_fail(why, "more than OMX_FILTER_MAX_SECTIONS sections together");
    omx_program_filter r{};
    r.n_sections = a->n_sections + b->n_sections;
    for (uint32_t k = 0; k < a->n_sections; ++k) r.section[k] = a->section[k];
    for (uint32_t k = 0; k < b->n_sections; ++k) r.section[a->n_sections + k] = b->section[k];
    *out = r;
    return OMX_NONE;
}

inline int fl_response(const omx_program_filter* f, double fs, double hz, double* magnitude_db, double* phase_rad, const char** why) {
    if (!f) return fl_fail(why, "null filter");
    if (f->n_sections < 1 || f->n_sections > OMX_FILTER_MAX_SECTIONS) return fl_fail(why, "n_sections outside 1 .. 2");
    if (!std::isfinite(fs) || !(fs > 0.0) || !std::isfinite(hz) || hz < 0.0)
        return fl_fail(why, "a rate or frequency that is not finite, a rate that is not positive, a negative frequency");
    const double w = 2.0 * kFlPi * hz / fs, c1 = std::cos(w), s1 = std::sin(w), c2 = std::cos(2.0 * w), s2 = std::sin(2.0 * w);
    double re = 1.0, im = 0.0;
    for (uint32_t k = 0; k < f->n_sections; ++k) {
        const omx_program_filter_section& s = f->section[k];
        const double nr = s.b0 + s.b1 * c1 + s.b2 * c2, ni = -(s.b1 * s1 + s.b2 * s2);
        const double dr = 1.0 + s.a1 * c1 + s.a2 * c2, di = -(s.a1 * s1 + s.a2 * s2);
        const double dd = dr * dr + di * di;
        const double hr = (nr * dr + ni * di) / dd, hi = (ni * dr - nr * di) / dd;
        const double r2 = re * hr - im * hi, i2 = re * hi + im * hr;
        re = r2;
        im = i2;
    }
    if (magnitude_db) *magnitude_db = 20.0 * std::log10(std::sqrt(re * re + im * im));
    if (phase_rad) *phase_rad = std::atan2(im, re);
    return OMX_NONE;
}

constexpr uint32_t fl_slot_shift(uint32_t channels) { return channels == 1 ? 0u : (channels == 2 ? 1u : (channels <= 4 ? 2u : 3u)); }

inline int fl_plan(uint32_t channels, double fs, omx_program_filter_info* info, const char** why) {
    if (!info) return fl_fail(why, "null info");
    if (channels < 1 || channels > OMX_MAX_CHANNELS) return fl_fail(why, "channels outside 1 .. 8");
    if (!std::isfinite(fs) || !(fs > 0.0)) return fl_fail(why, "a sample rate that is not finite or not positive");
    *info = omx_program_filter_info{kFlChunkFrames, kFlTile, channels, 64u >> fl_slot_shift(channels)};
    return OMX_NONE;
}

// ---- the tables of the time-parallel form.  The state of a channel is f = (s1, s2 of section 0, s1, s2 of section 1); a filter of
// one section runs the identity (b0 = 1) as its second, whose state stays zero.  One step is f' = A f + B x.  The entries of A^L
// cancel by many orders of magnitude over a work item, so the tables are made in double-double and rounded once, at the end.
struct FlDD {
    double h, l;
};
inline FlDD fl_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
inline FlDD fl_dd_add(FlDD a, FlDD b) {
    FlDD s = fl_two_sum(a.h, b.h);
    const FlDD t = fl_two_sum(a.l, b.l);
    s.l += t.h;
    s = {s.h + s.l, s.l - ((s.h + s.l) - s.h)};
    s.l += t.l;
    return {s.h + s.l, s.l - ((s.h + s.l) - s.h)};
}
inline FlDD fl_dd_mul_d(FlDD a, double b) {
    const double p = a.h * b, e = std::fma(a.h, b, -p) + a.l * b;
    return {p + e, e - ((p + e) - p)};
}
// one step of both sections on the state f with the input x, exact to double-double
inline void fl_dd_step(FlDD (&f)[4], FlDD x, const omx_program_filter_section (&sec)[2]) {
    FlDD v = x;
    for (int k = 0; k < 2; ++k) {
        const omx_program_filter_section& c = sec[k];
        const FlDD y = fl_dd_add(fl_dd_mul_d(v, c.b0), f[2 * k]);
        f[2 * k] = fl_dd_add(fl_dd_add(fl_dd_mul_d(v, c.b1), fl_dd_mul_d(y, -c.a1)), f[2 * k + 1]);
        f[2 * k + 1] = fl_dd_add(fl_dd_mul_d(v, c.b2), fl_dd_mul_d(y, -c.a2));
        v = y;
    }
}

struct FlTables {
    std::vector<double> weights;  // [padded L][4]: W[k][i] = (A^(L-1-k) B)_i, zeros behind L
    double transition[32];        // A^L: [i][k] high parts, then low parts
    double largest_entry;         // max |A^L|[i][k]
    double state_gain;            // max over i of sum over k of |W[k][i]|: the largest zero-state end state of a full-scale item
};

inline FlTables fl_tables(const omx_program_filter& filter, uint32_t L) {
    omx_program_filter_section sec[2] = {filter.section[0], {1.0, 0.0, 0.0, 0.0, 0.0}};
    if (filter.n_sections == 2) sec[1] = filter.section[1];
    FlTables t{};
    const uint32_t padded = (L + kFlTile - 1) / kFlTile * kFlTile;  // the pass reads whole tiles of weights
    t.weights.assign((size_t)padded * 4, 0.0);
    FlDD g[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    fl_dd_step(g, FlDD{1.0, 0.0}, sec);  // B
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t n = 0; n < L; ++n) {
        const uint32_t k = L - 1 - n;
        for (int i = 0; i < 4; ++i) {
            t.weights[(size_t)k * 4 + i] = g[i].h;
            sum[i] += std::fabs(g[i].h);
        }
        fl_dd_step(g, FlDD{0.0, 0.0}, sec);
    }
    for (int i = 0; i < 4; ++i) t.state_gain = std::fmax(t.state_gain, sum[i]);
    for (int m = 0; m < 4; ++m) {  // column m: the state that started as unit vector m
        FlDD f[4];
        for (int k = 0; k < 4; ++k) f[k] = {k == m ? 1.0 : 0.0, 0.0};
        for (uint32_t n = 0; n < L; ++n) fl_dd_step(f, FlDD{0.0, 0.0}, sec);
        for (int k = 0; k < 4; ++k) {
            t.transition[k * 4 + m] = f[k].h;
            t.transition[16 + k * 4 + m] = f[k].l;
            t.largest_entry = std::fmax(t.largest_entry, std::fabs(f[k].h));
        }
    }
    return t;
}

// Whether a filter may run in the time-parallel form ("Filter").  Either order rounds the state at every one of
// the L steps of a work item by 2^-53 of its size, which is at most state_gain per unit of input peak; A^n carries each rounding to
// the item's end, where it is the next item's start-state error, and largest_entry bounds that growth.  The form's bar is 2^-23 of
// the peak and the start state may take a quarter of it: L * largest_entry * state_gain * 2^-53 <= 2^-25.
inline double fl_predicted_start_error(const FlTables& t, uint32_t L) { return (double)L * t.largest_entry * t.state_gain * 0x1p-53; }
inline bool fl_time_parallel_ok(const FlTables& t, uint32_t L) { return fl_predicted_start_error(t, L) <= 0x1p-25; }

}  // namespace omx
