// The host-only half of the programme bank's spectrum stage (include/omx/program_spectrum.h): defaults, plan, window, the transform
// count, density, fractional-octave bands, the QC summary and the match-EQ design.  Plain C++ doubles and integers, no device and no
// HIP: program_spectrum.cpp wraps these for the C ABI, tools/spectrum_design_check.cpp drives them under the sanitizers.  Every
// function returns an OMX_* code and, refusing, the reason in *why; a refusal writes nothing.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/omx/program_spectrum.h"

namespace omx {

constexpr uint32_t kSpThreads = 256;            // threads per workgroup of every kernel
constexpr uint32_t kSpRun = OMX_SPECTRUM_RUN;   // R
constexpr double kSpFloor = OMX_SPECTRUM_DB_FLOOR;
constexpr double kSpPi = 3.14159265358979323846;

inline int sp_fail(const char** why, const char* text) {
    if (why) *why = text;
    return OMX_ERR_INVALID;
}

inline bool sp_size_ok(uint32_t n) { return n == 2048 || n == 4096 || n == 8192; }
inline bool sp_rate_ok(double fs) { return std::isfinite(fs) && fs > 200.0; }
inline bool sp_rule_ok(const omx_program_spectrum_rule* r) { return r && r->flags == 0 && sp_size_ok(r->fft_size); }
constexpr const char* kSpBadRule =
    "bad spectrum rule (null, a flag set, or fft_size not 2048, 4096 or 8192: 16384 points and more need the 512- and 1024-thread "
    "transforms and come next)";
constexpr const char* kSpBadSize = "fft_size not 2048, 4096 or 8192";
constexpr const char* kSpBadRate = "sample_rate not finite or not above 200 Hz";
constexpr const char* kSpBadDensity = "a density entry that is negative or not finite";

// the transform kernel's geometry: an N/2-point complex transform by N/32 threads, 16 values each
inline uint32_t sp_threads_per_transform(uint32_t n) { return n / 32; }
inline uint32_t sp_transforms_per_workgroup(uint32_t n) { return kSpThreads / sp_threads_per_transform(n); }
inline uint32_t sp_lds_slots(uint32_t n) { return n / 2 + n / 32; }  // padded complex slots of one transform
inline uint32_t sp_lds_bytes(uint32_t n) { return sp_transforms_per_workgroup(n) * (sp_lds_slots(n) * 8 + 16) + 256 * 8; }

inline uint64_t sp_transforms_of(uint64_t frames, bool finished, uint32_t n) {
    const uint64_t h = n / 2;
    if (finished) return (frames + h - 1) / h;
    return frames >= n ? (frames - n) / h + 1 : 0;
}
// runs the transforms [k0, k1) touch: the scratch rows of a call
inline uint64_t sp_runs_touched(uint64_t k0, uint64_t k1) { return k1 > k0 ? (k1 - 1) / kSpRun - k0 / kSpRun + 1 : 0; }

inline int sp_rule_default(omx_program_spectrum_rule* rule, const char** why) {
    if (!rule) return sp_fail(why, "null rule");
    rule->fft_size = OMX_SPECTRUM_DEFAULT_FFT_SIZE;
    rule->flags = 0;
    return OMX_NONE;
}
inline int sp_qc_default(omx_program_spectrum_qc* qc, const char** why) {
    if (!qc) return sp_fail(why, "null qc");
    omx_program_spectrum_qc out{};
    out.occupied_fraction = OMX_SPECTRUM_DEFAULT_OCCUPIED_FRACTION;
    out.bandwidth_min_ratio = OMX_SPECTRUM_DEFAULT_BANDWIDTH_MIN_RATIO;
    out.tone_db = OMX_SPECTRUM_DEFAULT_TONE_DB;
    const double probes[6] = {50.0, 100.0, 150.0, 60.0, 120.0, 180.0};
    for (int i = 0; i < 6; ++i) out.probe_hz[i] = probes[i];
    out.n_probes = 6;
    *qc = out;
    return OMX_NONE;
}
inline int sp_match_spec_default(double fs, omx_program_spectrum_match_spec* spec, const char** why) {
    if (!spec) return sp_fail(why, "null spec");
    if (!sp_rate_ok(fs)) return sp_fail(why, kSpBadRate);
    omx_program_spectrum_match_spec out{};
    out.max_boost_db = OMX_SPECTRUM_DEFAULT_MAX_BOOST_DB;
    out.max_cut_db = OMX_SPECTRUM_DEFAULT_MAX_CUT_DB;
    out.low_hz = OMX_SPECTRUM_DEFAULT_LOW_HZ;
    out.high_hz = OMX_SPECTRUM_DEFAULT_HIGH_RATIO * fs;
    *spec = out;
    return OMX_NONE;
}

inline int sp_plan(const omx_program_spectrum_rule* rule, uint32_t channels, uint64_t n_streams, uint64_t frames,
                   omx_program_spectrum_info* info, const char** why) {
    if (!info) return sp_fail(why, "null info");
    if (!sp_rule_ok(rule)) return sp_fail(why, kSpBadRule);
    if (channels < 1 || channels > OMX_MAX_CHANNELS) return sp_fail(why, "channels outside 1 .. 8");
    if (frames > 0xFFFFFFFFull) return sp_fail(why, "frames beyond 2^32 - 1");
    if (n_streams > 0xFFFFFFFFull) return sp_fail(why, "n_streams beyond 2^32 - 1");
    const uint32_t n = rule->fft_size;
    omx_program_spectrum_info out{};
    out.fft_size = n;
    out.hop = n / 2;
    out.bins = n / 2 + 1;
    out.threads = kSpThreads;
    out.transforms_per_workgroup = sp_transforms_per_workgroup(n);
    out.run = kSpRun;
    out.lds_bytes = sp_lds_bytes(n);
    out.channels = channels;
    // a call of f frames takes at most ceil(f / H) + 2 transforms (the carried frames and a finish), which touch at most ceil(that / R) + 1 runs
    const uint64_t most = (frames + out.hop - 1) / out.hop + 2;
    const uint64_t rows = (most + kSpRun - 1) / kSpRun + 1;
    out.scratch_bytes = n_streams * channels * rows * out.bins * 8;
    // sums, closed runs and the open run in f64, two carry buffers of N frames in f32
    out.state_bytes = n_streams * channels * ((uint64_t)out.bins * 8 * 3 + (uint64_t)n * 4 * 2);
    *info = out;
    return OMX_NONE;
}

inline float sp_window_at(uint32_t n, uint32_t i) { return (float)(0.5 - 0.5 * std::cos(2.0 * kSpPi * (double)i / (double)n)); }
inline int sp_window(uint32_t n, float* w, const char** why) {
    if (!w) return sp_fail(why, "null window");
    if (!sp_size_ok(n)) return sp_fail(why, kSpBadSize);
    for (uint32_t i = 0; i < n; ++i) w[i] = sp_window_at(n, i);
    return OMX_NONE;
}
inline double sp_window_power(uint32_t n) {  // W2
    double s = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const double w = (double)sp_window_at(n, i);
        s += w * w;
    }
    return s;
}

inline int sp_transforms(uint64_t frames, uint32_t finished, uint32_t n, uint64_t* count, const char** why) {
    if (!count) return sp_fail(why, "null count");
    if (!sp_size_ok(n)) return sp_fail(why, kSpBadSize);
    if (frames > 0xFFFFFFFFull) return sp_fail(why, "frames beyond 2^32 - 1");
    *count = sp_transforms_of(frames, finished != 0, n);
    return OMX_NONE;
}

inline int sp_density(const omx_program_spectrum_record* rec, const double* sums, uint32_t channel, double* density, const char** why) {
    if (!rec || !sums || !density) return sp_fail(why, "null pointer");
    if (!sp_size_ok(rec->fft_size)) return sp_fail(why, "record->fft_size not 2048, 4096 or 8192");
    if (rec->channels < 1 || rec->channels > OMX_MAX_CHANNELS) return sp_fail(why, "record->channels outside 1 .. 8");
    if (channel >= rec->channels) return sp_fail(why, "channel at or above record->channels");
    const uint32_t n = rec->fft_size, bins = n / 2 + 1;
    const double* s = sums + (size_t)channel * bins;
    const uint64_t t = rec->transforms[channel];
    if (t == 0) {
        for (uint32_t b = 0; b < bins; ++b) density[b] = 0.0;
        return OMX_NONE;
    }
    const double den = ((double)t * (double)n) * sp_window_power(n);
    for (uint32_t b = 0; b < bins; ++b) density[b] = ((b == 0 || b == n / 2 ? 1.0 : 2.0) * s[b]) / den;
    return OMX_NONE;
}

inline bool sp_density_ok(const double* d, uint32_t bins) {
    for (uint32_t b = 0; b < bins; ++b)
        if (!(d[b] >= 0.0) || !std::isfinite(d[b])) return false;
    return true;
}
inline double sp_db(double v) { return v > 0.0 ? std::fmax(10.0 * std::log10(v), kSpFloor) : kSpFloor; }  // dB(v) of the header
inline double sp_level(double power) { return sp_db(2.0 * power); }

inline int sp_bands(const double* d, uint32_t n, double fs, uint32_t fraction, double* centre_hz, double* level_db, uint32_t* count,
                    const char** why) {
    if (!d || !centre_hz || !level_db || !count) return sp_fail(why, "null pointer");
    if (!sp_size_ok(n)) return sp_fail(why, kSpBadSize);
    if (!sp_rate_ok(fs)) return sp_fail(why, kSpBadRate);
    if (fraction != 1 && fraction != 3) return sp_fail(why, "fraction other than 1 or 3");
    const uint32_t bins = n / 2 + 1;
    if (!sp_density_ok(d, bins)) return sp_fail(why, kSpBadDensity);
    const double df = fs / (double)n, nyq = fs / 2.0;
    const double down = std::pow(10.0, -0.15 / (double)fraction), up = std::pow(10.0, 0.15 / (double)fraction);
    double centres[OMX_SPECTRUM_MAX_BANDS], levels[OMX_SPECTRUM_MAX_BANDS];
    uint32_t found = 0;
    for (int x = -40 * (int)fraction; x <= 20 * (int)fraction; ++x) {
        const double centre = 1000.0 * std::pow(10.0, 0.3 * (double)x / (double)fraction);
        const double lo = centre * down, hi = centre * up;
        if (!(lo >= 4.0 * df) || !(hi <= nyq)) continue;
        if (found == OMX_SPECTRUM_MAX_BANDS) return sp_fail(why, "more bands than OMX_SPECTRUM_MAX_BANDS");
        double power = 0.0;
        for (uint32_t b = 0; b < bins; ++b) {
            const double b_lo = std::fmax(0.0, ((double)b - 0.5) * df), b_hi = std::fmin(nyq, ((double)b + 0.5) * df);
            const double inside = std::fmin(hi, b_hi) - std::fmax(lo, b_lo);
            const double share = inside > 0.0 ? inside / (b_hi - b_lo) : 0.0;
            power += d[b] * share;
        }
        centres[found] = centre;
        levels[found] = sp_level(power);
        ++found;
    }
    if (*count < found) return sp_fail(why, "a capacity below the number of bands");
    for (uint32_t i = 0; i < found; ++i) {
        centre_hz[i] = centres[i];
        level_db[i] = levels[i];
    }
    *count = found;
    return OMX_NONE;
}

inline bool sp_qc_ok(const omx_program_spectrum_qc* q) {
    if (!q || q->flags != 0 || q->n_probes > OMX_SPECTRUM_MAX_PROBES) return false;
    if (!(q->occupied_fraction > 0.0 && q->occupied_fraction <= 1.0)) return false;
    if (!(q->bandwidth_min_ratio >= 0.0 && q->bandwidth_min_ratio <= 1.0)) return false;
    if (!std::isfinite(q->tone_db) || !(q->tone_db >= 0.0)) return false;
    for (uint32_t i = 0; i < q->n_probes; ++i)
        if (!std::isfinite(q->probe_hz[i]) || !(q->probe_hz[i] > 0.0)) return false;
    return true;
}

inline int sp_summarize(const omx_program_spectrum_qc* qc, const double* d, uint32_t n, double fs, omx_program_spectrum_summary* summary,
                        const char** why) {
    if (!d || !summary) return sp_fail(why, "null pointer");
    if (!sp_qc_ok(qc))
        return sp_fail(why, "bad qc rule (null, occupied_fraction outside (0, 1], bandwidth_min_ratio outside [0, 1], tone_db negative or "
                            "not finite, more than 8 probes, a probe that is not finite or not above 0, or a flag set)");
    if (!sp_size_ok(n)) return sp_fail(why, kSpBadSize);
    if (!sp_rate_ok(fs)) return sp_fail(why, kSpBadRate);
    const uint32_t bins = n / 2 + 1, half = n / 2;
    if (!sp_density_ok(d, bins)) return sp_fail(why, kSpBadDensity);
    const double df = fs / (double)n, nyq = fs / 2.0;
    omx_program_spectrum_summary out{};
    out.n_probes = qc->n_probes;
    double total = 0.0;
    uint32_t pk = 0;
    for (uint32_t b = 0; b < bins; ++b) {
        total += d[b];
        if (d[b] > d[pk]) pk = b;
    }
    out.total_db = sp_level(total);
    double delta = 0.0, skew = 0.0;
    if (pk > 0 && pk < half && d[pk - 1] > 0.0 && d[pk + 1] > 0.0) {
        const double a = 10.0 * std::log10(d[pk - 1]), m = 10.0 * std::log10(d[pk]), c = 10.0 * std::log10(d[pk + 1]);
        const double q = a - 2.0 * m + c;
        delta = q < 0.0 ? 0.5 * (a - c) / q : 0.0;
        delta = std::fmin(std::fmax(delta, -0.5), 0.5);
        skew = a - c;
    }
    out.peak_hz = ((double)pk + delta) * df;
    out.peak_db = d[pk] > 0.0 ? std::fmax(10.0 * std::log10(2.0 * d[pk]) - 0.25 * skew * delta, kSpFloor) : kSpFloor;
    if (total > 0.0) {
        const double want = qc->occupied_fraction * total;
        double run = 0.0;
        uint32_t at = half;
        for (uint32_t b = 0; b < bins; ++b) {
            run += d[b];
            if (run >= want) {
                at = b;
                break;
            }
        }
        out.occupied_hz = std::fmin(((double)at + 0.5) * df, nyq);
    }
    const double third_down = std::pow(10.0, -0.1), third_up = std::pow(10.0, 0.1);
    std::vector<double> near;
    for (uint32_t i = 0; i < qc->n_probes; ++i) {
        const double f = qc->probe_hz[i];
        if (!(f < nyq)) continue;
        const long bc = (long)std::floor(f / df + 0.5);
        double strongest = 0.0;
        for (long b = bc - 1; b <= bc + 1; ++b)
            if (b >= 0 && b <= (long)half) strongest = std::fmax(strongest, d[b]);
        near.clear();
        const double f_lo = f * third_down, f_hi = f * third_up;
        for (long b = 1; b <= (long)half; ++b) {  // (at low frequencies a third octave is a bin or two: at least six bins either side)
            const double fb = (double)b * df;
            const long off = b > bc ? b - bc : bc - b;
            if (off > 2 && ((fb >= f_lo && fb <= f_hi) || off <= 6)) near.push_back(d[b]);
        }
        if (near.empty()) continue;
        std::sort(near.begin(), near.end());
        const size_t m = near.size();
        const double med = m % 2 ? near[m / 2] : 0.5 * (near[m / 2 - 1] + near[m / 2]);
        out.prominence_db[i] = sp_db(strongest) - sp_db(med);
        if (out.prominence_db[i] > qc->tone_db) out.verdict |= OMX_SPECTRUM_TONE;
    }
    if (total > 0.0 && out.occupied_hz < qc->bandwidth_min_ratio * nyq) out.verdict |= OMX_SPECTRUM_BANDLIMITED;
    *summary = out;
    return OMX_NONE;
}

inline bool sp_spec_ok(const omx_program_spectrum_match_spec* s, double fs) {
    return s && s->flags == 0 && std::isfinite(s->max_boost_db) && s->max_boost_db >= 0.0 && std::isfinite(s->max_cut_db) &&
           s->max_cut_db >= 0.0 && std::isfinite(s->low_hz) && s->low_hz >= 0.0 && std::isfinite(s->high_hz) && s->high_hz > s->low_hz &&
           s->high_hz <= fs / 2.0;
}

// Ds of the header: a boxcar of one third octave in log frequency
inline void sp_smooth(const double* d, uint32_t half, std::vector<double>& out) {
    std::vector<double> prefix(half + 2);
    prefix[0] = 0.0;
    for (uint32_t b = 0; b <= half; ++b) prefix[b + 1] = prefix[b] + d[b];
    const double c_lo = std::pow(10.0, -0.05), c_hi = std::pow(10.0, 0.05);
    out.resize(half + 1);
    out[0] = d[0];
    for (uint32_t b = 1; b <= half; ++b) {
        const long lo = std::max(1l, (long)std::ceil((double)b * c_lo)), hi = std::min((long)half, (long)std::floor((double)b * c_hi));
        out[b] = (prefix[hi + 1] - prefix[lo]) / (double)(hi - lo + 1);
    }
}

inline int sp_match(const double* d_source, const double* d_target, uint32_t n, double fs, const omx_program_spectrum_match_spec* spec,
                    float* taps, uint32_t n_taps, const char** why) {
    if (!d_source || !d_target || !taps) return sp_fail(why, "null pointer");
    if (!sp_size_ok(n)) return sp_fail(why, kSpBadSize);
    if (!sp_rate_ok(fs)) return sp_fail(why, kSpBadRate);
    if (!sp_spec_ok(spec, fs))
        return sp_fail(why, "bad match spec (null, a limit that is negative or not finite, low_hz negative, high_hz not above low_hz or "
                            "above sample_rate / 2, or a flag set)");
    if (n_taps == 0 || n_taps % 2 == 0 || n_taps > OMX_SPECTRUM_MAX_TAPS || n_taps >= n)
        return sp_fail(why, "n_taps even, 0, above OMX_SPECTRUM_MAX_TAPS or not below fft_size");
    const uint32_t half = n / 2;
    if (!sp_density_ok(d_source, half + 1) || !sp_density_ok(d_target, half + 1)) return sp_fail(why, kSpBadDensity);
    const double df = fs / (double)n;
    const long b_lo = std::max(1l, (long)std::ceil(spec->low_hz / df)), b_hi = std::min((long)half, (long)std::floor(spec->high_hz / df));
    if (b_lo > b_hi) return sp_fail(why, "no bin between low_hz and high_hz");
    std::vector<double> src, tgt, amp(half + 1);
    sp_smooth(d_source, half, src);
    sp_smooth(d_target, half, tgt);
    for (uint32_t b = 0; b <= half; ++b) {
        const double g = sp_db(tgt[b]) - sp_db(src[b]);  // the power ratio in dB is the filter's gain in dB
        amp[b] = std::fmin(std::fmax(g, -spec->max_cut_db), spec->max_boost_db);
    }
    for (long b = 0; b < b_lo; ++b) amp[b] = amp[b_lo];
    for (long b = b_hi + 1; b <= (long)half; ++b) amp[b] = amp[b_hi];
    for (uint32_t b = 0; b <= half; ++b) amp[b] = std::pow(10.0, amp[b] / 20.0);
    std::vector<double> cosine(n);
    for (uint32_t i = 0; i < n; ++i) cosine[i] = std::cos(2.0 * kSpPi * (double)i / (double)n);
    const uint32_t mid = (n_taps - 1) / 2;
    for (uint32_t m = 0; m <= mid; ++m) {
        double sum = 0.0;
        for (uint32_t b = 1; b < half; ++b) sum += amp[b] * cosine[((uint64_t)b * m) % n];
        const double h = (amp[0] + 2.0 * sum + amp[half] * cosine[((uint64_t)half * m) % n]) / (double)n;
        const float tap = (float)(h * (0.5 + 0.5 * std::cos(kSpPi * (double)m / (double)(mid + 1))));
        taps[mid + m] = tap;
        taps[mid - m] = tap;
    }
    return OMX_NONE;
}

}  // namespace omx
