// Stand-alone check of the host side of the programme bank's filter stage (openmeters_amd/csrc/program/program_filter_plan.hpp), for
// a sanitizer run on the CPU: no device, no HIP, its own main.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/filter_design_check.cpp -o filter_design_check
//   ./filter_design_check
//
// 1. Every kind at the rates 8 kHz .. 768 kHz and corner frequencies from 1 Hz to just below Nyquist: fl_design, fl_check on the result,
//    fl_response at DC, the corner and Nyquist against the gains the kind must have, fl_cascade with a DC blocker.
// 2. The tables of the time-parallel form (fl_tables) of every designed filter: the zero-state weights and the transition A^L, made in
//    double-double, against a plain f64 run of the definition over one work item from a random state and random input
//    (end state = A^L s + sum W[k] x[k]), and the fall-back rule's figure.
// 3. The refusals: every argument the header names, with nothing written.
// Prints what it compared; exit code 0 = everything agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../openmeters_amd/csrc/program/program_filter_plan.hpp"

using namespace omx;

static int failures = 0;
#define EXPECT(cond, ...)                          \
    do {                                           \
        if (!(cond)) {                             \
            if (++failures < 20) {                 \
                std::printf("FAILED %s: ", #cond); \
                std::printf(__VA_ARGS__);          \
                std::printf("\n");                 \
            }                                      \
        }                                          \
    } while (0)

static double gain_db(const omx_program_filter& f, double fs, double hz) {
    double db = 0.0;
    const char* why = nullptr;
    EXPECT(fl_response(&f, fs, hz, &db, nullptr, &why) == OMX_NONE, "response refused: %s", why ? why : "");
    return db;
}

// the definition in plain f64, one step of one channel
static double step(const omx_program_filter& f, double (&s)[4], double x) {
    double v = x;
    for (uint32_t k = 0; k < f.n_sections; ++k) {
        const omx_program_filter_section& c = f.section[k];
        const double y = c.b0 * v + s[2 * k];
        s[2 * k] = (c.b1 * v - c.a1 * y) + s[2 * k + 1];
        s[2 * k + 1] = c.b2 * v - c.a2 * y;
        v = y;
    }
    return v;
}

int main() {
    const double rates[] = {8000.0, 11025.0, 22050.0, 44100.0, 48000.0, 88200.0, 96000.0, 192000.0, 384000.0, 768000.0};
    const double corners[] = {1.0, 5.0, 20.0, 120.0, 1000.0, 3999.0, 10000.0, 20000.0, 95000.0, 383999.0};
    std::mt19937_64 rng(2024);
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    long designed = 0, refused_unstable = 0, tables = 0, rejected_by_rule = 0;
    double worst_table = 0.0, worst_figure = 0.0;
    for (double fs : rates) {
        for (double f : corners) {
            if (!(f < fs / 2.0)) continue;
            for (uint32_t kind = 0; kind <= OMX_FILTER_PREEMPHASIS; ++kind) {
                const bool pass = kind <= OMX_FILTER_LOWPASS;
                const uint32_t orders[3] = {pass ? 1u : 0u, pass ? 2u : 0u, pass ? 4u : 0u};
                for (int oi = 0; oi < (pass ? 3 : 1); ++oi) {
                    for (double gain : {-12.0, 6.0}) {
                        omx_program_filter_spec spec{};
                        spec.kind = kind;
                        spec.order = orders[oi];
                        spec.frequency_hz = f;
                        spec.q = oi == 1 ? 0.0 : 1.7;
                        spec.gain_db = gain;
                        spec.time_constant_us = gain < 0.0 ? 75.0 : 50.0;
                        spec.time_constant_zero_us = gain < 0.0 ? 0.0 : 15.0;
                        omx_program_filter filt;
                        std::memset(&filt, 0x5A, sizeof(filt));
                        const char* why = nullptr;
                        const int rc = fl_design(&spec, fs, &filt, &why);
                        if (rc == OMX_ERR_UNSUPPORTED) {  // a DC blocker far up, or pre-emphasis without a zero: nothing written
                            ++refused_unstable;
                            const unsigned char* raw = reinterpret_cast<const unsigned char*>(&filt);
                            bool untouched = true;
                            for (size_t i = 0; i < sizeof(filt); ++i) untouched = untouched && raw[i] == 0x5A;
                            EXPECT(untouched, "a refused design wrote (kind %u)", kind);
                            EXPECT(kind == OMX_FILTER_DC_BLOCK || kind == OMX_FILTER_PREEMPHASIS, "kind %u at %g / %g: %s", kind, f, fs, why);
                            continue;
                        }
                        EXPECT(rc == OMX_NONE, "kind %u order %u at %g / %g: %d %s", kind, spec.order, f, fs, rc, why ? why : "");
                        if (rc != OMX_NONE) continue;
                        ++designed;
                        EXPECT(fl_check(&filt, &why) == OMX_NONE, "check of a designed filter: %s", why);
                        EXPECT(filt.n_sections == (pass && spec.order == 4 ? 2u : 1u), "sections %u", filt.n_sections);
                        const double dc = gain_db(filt, fs, 0.0), ny = gain_db(filt, fs, fs / 2.0), at = gain_db(filt, fs, f);
                        // 1 -+ cos(w0) cancels: the coefficients of a corner at the distance d from DC or from Nyquist carry eps / d^2,
                        // and so do the gains
                        const double w0 = 2.0 * kFlPi * f / fs, d = std::fmin(w0, kFlPi - w0), tol = 1e-8 + 400.0 * 2.220446049250313e-16 / (d * d);
                        switch (kind) {
                            case OMX_FILTER_HIGHPASS: EXPECT(dc < -200.0 && std::fabs(ny) < tol, "highpass %g %g", dc, ny); break;
                            case OMX_FILTER_LOWPASS: EXPECT(std::fabs(dc) < tol && ny < -200.0, "lowpass %g %g", dc, ny); break;
                            case OMX_FILTER_LOW_SHELF: EXPECT(std::fabs(dc - gain) < tol && std::fabs(ny) < tol, "low shelf %g %g", dc, ny); break;
                            case OMX_FILTER_HIGH_SHELF: EXPECT(std::fabs(dc) < tol && std::fabs(ny - gain) < tol, "high shelf %g %g", dc, ny); break;
                            case OMX_FILTER_PEAKING: EXPECT(std::fabs(dc) < tol && std::fabs(ny) < tol && std::fabs(at - gain) < tol, "peaking %g %g %g", dc, ny, at); break;
                            case OMX_FILTER_NOTCH: EXPECT(std::fabs(dc) < tol && std::fabs(ny) < tol && at < -100.0, "notch %g %g %g", dc, ny, at); break;
                            case OMX_FILTER_DC_BLOCK: EXPECT(dc < -200.0, "dc block %g", dc); break;
                            default: EXPECT(std::fabs(dc) < tol, "emphasis %g", dc); break;
                        }
                        if (pass && (spec.order != 2 || spec.q == 0.0))
                            EXPECT(std::fabs(at - 10.0 * std::log10(0.5)) < tol, "corner of kind %u order %u at %g / %g: %.9f", kind, spec.order, f, fs, at);
                        // cascade with a DC blocker
                        omx_program_filter_spec dc_spec{};
                        dc_spec.kind = OMX_FILTER_DC_BLOCK;
                        dc_spec.frequency_hz = 5.0;
                        omx_program_filter blocker, both;
                        EXPECT(fl_design(&dc_spec, fs, &blocker, &why) == OMX_NONE, "dc blocker at %g", fs);
                        const int crc = fl_cascade(&blocker, &filt, &both, &why);
                        if (filt.n_sections == 1) {
                            EXPECT(crc == OMX_NONE && both.n_sections == 2 && std::memcmp(&both.section[1], &filt.section[0], sizeof(filt.section[0])) == 0,
                                   "cascade");
                        } else {
                            EXPECT(crc == OMX_ERR_INVALID, "cascade of three sections: %d", crc);
                        }
                        // the tables against a plain run of one work item
                        const omx_program_filter& use = filt.n_sections == 1 && crc == OMX_NONE ? both : filt;
                        const uint32_t L = kFlChunkFrames;
                        const FlTables t = fl_tables(use, L);
                        ++tables;
                        EXPECT(t.weights.size() == (size_t)L * 4, "weights %zu", t.weights.size());
                        double s[4], end[4] = {0.0, 0.0, 0.0, 0.0}, scale = 0.0;
                        for (int i = 0; i < 4; ++i) s[i] = uni(rng);
                        for (int i = 0; i < 4; ++i)
                            for (int k = 0; k < 4; ++k) {
                                end[i] += (t.transition[i * 4 + k] + t.transition[16 + i * 4 + k]) * s[k];
                                scale = std::fmax(scale, std::fabs(t.transition[i * 4 + k] * s[k]));
                            }
                        for (uint32_t n = 0; n < L; ++n) {
                            const double x = uni(rng);
                            for (int i = 0; i < 4; ++i) end[i] += t.weights[(size_t)n * 4 + i] * x;
                            step(use, s, x);
                        }
                        scale = std::fmax(scale, t.state_gain);
                        for (int i = 0; i < 4; ++i) {
                            const double err = std::fabs(end[i] - s[i]) / scale;
                            worst_table = std::fmax(worst_table, err);
                            EXPECT(err < 1e-9, "tables of kind %u at %g / %g: state %d differs by %g of %g", kind, f, fs, i, err, scale);
                        }
                        const double figure = fl_predicted_start_error(t, L);
                        worst_figure = std::fmax(worst_figure, figure);
                        if (!fl_time_parallel_ok(t, L)) ++rejected_by_rule;
                    }
                }
            }
        }
    }
    // the filter the rule rejects: two undamped resonators at 20 Hz and 768 kHz
    {
        const double w0 = 2.0 * kFlPi * 20.0 / 768000.0, r = 1.0 - 1e-6;
        omx_program_filter res{};
        res.n_sections = 2;
        res.section[0] = res.section[1] = omx_program_filter_section{1.0, 0.0, 0.0, -2.0 * r * std::cos(w0), r * r};
        const char* why = nullptr;
        EXPECT(fl_check(&res, &why) == OMX_NONE, "the resonator is strictly stable");
        const FlTables t = fl_tables(res, kFlChunkFrames);
        EXPECT(!fl_time_parallel_ok(t, kFlChunkFrames), "the rule takes the resonator: %g", fl_predicted_start_error(t, kFlChunkFrames));
        std::printf("resonator: largest entry %.3e, state gain %.3e, figure %.3e\n", t.largest_entry, t.state_gain,
                    fl_predicted_start_error(t, kFlChunkFrames));
    }
    // refusals
    {
        const char* why = nullptr;
        omx_program_filter f{}, g{};
        omx_program_filter_spec spec{};
        spec.kind = OMX_FILTER_HIGHPASS;
        spec.order = 2;
        spec.frequency_hz = 100.0;
        EXPECT(fl_design(nullptr, 48000.0, &f, &why) == OMX_ERR_INVALID && fl_design(&spec, 48000.0, nullptr, &why) == OMX_ERR_INVALID, "null");
        for (double fs : {0.0, -1.0, (double)NAN, (double)INFINITY}) EXPECT(fl_design(&spec, fs, &f, &why) == OMX_ERR_INVALID, "rate %g", fs);
        for (double hz : {0.0, -1.0, 24000.0, 1e9, (double)NAN, (double)INFINITY}) {
            spec.frequency_hz = hz;
            EXPECT(fl_design(&spec, 48000.0, &f, &why) == OMX_ERR_INVALID, "frequency %g", hz);
        }
        spec.frequency_hz = 100.0;
        for (uint32_t order : {0u, 3u, 5u, 8u}) {
            spec.order = order;
            EXPECT(fl_design(&spec, 48000.0, &f, &why) == OMX_ERR_INVALID, "order %u", order);
        }
        spec.order = 2;
        spec.kind = 9;
        EXPECT(fl_design(&spec, 48000.0, &f, &why) == OMX_ERR_INVALID, "kind 9");
        spec.kind = OMX_FILTER_PEAKING;
        spec.order = 0;
        spec.gain_db = (double)NAN;
        EXPECT(fl_design(&spec, 48000.0, &f, &why) == OMX_ERR_INVALID, "gain");
        f.n_sections = 1;
        f.section[0] = omx_program_filter_section{1.0, 0.0, 0.0, 0.0, 1.0};
        EXPECT(fl_check(&f, &why) == OMX_ERR_UNSUPPORTED, "a2 = 1");
        f.section[0] = omx_program_filter_section{1.0, 0.0, 0.0, 1.5, 0.5};
        EXPECT(fl_check(&f, &why) == OMX_ERR_UNSUPPORTED, "a1 = 1 + a2");
        f.section[0] = omx_program_filter_section{1.0, 0.0, 0.0, std::nextafter(1.5, 0.0), 0.5};
        EXPECT(fl_check(&f, &why) == OMX_NONE, "one ulp inside");
        f.section[0].b1 = (double)NAN;
        EXPECT(fl_check(&f, &why) == OMX_ERR_INVALID, "nan");
        f.n_sections = 3;
        EXPECT(fl_check(&f, &why) == OMX_ERR_INVALID && fl_cascade(&f, &f, &g, &why) == OMX_ERR_INVALID, "three sections");
        EXPECT(fl_check(nullptr, &why) == OMX_ERR_INVALID && fl_cascade(nullptr, &f, &g, &why) == OMX_ERR_INVALID, "null filter");
        omx_program_filter_info info;
        EXPECT(fl_plan(0, 48000.0, &info, &why) == OMX_ERR_INVALID && fl_plan(9, 48000.0, &info, &why) == OMX_ERR_INVALID &&
                   fl_plan(2, 0.0, &info, &why) == OMX_ERR_INVALID && fl_plan(2, 48000.0, nullptr, &why) == OMX_ERR_INVALID,
               "plan");
        EXPECT(fl_plan(8, 48000.0, &info, &why) == OMX_NONE && info.chunk_frames == kFlChunkFrames && info.streams_per_wavefront == 8, "plan of 8");
    }
    std::printf("designed %ld filters (%ld refused as unstable), checked %ld table sets: worst table error %.3e of the state's scale, largest "
                "rule figure %.3e against %.3e (%ld rejected)\n",
                designed, refused_unstable, tables, worst_table, worst_figure, 0x1p-25, rejected_by_rule);
    std::printf(failures ? "%d FAILURES\n" : "all agreed\n", failures);
    return failures ? 1 : 0;
}
