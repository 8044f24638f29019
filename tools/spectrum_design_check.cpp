// Stand-alone check of the host side of the programme bank's spectrum stage (openmeters_amd/csrc/program/program_spectrum_plan.hpp),
// for a sanitizer run on the CPU: no device, no HIP, its own main.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/spectrum_design_check.cpp -o spectrum_design_check
//   ./spectrum_design_check
//
// 1. Defaults, plan and window at every size, sp_transforms against the grid's own words for every frame count up to 3 N; their
//    refusals with the outputs still holding sentinels.
// 2. sp_density of a synthetic record into a heap array of exactly N/2 + 1 doubles (a write beyond it trips the sanitizer): Parseval
//    against a direct DFT of one windowed frame; its refusals.
// 3. sp_bands: a sine's level in its third-octave band, the octave bands of a flat density add up to what lies between their outer
//    edges, a capacity that is too small; sp_summarize: a flat density, a tone on a floor, a band-limited density; refusals.
// 4. sp_match: flat against flat gives a unit impulse, a tilt gives mirrored taps whose response follows the wanted gain, the limits
//    hold; every refusal with the taps untouched.
// Prints what it compared; exit code 0 = everything agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "../openmeters_amd/csrc/program/program_spectrum_plan.hpp"

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

namespace {

template <class T>
bool all_bytes(const T* p, size_t count, unsigned char byte) {
    const unsigned char* q = reinterpret_cast<const unsigned char*>(p);
    for (size_t i = 0; i < count * sizeof(T); ++i)
        if (q[i] != byte) return false;
    return true;
}

void check_plan_and_grid() {
    const char* why = nullptr;
    omx_program_spectrum_rule rule;
    EXPECT(sp_rule_default(&rule, &why) == OMX_NONE && rule.fft_size == 4096 && rule.flags == 0, "rule default");
    EXPECT(sp_rule_default(nullptr, &why) == OMX_ERR_INVALID && why, "null rule");
    omx_program_spectrum_qc qc;
    EXPECT(sp_qc_default(&qc, &why) == OMX_NONE && qc.n_probes == 6 && qc.probe_hz[3] == 60.0 && sp_qc_ok(&qc), "qc default");
    EXPECT(sp_qc_default(nullptr, &why) == OMX_ERR_INVALID, "null qc");
    omx_program_spectrum_match_spec spec;
    EXPECT(sp_match_spec_default(48000.0, &spec, &why) == OMX_NONE && spec.high_hz == 0.45 * 48000.0 && sp_spec_ok(&spec, 48000.0), "spec");
    EXPECT(sp_match_spec_default(0.0, &spec, &why) == OMX_ERR_INVALID && sp_match_spec_default(48000.0, nullptr, &why) == OMX_ERR_INVALID,
           "spec refusals");
    const uint32_t sizes[3] = {2048, 4096, 8192};
    for (uint32_t n : sizes) {
        omx_program_spectrum_rule r{n, 0};
        omx_program_spectrum_info info;
        EXPECT(sp_plan(&r, 2, 64, 1u << 20, &info, &why) == OMX_NONE, "plan %u", n);
        EXPECT(info.hop == n / 2 && info.bins == n / 2 + 1 && info.threads == 256 && info.run == OMX_SPECTRUM_RUN, "plan fields %u", n);
        EXPECT(info.transforms_per_workgroup * (n / 32) == 256, "transforms per workgroup %u", n);
        EXPECT(info.lds_bytes > 0 && info.lds_bytes <= 160 * 1024, "lds %u", n);
        EXPECT(info.scratch_bytes >= 64ull * 2 * ((1u << 20) / (n / 2) / OMX_SPECTRUM_RUN) * info.bins * 8, "scratch %u", n);
        std::unique_ptr<float[]> w(new float[n]);
        EXPECT(sp_window(n, w.get(), &why) == OMX_NONE && w[0] == 0.0f && w[n / 2] == 1.0f && w[1] == w[n - 1], "window %u", n);
        EXPECT(std::fabs(sp_window_power(n) - 0.375 * n) < 1e-3, "window power %u: %.17g", n, sp_window_power(n));
        for (uint64_t frames = 0; frames <= 3ull * n; ++frames)
            for (uint32_t fin = 0; fin < 2; ++fin) {
                uint64_t brute = 0, got = ~0ull;
                while (fin ? brute * (n / 2) < frames : brute * (n / 2) + n - 1 < frames) ++brute;
                EXPECT(sp_transforms(frames, fin, n, &got, &why) == OMX_NONE && got == brute, "transforms %llu %u %u",
                       (unsigned long long)frames, fin, n);
            }
    }
    omx_program_spectrum_info info;
    std::memset(&info, 0xA5, sizeof(info));
    omx_program_spectrum_rule good{4096, 0}, bad_size{1024, 0}, big{16384, 0}, flagged{4096, 1};
    EXPECT(sp_plan(&bad_size, 2, 1, 0, &info, &why) == OMX_ERR_INVALID && sp_plan(&big, 2, 1, 0, &info, &why) == OMX_ERR_INVALID &&
               sp_plan(&flagged, 2, 1, 0, &info, &why) == OMX_ERR_INVALID && sp_plan(nullptr, 2, 1, 0, &info, &why) == OMX_ERR_INVALID &&
               sp_plan(&good, 0, 1, 0, &info, &why) == OMX_ERR_INVALID && sp_plan(&good, 9, 1, 0, &info, &why) == OMX_ERR_INVALID &&
               sp_plan(&good, 2, 1, 1ull << 32, &info, &why) == OMX_ERR_INVALID && sp_plan(&good, 2, 1, 0, nullptr, &why) == OMX_ERR_INVALID,
           "plan refusals");
    EXPECT(all_bytes(&info, 1, 0xA5), "a refused plan wrote");
    float w4[4];
    std::memset(w4, 0xA5, sizeof(w4));
    uint64_t count = 0xA5A5A5A5A5A5A5A5ull;
    EXPECT(sp_window(1000, w4, &why) == OMX_ERR_INVALID && sp_window(4096, nullptr, &why) == OMX_ERR_INVALID && all_bytes(w4, 4, 0xA5),
           "window refusals");
    EXPECT(sp_transforms(5, 0, 1000, &count, &why) == OMX_ERR_INVALID && sp_transforms(1ull << 32, 0, 2048, &count, &why) == OMX_ERR_INVALID &&
               sp_transforms(5, 0, 2048, nullptr, &why) == OMX_ERR_INVALID && count == 0xA5A5A5A5A5A5A5A5ull,
           "transforms refusals");
    std::printf("plan, window, transforms: 3 sizes, every frame count up to 3 N\n");
}

void check_density() {
    const char* why = nullptr;
    const uint32_t n = 2048, bins = n / 2 + 1;
    std::unique_ptr<float[]> w(new float[n]);
    sp_window(n, w.get(), &why);
    // one windowed frame of two sines and an offset, its spectrum by a direct DFT in double
    std::unique_ptr<double[]> y(new double[n]), sums(new double[2 * bins]), dens(new double[bins]);
    double energy = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        y[i] = (double)w[i] * (0.1 + 0.5 * std::sin(2.0 * kSpPi * 100.25 * i / n) + 0.25 * std::cos(2.0 * kSpPi * 700.0 * i / n));
        energy += y[i] * y[i];
    }
    for (uint32_t b = 0; b < bins; ++b) {
        double re = 0.0, im = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const double a = 2.0 * kSpPi * (double)(((uint64_t)b * i) % n) / n;
            re += y[i] * std::cos(a);
            im -= y[i] * std::sin(a);
        }
        sums[b] = 0.0;
        sums[bins + b] = 3.0 * (re * re + im * im);
    }
    omx_program_spectrum_record rec{};
    rec.fft_size = n;
    rec.channels = 2;
    rec.transforms[1] = 3;
    EXPECT(sp_density(&rec, sums.get(), 1, dens.get(), &why) == OMX_NONE, "density");
    double total = 0.0;
    for (uint32_t b = 0; b < bins; ++b) total += dens[b];
    EXPECT(std::fabs(total - energy / sp_window_power(n)) <= 1e-12 * total, "Parseval: %.17g against %.17g", total, energy / sp_window_power(n));
    EXPECT(sp_density(&rec, sums.get(), 0, dens.get(), &why) == OMX_NONE && all_bytes(dens.get(), bins, 0), "no transforms: zeros");
    std::memset(dens.get(), 0xA5, bins * sizeof(double));
    omx_program_spectrum_record bad = rec;
    bad.fft_size = 1000;
    EXPECT(sp_density(&bad, sums.get(), 0, dens.get(), &why) == OMX_ERR_INVALID, "bad size");
    bad = rec;
    bad.channels = 9;
    EXPECT(sp_density(&bad, sums.get(), 0, dens.get(), &why) == OMX_ERR_INVALID, "bad channels");
    EXPECT(sp_density(&rec, sums.get(), 2, dens.get(), &why) == OMX_ERR_INVALID && sp_density(nullptr, sums.get(), 0, dens.get(), &why) == OMX_ERR_INVALID &&
               sp_density(&rec, nullptr, 0, dens.get(), &why) == OMX_ERR_INVALID && sp_density(&rec, sums.get(), 0, nullptr, &why) == OMX_ERR_INVALID,
           "density refusals");
    EXPECT(all_bytes(dens.get(), bins, 0xA5), "a refused density wrote");
    std::printf("density: Parseval to %.3g relative\n", std::fabs(total - energy / sp_window_power(n)) / total);
}

void check_bands_and_summary() {
    const char* why = nullptr;
    const uint32_t n = 4096, bins = n / 2 + 1;
    const double fs = 48000.0, df = fs / n;
    std::unique_ptr<double[]> d(new double[bins]);
    for (uint32_t b = 0; b < bins; ++b) d[b] = 1e-6;
    double centre[OMX_SPECTRUM_MAX_BANDS], level[OMX_SPECTRUM_MAX_BANDS];
    uint32_t count = OMX_SPECTRUM_MAX_BANDS;
    EXPECT(sp_bands(d.get(), n, fs, 1, centre, level, &count, &why) == OMX_NONE && count >= 8 && count <= 10, "octave bands: %u", count);
    // adjacent octave bands tile the axis: their powers add up to the flat density between the outer edges
    double power = 0.0;
    for (uint32_t i = 0; i < count; ++i) power += std::pow(10.0, level[i] / 10.0) / 2.0;
    const double lo = centre[0] * std::pow(10.0, -0.15), hi = centre[count - 1] * std::pow(10.0, 0.15);
    EXPECT(std::fabs(power - 1e-6 * (hi - lo) / df) <= 1e-9 * power, "octave tiling: %.17g against %.17g", power, 1e-6 * (hi - lo) / df);
    for (uint32_t i = 0; i + 1 < count; ++i) EXPECT(std::fabs(centre[i + 1] / centre[i] - std::pow(10.0, 0.3)) < 1e-12, "octave ratio");
    uint32_t third = OMX_SPECTRUM_MAX_BANDS;
    EXPECT(sp_bands(d.get(), n, fs, 3, centre, level, &third, &why) == OMX_NONE && third > 2 * count && third <= OMX_SPECTRUM_MAX_BANDS, "thirds %u", third);
    for (uint32_t i = 0; i < third; ++i)
        EXPECT(centre[i] * std::pow(10.0, -0.05) >= 4.0 * df && centre[i] * std::pow(10.0, 0.05) <= fs / 2.0, "a listed band outside the range");
    // a sine of amplitude 0.5 at bin 85 (996 Hz): all of its power 0.125 in the 1 kHz band
    for (uint32_t b = 0; b < bins; ++b) d[b] = 0.0;
    d[85] = 0.125;
    third = OMX_SPECTRUM_MAX_BANDS;
    sp_bands(d.get(), n, fs, 3, centre, level, &third, &why);
    bool found = false;
    for (uint32_t i = 0; i < third; ++i)
        if (std::fabs(centre[i] - 1000.0) < 1e-9) {
            found = true;
            EXPECT(std::fabs(level[i] - 10.0 * std::log10(0.25)) < 1e-12, "1 kHz band: %.17g", level[i]);
        } else {
            EXPECT(level[i] == kSpFloor, "an empty band above the floor");
        }
    EXPECT(found, "no 1 kHz band");
    double c2[2] = {-1.0, -1.0}, l2[2] = {-1.0, -1.0};
    uint32_t two = 2;
    EXPECT(sp_bands(d.get(), n, fs, 3, c2, l2, &two, &why) == OMX_ERR_INVALID && two == 2 && c2[0] == -1.0 && l2[1] == -1.0, "capacity");
    two = OMX_SPECTRUM_MAX_BANDS;
    EXPECT(sp_bands(d.get(), n, fs, 2, centre, level, &two, &why) == OMX_ERR_INVALID && sp_bands(d.get(), 1000, fs, 3, centre, level, &two, &why) == OMX_ERR_INVALID &&
               sp_bands(d.get(), n, 100.0, 3, centre, level, &two, &why) == OMX_ERR_INVALID && sp_bands(nullptr, n, fs, 3, centre, level, &two, &why) == OMX_ERR_INVALID &&
               sp_bands(d.get(), n, fs, 3, centre, level, nullptr, &why) == OMX_ERR_INVALID,
           "bands refusals");
    d[7] = -1.0;
    EXPECT(sp_bands(d.get(), n, fs, 3, centre, level, &two, &why) == OMX_ERR_INVALID, "negative density");
    d[7] = std::nan("");
    EXPECT(sp_bands(d.get(), n, fs, 3, centre, level, &two, &why) == OMX_ERR_INVALID && two == OMX_SPECTRUM_MAX_BANDS, "NaN density");

    omx_program_spectrum_qc qc;
    sp_qc_default(&qc, &why);
    omx_program_spectrum_summary s;
    for (uint32_t b = 0; b < bins; ++b) d[b] = 1e-6;
    EXPECT(sp_summarize(&qc, d.get(), n, fs, &s, &why) == OMX_NONE && s.verdict == 0 && s.occupied_hz > 0.99 * fs / 2, "flat: verdict %u", s.verdict);
    for (uint32_t i = 0; i < 6; ++i) EXPECT(s.prominence_db[i] == 0.0, "flat prominence");
    d[5] = 1e-2;  // 58.6 Hz: nearest to the 60 Hz probe
    d[4] = d[6] = 2.5e-3;
    EXPECT(sp_summarize(&qc, d.get(), n, fs, &s, &why) == OMX_NONE && (s.verdict & OMX_SPECTRUM_TONE) && s.prominence_db[3] > 20.0, "tone: %g", s.prominence_db[3]);
    EXPECT(std::fabs(s.peak_hz - 5.0 * df) < 1e-9 && s.peak_db > 10.0 * std::log10(2e-2) - 1e-9, "peak %.17g %.17g", s.peak_hz, s.peak_db);
    for (uint32_t b = 0; b < bins; ++b) d[b] = b * df < 15000.0 ? 1e-6 : 1e-14;
    EXPECT(sp_summarize(&qc, d.get(), n, fs, &s, &why) == OMX_NONE && (s.verdict & OMX_SPECTRUM_BANDLIMITED) && s.occupied_hz < 15100.0 && s.occupied_hz > 14900.0,
           "band-limited: %g", s.occupied_hz);
    for (uint32_t b = 0; b < bins; ++b) d[b] = 0.0;
    EXPECT(sp_summarize(&qc, d.get(), n, fs, &s, &why) == OMX_NONE && s.verdict == 0 && s.total_db == kSpFloor && s.peak_db == kSpFloor && s.occupied_hz == 0.0, "silence");
    std::memset(&s, 0xA5, sizeof(s));
    omx_program_spectrum_qc bad = qc;
    bad.occupied_fraction = 0.0;
    EXPECT(sp_summarize(&bad, d.get(), n, fs, &s, &why) == OMX_ERR_INVALID, "occupied_fraction 0");
    bad = qc;
    bad.n_probes = 9;
    EXPECT(sp_summarize(&bad, d.get(), n, fs, &s, &why) == OMX_ERR_INVALID, "9 probes");
    bad = qc;
    bad.probe_hz[2] = -1.0;
    EXPECT(sp_summarize(&bad, d.get(), n, fs, &s, &why) == OMX_ERR_INVALID, "negative probe");
    bad = qc;
    bad.tone_db = std::nan("");
    EXPECT(sp_summarize(&bad, d.get(), n, fs, &s, &why) == OMX_ERR_INVALID, "NaN tone_db");
    bad = qc;
    bad.flags = 1;
    EXPECT(sp_summarize(&bad, d.get(), n, fs, &s, &why) == OMX_ERR_INVALID && sp_summarize(nullptr, d.get(), n, fs, &s, &why) == OMX_ERR_INVALID &&
               sp_summarize(&qc, nullptr, n, fs, &s, &why) == OMX_ERR_INVALID && sp_summarize(&qc, d.get(), n, fs, nullptr, &why) == OMX_ERR_INVALID &&
               sp_summarize(&qc, d.get(), 512, fs, &s, &why) == OMX_ERR_INVALID && sp_summarize(&qc, d.get(), n, -1.0, &s, &why) == OMX_ERR_INVALID,
           "summarize refusals");
    EXPECT(all_bytes(&s, 1, 0xA5), "a refused summarize wrote");
    std::printf("bands and summary: %u octave and %u third-octave bands at %u points\n", count, third, n);
}

void check_match() {
    const char* why = nullptr;
    const uint32_t n = 4096, bins = n / 2 + 1, taps_n = 1023, mid = taps_n / 2;
    const double fs = 48000.0, df = fs / n;
    std::unique_ptr<double[]> flat(new double[bins]), tilt(new double[bins]);
    for (uint32_t b = 0; b < bins; ++b) {
        flat[b] = 1e-6;
        tilt[b] = 1e-6 * std::pow(std::fmax(b * df, 20.0) / 1000.0, -1.0);  // -3 dB per octave
    }
    omx_program_spectrum_match_spec spec;
    sp_match_spec_default(fs, &spec, &why);
    std::unique_ptr<float[]> taps(new float[taps_n]);  // exactly n_taps floats on the heap
    EXPECT(sp_match(flat.get(), flat.get(), n, fs, &spec, taps.get(), taps_n, &why) == OMX_NONE, "flat match");
    double rest = 0.0;
    for (uint32_t i = 0; i < taps_n; ++i)
        if (i != mid) rest = std::fmax(rest, std::fabs((double)taps[i]));
    EXPECT(std::fabs(taps[mid] - 1.0f) < 1e-6f && rest < 1e-9, "flat against flat: centre %.9g, the rest up to %.3g", taps[mid], rest);
    EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &spec, taps.get(), taps_n, &why) == OMX_NONE, "tilt match");
    for (uint32_t m = 1; m <= mid; ++m) EXPECT(std::memcmp(&taps[mid + m], &taps[mid - m], 4) == 0, "halves do not mirror at %u", m);
    double worst = 0.0;
    for (double f = 100.0; f <= 10000.0; f *= 1.25) {  // the response against the wanted gain, -3 dB per octave
        double re = (double)taps[mid];
        for (uint32_t m = 1; m <= mid; ++m) re += 2.0 * (double)taps[mid + m] * std::cos(2.0 * kSpPi * f / fs * m);
        worst = std::fmax(worst, std::fabs(20.0 * std::log10(std::fabs(re)) - 10.0 * std::log10(1000.0 / f)));
    }
    EXPECT(worst < 0.25, "response off the wanted gain by %.3f dB", worst);
    spec.max_boost_db = 1.0;
    spec.max_cut_db = 2.0;
    sp_match(flat.get(), tilt.get(), n, fs, &spec, taps.get(), taps_n, &why);
    double lo_gain = 0.0, hi_gain = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        const double f = pass ? 12000.0 : 50.0;
        double re = (double)taps[mid];
        for (uint32_t m = 1; m <= mid; ++m) re += 2.0 * (double)taps[mid + m] * std::cos(2.0 * kSpPi * f / fs * m);
        (pass ? hi_gain : lo_gain) = 20.0 * std::log10(std::fabs(re));
    }
    EXPECT(std::fabs(lo_gain - 1.0) < 0.3 && std::fabs(hi_gain + 2.0) < 0.1, "limits: %.3f and %.3f dB", lo_gain, hi_gain);
    float one[1];
    EXPECT(sp_match(flat.get(), flat.get(), n, fs, &spec, one, 1, &why) == OMX_NONE && std::fabs(one[0] - 1.0f) < 1e-6f, "one tap: %.9g", one[0]);

    sp_match_spec_default(fs, &spec, &why);
    std::memset(taps.get(), 0xA5, taps_n * sizeof(float));
    const uint32_t bad_taps[4] = {0, 1022, 4097, 4096};
    for (uint32_t t : bad_taps) EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &spec, taps.get(), t, &why) == OMX_ERR_INVALID, "n_taps %u", t);
    EXPECT(sp_match(flat.get(), tilt.get(), 2048, fs, &spec, taps.get(), 2049, &why) == OMX_ERR_INVALID, "n_taps not below fft_size");
    omx_program_spectrum_match_spec bad = spec;
    bad.max_boost_db = -1.0;
    EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &bad, taps.get(), taps_n, &why) == OMX_ERR_INVALID, "negative boost");
    bad = spec;
    bad.high_hz = 30000.0;
    EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &bad, taps.get(), taps_n, &why) == OMX_ERR_INVALID, "high_hz above fs / 2");
    bad = spec;
    bad.low_hz = bad.high_hz;
    EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &bad, taps.get(), taps_n, &why) == OMX_ERR_INVALID, "low_hz == high_hz");
    bad = spec;
    bad.low_hz = 100.0;
    bad.high_hz = 105.0;  // no bin between them
    EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &bad, taps.get(), taps_n, &why) == OMX_ERR_INVALID, "no bin in the band");
    bad = spec;
    bad.flags = 2;
    EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &bad, taps.get(), taps_n, &why) == OMX_ERR_INVALID &&
               sp_match(nullptr, tilt.get(), n, fs, &spec, taps.get(), taps_n, &why) == OMX_ERR_INVALID &&
               sp_match(flat.get(), nullptr, n, fs, &spec, taps.get(), taps_n, &why) == OMX_ERR_INVALID &&
               sp_match(flat.get(), tilt.get(), n, fs, nullptr, taps.get(), taps_n, &why) == OMX_ERR_INVALID &&
               sp_match(flat.get(), tilt.get(), n, fs, &spec, nullptr, taps_n, &why) == OMX_ERR_INVALID &&
               sp_match(flat.get(), tilt.get(), 1000, fs, &spec, taps.get(), 255, &why) == OMX_ERR_INVALID &&
               sp_match(flat.get(), tilt.get(), n, 0.0, &spec, taps.get(), taps_n, &why) == OMX_ERR_INVALID,
           "match refusals");
    tilt[9] = std::numeric_limits<double>::infinity();
    EXPECT(sp_match(flat.get(), tilt.get(), n, fs, &spec, taps.get(), taps_n, &why) == OMX_ERR_INVALID, "infinite density");
    EXPECT(all_bytes(taps.get(), taps_n, 0xA5), "a refused match wrote");
    std::printf("match: %u taps, response within %.3f dB of the wanted gain\n", taps_n, worst);
}

}  // namespace

int main() {
    check_plan_and_grid();
    check_density();
    check_bands_and_summary();
    check_match();
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("spectrum host functions: every check agreed\n");
    return 0;
}
