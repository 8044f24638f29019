// Stand-alone check of the host side of the programme bank's convolve stage (openmeters_amd/csrc/program/program_convolve_plan.hpp),
// for a sanitizer run on the CPU: no device, no HIP, its own main.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/convolve_design_check.cpp -o convolve_design_check
//   ./convolve_design_check
//
// 1. cv_design over every kind at tap counts 3 .. 4095 into a buffer of exactly n_taps floats between guard floats: symmetry on bits,
//    the tap sums (low-pass and band-stop 1, high-pass and band-pass 0, within T * 2^-24), the guards untouched, cv_check on the result;
//    every refusal with the buffer still holding its sentinel.
// 2. cv_response against a direct sum in long double at a few frequencies, the passband and stopband of a 255-tap low-pass, its
//    refusals with the outputs untouched.
// 3. cv_check on heap arrays of exactly n_taps floats (a read past the end would trip the sanitizer), and its refusals.
// 4. cv_frames against a frame-by-frame model of the streaming rule over random schedules, and its refusals; cv_plan.
// Prints what it compared; exit code 0 = everything agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "../openmeters_amd/csrc/program/program_convolve_plan.hpp"

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

int main() {
    std::mt19937_64 rng(20241021);
    const double fs = 48000.0;
    const float kGuard = 777.25f;

    // ---- 1. design
    uint64_t designs = 0, design_refusals = 0;
    const uint32_t tap_counts[] = {3, 5, 15, 63, 255, 1023, 4095};
    for (uint32_t kind = 0; kind <= OMX_CONVOLVE_BANDSTOP; ++kind)
        for (uint32_t T : tap_counts)
            for (double beta : {0.0, 6.0, 20.0}) {
                omx_program_convolve_spec spec{kind, T, 300.0 + (double)(rng() % 3000), 4000.0 + (double)(rng() % 19000), beta};
                std::vector<float> buf(T + 2, kGuard);
                const char* why = nullptr;
                const int rc = cv_design(&spec, fs, buf.data() + 1, T, &why);
                EXPECT(rc == OMX_NONE, "kind %u T %u: %s", kind, T, why ? why : "?");
                EXPECT(buf[0] == kGuard && buf[T + 1] == kGuard, "kind %u T %u: a guard was written", kind, T);
                double sum = 0.0;
                bool symmetric = true;
                for (uint32_t k = 0; k < T; ++k) {
                    sum += (double)buf[1 + k];
                    symmetric = symmetric && std::memcmp(&buf[1 + k], &buf[T - k], sizeof(float)) == 0;
                }
                const double want = (kind == OMX_CONVOLVE_LOWPASS || kind == OMX_CONVOLVE_BANDSTOP) ? 1.0 : 0.0;
                EXPECT(symmetric, "kind %u T %u: not symmetric on bits", kind, T);
                EXPECT(std::fabs(sum - want) <= (double)T * 0x1p-24, "kind %u T %u: tap sum %.9g", kind, T, sum);
                const omx_program_fir fir{buf.data() + 1, T, 0};
                EXPECT(cv_check(&fir, &why) == OMX_NONE, "kind %u T %u: check refuses the design", kind, T);
                ++designs;
            }
    {
        const omx_program_convolve_spec good{OMX_CONVOLVE_BANDPASS, 31, 300.0, 3400.0, 8.0};
        std::vector<omx_program_convolve_spec> bad;
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        for (uint32_t T : {0u, 1u, 2u, 30u, 4096u, 4097u, 0xFFFFFFFFu}) bad.push_back({good.kind, T, good.f_lo_hz, good.f_hi_hz, good.beta});
        bad.push_back({4u, 31, 300.0, 3400.0, 8.0});
        for (double f : {0.0, -1.0, 24000.0, nan, inf}) {
            bad.push_back({good.kind, 31, f, good.f_hi_hz, good.beta});
            bad.push_back({good.kind, 31, good.f_lo_hz, f, good.beta});
        }
        bad.push_back({good.kind, 31, 3400.0, 3400.0, 8.0});
        for (double b : {-0.5, 20.5, nan, inf}) bad.push_back({good.kind, 31, 300.0, 3400.0, b});
        for (const auto& spec : bad) {
            std::vector<float> buf(4100, kGuard);
            const char* why = nullptr;
            const int rc = cv_design(&spec, fs, buf.data(), spec.n_taps, &why);
            bool clean = true;
            for (float v : buf) clean = clean && v == kGuard;
            EXPECT(rc == OMX_ERR_INVALID && why && clean, "a bad spec (T %u) was not refused cleanly", spec.n_taps);
            ++design_refusals;
        }
        std::vector<float> buf(64, kGuard);
        const char* why = nullptr;
        for (double rate : {0.0, -1.0, nan, inf}) EXPECT(cv_design(&good, rate, buf.data(), 31, &why) == OMX_ERR_INVALID, "a bad rate");
        EXPECT(cv_design(&good, fs, buf.data(), 30, &why) == OMX_ERR_INVALID && cv_design(&good, fs, buf.data(), 32, &why) == OMX_ERR_INVALID,
               "n_floats != n_taps");
        EXPECT(cv_design(nullptr, fs, buf.data(), 31, &why) == OMX_ERR_INVALID && cv_design(&good, fs, nullptr, 31, &why) == OMX_ERR_INVALID,
               "a null pointer");
        bool clean = true;
        for (float v : buf) clean = clean && v == kGuard;
        EXPECT(clean, "a refusal wrote taps");
    }

    // ---- 2. response
    uint64_t responses = 0;
    {
        const omx_program_convolve_spec spec{OMX_CONVOLVE_LOWPASS, 255, 0.0, 8000.0, 9.0};
        std::vector<float> taps(255);
        const char* why = nullptr;
        EXPECT(cv_design(&spec, fs, taps.data(), 255, &why) == OMX_NONE, "the 255-tap low-pass");
        const omx_program_fir fir{taps.data(), 255, 0};
        for (double hz : {0.0, 1.0, 997.0, 7000.0, 8000.0, 9500.0, 12000.0, 23999.0, 24000.0, 50000.0}) {
            double db = 0.0, ph = 0.0;
            EXPECT(cv_response(&fir, fs, hz, &db, &ph, &why) == OMX_NONE, "response at %.0f Hz", hz);
            long double re = 0.0L, im = 0.0L;
            const long double w = 2.0L * 3.14159265358979323846264338327950288L * (long double)hz / (long double)fs;
            for (uint32_t k = 0; k < 255; ++k) {
                re += (long double)taps[k] * std::cos(w * (long double)k);
                im -= (long double)taps[k] * std::sin(w * (long double)k);
            }
            const double want = (double)(20.0L * std::log10(std::sqrt(re * re + im * im)));
            EXPECT(want < -80.0 || std::fabs(db - want) <= 1e-9, "%.0f Hz: %.12f dB against %.12f dB", hz, db, want);
            if (hz <= 7000.0) EXPECT(std::fabs(db) <= 0.01, "%.0f Hz lies in the passband: %.6f dB", hz, db);
            if (hz >= 9500.0 && hz <= 24000.0) EXPECT(db <= -80.0, "%.0f Hz lies in the stopband: %.3f dB", hz, db);
            ++responses;
        }
        double db = kGuard, ph = kGuard;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        EXPECT(cv_response(&fir, 0.0, 1.0, &db, &ph, &why) == OMX_ERR_INVALID && cv_response(&fir, fs, -1.0, &db, &ph, &why) == OMX_ERR_INVALID &&
                   cv_response(&fir, nan, 1.0, &db, &ph, &why) == OMX_ERR_INVALID && cv_response(nullptr, fs, 1.0, &db, &ph, &why) == OMX_ERR_INVALID &&
                   db == kGuard && ph == kGuard,
               "response refusals");
        EXPECT(cv_response(&fir, fs, 1.0, nullptr, nullptr, &why) == OMX_NONE, "null result pointers");
    }

    // ---- 3. check
    uint64_t checks = 0;
    for (uint32_t n : {1u, 2u, 7u, 4095u, 4096u}) {
        float* heap = new float[n];  // exactly n floats
        for (uint32_t k = 0; k < n; ++k) heap[k] = (float)((double)(rng() % 2001) / 1000.0 - 1.0);
        omx_program_fir fir{heap, n, 0};
        const char* why = nullptr;
        EXPECT(cv_check(&fir, &why) == OMX_NONE, "a good FIR of %u taps", n);
        heap[n - 1] = std::numeric_limits<float>::infinity();
        EXPECT(cv_check(&fir, &why) == OMX_ERR_INVALID, "an infinite last tap of %u", n);
        heap[n - 1] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(cv_check(&fir, &why) == OMX_ERR_INVALID, "a NaN last tap of %u", n);
        heap[n - 1] = 0.0f;
        fir.flags = 1;
        EXPECT(cv_check(&fir, &why) == OMX_ERR_INVALID, "a flag");
        fir.flags = 0;
        fir.n_taps = 0;
        EXPECT(cv_check(&fir, &why) == OMX_ERR_INVALID, "no taps");
        fir.n_taps = 4097;
        EXPECT(cv_check(&fir, &why) == OMX_ERR_INVALID, "too many taps (refused before any tap is read)");
        fir.taps = nullptr;
        fir.n_taps = n;
        EXPECT(cv_check(&fir, &why) == OMX_ERR_INVALID && cv_check(nullptr, &why) == OMX_ERR_INVALID, "null");
        delete[] heap;
        ++checks;
    }

    // ---- 4. frames and plan
    uint64_t schedules = 0;
    for (uint32_t trial = 0; trial < 2000; ++trial) {
        const uint32_t delay = (uint32_t)(rng() % 4) == 0 ? (uint32_t)(rng() % 4096) : (uint32_t)(rng() % 9);
        uint64_t n = 0, e = 0;
        const uint32_t calls = 1 + (uint32_t)(rng() % 8);
        for (uint32_t c = 0; c < calls; ++c) {
            const uint64_t f = rng() % 3 == 0 ? 0 : rng() % (2 * (uint64_t)delay + 40);
            const bool flush = c + 1 == calls;
            uint64_t got = ~0ull;
            const char* why = nullptr;
            EXPECT(cv_frames(delay, n, e, f, flush ? 1u : 0u, &got, &why) == OMX_NONE, "frames");
            // the model: a frame m is complete once frame m + delay has been taken, or at a flush
            uint64_t want = 0;
            for (uint64_t m = e; m < n + f; ++m) want += (flush || m + delay < n + f) ? 1 : 0;
            EXPECT(got == want, "delay %u n %llu e %llu f %llu flush %d: %llu against %llu", delay, (unsigned long long)n,
                   (unsigned long long)e, (unsigned long long)f, (int)flush, (unsigned long long)got, (unsigned long long)want);
            n += f;
            e += got;
        }
        EXPECT(e == n, "a flushed stream has emitted what it took");
        ++schedules;
    }
    {
        uint64_t out = 77;
        const char* why = nullptr;
        EXPECT(cv_frames(4096, 0, 0, 1, 0, &out, &why) == OMX_ERR_INVALID && cv_frames(1, (1ull << 63) + 1, 0, 0, 0, &out, &why) == OMX_ERR_INVALID &&
                   cv_frames(1, 1ull << 62, 0, 1ull << 63, 0, &out, &why) == OMX_ERR_INVALID && cv_frames(1, 5, 6, 1, 0, &out, &why) == OMX_ERR_INVALID &&
                   cv_frames(1, 0, 0, 1, 0, nullptr, &why) == OMX_ERR_INVALID && out == 77,
               "frames refusals");
        for (uint32_t ch = 1; ch <= 8; ++ch) {
            omx_program_convolve_info info{};
            EXPECT(cv_plan(ch, 4096, &info, &why) == OMX_NONE && info.channels == ch && info.tile_frames % (64 * info.frames_per_thread) == 0 &&
                       info.tap_block % info.frames_per_thread == 0,
                   "plan at %u channels", ch);
        }
        omx_program_convolve_info info{1, 2, 3, 4};
        EXPECT(cv_plan(0, 1, &info, &why) == OMX_ERR_INVALID && cv_plan(9, 1, &info, &why) == OMX_ERR_INVALID &&
                   cv_plan(2, 0, &info, &why) == OMX_ERR_INVALID && cv_plan(2, 4097, &info, &why) == OMX_ERR_INVALID &&
                   cv_plan(2, 1, nullptr, &why) == OMX_ERR_INVALID && info.tile_frames == 1 && info.channels == 4,
               "plan refusals");
    }

    std::printf("convolve_design_check: %llu designs, %llu design refusals, %llu responses, %llu checks, %llu schedules; %d failures\n",
                (unsigned long long)designs, (unsigned long long)design_refusals, (unsigned long long)responses, (unsigned long long)checks,
                (unsigned long long)schedules, failures);
    return failures == 0 ? 0 : 1;
}
