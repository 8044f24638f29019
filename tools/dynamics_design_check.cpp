// Stand-alone check of the host side of the programme bank's dynamics stage (openmeters_amd/csrc/program/program_dynamics_plan.hpp),
// for a sanitizer run on the CPU: no device, no HIP, its own main.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/dynamics_design_check.cpp -o dynamics_design_check
//   ./dynamics_design_check
//
// 1. The tables: LOG and EXP against long double log2 / exp2 (within one unit: the literals are exact, the library functions are not),
//    monotone, their ends exact.
// 2. dy_design and dy_from_points into a curve that lies between guard words on the heap: every entry inside the gain limits, the
//    guards and the curve's other fields untouched, the shape (no gain below the threshold, the slope above it, the expander's range,
//    slope 1 outside the points), dy_check on the result; every refusal with the curve still holding its sentinel.
// 3. dy_gain_db at every table level (the entry itself), between entries (inside the neighbours) and far outside the table (the end
//    entries: the lerp never reads T[769]); its refusals.
// 4. dy_time, dy_latency, dy_plan and their refusals; dy_frames against a frame-by-frame model of the streaming rule over random
//    schedules, and its refusals.
// Prints what it compared; exit code 0 = everything agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "../openmeters_amd/csrc/program/program_dynamics_plan.hpp"

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

constexpr uint32_t kGuard = 0xA5A5A5A5u;
struct Guarded {  // a curve between guard words, on the heap: a write outside it trips the sanitizer or a guard
    uint32_t before[2];
    omx_program_dynamics_curve curve;
    uint32_t after[2];
};

std::unique_ptr<Guarded> sentinel_curve() {
    auto g = std::make_unique<Guarded>();
    std::memset(g.get(), 0xA5, sizeof(Guarded));
    return g;
}
bool untouched(const Guarded& g) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&g);
    for (size_t i = 0; i < sizeof(Guarded); ++i)
        if (p[i] != 0xA5) return false;
    return true;
}
bool only_table_written(const Guarded& g) {
    return g.before[0] == kGuard && g.before[1] == kGuard && g.after[0] == kGuard && g.after[1] == kGuard && g.curve.detector_mask == kGuard &&
           g.curve.attack_frames == kGuard && g.curve.hold_frames == kGuard && g.curve.release_step == (int64_t)0xA5A5A5A5A5A5A5A5ull;
}
double entry_db(const omx_program_dynamics_curve& c, uint32_t k) { return (double)c.T[k] / 65536.0 * kDyOctave; }

}  // namespace

int main() {
    std::mt19937_64 rng(20241021);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- 1. tables
    for (uint32_t i = 0; i <= 256; ++i) {
        const long double lg = 65536.0L * log2l(1.0L + (long double)i / 256.0L), ex = exp2l(40.0L + (long double)i / 256.0L);
        EXPECT(std::fabs((double)((long double)kDyLog[i] - floorl(lg))) <= 1.0, "LOG[%u]", i);
        EXPECT(std::fabs((double)((long double)kDyExp[i] - floorl(ex))) <= 1.0, "EXP[%u]", i);
        if (i != 0) EXPECT(kDyLog[i] > kDyLog[i - 1] && kDyExp[i] > kDyExp[i - 1], "tables not monotone at %u", i);
    }
    EXPECT(kDyLog[0] == 0 && kDyLog[256] == 65536 && kDyExp[0] == (1ull << 40) && kDyExp[256] == (1ull << 41), "table ends");

    // ---- 2. design and points
    uint64_t designs = 0, refusals = 0;
    for (double threshold : {-60.0, -20.0, -3.0, 12.0})
        for (double ratio : {1.0, 2.0, 4.0, 20.0, inf})
            for (double knee : {0.0, 6.0, 24.0})
                for (double expander_ratio : {1.0, 2.0, 10.0}) {
                    const double range = (rng() & 1) ? 24.0 : inf, makeup = (double)(rng() % 13) - 3.0, et = threshold - 25.0;
                    const omx_program_dynamics_spec spec{threshold, ratio, knee, et, expander_ratio, range, makeup};
                    auto g = sentinel_curve();
                    const char* why = nullptr;
                    EXPECT(dy_design(&spec, &g->curve, &why) == OMX_NONE, "design: %s", why ? why : "?");
                    EXPECT(only_table_written(*g), "design wrote outside the table");
                    EXPECT(dy_table_ok(g->curve.T), "design left an entry beyond the limits");
                    ++designs;
                    const double lim = 40.0 * kDyOctave;
                    for (uint32_t k = 0; k < OMX_DYNAMICS_CURVE_POINTS; ++k) {
                        const double x = dy_entry_level_db(k), got = entry_db(g->curve, k), half = kDyOctave / 65536.0;
                        double want;
                        const bool in_knee = knee > 0.0 && std::fabs(2.0 * (x - threshold)) <= knee;
                        if (in_knee) continue;  // (the quadratic is checked at its ends by the two branches beside it)
                        want = x > threshold ? (1.0 / ratio - 1.0) * (x - threshold) : 0.0;
                        if (expander_ratio != 1.0 && x < et) want += std::max((x - et) * (expander_ratio - 1.0), -range);
                        want = std::min(std::max(want + makeup, -lim), lim);
                        EXPECT(std::fabs(got - want) <= half, "design entry %u: %.9f against %.9f", k, got, want);
                    }
                    g->curve.detector_mask = 1;
                    g->curve.attack_frames = 1;
                    g->curve.hold_frames = 0;
                    g->curve.release_step = 1;
                    EXPECT(dy_check(&g->curve, &why) == OMX_NONE, "check of a designed curve: %s", why ? why : "?");
                }
    {
        const omx_program_dynamics_spec good{-20.0, 4.0, 6.0, -60.0, 2.0, 24.0, 0.0};
        omx_program_dynamics_spec bad[12];
        for (auto& b : bad) b = good;
        bad[0].threshold_db = nan, bad[1].threshold_db = 49.0, bad[2].ratio = 0.5, bad[3].ratio = nan, bad[4].knee_db = -1.0, bad[5].knee_db = inf;
        bad[6].expander_ratio = 0.9, bad[7].expander_ratio = inf, bad[8].expander_threshold_db = -241.0, bad[9].range_db = -1.0;
        bad[10].range_db = nan, bad[11].makeup_db = inf;
        for (const auto& b : bad) {
            auto g = sentinel_curve();
            const char* why = nullptr;
            EXPECT(dy_design(&b, &g->curve, &why) == OMX_ERR_INVALID && why && untouched(*g), "a bad spec was not refused cleanly");
            ++refusals;
        }
        auto g = sentinel_curve();
        EXPECT(dy_design(nullptr, &g->curve, nullptr) == OMX_ERR_INVALID && dy_design(&good, nullptr, nullptr) == OMX_ERR_INVALID && untouched(*g), "null");
        omx_program_dynamics_spec off = good;
        off.expander_ratio = 1.0;
        off.expander_threshold_db = nan;  // not looked at without an expander
        EXPECT(dy_design(&off, &g->curve, nullptr) == OMX_NONE, "an unused expander threshold was looked at");
    }
    uint64_t point_sets = 0;
    for (uint32_t n = 1; n <= OMX_DYNAMICS_MAX_POINTS; ++n) {
        std::unique_ptr<omx_program_dynamics_point[]> pts(new omx_program_dynamics_point[n]);  // exactly n: a read past it trips the sanitizer
        double in = -90.0 - (double)(rng() % 40);
        for (uint32_t i = 0; i < n; ++i) {
            in += 0.5 + (double)(rng() % 1200) / 100.0;
            pts[i] = {in, in + (double)(rng() % 4000) / 100.0 - 20.0};
        }
        auto g = sentinel_curve();
        const char* why = nullptr;
        EXPECT(dy_from_points(pts.get(), n, &g->curve, &why) == OMX_NONE, "points: %s", why ? why : "?");
        EXPECT(only_table_written(*g) && dy_table_ok(g->curve.T), "points wrote outside the table or beyond the limits");
        const double half = kDyOctave / 65536.0;
        for (uint32_t k = 0; k < OMX_DYNAMICS_CURVE_POINTS; ++k) {
            const double x = dy_entry_level_db(k), got = entry_db(g->curve, k);
            if (x <= pts[0].in_db) EXPECT(std::fabs(got - (pts[0].out_db - pts[0].in_db)) <= half, "slope 1 below the points at %u", k);
            if (x >= pts[n - 1].in_db) EXPECT(std::fabs(got - (pts[n - 1].out_db - pts[n - 1].in_db)) <= half, "slope 1 above the points at %u", k);
            for (uint32_t i = 0; i + 1 < n; ++i)
                if (x >= pts[i].in_db && x <= pts[i + 1].in_db) {
                    const double a = pts[i].out_db - pts[i].in_db, b = pts[i + 1].out_db - pts[i + 1].in_db;
                    EXPECT(got >= std::min(a, b) - half && got <= std::max(a, b) + half, "between points %u and %u at %u", i, i + 1, k);
                }
        }
        ++point_sets;
    }
    {
        omx_program_dynamics_point two[2] = {{-40.0, -40.0}, {-20.0, -30.0}};
        auto g = sentinel_curve();
        const char* why = nullptr;
        EXPECT(dy_from_points(two, 0, &g->curve, &why) == OMX_ERR_INVALID && untouched(*g), "n = 0");
        EXPECT(dy_from_points(two, 17, &g->curve, &why) == OMX_ERR_INVALID && untouched(*g), "n = 17");
        EXPECT(dy_from_points(nullptr, 2, &g->curve, &why) == OMX_ERR_INVALID && dy_from_points(two, 2, nullptr, &why) == OMX_ERR_INVALID, "null");
        two[1].in_db = -40.0;
        EXPECT(dy_from_points(two, 2, &g->curve, &why) == OMX_ERR_INVALID && untouched(*g), "in_db not increasing");
        two[1].in_db = nan;
        EXPECT(dy_from_points(two, 2, &g->curve, &why) == OMX_ERR_INVALID && untouched(*g), "a NaN point");
        two[1] = {-20.0, inf};
        EXPECT(dy_from_points(two, 2, &g->curve, &why) == OMX_ERR_INVALID && untouched(*g), "an infinite point");
        refusals += 7;
    }

    // ---- 3. gain
    uint64_t gains = 0;
    {
        auto c = std::make_unique<omx_program_dynamics_curve>();
        for (uint32_t k = 0; k < OMX_DYNAMICS_CURVE_POINTS; ++k) c->T[k] = (int32_t)(rng() % (2 * OMX_DYNAMICS_MAX_GAIN + 1)) - OMX_DYNAMICS_MAX_GAIN;
        for (uint32_t k = 0; k < OMX_DYNAMICS_CURVE_POINTS; ++k) {
            EXPECT(dy_curve_at(c->T, kDyLMin + 4096 * (int32_t)k) == c->T[k], "the entry itself at %u", k);
            if (k + 1 < OMX_DYNAMICS_CURVE_POINTS)
                for (int32_t f : {1, 2047, 2048, 4095}) {
                    const int32_t v = dy_curve_at(c->T, kDyLMin + 4096 * (int32_t)k + f);
                    EXPECT(v >= std::min(c->T[k], c->T[k + 1]) && v <= std::max(c->T[k], c->T[k + 1]), "between entries %u and %u", k, k + 1);
                    ++gains;
                }
        }
        double g = 777.25;
        const char* why = nullptr;
        for (double level : {-inf, -1000.0, -240.9, (double)kDyLMin / 65536.0 * kDyOctave}) {
            EXPECT(dy_gain_db(c.get(), level, &g, &why) == OMX_NONE && g == (double)c->T[0] * (kDyOctave / 65536.0), "below the table at %g", level);
        }
        for (double level : {inf, 1000.0, 48.2, (double)kDyLMax / 65536.0 * kDyOctave}) {
            EXPECT(dy_gain_db(c.get(), level, &g, &why) == OMX_NONE && g == (double)c->T[768] * (kDyOctave / 65536.0), "above the table at %g", level);
        }
        g = 777.25;
        EXPECT(dy_gain_db(c.get(), nan, &g, &why) == OMX_ERR_INVALID && g == 777.25, "a NaN level");
        EXPECT(dy_gain_db(nullptr, 0.0, &g, &why) == OMX_ERR_INVALID && dy_gain_db(c.get(), 0.0, nullptr, &why) == OMX_ERR_INVALID, "null");
        c->T[5] = OMX_DYNAMICS_MAX_GAIN + 1;
        EXPECT(dy_gain_db(c.get(), 0.0, &g, &why) == OMX_ERR_INVALID && g == 777.25, "an entry beyond the limit");
        c->detector_mask = 1, c->attack_frames = 1, c->hold_frames = 0, c->release_step = 1;
        EXPECT(dy_check(c.get(), &why) == OMX_ERR_INVALID, "check of an entry beyond the limit");
        c->T[5] = -OMX_DYNAMICS_MAX_GAIN;
        EXPECT(dy_check(c.get(), &why) == OMX_NONE, "check: %s", why ? why : "?");
        uint32_t lat = 777;
        for (int field = 0; field < 7; ++field) {
            omx_program_dynamics_curve b = *c;
            if (field == 0) b.detector_mask = 0;
            if (field == 1) b.detector_mask = 256;
            if (field == 2) b.attack_frames = 0;
            if (field == 3) b.attack_frames = 4097;
            if (field == 4) b.hold_frames = 16385;
            if (field == 5) b.release_step = 0;
            if (field == 6) b.release_step = OMX_DYNAMICS_MAX_STEP + 1;
            EXPECT(dy_check(&b, &why) == OMX_ERR_INVALID && dy_latency(&b, &lat, &why) == OMX_ERR_INVALID && lat == 777, "check field %d", field);
            ++refusals;
        }
        c->attack_frames = 4096, c->hold_frames = 16384, c->release_step = OMX_DYNAMICS_MAX_STEP, c->detector_mask = 255;
        EXPECT(dy_check(c.get(), &why) == OMX_NONE && dy_latency(c.get(), &lat, &why) == OMX_NONE && lat == 4095, "the largest curve");
        EXPECT(dy_latency(c.get(), nullptr, &why) == OMX_ERR_INVALID && dy_check(nullptr, &why) == OMX_ERR_INVALID, "null");
    }

    // ---- 4. time, plan, frames
    {
        uint32_t a = 7, h = 7;
        int64_t d = 7;
        const char* why = nullptr;
        EXPECT(dy_time(48000.0, 1.0, 10.0, 60.0, &a, &h, &d, &why) == OMX_NONE && a == 48 && h == 480 && d == 891723, "time: %u %u %lld", a, h, (long long)d);
        EXPECT(dy_time(48000.0, 0.0, 0.0, inf, &a, &h, &d, &why) == OMX_NONE && a == 1 && h == 0 && d == OMX_DYNAMICS_MAX_STEP, "time at the ends");
        EXPECT(dy_time(48000.0, 0.0, 0.0, 1e-9, &a, nullptr, &d, &why) == OMX_NONE && d == 1, "the smallest step");
        a = h = 7, d = 7;
        const double bad[][4] = {{0.0, 1, 1, 1}, {nan, 1, 1, 1}, {inf, 1, 1, 1}, {48000, -1, 1, 1}, {48000, nan, 1, 1}, {48000, 1, -1, 1}, {48000, 1, inf, 1},
                                 {48000, 85.4, 1, 1}, {48000, 1, 341.4, 1}, {48000, 1, 1, 0}, {48000, 1, 1, -3}, {48000, 1, 1, nan}};
        for (const auto& b : bad) {
            EXPECT(dy_time(b[0], b[1], b[2], b[3], &a, &h, &d, &why) == OMX_ERR_INVALID && a == 7 && h == 7 && d == 7, "time refusal");
            ++refusals;
        }
        omx_program_dynamics_info info;
        std::memset(&info, 0xA5, sizeof(info));
        EXPECT(dy_plan(0, &info, &why) == OMX_ERR_INVALID && dy_plan(9, &info, &why) == OMX_ERR_INVALID && info.channels == kGuard, "plan refusals");
        EXPECT(dy_plan(2, nullptr, &why) == OMX_ERR_INVALID, "plan null");
        for (uint32_t ch = 1; ch <= 8; ++ch) {
            EXPECT(dy_plan(ch, &info, &why) == OMX_NONE && info.channels == ch && info.release_tile == kDyReleaseTile && info._pad == 0, "plan %u", ch);
            // the apply pass's LDS at the longest attack fits the 64 KiB a launch may ask for
            const uint32_t per = ((info.smooth_tile + OMX_DYNAMICS_MAX_ATTACK - 1 + kDyThreads - 1) / kDyThreads) | 1u;
            EXPECT((kDyThreads * per + 4 + info.smooth_tile + 258 + 24) * 8 + info.smooth_tile * 4 <= 65536, "apply LDS");
        }
    }
    uint64_t schedules = 0;
    for (int trial = 0; trial < 200; ++trial) {
        static const uint32_t kFirst[4] = {0, 1, 4095, 63};
        const uint32_t latency = trial < 4 ? kFirst[trial] : (uint32_t)(rng() % 4096);
        uint64_t n = 0, e = 0;
        bool flushed = false;
        for (int call = 0; call < 12 && !flushed; ++call) {
            const uint64_t f = (rng() % 3 == 0) ? 0 : rng() % (2 * (uint64_t)latency + 50);
            const bool flush = call == 11 || rng() % 9 == 0;
            uint64_t got = 777;
            const char* why = nullptr;
            EXPECT(dy_frames(latency, n, e, f, flush ? 1 : 0, &got, &why) == OMX_NONE, "frames: %s", why ? why : "?");
            // frame by frame: frame j is emitted once frame j + latency has been taken, or with the flush
            uint64_t model = 0;
            for (uint64_t j = e; j < n + f; ++j)
                if (flush || j + latency < n + f) ++model;
            EXPECT(got == model, "frames %u: n %llu e %llu f %llu flush %d: %llu against %llu", latency, (unsigned long long)n, (unsigned long long)e,
                   (unsigned long long)f, (int)flush, (unsigned long long)got, (unsigned long long)model);
            n += f;
            e += got;
            flushed = flush;
            ++schedules;
        }
        EXPECT(e == n, "a flushed stream has emitted everything");
    }
    {
        uint64_t out = 777;
        const char* why = nullptr;
        EXPECT(dy_frames(4096, 0, 0, 1, 0, &out, &why) == OMX_ERR_INVALID && out == 777, "latency above 4095");
        EXPECT(dy_frames(1, (1ull << 63) + 1, 0, 0, 0, &out, &why) == OMX_ERR_INVALID && out == 777, "n beyond 2^63");
        EXPECT(dy_frames(1, 1ull << 62, 0, 1ull << 63, 0, &out, &why) == OMX_ERR_INVALID && out == 777, "n + f beyond 2^63");
        EXPECT(dy_frames(1, 5, 6, 1, 0, &out, &why) == OMX_ERR_INVALID && out == 777, "e above n");
        EXPECT(dy_frames(1, 0, 0, 1, 0, nullptr, &why) == OMX_ERR_INVALID, "null");
        refusals += 5;
    }

    std::printf("dynamics_design_check: %llu designs, %llu point sets, %llu gains between entries, %llu streaming calls, %llu refusals; %d failures\n",
                (unsigned long long)designs, (unsigned long long)point_sets, (unsigned long long)gains, (unsigned long long)schedules,
                (unsigned long long)refusals, failures);
    return failures == 0 ? 0 : 1;
}
