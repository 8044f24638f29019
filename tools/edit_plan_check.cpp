// Stand-alone check of the host side of the programme bank's edit pass (openmeters_amd/csrc/program/program_edit_plan.hpp), for a
// sanitizer run on the CPU: no device, no HIP, its own main.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/edit_plan_check.cpp -o edit_plan_check
//   ./edit_plan_check
//
// 1. Random clip tables (a fixed seed): ed_validate against a brute-force per-frame cover count and a plain restatement of every other
//    rule; for the accepted tables ed_build_spans against the same per-frame picture (which clips cover a frame, in table order, and
//    which fades apply there), ed_extent, and ed_window_counts of random windows against counts made frame by frame.
// 2. The phase: ed_phase against the product in 128-bit integers (it must fit 64 bits and give a p below 2^24 that lies within one
//    step of (i + 1/2) / F), and ed_gain against the table walked with plain integers.
// 3. ed_trim against its definition on random records.
// Prints what it compared; exit code 0 = everything agreed.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../openmeters_amd/csrc/program/program_edit_plan.hpp"

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

struct Frame {
    uint32_t n = 0;
    uint32_t clip[3] = {0, 0, 0};
    uint32_t flags = 0;
};

int main() {
    std::mt19937_64 rng(20240607);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };  // inclusive

    // ---- 1. tables
    const uint32_t kTables = 4000, kSpace = 256;
    uint64_t accepted = 0, refused = 0, spans_seen = 0, windows = 0;
    for (uint32_t trial = 0; trial < kTables; ++trial) {
        const uint32_t n_in = (uint32_t)pick(1, 3), n_out = (uint32_t)pick(1, 3);
        std::vector<uint32_t> frames_in(n_in);
        for (auto& f : frames_in) f = (uint32_t)pick(0, 60);
        std::vector<omx_program_edit_clip> clips;
        for (uint32_t o = 0; o < n_out; ++o) {
            uint64_t at = 0;
            const uint32_t count = (uint32_t)pick(0, 6);
            for (uint32_t k = 0; k < count; ++k) {
                omx_program_edit_clip c{};
                c.src_stream = (uint32_t)pick(0, n_in - 1);
                c.dst_stream = o;
                c.frames = pick(0, frames_in[c.src_stream]);
                c.src_first = pick(0, frames_in[c.src_stream] - c.frames);
                at += pick(0, 25);
                c.dst_first = at > 12 ? at - 12 : 0;  // mostly sorted, often overlapping
                if (trial % 5 != 4) c.dst_first = std::max<uint64_t>(c.dst_first, clips.empty() || clips.back().dst_stream != o ? 0 : clips.back().dst_first);
                c.fade_in_frames = (uint32_t)pick(0, c.frames);
                c.fade_out_frames = (uint32_t)pick(0, c.frames);
                c.fade_in_curve = (uint8_t)pick(0, 2);
                c.fade_out_curve = (uint8_t)pick(0, 2);
                c.gain = k % 2 ? 1.0f : 0.5f;
                if (trial % 97 == 96 && k == 1) c.fade_in_frames = (uint32_t)c.frames + 1;
                if (trial % 89 == 88 && k == 0) c.flags = 1;
                clips.push_back(c);
            }
        }
        // the brute-force picture
        bool ok = true;
        std::vector<std::vector<Frame>> picture(n_out, std::vector<Frame>(kSpace));
        for (size_t k = 0; k < clips.size() && ok; ++k) {
            const auto& c = clips[k];
            ok = c.flags == 0 && c.fade_in_frames <= c.frames && c.fade_out_frames <= c.frames && c.src_first + c.frames <= frames_in[c.src_stream];
            if (k && ok) ok = clips[k - 1].dst_stream < c.dst_stream || (clips[k - 1].dst_stream == c.dst_stream && clips[k - 1].dst_first <= c.dst_first);
            for (uint64_t j = 0; j < c.frames && ok; ++j) {
                Frame& f = picture[c.dst_stream][c.dst_first + j];
                if (f.n == 2) {
                    ok = false;
                    break;
                }
                if (j < c.fade_in_frames) f.flags |= f.n ? kEdFadeInB : kEdFadeInA;
                if (c.frames - 1 - j < c.fade_out_frames) f.flags |= f.n ? kEdFadeOutB : kEdFadeOutA;
                f.clip[f.n++] = (uint32_t)k;
            }
        }
        const char* why = ed_validate(clips.data(), clips.size(), n_in, frames_in.data(), 0, n_out);
        EXPECT((why == nullptr) == ok, "trial %u: validate says %s, brute force says %d", trial, why ? why : "fine", (int)ok);
        if (why || !ok) {
            ++refused;
            continue;
        }
        ++accepted;
        std::vector<EdSpan> spans;
        std::vector<uint32_t> begin;
        ed_build_spans(clips.data(), clips.size(), n_out, spans, begin);
        std::vector<uint64_t> extent(n_out);
        ed_extent(clips.data(), clips.size(), n_out, extent.data());
        uint64_t clip_at = 0;
        for (uint32_t o = 0; o < n_out; ++o) {
            const uint64_t clip_begin = clip_at;
            while (clip_at < clips.size() && clips[clip_at].dst_stream == o) ++clip_at;
            EXPECT(begin[o] < begin[o + 1] && spans[begin[o]].first == 0 && spans[begin[o + 1] - 1].end == kEdMaxPosition, "trial %u: ends", trial);
            uint64_t covered = 0;
            for (uint32_t i = begin[o]; i < begin[o + 1]; ++i) {
                const EdSpan& s = spans[i];
                ++spans_seen;
                EXPECT(s.first < s.end, "trial %u: an empty span", trial);
                if (i > begin[o]) {
                    const EdSpan& p = spans[i - 1];
                    EXPECT(p.end == s.first, "trial %u: a gap between spans", trial);
                    EXPECT(p.n_clips != s.n_clips || p.flags != s.flags || p.a != s.a || p.b != s.b, "trial %u: two equal neighbours", trial);
                }
                for (uint64_t x = s.first; x < std::min<uint64_t>(s.end, kSpace); ++x) {
                    const Frame& f = picture[o][x];
                    EXPECT(f.n == s.n_clips && f.flags == s.flags, "trial %u: output %u frame %lu: %u clips, flags %u, span says %u, %u", trial, o,
                           (unsigned long)x, f.n, f.flags, s.n_clips, s.flags);
                    if (f.n >= 1 && s.n_clips >= 1) EXPECT(f.clip[0] == s.a, "trial %u: first clip", trial);
                    if (f.n >= 2 && s.n_clips >= 2) EXPECT(f.clip[1] == s.b, "trial %u: second clip", trial);
                    if (f.n) covered = x + 1;
                }
            }
            EXPECT(covered == extent[o], "trial %u: extent %lu, brute force %lu", trial, (unsigned long)extent[o], (unsigned long)covered);
            for (int w = 0; w < 3; ++w) {
                const uint64_t first = pick(0, kSpace - 1), frames = pick(0, kSpace - first);
                EdStreamCall call{};
                ed_window_counts(clips.data(), clip_begin, clip_at, spans.data() + begin[o], begin[o + 1] - begin[o], first, frames, call);
                uint64_t silent = 0, faded = 0, mixed = 0;
                for (uint64_t x = first; x < first + frames; ++x) {
                    silent += picture[o][x].n == 0;
                    faded += picture[o][x].flags != 0;
                    mixed += picture[o][x].n == 2;
                }
                uint32_t touching = 0;
                for (uint64_t k = clip_begin; k < clip_at; ++k) {
                    bool touches = false;
                    for (uint64_t j = 0; j < clips[k].frames; ++j) touches = touches || (clips[k].dst_first + j >= first && clips[k].dst_first + j < first + frames);
                    touching += touches;
                }
                EXPECT(call.silent_frames == silent && call.faded_frames == faded && call.mixed_frames == mixed && call.clips == touching,
                       "trial %u: window counts", trial);
                ++windows;
            }
        }
    }
    std::printf("tables: %lu accepted, %lu refused, %lu spans and %lu windows against the per-frame picture\n", (unsigned long)accepted,
                (unsigned long)refused, (unsigned long)spans_seen, (unsigned long)windows);
    EXPECT(accepted > kTables / 4 && refused > kTables / 20, "the tables do not exercise both outcomes");

    // ---- 2. phase and gain
    std::vector<float> tabs((size_t)kEdCurves * kEdCurvePoints);
    for (uint32_t c = 0; c < kEdCurves; ++c) {
        ed_curve_table(c, tabs.data() + (size_t)c * kEdCurvePoints);
        for (uint32_t k = 0; k + 1 < kEdCurvePoints; ++k) EXPECT(tabs[c * kEdCurvePoints + k] <= tabs[c * kEdCurvePoints + k + 1], "curve %u falls at %u", c, k);
        EXPECT(tabs[c * kEdCurvePoints] == 0.0f && tabs[c * kEdCurvePoints + 4096] == 1.0f, "curve %u ends", c);
    }
    uint64_t phases = 0;
    const uint32_t fades[] = {1, 2, 3, 5, 63, 64, 65, 1000, 48000, (1u << 24) - 1, 1u << 24};
    for (const uint32_t fade : fades) {
        const uint64_t m = ed_fade_m(fade);
        const uint32_t count = fade <= 1000 ? fade : 20000;
        float before[kEdCurves] = {0.0f, 0.0f, 0.0f};
        uint64_t last_i = 0;
        for (uint32_t q = 0; q < count; ++q) {
            uint64_t i = fade <= 1000 ? q : (q == 0 ? 0 : (q == count - 1 ? fade - 1 : std::min<uint64_t>(fade - 1, last_i + 1 + rng() % (2 * (uint64_t)fade / count))));
            last_i = i;
            const unsigned __int128 wide = (unsigned __int128)(2 * i + 1) * m;
            EXPECT((wide >> 64) == 0, "F %u i %lu: the product leaves 64 bits", fade, (unsigned long)i);
            const uint64_t p = (uint64_t)(wide >> 40);
            EXPECT(p == ed_phase(m, i) && p < (1u << 24), "F %u i %lu: phase", fade, (unsigned long)i);
            const unsigned __int128 exact = ((unsigned __int128)(2 * i + 1) << 23) / fade;  // floor((i + 1/2) / F * 2^24)
            EXPECT(p <= exact && exact - p <= 1, "F %u i %lu: phase %lu against %lu", fade, (unsigned long)i, (unsigned long)p, (unsigned long)exact);
            for (uint32_t c = 0; c < kEdCurves; ++c) {
                const float* tab = tabs.data() + (size_t)c * kEdCurvePoints;
                const uint64_t k = p / 4096, low = p % 4096;
                const float a = tab[k], b = tab[k + 1];
                const float d = b - a;
                const float t = d * ((float)low / 4096.0f);
                const float want = a + t;
                const float got = ed_gain(tab, m, i);
                EXPECT(got == want && got >= 0.0f && got <= 1.0f && got >= before[c], "F %u i %lu curve %u: gain %.9g against %.9g", fade,
                       (unsigned long)i, c, (double)got, (double)want);
                before[c] = got;
            }
            ++phases;
        }
    }
    std::printf("phase and gain: %lu indices at %zu fade lengths, three curves\n", (unsigned long)phases, sizeof(fades) / sizeof(fades[0]));

    // ---- 3. trim
    uint64_t trims = 0;
    for (uint32_t trial = 0; trial < 20000; ++trial) {
        omx_program_inspect_record r{};
        r.frames = pick(0, 3000);
        r.leading_silence = pick(0, r.frames);
        r.trailing_silence = r.leading_silence == r.frames ? r.frames : pick(0, r.frames - r.leading_silence);
        omx_program_trim_rule rule{};
        rule.keep_head = pick(0, 4) ? pick(0, 500) : ~0ull;
        rule.keep_tail = pick(0, 500);
        rule.pad_head = pick(0, 100);
        rule.pad_tail = pick(0, 100);
        rule.fade_in_frames = (uint32_t)pick(0, 600);
        rule.fade_out_frames = (uint32_t)pick(0, 600);
        rule.fade_out_curve = 2;
        omx_program_edit_clip c{};
        uint64_t total = 0;
        const char* why = ed_trim(&r, &rule, 1, 2, &c, &total);
        EXPECT(why == nullptr, "trim trial %u refused: %s", trial, why ? why : "");
        if (why) continue;
        const uint64_t head = r.leading_silence == r.frames ? 0 : r.leading_silence - std::min(rule.keep_head, r.leading_silence);
        const uint64_t tail = r.leading_silence == r.frames ? 0 : r.trailing_silence - std::min(rule.keep_tail, r.trailing_silence);
        const uint64_t kept = r.leading_silence == r.frames ? 0 : r.frames - head - tail;
        EXPECT(c.frames == kept && c.src_first == head && c.dst_first == rule.pad_head && total == rule.pad_head + kept + rule.pad_tail, "trim trial %u", trial);
        EXPECT(c.fade_in_frames == std::min<uint64_t>(rule.fade_in_frames, kept) && c.fade_out_frames == std::min<uint64_t>(rule.fade_out_frames, kept) &&
                   c.gain == 1.0f && c.src_stream == 1 && c.dst_stream == 2 && c.fade_out_curve == 2,
               "trim trial %u: fades", trial);
        const uint32_t have[2] = {0, (uint32_t)r.frames};
        EXPECT(ed_validate(&c, 1, 2, have, 0, 3) == nullptr, "trim trial %u: the clip is refused", trial);
        ++trims;
    }
    std::printf("trim: %lu records\n", (unsigned long)trims);
    std::printf(failures ? "%d FAILURES\n" : "all agreed\n", failures);
    return failures ? 1 : 0;
}
