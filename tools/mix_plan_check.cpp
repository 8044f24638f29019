// Stand-alone check of the host side of the programme bank's mix pass (openmeters_amd/csrc/program/program_mix_plan.hpp), for a
// sanitizer run on the CPU: no device, no HIP, its own main.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/mix_plan_check.cpp -o mix_plan_check
//   ./mix_plan_check
//
// 1. Random send tables (a fixed seed; shallow ones, and deep ones that pile up to 70 sends over a frame): mx_validate against a
//    brute-force per-frame list of the covering sends and a plain restatement of every other rule; for the accepted tables
//    mx_build_spans against the same per-frame picture (which sends cover a frame, in table order), mx_extent, and mx_window_counts
//    of random windows against counts made frame by frame.
// 2. mx_null against its definition, its refusals, and its table through mx_validate.
// Prints what it compared; exit code 0 = everything agreed.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../openmeters_amd/csrc/program/program_mix_plan.hpp"

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
    std::mt19937_64 rng(20240921);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };  // inclusive

    // ---- 1. tables
    const uint32_t kTables = 3000, kSpace = 256;
    uint64_t accepted = 0, refused = 0, too_deep = 0, spans_seen = 0, layers_seen = 0, windows = 0;
    uint32_t deepest = 0;
    for (uint32_t trial = 0; trial < kTables; ++trial) {
        const bool deep = trial % 4 == 3;
        const uint32_t n_in = (uint32_t)pick(1, 3), n_out = (uint32_t)pick(1, 3);
        std::vector<uint32_t> frames_in(n_in);
        for (auto& f : frames_in) f = (uint32_t)pick(deep ? 40 : 0, 60);
        std::vector<omx_program_mix_send> sends;
        for (uint32_t o = 0; o < n_out; ++o) {
            uint64_t at = 0;
            const uint32_t count = (uint32_t)(deep ? pick(50, 70) : pick(0, 7));
            for (uint32_t k = 0; k < count; ++k) {
                omx_program_mix_send c{};
                c.src_stream = (uint32_t)pick(0, n_in - 1);
                c.dst_bus = o;
                c.frames = deep ? pick(frames_in[c.src_stream] * 3 / 4, frames_in[c.src_stream]) : pick(0, frames_in[c.src_stream]);
                c.src_first = pick(0, frames_in[c.src_stream] - c.frames);
                at += deep ? pick(0, 1) * pick(0, 1) : pick(0, 25);
                c.dst_first = deep ? at : (at > 12 ? at - 12 : 0);  // mostly sorted, often overlapping
                if (trial % 5 != 4) c.dst_first = std::max<uint64_t>(c.dst_first, sends.empty() || sends.back().dst_bus != o ? 0 : sends.back().dst_first);
                c.gain = k % 3 == 0 ? 1.0f : (k % 3 == 1 ? -0.5f : 0.25f);
                if (trial % 97 == 96 && k == 1) c.gain = std::numeric_limits<float>::infinity();
                if (trial % 89 == 88 && k == 0) c.flags = 1;
                if (trial % 83 == 82 && k == 0) c.src_first = frames_in[c.src_stream] - c.frames + 1;
                sends.push_back(c);
            }
        }
        // the brute-force picture: the sends over every frame, in table order
        bool ok = true, depth_ok = true;
        std::vector<std::vector<std::vector<uint32_t>>> picture(n_out, std::vector<std::vector<uint32_t>>(kSpace));
        for (size_t k = 0; k < sends.size() && ok; ++k) {
            const auto& c = sends[k];
            ok = c.flags == 0 && std::isfinite(c.gain) && c.src_first + c.frames <= frames_in[c.src_stream];
            if (k && ok) ok = sends[k - 1].dst_bus < c.dst_bus || (sends[k - 1].dst_bus == c.dst_bus && sends[k - 1].dst_first <= c.dst_first);
            for (uint64_t j = 0; j < c.frames && ok; ++j) {
                auto& f = picture[c.dst_bus][c.dst_first + j];
                if (f.size() == kMxMaxLayers) {
                    ok = depth_ok = false;
                    break;
                }
                f.push_back((uint32_t)k);
            }
        }
        const char* why = mx_validate(sends.data(), sends.size(), n_in, frames_in.data(), 0, n_out);
        EXPECT((why == nullptr) == ok, "trial %u: validate says %s, brute force says %d", trial, why ? why : "fine", (int)ok);
        if (why || !ok) {
            ++refused;
            too_deep += !depth_ok;
            continue;
        }
        ++accepted;
        std::vector<MxSpan> spans;
        std::vector<uint32_t> list, begin;
        mx_build_spans(sends.data(), sends.size(), n_out, spans, list, begin);
        std::vector<uint64_t> extent(n_out);
        mx_extent(sends.data(), sends.size(), n_out, extent.data());
        uint64_t send_at = 0;
        for (uint32_t o = 0; o < n_out; ++o) {
            const uint64_t send_begin = send_at;
            while (send_at < sends.size() && sends[send_at].dst_bus == o) ++send_at;
            EXPECT(begin[o] < begin[o + 1] && spans[begin[o]].first == 0 && spans[begin[o + 1] - 1].end == kMxMaxPosition, "trial %u: ends", trial);
            uint64_t covered = 0;
            for (uint32_t i = begin[o]; i < begin[o + 1]; ++i) {
                const MxSpan& s = spans[i];
                ++spans_seen;
                layers_seen += s.n_layers;
                deepest = std::max(deepest, s.n_layers);
                EXPECT(s.first < s.end, "trial %u: an empty span", trial);
                EXPECT(s.n_layers <= kMxMaxLayers && (size_t)s.list_begin + s.n_layers <= list.size(), "trial %u: a list out of range", trial);
                if (i > begin[o]) EXPECT(spans[i - 1].end == s.first, "trial %u: a gap between spans", trial);
                for (uint64_t x = s.first; x < std::min<uint64_t>(s.end, kSpace); ++x) {
                    const auto& f = picture[o][x];
                    EXPECT(f.size() == s.n_layers, "trial %u: bus %u frame %lu: %zu sends, span says %u", trial, o, (unsigned long)x, f.size(), s.n_layers);
                    for (uint32_t q = 0; q < s.n_layers && q < f.size(); ++q)
                        EXPECT(list[s.list_begin + q] == f[q], "trial %u: bus %u frame %lu layer %u", trial, o, (unsigned long)x, q);
                    if (!f.empty()) covered = x + 1;
                }
            }
            EXPECT(covered == extent[o], "trial %u: extent %lu, brute force %lu", trial, (unsigned long)extent[o], (unsigned long)covered);
            for (int w = 0; w < 3; ++w) {
                const uint64_t first = pick(0, kSpace - 1), frames = pick(0, kSpace - first);
                MxBusCall call{};
                mx_window_counts(sends.data(), send_begin, send_at, spans.data() + begin[o], begin[o + 1] - begin[o], first, frames, call);
                uint64_t silent = 0, mixed = 0;
                uint32_t layers = 0;
                for (uint64_t x = first; x < first + frames; ++x) {
                    silent += picture[o][x].empty();
                    mixed += picture[o][x].size() >= 2;
                    layers = std::max<uint32_t>(layers, (uint32_t)picture[o][x].size());
                }
                uint32_t touching = 0;
                for (uint64_t k = send_begin; k < send_at; ++k) {
                    bool touches = false;
                    for (uint64_t j = 0; j < sends[k].frames; ++j) touches = touches || (sends[k].dst_first + j >= first && sends[k].dst_first + j < first + frames);
                    touching += touches;
                }
                EXPECT(call.silent_frames == silent && call.mixed_frames == mixed && call.sends == touching && call.max_layers == layers,
                       "trial %u: window counts", trial);
                ++windows;
            }
        }
    }
    std::printf("tables: %lu accepted, %lu refused (%lu for a 65th layer), %lu spans with %lu layers (deepest %u) and %lu windows against the per-frame picture\n",
                (unsigned long)accepted, (unsigned long)refused, (unsigned long)too_deep, (unsigned long)spans_seen, (unsigned long)layers_seen, deepest,
                (unsigned long)windows);
    EXPECT(accepted > kTables / 4 && refused > kTables / 20 && too_deep > 20 && deepest == kMxMaxLayers, "the tables do not exercise every outcome");

    // ---- 2. the null test's table
    uint64_t nulls = 0;
    for (uint32_t trial = 0; trial < 5000; ++trial) {
        const uint32_t n = (uint32_t)pick(1, 63), ref = (uint32_t)pick(0, 70), bus = (uint32_t)pick(0, 9);
        const uint64_t frames = pick(0, 4) ? pick(0, 5000) : kMxMaxPosition;
        std::vector<uint32_t> stems(n);
        for (auto& s : stems) s = (uint32_t)pick(0, 70);
        std::vector<omx_program_mix_send> out(n + 1);
        const char* why = mx_null(stems.data(), n, ref, frames, bus, out.data());
        EXPECT(why == nullptr, "null trial %u refused: %s", trial, why ? why : "");
        if (why) continue;
        for (uint32_t i = 0; i <= n; ++i)
            EXPECT(out[i].src_stream == (i < n ? stems[i] : ref) && out[i].dst_bus == bus && out[i].src_first == 0 && out[i].dst_first == 0 &&
                       out[i].frames == frames && out[i].gain == (i < n ? 1.0f : -1.0f) && out[i].flags == 0,
                   "null trial %u send %u", trial, i);
        if (frames <= 5000) {
            std::vector<uint32_t> have(71, (uint32_t)frames);
            EXPECT(mx_validate(out.data(), out.size(), 71, have.data(), 0, 10) == nullptr, "null trial %u: the table is refused", trial);
        }
        ++nulls;
    }
    {
        uint32_t stems[64] = {0};
        omx_program_mix_send out[65];
        EXPECT(mx_null(nullptr, 3, 0, 1, 0, out) && mx_null(stems, 3, 0, 1, 0, nullptr) && mx_null(stems, 0, 0, 1, 0, out) &&
                   mx_null(stems, 64, 0, 1, 0, out) && mx_null(stems, 3, 0, kMxMaxPosition + 1, 0, out),
               "a null-test table that should have been refused");
    }
    std::printf("null test: %lu tables\n", (unsigned long)nulls);
    std::printf(failures ? "%d FAILURES\n" : "all agreed\n", failures);
    return failures ? 1 : 0;
}
