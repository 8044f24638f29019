// Stand-alone check of what the carried stages of the programme bank (resample, convolve, dynamics, the limiter) share on the host
// (openmeters_amd/csrc/program/program_carried.hpp), for a sanitizer run on the CPU: no device, no HIP, its own main.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/carried_ledger_check.cpp -o carried_ledger_check
//   ./carried_ledger_check
//
// 1. The sweep n_before 0 .. 40 x frames 0 .. 40 x latency 0 .. 9 x flush off / on: carry_emitted against the rule written out here;
//    a step and its commit keep E <= N and never lower E; a flushed entry refuses frames and accepts none; a refused step (frames
//    beyond the row, frames for a flushed stream, more than out_capacity to emit) leaves the entry and the step as they were.
// 2. Per latency, a programme cut into calls of 0, 1, latency and latency + 1 frames, in every order, and an empty flushing call: the
//    emitted counts add up to what one call and a flush emit.
// 3. carry_reset under a mask and carry_holds_frames.
// Prints what it compared; exit code 0 = everything agreed.
#include <cstdio>
#include <cstdlib>

#include "../openmeters_amd/csrc/program/program_carried.hpp"

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

struct Call {  // what carry_commit and carry_reset need of a stage's table entry
    uint32_t frames = 0, emit = 0, flags = 0;
};

static bool same(const CarryLedger& a, const CarryLedger& b) { return a.n == b.n && a.e == b.e && a.flushed == b.flushed; }

// One stream, one call through the shared step and commit: the frames emitted, or -1 for a refusal
static long long call(std::vector<CarryLedger>& ledger, uint32_t latency, uint32_t frames, bool flush, uint64_t frames_capacity = 1000,
                      uint64_t out_capacity = 1000) {
    const uint8_t mask = flush ? 1 : 0;
    const CarryLedger before = ledger[0];
    CarryStep step{777, 777, true};
    const auto emitted = [&](uint64_t n, uint64_t e, bool fl) { return carry_emitted(latency, n, e, fl); };
    const char* why = carry_step(ledger[0], &frames, frames_capacity, &mask, 0, out_capacity, emitted, step);
    if (why) {
        EXPECT(same(ledger[0], before) && step.frames == 777 && step.emit == 777 && step.flush, "a refusal (%s) wrote something", why);
        return -1;
    }
    std::vector<Call> calls(1);
    calls[0].frames = (uint32_t)step.frames;
    calls[0].emit = (uint32_t)step.emit;
    calls[0].flags = step.flush ? kCarryFlagFlush : 0u;
    carry_commit(ledger, calls);
    EXPECT(step.frames == frames && ledger[0].n == before.n + frames && ledger[0].e == before.e + step.emit, "the commit");
    EXPECT(ledger[0].e <= ledger[0].n && ledger[0].e >= before.e, "E %llu -> %llu of N %llu", (unsigned long long)before.e,
           (unsigned long long)ledger[0].e, (unsigned long long)ledger[0].n);
    EXPECT(ledger[0].flushed == (before.flushed || flush), "the flushed flag");
    return (long long)step.emit;
}

int main() {
    uint64_t rules = 0, steps = 0, refusals = 0, schedules = 0;

    // ---- 1. the sweep
    for (uint32_t latency = 0; latency <= 9; ++latency)
        for (uint32_t n_before = 0; n_before <= 40; ++n_before)
            for (uint32_t frames = 0; frames <= 40; ++frames)
                for (int flush = 0; flush <= 1; ++flush) {
                    // the entry of a running stream that has taken n_before frames, and the same stream flushed
                    const uint64_t e_before = n_before > latency ? n_before - latency : 0;
                    const uint64_t n = (uint64_t)n_before + frames;
                    const uint64_t ready = n > latency ? n - latency : 0;
                    const uint64_t want = flush ? n : (e_before > ready ? e_before : ready);
                    EXPECT(carry_emitted(latency, n, e_before, flush != 0) == want, "latency %u, N %u + %u, flush %d", latency, n_before, frames, flush);
                    ++rules;

                    std::vector<CarryLedger> running(1, CarryLedger{n_before, e_before, false});
                    const long long emit = call(running, latency, frames, flush != 0);
                    EXPECT(emit == (long long)(want - e_before), "a running stream: latency %u, N %u + %u, flush %d", latency, n_before, frames, flush);
                    ++steps;

                    std::vector<CarryLedger> flushed(1, CarryLedger{n_before, n_before, true});
                    const long long after = call(flushed, latency, frames, flush != 0);
                    EXPECT(after == (frames != 0 ? -1 : 0), "a flushed stream took %u frames: %lld", frames, after);
                    refusals += frames != 0;

                    // the other refusals: a count beyond the row, more to emit than d_out's rows hold
                    std::vector<CarryLedger> again(1, CarryLedger{n_before, e_before, false});
                    if (frames != 0) {
                        EXPECT(call(again, latency, frames, flush != 0, frames - 1) == -1, "frames[s] > frames_capacity went through");
                        ++refusals;
                    }
                    if (want != e_before) {
                        EXPECT(call(again, latency, frames, flush != 0, 1000, want - e_before - 1) == -1, "more than out_capacity went through");
                        ++refusals;
                    }
                    EXPECT(call(again, latency, frames, flush != 0, frames, want - e_before) == emit, "the tightest capacities were refused");
                }

    // ---- 2. cuts
    for (uint32_t latency = 0; latency <= 9; ++latency) {
        const uint32_t cuts[4] = {0, 1, latency, latency + 1};
        std::vector<CarryLedger> whole(1);
        const long long one = call(whole, latency, 2 * latency + 2, false) + call(whole, latency, 0, true);
        EXPECT(one == 2 * latency + 2 && whole[0].flushed, "one call and a flush emit every frame");
        int order[4] = {0, 1, 2, 3};
        do {
            std::vector<CarryLedger> cut(1);
            long long sum = 0;
            for (int k : order) sum += call(cut, latency, cuts[k], false);
            sum += call(cut, latency, 0, true);
            EXPECT(sum == one && same(cut[0], whole[0]), "latency %u, order %d %d %d %d: %lld of %lld", latency, order[0], order[1], order[2], order[3], sum, one);
            ++schedules;
        } while (std::next_permutation(order, order + 4));
    }

    // ---- 3. reset and configure's guard
    {
        std::vector<CarryLedger> ledger = {{5, 2, false}, {0, 0, false}, {7, 7, true}};
        std::vector<Call> calls(3);
        EXPECT(carry_holds_frames(ledger), "a ledger with frames");
        const uint8_t mask[3] = {0, 1, 1};
        carry_reset(ledger, calls, mask, [](const CarryLedger& m) { return Call{(uint32_t)m.n, 9, 9}; });
        EXPECT(same(ledger[0], CarryLedger{5, 2, false}) && calls[0].frames == 5 && calls[0].flags == 9, "an unmasked stream was reset");
        EXPECT(same(ledger[2], CarryLedger{}) && calls[2].frames == 7 && calls[2].flags == kCarryFlagClear, "a masked stream was not");
        EXPECT(carry_holds_frames(ledger), "stream 0 still holds frames");
        carry_reset(ledger, calls, nullptr, [](const CarryLedger&) { return Call{}; });
        EXPECT(!carry_holds_frames(ledger) && calls[0].flags == kCarryFlagClear && calls[1].flags == kCarryFlagClear, "a reset of every stream");
    }

    std::printf("carried_ledger_check: %llu rules, %llu steps, %llu refusals, %llu schedules; %d failures\n", (unsigned long long)rules,
                (unsigned long long)steps, (unsigned long long)refusals, (unsigned long long)schedules, failures);
    return failures == 0 ? 0 : 1;
}
