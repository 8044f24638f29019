// What the stages of the programme loudness bank that carry state from call to call (resample, convolve, dynamics, the limiter) share on
// the host: the ledger of a stream (frames taken, frames emitted, flushed), the emitted-frames rule of a fixed latency, the head of a
// call's per-stream loop with its refusals, the commit behind the last check, and the loops of a reset and of configure's guard.
// Plain C++, no device and no HIP: tools/carried_ledger_check.cpp drives this file alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace omx {

// Flag bits of a call table's entry (the uploaded tables only, never the ABI); a stage's own flags go above them
constexpr uint32_t kCarryFlagClear = 1u;  // the record is cleared before anything else (a reset)
constexpr uint32_t kCarryFlagFlush = 2u;  // nothing is taken at and beyond the last frame; the stream is flushed afterwards

// What the host mirrors of one stream
struct CarryLedger {
    uint64_t n = 0, e = 0;  // N frames taken, E frames emitted
    bool flushed = false;
};

// E' of a stream of fixed latency with N frames taken (E emitted before), flushed or not
inline uint64_t carry_emitted(uint64_t latency, uint64_t n, uint64_t e, bool flush) {
    if (flush) return n;
    return std::max<uint64_t>(e, n > latency ? n - latency : 0);
}

// The frames stream s brings to a call: frames[s], or the whole row where the call gives no counts.  Null, or why the count is refused
// (pl_stream_frames of program_stage.hpp is this rule under pl_refuse, for the stages that carry nothing).
inline const char* carry_frames_of(const uint32_t* frames, uint64_t frames_capacity, uint32_t s, uint64_t& f) {
    f = frames ? frames[s] : frames_capacity;
    return f > frames_capacity ? "frames[s] > frames_capacity" : nullptr;
}

// What a call does to one stream's ledger
struct CarryStep {
    uint64_t frames = 0;  // F: frames taken
    uint64_t emit = 0;    // E' - E: frames emitted
    bool flush = false;
};

// The head of a call's per-stream loop: stream s brings frames[s] frames (the whole row where the call gives no counts) and emits up to
// emitted(N', E, flush).  Null, or why the call is refused; nothing but `step` is written.
template <class Emitted>
inline const char* carry_step(const CarryLedger& m, const uint32_t* frames, uint64_t frames_capacity, const uint8_t* flush_mask, uint32_t s,
                              uint64_t out_capacity, Emitted&& emitted, CarryStep& step) {
    uint64_t f;
    if (const char* why = carry_frames_of(frames, frames_capacity, s, f)) return why;
    if (f != 0 && m.flushed) return "frames for a flushed stream (reset it first)";
    const bool flush = m.flushed || (flush_mask && flush_mask[s]);
    const uint64_t e_new = emitted(m.n + f, m.e, flush);
    if (e_new - m.e > out_capacity) return "a stream would emit more than out_capacity frames";
    step = CarryStep{f, e_new - m.e, flush};
    return nullptr;
}

// What a call's steps add up to: whether any stream takes or emits a frame, and the longest of each
struct CarryTotals {
    bool any_in = false, any_out = false;
    uint32_t max_frames = 0, max_emit = 0;
    void take(const CarryStep& step) {
        any_in = any_in || step.frames != 0;
        any_out = any_out || step.emit != 0;
        max_frames = std::max(max_frames, (uint32_t)step.frames);
        max_emit = std::max(max_emit, (uint32_t)step.emit);
    }
    bool null_pcm(const void* d_in, const void* d_out) const { return (any_in && !d_in) || (any_out && !d_out); }
};

// Behind a call's last check: the ledger takes what the call's table says.  Entry is CarryLedger or begins with one.
template <class Entry, class Call>
inline void carry_commit(std::vector<Entry>& ledger, const std::vector<Call>& calls) {
    for (size_t s = 0; s < ledger.size(); ++s) {
        CarryLedger& m = ledger[s];
        m.n += calls[s].frames;
        m.e += calls[s].emit;
        m.flushed = (calls[s].flags & kCarryFlagFlush) != 0;
    }
}

// configure's guard: a stream has taken frames since its reset
template <class Entry>
inline bool carry_holds_frames(const std::vector<Entry>& ledger) {
    return std::any_of(ledger.begin(), ledger.end(), [](const CarryLedger& m) { return m.n != 0; });
}

// The table of a reset: blank(entry) per stream, with the ledger cleared and the clear flag set where the mask (null: everywhere) says so
template <class Entry, class Call, class Blank>
inline void carry_reset(std::vector<Entry>& ledger, std::vector<Call>& calls, const uint8_t* reset_mask, Blank&& blank) {
    for (size_t s = 0; s < ledger.size(); ++s) {
        Call c = blank(ledger[s]);
        if (!reset_mask || reset_mask[s]) {
            static_cast<CarryLedger&>(ledger[s]) = CarryLedger{};
            c.flags = kCarryFlagClear;
        }
        calls[s] = c;
    }
}

}  // namespace omx
