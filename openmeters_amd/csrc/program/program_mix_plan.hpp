// Everything of the programme bank's mix pass (include/omx/program_mix.h states the definition) that needs no device: the validation
// of a send table (one pass, the cover depth tracked with a heap of ends), the null-test table, and the cut of every bus into SPANS,
// the runs of bus frames between neighbouring send boundaries, each with the list of the sends that cover it in table order.  Free of
// HIP on purpose: a stand-alone CPU program (tools/mix_plan_check.cpp) includes this file alone.  Host work is
// O(sends log sends + sum of layers over the spans), never O(frames).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <queue>
#include <vector>

#include "../../../include/omx/program_mix.h"

namespace omx {

constexpr uint32_t kMxThreads = 256;        // threads per workgroup of the main kernel
constexpr uint32_t kMxLayersPerBatch = 4;   // sources whose loads are in flight together
constexpr uint32_t kMxMaxLayers = OMX_MIX_MAX_LAYERS;
constexpr uint64_t kMxMaxSends = OMX_MIX_MAX_SENDS;
constexpr uint64_t kMxMaxPosition = OMX_MIX_MAX_POSITION;

// Bus frames of a tile: 8 KiB of PCM per workgroup (6 to 8 at the channel counts that do not divide it), that is two 16-byte vectors
// per thread; with four layers in a batch eight vector loads (128 B) per thread are in flight before the batch's first add, as many
// as the edit pass holds, and the eight f64 accumulators of the two vectors cost 16 registers.
constexpr uint32_t mx_tile_frames(uint32_t channels) { return channels == 1 ? 2048 : (channels == 2 ? 1024 : (channels <= 4 ? 512 : 256)); }
// 16-byte vectors a thread holds per layer: every vector of a full tile in one round
constexpr uint32_t mx_in_flight(uint32_t channels) { return (mx_tile_frames(channels) * channels / 4 + kMxThreads - 1) / kMxThreads; }

// A send as the kernel reads it
struct MxSend {
    uint64_t dst_first;
    uint64_t src_base;  // src_stream * frames_capacity + src_first: the frame of d_in that lands at dst_first
    float gain;
    uint32_t _pad;
};
static_assert(sizeof(MxSend) == 24, "MxSend is part of the call's blob");

// Bus frames [first, end) under the same sends: entries [list_begin, list_begin + n_layers) of the call's index list, table indices in
// table order.  The spans of a bus lie one behind the other and tile [0, 2^40).
struct MxSpan {
    uint64_t first, end;
    uint32_t list_begin;
    uint32_t n_layers;  // 0: zero fill
};
static_assert(sizeof(MxSpan) == 24, "MxSpan is part of the call's blob");

// What one call does to one bus; the counts of the record follow from the spans and the window on the host
struct MxBusCall {
    uint64_t out_first;
    uint32_t out_frames;
    uint32_t span_begin;  // the bus's spans: [span_begin, span_begin + span_count) of the call's span list
    uint32_t span_count;
    uint32_t sends;       // sends that touch the window
    uint64_t silent_frames, mixed_frames;
    uint32_t max_layers;
    uint32_t _pad;
};
static_assert(sizeof(MxBusCall) == 48, "MxBusCall is part of the call's blob");

// ---------------------------------------------------------------- validation
// nullptr, or why the table is refused.  frames_in NULL: every input stream holds frames_default frames.  One pass; the ends of the
// sends that cover the current position sit in a min-heap, so the depth at a send's start is the heap's size once the ends at or
// before it are popped (the table is sorted, and the deepest cover of a bus begins at some send's start).
inline const char* mx_validate(const omx_program_mix_send* sends, uint64_t n_sends, uint32_t n_in, const uint32_t* frames_in,
                               uint64_t frames_default, uint32_t n_out) {
    if (n_sends && !sends) return "null sends";
    if (n_sends > kMxMaxSends) return "more than 2^20 sends";
    std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> ends;
    for (uint64_t k = 0; k < n_sends; ++k) {
        const omx_program_mix_send& c = sends[k];
        if (c.src_stream >= n_in) return "src_stream out of range";
        if (c.dst_bus >= n_out) return "dst_bus out of range";
        if (c.flags != 0) return "a send with a flag set";
        if (!std::isfinite(c.gain)) return "a gain that is not finite";
        const uint64_t have = frames_in ? frames_in[c.src_stream] : frames_default;
        if (c.frames > have || c.src_first > have - c.frames) return "a send reads beyond the frames of its input stream";
        if (c.frames > kMxMaxPosition || c.dst_first > kMxMaxPosition - c.frames) return "dst_first + frames beyond 2^40";
        if (k > 0) {
            const omx_program_mix_send& p = sends[k - 1];
            if (p.dst_bus > c.dst_bus || (p.dst_bus == c.dst_bus && p.dst_first > c.dst_first))
                return "the table is not sorted by (dst_bus, dst_first)";
            if (p.dst_bus != c.dst_bus) ends = {};
        }
        if (c.frames == 0) continue;
        while (!ends.empty() && ends.top() <= c.dst_first) ends.pop();
        if (ends.size() >= kMxMaxLayers) return "more than 64 sends cover a bus frame";
        ends.push(c.dst_first + c.frames);
    }
    return nullptr;
}

// per bus one past its last covered frame (the table has been validated)
inline void mx_extent(const omx_program_mix_send* sends, uint64_t n_sends, uint32_t n_out, uint64_t* out_frames) {
    for (uint32_t o = 0; o < n_out; ++o) out_frames[o] = 0;
    for (uint64_t k = 0; k < n_sends; ++k)
        if (sends[k].frames) out_frames[sends[k].dst_bus] = std::max(out_frames[sends[k].dst_bus], sends[k].dst_first + sends[k].frames);
}

// ---------------------------------------------------------------- null test
// nullptr, or why the call is refused; the header states the table
inline const char* mx_null(const uint32_t* stems, uint32_t n_stems, uint32_t reference_stream, uint64_t frames, uint32_t bus,
                           omx_program_mix_send* sends_out) {
    if (!stems || !sends_out) return "null pointer";
    if (n_stems == 0 || n_stems > kMxMaxLayers - 1) return "n_stems 0 or above 63";
    if (frames > kMxMaxPosition) return "frames beyond 2^40";
    for (uint32_t i = 0; i <= n_stems; ++i) {
        omx_program_mix_send s{};
        s.src_stream = i < n_stems ? stems[i] : reference_stream;
        s.dst_bus = bus;
        s.frames = frames;
        s.gain = i < n_stems ? 1.0f : -1.0f;
        sends_out[i] = s;
    }
    return nullptr;
}

// ---------------------------------------------------------------- spans
inline MxSend mx_device_send(const omx_program_mix_send& c, uint64_t frames_capacity) {
    MxSend d{};
    d.dst_first = c.dst_first;
    d.src_base = (uint64_t)c.src_stream * frames_capacity + c.src_first;
    d.gain = c.gain;
    return d;
}

// The spans of every bus of a validated table, appended to `spans`, and the table indices of the sends that cover each, appended to
// `list`; span_begin gets n_out + 1 entries.  Per bus: the boundaries (a send's start, its end) in order, and between two of them
// the sends that cover the stretch, in table order.  A send joins the active list at its start (the table is sorted by start, so the
// list stays in table order) and leaves it at its end.
inline void mx_build_spans(const omx_program_mix_send* sends, uint64_t n_sends, uint32_t n_out, std::vector<MxSpan>& spans,
                           std::vector<uint32_t>& list, std::vector<uint32_t>& span_begin) {
    span_begin.assign((size_t)n_out + 1, 0);
    std::vector<uint64_t> cuts;
    std::vector<uint32_t> active;
    uint64_t k = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        span_begin[o] = (uint32_t)spans.size();
        const uint64_t k0 = k;
        while (k < n_sends && sends[k].dst_bus == o) ++k;
        cuts.clear();
        cuts.push_back(0);
        cuts.push_back(kMxMaxPosition);
        for (uint64_t i = k0; i < k; ++i) {
            if (!sends[i].frames) continue;
            cuts.push_back(sends[i].dst_first);
            cuts.push_back(sends[i].dst_first + sends[i].frames);
        }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        uint64_t next = k0;  // the first send that has not started yet
        active.clear();
        for (size_t i = 0; i + 1 < cuts.size(); ++i) {
            const uint64_t x = cuts[i];
            size_t kept = 0;
            for (size_t q = 0; q < active.size(); ++q)
                if (sends[active[q]].dst_first + sends[active[q]].frames > x) active[kept++] = active[q];
            active.resize(kept);
            while (next < k && (sends[next].frames == 0 || sends[next].dst_first <= x)) {
                if (sends[next].frames) active.push_back((uint32_t)next);  // (it starts AT x: every start is a cut)
                ++next;
            }
            MxSpan s{};
            s.first = x;
            s.end = cuts[i + 1];
            s.list_begin = (uint32_t)list.size();
            s.n_layers = (uint32_t)active.size();
            list.insert(list.end(), active.begin(), active.end());
            spans.push_back(s);
        }
    }
    span_begin[n_out] = (uint32_t)spans.size();
}

// What the window [first, first + frames) of a bus holds: the record's counts and the sends that touch it
inline void mx_window_counts(const omx_program_mix_send* sends, uint64_t send_begin, uint64_t send_end, const MxSpan* spans, uint32_t n_spans,
                             uint64_t first, uint64_t frames, MxBusCall& call) {
    const uint64_t last = first + frames;
    call.silent_frames = call.mixed_frames = 0;
    call.sends = call.max_layers = 0;
    for (uint32_t i = 0; i < n_spans; ++i) {
        const uint64_t lo = std::max(first, spans[i].first), hi = std::min(last, spans[i].end);
        if (lo >= hi) continue;
        if (spans[i].n_layers == 0) call.silent_frames += hi - lo;
        if (spans[i].n_layers >= 2) call.mixed_frames += hi - lo;
        call.max_layers = std::max(call.max_layers, spans[i].n_layers);
    }
    for (uint64_t k = send_begin; k < send_end && frames != 0; ++k)  // (no send touches a window without frames)
        if (sends[k].frames && sends[k].dst_first < last && sends[k].dst_first + sends[k].frames > first) ++call.sends;
}

}  // namespace omx
