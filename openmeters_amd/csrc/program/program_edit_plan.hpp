// Everything of the programme bank's edit pass (include/omx/program_edit.h states the definition) that needs no device: the phase
// and curve function (ONE inline function for the host, omx_program_edit_gain, and the kernel: they cannot drift apart), the curve
// tables, the validation of a clip table, the trim helper, and the cut of every output stream into SPANS, the maximal runs of output
// frames under the same 0, 1 or 2 clips with the same fades active.  Free of HIP on purpose: a stand-alone CPU program
// (tools/edit_plan_check.cpp) includes this file alone.  Host work is O(clips log clips), never O(frames / tile).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/omx/program_edit.h"

#if defined(__HIPCC__)
#define OMX_EDIT_HD __host__ __device__
#else
#define OMX_EDIT_HD
#endif

namespace omx {

constexpr uint32_t kEdThreads = 256;   // threads per workgroup of the main kernel
constexpr uint32_t kEdCurves = 3;
constexpr uint32_t kEdCurvePoints = OMX_EDIT_CURVE_POINTS;
constexpr uint64_t kEdMaxPosition = OMX_EDIT_MAX_POSITION;

// Output frames of a tile: 16 KiB of PCM per workgroup (12 to 16 at the channel counts that do not divide it), that is three or four
// 16-byte vectors per thread, all in flight before the first store.
constexpr uint32_t ed_tile_frames(uint32_t channels) { return channels == 1 ? 4096 : (channels == 2 ? 2048 : (channels <= 4 ? 1024 : 512)); }
// 16-byte vectors a thread holds in flight: every vector of a full tile in one round
constexpr uint32_t ed_in_flight(uint32_t channels) { return (ed_tile_frames(channels) * channels / 4 + kEdThreads - 1) / kEdThreads; }

// span flags: which fade factors apply to which of the span's clips
constexpr uint32_t kEdFadeInA = 1, kEdFadeOutA = 2, kEdFadeInB = 4, kEdFadeOutB = 8;

// A clip as the kernel reads it
struct EdClip {
    uint64_t dst_first, frames;
    uint64_t src_base;      // src_stream * frames_capacity + src_first: the frame of d_in that lands at dst_first
    uint64_t m_in, m_out;   // floor(2^63 / fade frames), 0 without a fade
    uint32_t fade_in, fade_out;
    uint32_t curve_in, curve_out;
    float gain;
    uint32_t _pad;
};
static_assert(sizeof(EdClip) == 64, "EdClip is part of the call's blob");

// Output frames [first, end) of one stream under the same clips (table indices a, then b) and the same active fades.  The spans of a
// stream lie one behind the other and tile [0, 2^40).
struct EdSpan {
    uint64_t first, end;
    uint32_t n_clips;  // 0: zero fill
    uint32_t flags;    // kEdFade*: 0 = plain
    uint32_t a, b;
};
static_assert(sizeof(EdSpan) == 32, "EdSpan is part of the call's blob");

// What one call does to one output stream; the counts of the record follow from the spans and the window on the host
struct EdStreamCall {
    uint64_t out_first;
    uint32_t out_frames;
    uint32_t span_begin;  // the stream's spans: [span_begin, span_begin + span_count) of the call's span list
    uint32_t span_count;
    uint32_t clips;       // clips that touch the window
    uint64_t silent_frames, faded_frames, mixed_frames;
};
static_assert(sizeof(EdStreamCall) == 48, "EdStreamCall is part of the call's blob");

// ---------------------------------------------------------------- phase and curve
inline uint64_t ed_fade_m(uint32_t fade_frames) { return fade_frames ? (1ull << 63) / fade_frames : 0; }

// the 24-bit fixed-point value of (i + 1/2) / F; i < F <= 2^24
OMX_EDIT_HD inline uint32_t ed_phase(uint64_t m, uint64_t i) { return (uint32_t)(((2 * i + 1) * m) >> 40); }

// g of the header's DEFINITION: three f32 operations, each rounded (the library is built with -ffp-contract=off)
OMX_EDIT_HD inline float ed_gain(const float* tab, uint64_t m, uint64_t i) {
    const uint32_t p = ed_phase(m, i);
    const float a = tab[p >> 12], b = tab[(p >> 12) + 1];
    const float fr = (float)(p & 4095u) * 0.000244140625f;  // 2^-12: exact
    const float d = b - a;
    const float t = d * fr;
    return a + t;
}

// The weight of clip c at output frame n of a span in which fade_in / fade_out say which factors apply (uniform over the span).  The
// indices are clamped to the fade: a caller may ask for a frame next to the span (a vector's neighbour) and keep nothing of it.
OMX_EDIT_HD inline float ed_weight(const EdClip& c, const float* tabs, uint64_t n, bool fade_in, bool fade_out) {
    const uint64_t j = n - c.dst_first;
    float w = c.gain;
    if (fade_in) {
        const uint64_t i = j < c.fade_in ? j : (uint64_t)c.fade_in - 1;
        w = w * ed_gain(tabs + c.curve_in * kEdCurvePoints, c.m_in, i);
    }
    if (fade_out) {
        const uint64_t r = c.frames - 1 - j;
        const uint64_t i = r < c.fade_out ? r : (uint64_t)c.fade_out - 1;
        w = w * ed_gain(tabs + c.curve_out * kEdCurvePoints, c.m_out, i);
    }
    return w;
}

// The table of one curve, in double, rounded once
inline void ed_curve_table(uint32_t curve, float* dst) {
    for (uint32_t k = 0; k < kEdCurvePoints; ++k) {
        const double x = (double)k / 4096.0;
        double v = x;
        if (curve == OMX_EDIT_CURVE_EQUAL_POWER) v = std::sin(M_PI / 2.0 * x);
        else if (curve == OMX_EDIT_CURVE_RAISED_COSINE) v = 0.5 - 0.5 * std::cos(M_PI * x);
        dst[k] = (float)v;
    }
    dst[0] = 0.0f;
    dst[kEdCurvePoints - 1] = 1.0f;
}

// ---------------------------------------------------------------- validation
// nullptr, or why the table is refused.  frames_in NULL: every input stream holds frames_default frames.
inline const char* ed_validate(const omx_program_edit_clip* clips, uint64_t n_clips, uint32_t n_in, const uint32_t* frames_in,
                               uint64_t frames_default, uint32_t n_out) {
    if (n_clips && !clips) return "null clips";
    uint64_t end1 = 0, end2 = 0;  // the two largest ends among the earlier clips of the output stream, end1 >= end2
    for (uint64_t k = 0; k < n_clips; ++k) {
        const omx_program_edit_clip& c = clips[k];
        if (c.src_stream >= n_in) return "src_stream out of range";
        if (c.dst_stream >= n_out) return "dst_stream out of range";
        if (c.flags != 0) return "a clip with a flag set";
        if (!std::isfinite(c.gain)) return "a gain that is not finite";
        if (c.fade_in_curve >= kEdCurves || c.fade_out_curve >= kEdCurves) return "unknown curve";
        if (c.fade_in_frames > OMX_EDIT_MAX_FADE || c.fade_out_frames > OMX_EDIT_MAX_FADE) return "a fade longer than 2^24 frames";
        if (c.fade_in_frames > c.frames || c.fade_out_frames > c.frames) return "a fade longer than its clip";
        const uint64_t have = frames_in ? frames_in[c.src_stream] : frames_default;
        if (c.frames > have || c.src_first > have - c.frames) return "a clip reads beyond the frames of its input stream";
        if (c.frames > kEdMaxPosition || c.dst_first > kEdMaxPosition - c.frames) return "dst_first + frames beyond 2^40";
        if (k > 0) {
            const omx_program_edit_clip& p = clips[k - 1];
            if (p.dst_stream > c.dst_stream || (p.dst_stream == c.dst_stream && p.dst_first > c.dst_first))
                return "the table is not sorted by (dst_stream, dst_first)";
            if (p.dst_stream != c.dst_stream) end1 = end2 = 0;
        }
        if (c.frames == 0) continue;
        if (end2 > c.dst_first) return "more than two clips cover an output frame";
        const uint64_t end = c.dst_first + c.frames;
        if (end >= end1) {
            end2 = end1;
            end1 = end;
        } else if (end > end2) {
            end2 = end;
        }
    }
    return nullptr;
}

// per output stream one past its last covered frame (the table has been validated)
inline void ed_extent(const omx_program_edit_clip* clips, uint64_t n_clips, uint32_t n_out, uint64_t* out_frames) {
    for (uint32_t o = 0; o < n_out; ++o) out_frames[o] = 0;
    for (uint64_t k = 0; k < n_clips; ++k)
        if (clips[k].frames) out_frames[clips[k].dst_stream] = std::max(out_frames[clips[k].dst_stream], clips[k].dst_first + clips[k].frames);
}

// ---------------------------------------------------------------- trim
// nullptr, or why the call is refused; the header states the clip
inline const char* ed_trim(const omx_program_inspect_record* record, const omx_program_trim_rule* rule, uint32_t src_stream, uint32_t dst_stream,
                           omx_program_edit_clip* clip, uint64_t* out_frames) {
    if (!record || !rule || !clip || !out_frames) return "null pointer";
    if (rule->flags != 0 || rule->_pad != 0) return "a rule with a flag set";
    if (rule->fade_in_curve >= kEdCurves || rule->fade_out_curve >= kEdCurves) return "unknown curve";
    if (rule->fade_in_frames > OMX_EDIT_MAX_FADE || rule->fade_out_frames > OMX_EDIT_MAX_FADE) return "a fade longer than 2^24 frames";
    const uint64_t n = record->frames, lead = record->leading_silence, trail = record->trailing_silence;
    if (n > 0xFFFFFFFFull) return "a record of more than 2^32 - 1 frames";
    if (lead > n || trail > n || (lead < n && lead + trail > n)) return "a record whose silences do not fit its frames";
    if (rule->pad_head > kEdMaxPosition || rule->pad_tail > kEdMaxPosition) return "out_frames beyond 2^40";
    omx_program_edit_clip c{};
    c.src_stream = src_stream;
    c.dst_stream = dst_stream;
    c.dst_first = rule->pad_head;
    c.fade_in_curve = rule->fade_in_curve;
    c.fade_out_curve = rule->fade_out_curve;
    c.gain = 1.0f;
    if (lead < n) {
        c.src_first = lead - std::min(rule->keep_head, lead);
        c.frames = n - c.src_first - (trail - std::min(rule->keep_tail, trail));
        c.fade_in_frames = (uint32_t)std::min<uint64_t>(rule->fade_in_frames, c.frames);
        c.fade_out_frames = (uint32_t)std::min<uint64_t>(rule->fade_out_frames, c.frames);
    }
    const uint64_t total = rule->pad_head + c.frames + rule->pad_tail;
    if (total > kEdMaxPosition) return "out_frames beyond 2^40";
    *clip = c;
    *out_frames = total;
    return nullptr;
}

// ---------------------------------------------------------------- spans
inline EdClip ed_device_clip(const omx_program_edit_clip& c, uint64_t frames_capacity) {
    EdClip d{};
    d.dst_first = c.dst_first;
    d.frames = c.frames;
    d.src_base = (uint64_t)c.src_stream * frames_capacity + c.src_first;
    d.m_in = ed_fade_m(c.fade_in_frames);
    d.m_out = ed_fade_m(c.fade_out_frames);
    d.fade_in = c.fade_in_frames;
    d.fade_out = c.fade_out_frames;
    d.curve_in = c.fade_in_curve;
    d.curve_out = c.fade_out_curve;
    d.gain = c.gain;
    return d;
}

// The spans of every output stream of a validated table, appended to `spans`; span_begin gets n_out + 1 entries.  Per stream: the
// breakpoints (a clip's start, the end of its fade-in, the start of its fade-out, its end) in order, and between two of them the
// clips that cover the stretch (at most two, the earlier of the table first) with the fades that apply there.
inline void ed_build_spans(const omx_program_edit_clip* clips, uint64_t n_clips, uint32_t n_out, std::vector<EdSpan>& spans,
                           std::vector<uint32_t>& span_begin) {
    span_begin.assign((size_t)n_out + 1, 0);
    std::vector<uint64_t> cuts;
    uint64_t k = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        span_begin[o] = (uint32_t)spans.size();
        const uint64_t k0 = k;
        while (k < n_clips && clips[k].dst_stream == o) ++k;
        cuts.clear();
        cuts.push_back(0);
        cuts.push_back(kEdMaxPosition);
        for (uint64_t i = k0; i < k; ++i) {
            const omx_program_edit_clip& c = clips[i];
            if (!c.frames) continue;
            cuts.push_back(c.dst_first);
            cuts.push_back(c.dst_first + c.frames);
            if (c.fade_in_frames) cuts.push_back(c.dst_first + c.fade_in_frames);
            if (c.fade_out_frames) cuts.push_back(c.dst_first + c.frames - c.fade_out_frames);
        }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        uint64_t next = k0;          // the first clip that has not started yet
        uint64_t active[2] = {0, 0};  // table indices of the clips that cover the stretch, in table order
        uint32_t n_active = 0;
        for (size_t i = 0; i + 1 < cuts.size(); ++i) {
            const uint64_t x = cuts[i];
            uint32_t kept = 0;
            for (uint32_t q = 0; q < n_active; ++q)
                if (clips[active[q]].dst_first + clips[active[q]].frames > x) active[kept++] = active[q];
            n_active = kept;
            while (next < k && (clips[next].frames == 0 || clips[next].dst_first <= x)) {
                if (clips[next].frames && clips[next].dst_first + clips[next].frames > x && n_active < 2) active[n_active++] = next;
                ++next;
            }
            EdSpan s{};
            s.first = x;
            s.end = cuts[i + 1];
            s.n_clips = n_active;
            for (uint32_t q = 0; q < n_active; ++q) {
                const omx_program_edit_clip& c = clips[active[q]];
                (q ? s.b : s.a) = (uint32_t)active[q];
                if (x < c.dst_first + c.fade_in_frames) s.flags |= q ? kEdFadeInB : kEdFadeInA;
                if (x >= c.dst_first + c.frames - c.fade_out_frames) s.flags |= q ? kEdFadeOutB : kEdFadeOutA;
            }
            // (two stretches under no clip cannot touch; stretches under clips differ in a clip or a fade by construction)
            spans.push_back(s);
        }
    }
    span_begin[n_out] = (uint32_t)spans.size();
}

// What the window [first, first + frames) of an output stream holds: the record's counts and the clips that touch it
inline void ed_window_counts(const omx_program_edit_clip* clips, uint64_t clip_begin, uint64_t clip_end, const EdSpan* spans, uint32_t n_spans,
                             uint64_t first, uint64_t frames, EdStreamCall& call) {
    const uint64_t last = first + frames;
    call.silent_frames = call.faded_frames = call.mixed_frames = 0;
    call.clips = 0;
    for (uint32_t i = 0; i < n_spans; ++i) {
        const uint64_t lo = std::max(first, spans[i].first), hi = std::min(last, spans[i].end);
        if (lo >= hi) continue;
        if (spans[i].n_clips == 0) call.silent_frames += hi - lo;
        if (spans[i].n_clips == 2) call.mixed_frames += hi - lo;
        if (spans[i].flags) call.faded_frames += hi - lo;
    }
    for (uint64_t k = clip_begin; k < clip_end && frames != 0; ++k)  // (no clip touches a window without frames)
        if (clips[k].frames && clips[k].dst_first < last && clips[k].dst_first + clips[k].frames > first) ++call.clips;
}

}  // namespace omx
