// Host side of the programme bank's edit pass (include/omx/program_edit.h): the host-only functions (program_edit_plan.hpp does the
// work; here they get their refusals) and the calls.  Every call is checked before anything is touched, the call's tables (the
// per-output entries, the spans and the clips) go up in one upload, every launch is on the caller's stream.  Nothing here
// synchronises except fetch_edited and edit_configure.
#include "program_loudness.hpp"

namespace omx {

namespace {

int ed_plan(uint32_t channels, omx_program_edit_info* info) {
    if (!info) return pl_refuse("edit plan", "null info");
    if (!pl_channels_ok(channels)) return pl_refuse("edit plan", "channels outside 1 .. 8");
    omx_program_edit_info out{};
    out.tile_frames = ed_tile_frames(channels);
    out.channels = channels;
    *info = out;
    return OMX_NONE;
}

const std::vector<float>& ed_tables() {  // [3][4097]
    static const std::vector<float> tabs = [] {
        std::vector<float> t((size_t)kEdCurves * kEdCurvePoints);
        for (uint32_t c = 0; c < kEdCurves; ++c) ed_curve_table(c, t.data() + (size_t)c * kEdCurvePoints);
        return t;
    }();
    return tabs;
}

}  // namespace

int ProgramLoudnessBank::edit_configure(uint32_t channels, uint32_t max_outputs) {
    const char* who = "edit_configure";
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (max_outputs == 0 || max_outputs > OMX_EDIT_MAX_OUTPUTS) return pl_refuse(who, "max_outputs 0 or above 2^24");
    // An edit call enqueued on ANY stream may still read the tables and the records that go now: wait for the whole device.
    if (edit_) OMX_HIP(hipDeviceSynchronize());
    auto ed = std::make_unique<ProgramEdit>();
    ed->channels = channels;
    ed->max_outputs = max_outputs;
    ed->tabs.upload(ed_tables(), last_stream_);
    ed->records.reserve(max_outputs);
    edit_ = std::move(ed);  // (the earlier buffers are released here, behind the wait above)
    // the records of a call that brought nothing, so that fetch_edited has something to say before the first call
    EdArgs a{};
    a.n_out = max_outputs;
    a.channels = channels;
    a.floor_db = cfg_.floor_db;
    a.records = edit_->records.ptr;
    launch_ed_begin(a, last_stream_);
    OMX_HIP(hipGetLastError());
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first edit call may come on another stream)
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out and the records as they were.
int ProgramLoudnessBank::edit(const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in, const omx_program_edit_clip* clips,
                              uint64_t n_clips, float* d_out, uint64_t out_capacity, uint32_t n_out, const uint64_t* out_first,
                              const uint32_t* out_frames, hipStream_t stream, const omx_program_edit_record** d_edited) {
    const char* who = "edit";
    if (!edit_) return pl_refuse(who, "the edit pass is not configured (omx_program_loudness_bank_edit_configure)");
    ProgramEdit& ed = *edit_;
    if (!d_edited) return pl_refuse(who, "null d_edited");
    if (n_out == 0 || n_out > ed.max_outputs) return pl_refuse(who, "n_out 0 or above max_outputs");
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    if (!pl_capacity_ok(out_capacity)) return pl_refuse(who, "out_capacity beyond 2^32 - 1");
    if (n_clips > kEdMaxClips) return pl_refuse(who, "more than 2^26 clips");
    if (!out_frames) return pl_refuse(who, "null out_frames");
    if (frames_in)
        for (uint32_t s = 0; s < n_streams_; ++s)
            if (frames_in[s] > frames_capacity) return pl_refuse(who, "frames_in[s] > frames_capacity");
    if (const char* why = ed_validate(clips, n_clips, n_streams_, frames_in, frames_capacity, n_out)) return pl_refuse(who, why);
    uint32_t max_frames = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        if (out_frames[o] > out_capacity) return pl_refuse(who, "out_frames[o] > out_capacity");
        if ((out_first ? out_first[o] : 0) > kEdMaxPosition - out_frames[o]) return pl_refuse(who, "out_first[o] + out_frames[o] beyond 2^40");
        max_frames = std::max(max_frames, out_frames[o]);
    }
    const bool any = max_frames != 0;
    bool reads = false;
    for (uint64_t k = 0; k < n_clips && !reads; ++k) reads = clips[k].frames != 0;
    if (any && !d_out) return pl_refuse(who, "null d_out");
    if (reads && !d_in) return pl_refuse(who, "null d_in");
    // out of place only: a tile would read what another has already written
    const unsigned __int128 frame_bytes = (unsigned __int128)ed.channels * sizeof(float);
    if (d_in && d_out && pl_ranges_overlap(d_in, frame_bytes * n_streams_ * frames_capacity, d_out, frame_bytes * n_out * out_capacity))
        return pl_refuse(who, "d_in and d_out overlap");

    // ---- the call's tables: [EdStreamCall x n_out][EdSpan x spans][EdClip x n_clips]
    ed.h_spans.clear();
    ed_build_spans(clips, n_clips, n_out, ed.h_spans, ed.h_span_begin);
    const size_t spans_at = (size_t)n_out * sizeof(EdStreamCall), clips_at = spans_at + ed.h_spans.size() * sizeof(EdSpan);
    ed.h_tables.resize(clips_at + (size_t)n_clips * sizeof(EdClip));
    EdStreamCall* calls = reinterpret_cast<EdStreamCall*>(ed.h_tables.data());
    uint64_t k = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        const uint64_t k0 = k;
        while (k < n_clips && clips[k].dst_stream == o) ++k;
        EdStreamCall c{};
        c.out_first = out_first ? out_first[o] : 0;
        c.out_frames = out_frames[o];
        c.span_begin = ed.h_span_begin[o];
        c.span_count = ed.h_span_begin[o + 1] - ed.h_span_begin[o];
        ed_window_counts(clips, k0, k, ed.h_spans.data() + c.span_begin, c.span_count, c.out_first, c.out_frames, c);
        calls[o] = c;
    }
    if (!ed.h_spans.empty()) std::memcpy(ed.h_tables.data() + spans_at, ed.h_spans.data(), ed.h_spans.size() * sizeof(EdSpan));
    EdClip* d_clips = reinterpret_cast<EdClip*>(ed.h_tables.data() + clips_at);
    for (uint64_t i = 0; i < n_clips; ++i) d_clips[i] = ed_device_clip(clips[i], frames_capacity);

    last_stream_ = stream;
    ed.tables.reserve(ed.h_tables.size());
    pl_upload_table(ed.staging, ed.h_tables, ed.tables.ptr, stream);
    EdArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.out_capacity = out_capacity;
    a.n_out = n_out;
    a.channels = ed.channels;
    a.max_frames = max_frames;
    a.floor_db = cfg_.floor_db;
    a.tabs = ed.tabs.ptr;
    a.calls = reinterpret_cast<const EdStreamCall*>(ed.tables.ptr);
    a.spans = reinterpret_cast<const EdSpan*>(ed.tables.ptr + spans_at);
    a.clips = reinterpret_cast<const EdClip*>(ed.tables.ptr + clips_at);
    a.records = ed.records.ptr;
    launch_ed_begin(a, stream);
    if (any) launch_ed_main(a, stream);
    launch_ed_finish(a, stream);
    OMX_HIP(hipGetLastError());
    *d_edited = ed.records.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_edited(uint64_t output_index, omx_program_edit_record* dst) {
    if (!edit_ || output_index >= edit_->max_outputs)
        return pl_refuse("fetch_edited", "the edit pass is not configured, or output index out of range");
    copy_out(dst, edit_->records.ptr + output_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_edit_plan(uint32_t channels, omx_program_edit_info* info) { return ed_plan(channels, info); }
int omx_program_edit_curve(uint32_t curve, float* dst) {
    if (!dst) return pl_refuse("edit curve", "null dst");
    if (curve >= kEdCurves) return pl_refuse("edit curve", "unknown curve");
    std::memcpy(dst, ed_tables().data() + (size_t)curve * kEdCurvePoints, kEdCurvePoints * sizeof(float));
    return OMX_NONE;
}
int omx_program_edit_gain(uint32_t curve, uint32_t fade_frames, uint32_t index, float* g) {
    const char* who = "edit gain";
    if (!g) return pl_refuse(who, "null g");
    if (curve >= kEdCurves) return pl_refuse(who, "unknown curve");
    if (fade_frames == 0 || fade_frames > OMX_EDIT_MAX_FADE) return pl_refuse(who, "fade_frames 0 or above 2^24");
    if (index >= fade_frames) return pl_refuse(who, "index at or beyond fade_frames");
    *g = ed_gain(ed_tables().data() + (size_t)curve * kEdCurvePoints, ed_fade_m(fade_frames), index);
    return OMX_NONE;
}
int omx_program_edit_extent(const omx_program_edit_clip* clips, uint64_t n_clips, uint32_t n_in, const uint32_t* frames_in, uint32_t n_out,
                            uint64_t* out_frames) {
    const char* who = "edit extent";
    if ((n_in && !frames_in) || (n_out && !out_frames)) return pl_refuse(who, "null pointer");
    if (const char* why = ed_validate(clips, n_clips, n_in, frames_in, 0, n_out)) return pl_refuse(who, why);
    ed_extent(clips, n_clips, n_out, out_frames);
    return OMX_NONE;
}
int omx_program_edit_trim(const omx_program_inspect_record* record, const omx_program_trim_rule* rule, uint32_t src_stream, uint32_t dst_stream,
                          omx_program_edit_clip* clip, uint64_t* out_frames) {
    if (const char* why = ed_trim(record, rule, src_stream, dst_stream, clip, out_frames)) return pl_refuse("edit trim", why);
    return OMX_NONE;
}
int omx_program_loudness_bank_edit_configure(omx_program_loudness_bank* b, uint32_t channels, uint32_t max_outputs) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.edit_configure(channels, max_outputs); });
}
int omx_program_loudness_bank_edit(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in,
                                   const omx_program_edit_clip* clips, uint64_t n_clips, float* d_out, uint64_t out_capacity, uint32_t n_out,
                                   const uint64_t* out_first, const uint32_t* out_frames, void* stream,
                                   const omx_program_edit_record** d_edited) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.edit(d_in, frames_capacity, frames_in, clips, n_clips, d_out, out_capacity, n_out, out_first, out_frames,
                            static_cast<hipStream_t>(stream), d_edited);
    });
}
int omx_program_loudness_bank_fetch_edited(omx_program_loudness_bank* b, uint64_t output_index, omx_program_edit_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_edited(output_index, dst); });
}

}  // extern "C"
