// Host side of the programme bank's mix pass (include/omx/program_mix.h): the host-only functions (program_mix_plan.hpp does the
// work; here they get their refusals) and the calls.  Every call is checked before anything is touched, the call's tables (the
// per-bus entries, the spans, the sends and the index list) go up in one upload, every launch is on the caller's stream.  Nothing
// here synchronises except fetch_mixed and mix_configure.
#include "program_loudness.hpp"

namespace omx {

int ProgramLoudnessBank::mix_configure(uint32_t channels, uint32_t max_buses) {
    const char* who = "mix_configure";
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (max_buses == 0 || max_buses > OMX_MIX_MAX_BUSES) return pl_refuse(who, "max_buses 0 or above 2^24");
    // A mix call enqueued on ANY stream may still read the tables and the records that go now: wait for the whole device.
    if (mix_) OMX_HIP(hipDeviceSynchronize());
    auto mx = std::make_unique<ProgramMix>();
    mx->channels = channels;
    mx->max_buses = max_buses;
    mx->records.reserve(max_buses);
    mix_ = std::move(mx);  // (the earlier buffers are released here, behind the wait above)
    // the records of a call that brought nothing, so that fetch_mixed has something to say before the first call
    MxArgs a{};
    a.n_out = max_buses;
    a.channels = channels;
    a.floor_db = cfg_.floor_db;
    a.records = mix_->records.ptr;
    launch_mx_begin(a, last_stream_);
    OMX_HIP(hipGetLastError());
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first mix call may come on another stream)
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out and the records as they were.
int ProgramLoudnessBank::mix(const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in, const omx_program_mix_send* sends,
                             uint64_t n_sends, float* d_out, uint64_t out_capacity, uint32_t n_out, const uint64_t* out_first,
                             const uint32_t* out_frames, hipStream_t stream, const omx_program_mix_record** d_mixed) {
    const char* who = "mix";
    if (!mix_) return pl_refuse(who, "the mix pass is not configured (omx_program_loudness_bank_mix_configure)");
    ProgramMix& mx = *mix_;
    if (!d_mixed) return pl_refuse(who, "null d_mixed");
    if (n_out == 0 || n_out > mx.max_buses) return pl_refuse(who, "n_out 0 or above max_buses");
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    if (!pl_capacity_ok(out_capacity)) return pl_refuse(who, "out_capacity beyond 2^32 - 1");
    if (!out_frames) return pl_refuse(who, "null out_frames");
    if (frames_in)
        for (uint32_t s = 0; s < n_streams_; ++s)
            if (frames_in[s] > frames_capacity) return pl_refuse(who, "frames_in[s] > frames_capacity");
    if (const char* why = mx_validate(sends, n_sends, n_streams_, frames_in, frames_capacity, n_out)) return pl_refuse(who, why);
    uint32_t max_frames = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        if (out_frames[o] > out_capacity) return pl_refuse(who, "out_frames[o] > out_capacity");
        if ((out_first ? out_first[o] : 0) > kMxMaxPosition - out_frames[o]) return pl_refuse(who, "out_first[o] + out_frames[o] beyond 2^40");
        max_frames = std::max(max_frames, out_frames[o]);
    }
    const bool any = max_frames != 0;
    bool reads = false;
    for (uint64_t k = 0; k < n_sends && !reads; ++k) reads = sends[k].frames != 0;
    if (any && !d_out) return pl_refuse(who, "null d_out");
    if (reads && !d_in) return pl_refuse(who, "null d_in");
    // out of place only: a tile would read what another has already written
    const unsigned __int128 frame_bytes = (unsigned __int128)mx.channels * sizeof(float);
    if (d_in && d_out && pl_ranges_overlap(d_in, frame_bytes * n_streams_ * frames_capacity, d_out, frame_bytes * n_out * out_capacity))
        return pl_refuse(who, "d_in and d_out overlap");

    // ---- the call's tables: [MxBusCall x n_out][MxSpan x spans][MxSend x n_sends][u32 x layers]
    mx.h_spans.clear();
    mx.h_list.clear();
    mx_build_spans(sends, n_sends, n_out, mx.h_spans, mx.h_list, mx.h_span_begin);
    const size_t spans_at = (size_t)n_out * sizeof(MxBusCall), sends_at = spans_at + mx.h_spans.size() * sizeof(MxSpan);
    const size_t list_at = sends_at + (size_t)n_sends * sizeof(MxSend);
    mx.h_tables.resize(list_at + mx.h_list.size() * sizeof(uint32_t));
    MxBusCall* calls = reinterpret_cast<MxBusCall*>(mx.h_tables.data());
    uint64_t k = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        const uint64_t k0 = k;
        while (k < n_sends && sends[k].dst_bus == o) ++k;
        MxBusCall c{};
        c.out_first = out_first ? out_first[o] : 0;
        c.out_frames = out_frames[o];
        c.span_begin = mx.h_span_begin[o];
        c.span_count = mx.h_span_begin[o + 1] - mx.h_span_begin[o];
        mx_window_counts(sends, k0, k, mx.h_spans.data() + c.span_begin, c.span_count, c.out_first, c.out_frames, c);
        calls[o] = c;
    }
    if (!mx.h_spans.empty()) std::memcpy(mx.h_tables.data() + spans_at, mx.h_spans.data(), mx.h_spans.size() * sizeof(MxSpan));
    MxSend* d_sends = reinterpret_cast<MxSend*>(mx.h_tables.data() + sends_at);
    for (uint64_t i = 0; i < n_sends; ++i) d_sends[i] = mx_device_send(sends[i], frames_capacity);
    if (!mx.h_list.empty()) std::memcpy(mx.h_tables.data() + list_at, mx.h_list.data(), mx.h_list.size() * sizeof(uint32_t));

    last_stream_ = stream;
    mx.tables.reserve(mx.h_tables.size());
    pl_upload_table(mx.staging, mx.h_tables, mx.tables.ptr, stream);
    MxArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.out_capacity = out_capacity;
    a.n_out = n_out;
    a.channels = mx.channels;
    a.max_frames = max_frames;
    a.floor_db = cfg_.floor_db;
    a.calls = reinterpret_cast<const MxBusCall*>(mx.tables.ptr);
    a.spans = reinterpret_cast<const MxSpan*>(mx.tables.ptr + spans_at);
    a.sends = reinterpret_cast<const MxSend*>(mx.tables.ptr + sends_at);
    a.list = reinterpret_cast<const uint32_t*>(mx.tables.ptr + list_at);
    a.records = mx.records.ptr;
    launch_mx_begin(a, stream);
    if (any) launch_mx_main(a, stream);
    launch_mx_finish(a, stream);
    OMX_HIP(hipGetLastError());
    *d_mixed = mx.records.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_mixed(uint64_t bus, omx_program_mix_record* dst) {
    if (!mix_ || bus >= mix_->max_buses) return pl_refuse("fetch_mixed", "the mix pass is not configured, or bus index out of range");
    copy_out(dst, mix_->records.ptr + bus, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_mix_plan(uint32_t channels, omx_program_mix_info* info) {
    if (!info) return pl_refuse("mix plan", "null info");
    if (!pl_channels_ok(channels)) return pl_refuse("mix plan", "channels outside 1 .. 8");
    omx_program_mix_info out{};
    out.tile_frames = mx_tile_frames(channels);
    out.layers_per_batch = kMxLayersPerBatch;
    out.channels = channels;
    *info = out;
    return OMX_NONE;
}
int omx_program_mix_extent(const omx_program_mix_send* sends, uint64_t n_sends, uint32_t n_in, const uint32_t* frames_in, uint32_t n_out,
                           uint64_t* out_frames) {
    const char* who = "mix extent";
    if ((n_in && !frames_in) || (n_out && !out_frames)) return pl_refuse(who, "null pointer");
    if (const char* why = mx_validate(sends, n_sends, n_in, frames_in, 0, n_out)) return pl_refuse(who, why);
    mx_extent(sends, n_sends, n_out, out_frames);
    return OMX_NONE;
}
int omx_program_mix_null(const uint32_t* stems, uint32_t n_stems, uint32_t reference_stream, uint64_t frames, uint32_t bus,
                         omx_program_mix_send* sends_out) {
    if (const char* why = mx_null(stems, n_stems, reference_stream, frames, bus, sends_out)) return pl_refuse("mix null", why);
    return OMX_NONE;
}
int omx_program_loudness_bank_mix_configure(omx_program_loudness_bank* b, uint32_t channels, uint32_t max_buses) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.mix_configure(channels, max_buses); });
}
int omx_program_loudness_bank_mix(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in,
                                  const omx_program_mix_send* sends, uint64_t n_sends, float* d_out, uint64_t out_capacity, uint32_t n_out,
                                  const uint64_t* out_first, const uint32_t* out_frames, void* stream, const omx_program_mix_record** d_mixed) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.mix(d_in, frames_capacity, frames_in, sends, n_sends, d_out, out_capacity, n_out, out_first, out_frames,
                           static_cast<hipStream_t>(stream), d_mixed);
    });
}
int omx_program_loudness_bank_fetch_mixed(omx_program_loudness_bank* b, uint64_t bus, omx_program_mix_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_mixed(bus, dst); });
}

}  // extern "C"
