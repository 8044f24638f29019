// Host side of the programme bank's filter stage (include/omx/program_filter.h): the C ABI of the host-only functions
// (program_filter_plan.hpp holds them), the tables of a configured filter table, and the calls.  Every call is checked before anything
// is touched, the per-stream table of a call goes up in one upload, every launch is on the caller's stream.  Nothing here synchronises
// except fetch_filtered and filter_configure.
#include "program_loudness.hpp"

namespace omx {

namespace {

int fl_refusal(const char* who, int rc, const char* why) {
    pl_refuse(who, why ? why : "refused");
    return rc;
}

}  // namespace

int ProgramLoudnessBank::filter_configure(uint32_t channels, double sample_rate, const omx_program_filter* filters, uint32_t n_filters,
                                          const uint32_t* filter_of_channel) {
    const char* who = "filter configure";
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (!std::isfinite(sample_rate) || !(sample_rate > 0.0)) return pl_refuse(who, "a sample rate that is not finite or not positive");
    if (!filters) return pl_refuse(who, "null table");
    if (n_filters == 0 || n_filters > OMX_FILTER_MAX_FILTERS) return pl_refuse(who, "n_filters 0 or above OMX_FILTER_MAX_FILTERS");
    for (uint32_t k = 0; k < n_filters; ++k) {
        const char* why = nullptr;
        const int rc = fl_check(filters + k, &why);
        if (rc != OMX_NONE) return fl_refusal(who, rc, why);
    }
    std::vector<uint32_t> lane_filter((size_t)n_streams_ * kFlSlots, OMX_FILTER_BYPASS);
    for (uint32_t s = 0; s < n_streams_; ++s)
        for (uint32_t c = 0; c < channels; ++c) {
            const uint32_t f = filter_of_channel ? filter_of_channel[(size_t)s * channels + c] : 0u;
            if (f != OMX_FILTER_BYPASS && f >= n_filters) return pl_refuse(who, "a filter index that is neither below n_filters nor OMX_FILTER_BYPASS");
            lane_filter[(size_t)s * kFlSlots + c] = f;
        }
    if (filter_)
        for (const uint64_t n : filter_->h_total)
            if (n != 0) return pl_refuse(who, "a stream holds filter state (reset every stream first)");
    if (filter_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the old buffers may still be in flight)

    // the tables of the time-parallel form, and whether every filter may run in it
    const uint32_t L = kFlChunkFrames;
    const uint64_t weights_stride = (uint64_t)((L + kFlTile - 1) / kFlTile * kFlTile) * 4;
    std::vector<double> W((size_t)n_filters * weights_stride), T((size_t)n_filters * 32);
    bool ok = true;
    for (uint32_t k = 0; k < n_filters; ++k) {
        const FlTables t = fl_tables(filters[k], L);
        std::copy(t.weights.begin(), t.weights.end(), W.begin() + (size_t)k * weights_stride);
        std::copy(t.transition, t.transition + 32, T.begin() + (size_t)k * 32);
        ok = ok && fl_time_parallel_ok(t, L);
    }

    auto fl = filter_ ? std::move(filter_) : std::make_unique<ProgramFilter>();
    fl->channels = channels;
    fl->n_filters = n_filters;
    fl->sample_rate = sample_rate;
    fl->time_parallel_ok = ok;
    fl->weights_stride = weights_stride;
    fl->h_total.assign(n_streams_, 0);
    fl->h_calls.assign(n_streams_, FlStreamCall{});
    fl->calls.reserve(n_streams_);
    fl->records.reserve(n_streams_);
    fl->state.reserve((size_t)n_streams_ * kFlSlots * 4);
    fl->partials.reserve((size_t)n_streams_ * kFlSlots);
    fl->lane_filter.upload(lane_filter, last_stream_);
    fl->filters.upload(std::vector<omx_program_filter>(filters, filters + n_filters), last_stream_);
    fl->zs_weights.upload(W, last_stream_);
    fl->transition.upload(T, last_stream_);
    filter_ = std::move(fl);
    filter_last_form_ = 0;
    const int rc = filter_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first filter call may come on another stream)
    return rc;
}

FlArgs ProgramLoudnessBank::filter_args() const {
    const ProgramFilter& fl = *filter_;
    FlArgs a{};
    a.n_streams = n_streams_;
    a.channels = fl.channels;
    a.slot_shift = fl_slot_shift(fl.channels);
    a.chunk = 1;
    a.n_chunks = 1;
    a.floor_db = cfg_.floor_db;
    a.calls = fl.calls.ptr;
    a.lane_filter = fl.lane_filter.ptr;
    a.filters = fl.filters.ptr;
    a.state = fl.state.ptr;
    a.starts = fl.state.ptr;
    a.partials = fl.partials.ptr;
    a.zs_weights = fl.zs_weights.ptr;
    a.transition = fl.transition.ptr;
    a.weights_stride = fl.weights_stride;
    a.records = fl.records.ptr;
    return a;
}

int ProgramLoudnessBank::filter_reset(const uint8_t* reset_mask) {
    if (!filter_) return pl_refuse("filter reset", "the filter is not configured (omx_program_loudness_bank_filter_configure)");
    ProgramFilter& fl = *filter_;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const bool clear = !reset_mask || reset_mask[s];
        if (clear) fl.h_total[s] = 0;
        fl.h_calls[s] = FlStreamCall{clear ? 1u : 0u, 0u, 0};
    }
    pl_upload_table(fl.staging, fl.h_calls, fl.calls.ptr, last_stream_);
    launch_fl_reset(filter_args(), last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out, the state and the records as they were.
int ProgramLoudnessBank::filter(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, hipStream_t stream,
                                const omx_program_filter_record** d_filtered) {
    const char* who = "filter";
    if (!filter_) return pl_refuse(who, "the filter is not configured (omx_program_loudness_bank_filter_configure)");
    ProgramFilter& fl = *filter_;
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    uint32_t max_frames = 0;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        fl.h_calls[s] = FlStreamCall{(uint32_t)f, 0u, fl.h_total[s] + f};  // (host scratch only)
        max_frames = std::max(max_frames, (uint32_t)f);
    }
    const bool any = max_frames != 0;
    if (any && (!d_in || !d_out)) return pl_refuse(who, "null pcm");
    // in place (the same rows) or apart: a tile would read what another call's row has already written
    const unsigned __int128 bytes = (unsigned __int128)n_streams_ * frames_capacity * fl.channels * sizeof(float);
    if (d_in && d_out && d_in != d_out && pl_ranges_overlap(d_in, bytes, d_out, bytes)) return pl_refuse(who, "d_in and d_out overlap without being the same");

    last_stream_ = stream;
    for (uint32_t s = 0; s < n_streams_; ++s) fl.h_total[s] = fl.h_calls[s].frames_total;
    pl_upload_table(fl.staging, fl.h_calls, fl.calls.ptr, stream);
    FlArgs a = filter_args();
    a.in = d_in;
    a.out = d_out;
    a.frames_capacity = frames_capacity;
    if (any) {
        // Which evaluation order, as the loudness pass decides it: the reference-order pass runs one wavefront per 64 (stream, channel)
        // slots however long the call is; the time-parallel pass reads the PCM twice but fills the card when the call is long.  A table
        // with a filter that cannot hold the parity bar runs in reference order whatever is asked for, and last_form says so.
        const uint64_t waves = ((uint64_t)n_streams_ << a.slot_shift) / 64 + 1;
        const bool by_shape = max_frames >= 4 * kFlChunkFrames && waves * 4 < 2048;
        const bool time_parallel = fl.time_parallel_ok && (filter_form_ == 2 || (filter_form_ == 0 && by_shape));
        if (time_parallel) {
            a.chunk = kFlChunkFrames;
            a.n_chunks = (max_frames + kFlChunkFrames - 1) / kFlChunkFrames;
            a.form = 2;
            const size_t items = (size_t)n_streams_ * kFlSlots * a.n_chunks;
            fl.starts.reserve(items * 4);
            fl.partials.reserve(items);
            a.starts = fl.starts.ptr;
            a.partials = fl.partials.ptr;
            launch_fl_time_parallel(a, stream);
        } else {
            a.chunk = max_frames;
            a.n_chunks = 1;
            a.form = 1;
            launch_fl_reference_order(a, stream);
        }
        filter_last_form_ = (int)a.form;
    }
    launch_fl_fold(a, stream);
    OMX_HIP(hipGetLastError());
    *d_filtered = fl.records.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_filtered(uint64_t stream_index, omx_program_filter_record* dst) {
    if (!filter_ || stream_index >= n_streams_) return pl_refuse("filter fetch", "the filter is not configured, or stream index out of range");
    copy_out(dst, filter_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

int ProgramLoudnessBank::filter_set_form(uint32_t form) {
    if (form > 2) return pl_refuse("filter set_form", "a form other than 0, 1 or 2");
    filter_form_ = (int)form;
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_filter_design(const omx_program_filter_spec* spec, double sample_rate, omx_program_filter* filter) {
    const char* why = nullptr;
    const int rc = fl_design(spec, sample_rate, filter, &why);
    return rc == OMX_NONE ? rc : fl_refusal("filter design", rc, why);
}
int omx_program_filter_cascade(const omx_program_filter* a, const omx_program_filter* b, omx_program_filter* out) {
    const char* why = nullptr;
    const int rc = fl_cascade(a, b, out, &why);
    return rc == OMX_NONE ? rc : fl_refusal("filter cascade", rc, why);
}
int omx_program_filter_check(const omx_program_filter* filter) {
    const char* why = nullptr;
    const int rc = fl_check(filter, &why);
    return rc == OMX_NONE ? rc : fl_refusal("filter check", rc, why);
}
int omx_program_filter_response(const omx_program_filter* filter, double sample_rate, double frequency_hz, double* magnitude_db,
                                double* phase_rad) {
    const char* why = nullptr;
    const int rc = fl_response(filter, sample_rate, frequency_hz, magnitude_db, phase_rad, &why);
    return rc == OMX_NONE ? rc : fl_refusal("filter response", rc, why);
}
int omx_program_filter_plan(uint32_t channels, double sample_rate, omx_program_filter_info* info) {
    const char* why = nullptr;
    const int rc = fl_plan(channels, sample_rate, info, &why);
    return rc == OMX_NONE ? rc : fl_refusal("filter plan", rc, why);
}
int omx_program_loudness_bank_filter_configure(omx_program_loudness_bank* b, uint32_t channels, double sample_rate,
                                               const omx_program_filter* filters, uint32_t n_filters, const uint32_t* filter_of_channel) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.filter_configure(channels, sample_rate, filters, n_filters, filter_of_channel); });
}
int omx_program_loudness_bank_filter_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.filter_reset(reset_mask); });
}
int omx_program_loudness_bank_filter(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                     float* d_out, void* stream, const omx_program_filter_record** d_filtered) {
    if (!b || !d_filtered) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.filter(d_in, frames_capacity, frames, d_out, static_cast<hipStream_t>(stream), d_filtered); });
}
int omx_program_loudness_bank_fetch_filtered(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_filter_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_filtered(stream_index, dst); });
}
int omx_program_loudness_bank_filter_set_form(omx_program_loudness_bank* b, uint32_t form) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.filter_set_form(form); });
}
int omx_debug_program_loudness_bank_filter_last_form(const omx_program_loudness_bank* b) {
    return b ? b->impl.filter_last_form() : OMX_ERR_INVALID;
}

}  // extern "C"
