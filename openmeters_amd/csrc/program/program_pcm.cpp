// Host side of the programme bank's PCM formats (include/omx/program_pcm.h): the rule and every call are checked against the host's
// own values, the mirror of the export positions among them, before anything is touched; the per-stream table of a call goes up in
// one upload, every launch is on the caller's stream.  Nothing here synchronises except fetch_exported, export_configure and
// export_reset's wait for its own upload slot.
#include "program_loudness.hpp"

namespace omx {

namespace {

bool pc_rule_valid(const omx_program_export_rule* rule) {
    if (!rule) return false;
    if (pc_format_bytes(rule->format) == 0) return false;
    if (rule->dither != OMX_DITHER_NONE && rule->dither != OMX_DITHER_TPDF) return false;
    return rule->flags == 0;
}

}  // namespace

// Everything is checked before anything is touched: a refused call leaves d_out as it was.
int ProgramLoudnessBank::import_pcm(const void* d_in, uint32_t format, float* d_out, uint64_t frames_capacity, const uint32_t* frames,
                                    uint32_t channels, hipStream_t stream) {
    const char* who = "import_pcm";
    const uint32_t bytes = pc_format_bytes(format);
    if (bytes == 0) return pl_refuse(who, "unknown format");
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (reinterpret_cast<uintptr_t>(d_in) & 3u) return pl_refuse(who, "d_in is not 4-byte aligned");
    bool any = false;
    uint64_t max_n = 0;
    h_import_calls_.resize(n_streams_);  // (host scratch only)
    for (uint32_t s = 0; s < n_streams_; ++s) {
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        any = any || f != 0;
        h_import_calls_[s] = PcStreamCall{f * channels, 0, 0, 0, 0};
        max_n = std::max(max_n, f * channels);
    }
    if (any && (!d_in || !d_out)) return pl_refuse(who, "null pcm");
    const unsigned __int128 samples = (unsigned __int128)n_streams_ * frames_capacity * channels;
    if (d_in && d_out && pl_ranges_overlap(d_in, samples * bytes, d_out, samples * sizeof(float)))
        return pl_refuse(who, "d_in and d_out overlap");
    if (!any) return OMX_NONE;

    last_stream_ = stream;
    import_calls_.reserve(n_streams_);
    pl_upload_table(import_staging_, h_import_calls_, import_calls_.ptr, stream);
    PcArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.row = frames_capacity * channels;
    a.calls = import_calls_.ptr;
    a.n_streams = n_streams_;
    a.channels = channels;
    a.format = format;
    launch_pc_import(a, max_n, stream);
    OMX_HIP(hipGetLastError());
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::export_configure(const omx_program_export_rule* rule, uint32_t channels) {
    const char* who = "export_configure";
    if (!pc_rule_valid(rule)) return pl_refuse(who, "bad export rule (null, an unknown format or dither, or a flag set)");
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (exporter_)
        for (const uint64_t pos : exporter_->h_pos)
            if (pos != 0) return pl_refuse(who, "a stream's export position is not 0 (reset every stream first)");
    if (exporter_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that writes the records may still be in flight)
    auto ex = exporter_ ? std::move(exporter_) : std::make_unique<ProgramExporter>();
    ex->rule = *rule;
    ex->channels = channels;
    ex->h_pos.assign(n_streams_, 0);
    ex->h_calls.assign(n_streams_, PcStreamCall{});
    ex->calls.reserve(n_streams_);
    ex->records.reserve(n_streams_);
    exporter_ = std::move(ex);
    const int rc = export_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first export_pcm call may come on another stream)
    return rc;
}

int ProgramLoudnessBank::export_reset(const uint8_t* reset_mask) {
    if (!exporter_) return pl_refuse("export_reset", "the export is not configured (omx_program_loudness_bank_export_configure)");
    ProgramExporter& ex = *exporter_;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        PcStreamCall c{};
        if (!reset_mask || reset_mask[s]) {
            ex.h_pos[s] = 0;
            c.flags = kPcFlagClear;
        } else {
            c.flags = kPcFlagKeep;
        }
        ex.h_calls[s] = c;
    }
    pl_upload_table(ex.staging, ex.h_calls, ex.calls.ptr, last_stream_);
    PcArgs a{};
    a.calls = ex.calls.ptr;
    a.records = ex.records.ptr;
    a.n_streams = n_streams_;
    a.channels = ex.channels;
    a.format = ex.rule.format;
    a.dither = ex.rule.dither;
    a.floor_db = cfg_.floor_db;
    launch_pc_export_begin(a, last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out, the records and the positions as they were.
int ProgramLoudnessBank::export_pcm(const float* d_in, void* d_out, uint64_t frames_capacity, const uint32_t* frames, hipStream_t stream,
                                    const omx_program_export_record** d_exported) {
    const char* who = "export_pcm";
    if (!exporter_) return pl_refuse(who, "the export is not configured (omx_program_loudness_bank_export_configure)");
    ProgramExporter& ex = *exporter_;
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return pl_refuse(who, "d_out is not 4-byte aligned");
    const uint32_t bytes = pc_format_bytes(ex.rule.format), channels = ex.channels;
    bool any = false;
    uint64_t max_n = 0;
    for (uint32_t s = 0; s < n_streams_; ++s) {  // (host scratch only: the positions are committed below, after the last check)
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        any = any || f != 0;
        ex.h_calls[s] = PcStreamCall{f * channels, ex.h_pos[s], pc_stream_key(ex.rule.seed, s), 0, 0};
        max_n = std::max(max_n, f * channels);
    }
    if (any && (!d_in || !d_out)) return pl_refuse(who, "null pcm");
    const unsigned __int128 samples = (unsigned __int128)n_streams_ * frames_capacity * channels;
    if (d_in && d_out && pl_ranges_overlap(d_in, samples * sizeof(float), d_out, samples * bytes))
        return pl_refuse(who, "d_in and d_out overlap");

    for (uint32_t s = 0; s < n_streams_; ++s) ex.h_pos[s] += ex.h_calls[s].n / channels;
    last_stream_ = stream;
    pl_upload_table(ex.staging, ex.h_calls, ex.calls.ptr, stream);
    PcArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.row = frames_capacity * channels;
    a.calls = ex.calls.ptr;
    a.records = ex.records.ptr;
    a.n_streams = n_streams_;
    a.channels = channels;
    a.format = ex.rule.format;
    a.dither = ex.rule.dither;
    a.floor_db = cfg_.floor_db;
    launch_pc_export_begin(a, stream);
    if (any) launch_pc_export(a, max_n, stream);
    launch_pc_export_finish(a, stream);
    OMX_HIP(hipGetLastError());
    if (d_exported) *d_exported = ex.records.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_exported(uint64_t stream_index, omx_program_export_record* dst) {
    if (!exporter_ || stream_index >= n_streams_)
        return pl_refuse("fetch_exported", "the export is not configured, or stream index out of range");
    copy_out(dst, exporter_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_pcm_format_bytes(uint32_t format, uint32_t* bytes) {
    const uint32_t n = pc_format_bytes(format);
    if (!bytes || n == 0) return OMX_ERR_INVALID;
    *bytes = n;
    return OMX_NONE;
}
int omx_program_dither_evaluate(const omx_program_export_rule* rule, uint64_t stream, uint64_t frame, uint32_t channel, double* d) {
    if (!d || !pc_rule_valid(rule) || channel >= OMX_MAX_CHANNELS) return OMX_ERR_INVALID;
    *d = rule->dither == OMX_DITHER_TPDF ? pc_dither(pc_stream_key(rule->seed, stream), kPcGolden * (frame * 8 + channel)) : 0.0;
    return OMX_NONE;
}
int omx_program_loudness_bank_import_pcm(omx_program_loudness_bank* b, const void* d_in, uint32_t format, float* d_out,
                                         uint64_t frames_capacity, const uint32_t* frames, uint32_t channels, void* stream) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.import_pcm(d_in, format, d_out, frames_capacity, frames, channels, static_cast<hipStream_t>(stream)); });
}
int omx_program_loudness_bank_export_configure(omx_program_loudness_bank* b, const omx_program_export_rule* rule, uint32_t channels) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.export_configure(rule, channels); });
}
int omx_program_loudness_bank_export_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.export_reset(reset_mask); });
}
int omx_program_loudness_bank_export_pcm(omx_program_loudness_bank* b, const float* d_in, void* d_out, uint64_t frames_capacity,
                                         const uint32_t* frames, void* stream, const omx_program_export_record** d_exported) {
    if (!b || !d_exported) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.export_pcm(d_in, d_out, frames_capacity, frames, static_cast<hipStream_t>(stream), d_exported); });
}
int omx_program_loudness_bank_fetch_exported(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_export_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_exported(stream_index, dst); });
}

}  // extern "C"
