// Host side of the programme bank's signal QC (include/omx/program_inspect.h): the rule's defaults, the plan and the summary (plain
// C double arithmetic, no device), and the calls.  Every call is checked before anything is touched, the per-stream frame counts of
// a call go up in one upload, every launch is on the caller's stream.  Nothing here synchronises except fetch_inspected and
// inspect_configure.
#include "program_loudness.hpp"

namespace omx {

namespace {

bool in_rule_valid(const omx_program_inspect_rule* r) {
    return r && std::isfinite(r->clip_level) && r->clip_level > 0.0f && r->clip_min_run >= 1 && r->clip_min_run <= OMX_INSPECT_MAX_CLIP_MIN_RUN &&
           std::isfinite(r->silence_level) && r->silence_level >= 0.0f && r->silence_min_run >= 1 &&
           r->silence_min_run <= OMX_INSPECT_MAX_SILENCE_MIN_RUN && std::isfinite(r->dc_limit) && r->dc_limit >= 0.0f &&
           r->correlation_min >= -1.0f && r->correlation_min <= 1.0f && r->flags == 0;
}

const char* kBadRule =
    "bad inspect rule (null, clip_level not finite or <= 0, clip_min_run outside 1 .. 65535, silence_level not finite or < 0, "
    "silence_min_run outside 1 .. 2^24, dc_limit not finite or < 0, correlation_min outside [-1, 1] or a flag set)";

}  // namespace

int in_rule_default(omx_program_inspect_rule* rule) {
    if (!rule) return pl_refuse("inspect rule_default", "null rule");
    omx_program_inspect_rule out{};
    out.clip_level = OMX_INSPECT_DEFAULT_CLIP_LEVEL;
    out.clip_min_run = OMX_INSPECT_DEFAULT_CLIP_MIN_RUN;
    out.silence_level = OMX_INSPECT_DEFAULT_SILENCE_LEVEL;
    out.silence_min_run = OMX_INSPECT_DEFAULT_SILENCE_MIN_RUN;
    out.dc_limit = OMX_INSPECT_DEFAULT_DC_LIMIT;
    out.correlation_min = OMX_INSPECT_DEFAULT_CORRELATION_MIN;
    out.flags = 0;
    *rule = out;
    return OMX_NONE;
}

int in_plan(uint32_t channels, omx_program_inspect_info* info) {
    if (!info) return pl_refuse("inspect plan", "null info");
    if (!pl_channels_ok(channels)) return pl_refuse("inspect plan", "channels outside 1 .. 8");
    omx_program_inspect_info out{};
    out.tile_frames = in_tile_frames(channels);
    out.channels = channels;
    *info = out;
    return OMX_NONE;
}

int in_summarize(const omx_program_inspect_rule* rule, const omx_program_inspect_record* record, omx_program_inspect_summary* summary) {
    const char* who = "inspect summarize";
    if (!record || !summary) return pl_refuse(who, "null pointer");
    if (!in_rule_valid(rule)) return pl_refuse(who, kBadRule);
    if (!pl_channels_ok(record->channels)) return pl_refuse(who, "record->channels outside 1 .. 8");
    if (record->n_pairs > OMX_INSPECT_MAX_PAIRS) return pl_refuse(who, "record->n_pairs above OMX_INSPECT_MAX_PAIRS");
    omx_program_inspect_summary out{};
    out.channels = record->channels;
    out.n_pairs = record->n_pairs;
    uint32_t verdict = 0;
    for (uint32_t c = 0; c < record->channels; ++c) {
        const omx_program_inspect_channel& ch = record->channel[c];
        const float dc = record->frames ? (float)((double)ch.dc_sum / 268435456.0 / (double)record->frames) : 0.0f;
        out.dc_offset[c] = dc;
        const double mag = std::fabs((double)dc);
        out.dc_offset_db[c] = mag > 0.0 ? (float)std::fmax(20.0 * std::log10(mag), (double)OMX_INSPECT_DB_FLOOR) : OMX_INSPECT_DB_FLOOR;
        if (ch.nan_samples) verdict |= OMX_INSPECT_NAN;
        if (ch.clip_runs) verdict |= OMX_INSPECT_CLIPPED;
        if (std::fabs(dc) > rule->dc_limit) verdict |= OMX_INSPECT_DC;
    }
    for (uint32_t p = 0; p < record->n_pairs; ++p) {
        const omx_program_inspect_pair& pr = record->pair[p];
        const bool valid = pr.sum_aa > 0 && pr.sum_bb > 0;
        float corr = 0.0f;
        if (valid) {
            const double v = (double)pr.sum_ab / std::sqrt((double)pr.sum_aa * (double)pr.sum_bb);
            corr = (float)std::fmin(std::fmax(v, -1.0), 1.0);
        }
        out.correlation[p] = corr;
        out.correlation_valid[p] = valid ? 1u : 0u;
        if (valid && corr < rule->correlation_min) verdict |= OMX_INSPECT_ANTIPHASE;
    }
    const uint64_t lead = record->leading_silence >= rule->silence_min_run ? 1 : 0;
    const uint64_t trail = (record->trailing_silence >= rule->silence_min_run && record->leading_silence < record->frames) ? 1 : 0;
    out.interior_silent_runs = record->silent_runs - lead - trail;
    if (out.interior_silent_runs > 0) verdict |= OMX_INSPECT_DROPOUT;
    if (record->frames > 0 && record->leading_silence == record->frames) verdict |= OMX_INSPECT_ALL_SILENT;
    out.verdict = verdict;
    *summary = out;
    return OMX_NONE;
}

int ProgramLoudnessBank::inspect_configure(const omx_program_inspect_rule* rule, uint32_t channels, const uint32_t* pairs, uint32_t n_pairs) {
    const char* who = "inspect_configure";
    if (!in_rule_valid(rule)) return pl_refuse(who, kBadRule);
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (n_pairs > OMX_INSPECT_MAX_PAIRS) return pl_refuse(who, "n_pairs above OMX_INSPECT_MAX_PAIRS");
    if (n_pairs && !pairs) return pl_refuse(who, "null pairs");
    for (uint32_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= channels || pairs[2 * p + 1] >= channels || pairs[2 * p] == pairs[2 * p + 1])
            return pl_refuse(who, "a pair index at or above channels, or a pair of one channel");
    if (inspector_)
        for (const uint64_t n : inspector_->h_frames)
            if (n != 0) return pl_refuse(who, "a stream of the inspector holds frames (reset every stream first)");
    if (inspector_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the old buffers may still be in flight)
    auto in = inspector_ ? std::move(inspector_) : std::make_unique<ProgramInspector>();
    in->rule = *rule;
    in->channels = channels;
    in->n_pairs = n_pairs;
    for (uint32_t p = 0; p < OMX_INSPECT_MAX_PAIRS; ++p) {
        in->pair_a[p] = p < n_pairs ? pairs[2 * p] : 0;
        in->pair_b[p] = p < n_pairs ? pairs[2 * p + 1] : 0;
    }
    in->h_frames.assign(n_streams_, 0);
    in->h_call.assign(n_streams_, 0);
    in->call.reserve(n_streams_);
    in->records.reserve(n_streams_);
    inspector_ = std::move(in);
    const int rc = inspect_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first inspect call may come on another stream)
    return rc;
}

InArgs ProgramLoudnessBank::inspect_args() const {
    const ProgramInspector& in = *inspector_;
    InArgs a{};
    a.n_streams = n_streams_;
    a.channels = in.channels;
    a.n_pairs = in.n_pairs;
    a.clip_min_run = in.rule.clip_min_run;
    a.silence_min_run = in.rule.silence_min_run;
    a.clip_level = in.rule.clip_level;
    a.silence_level = in.rule.silence_level;
    for (uint32_t p = 0; p < OMX_INSPECT_MAX_PAIRS; ++p) {
        a.pair_a[p] = in.pair_a[p];
        a.pair_b[p] = in.pair_b[p];
    }
    a.frames = in.call.ptr;
    a.records = in.records.ptr;
    a.runs = in.runs.ptr;
    a.sums = in.sums.ptr;
    return a;
}

int ProgramLoudnessBank::inspect_reset(const uint8_t* reset_mask) {
    if (!inspector_) return pl_refuse("inspect_reset", "the inspector is not configured (omx_program_loudness_bank_inspect_configure)");
    ProgramInspector& in = *inspector_;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const bool clear = !reset_mask || reset_mask[s];
        if (clear) in.h_frames[s] = 0;
        in.h_call[s] = clear ? 1u : 0u;
    }
    pl_upload_table(in.staging, in.h_call, in.call.ptr, last_stream_);
    launch_in_reset(inspect_args(), last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves the records and the host's mirror as they were.
int ProgramLoudnessBank::inspect(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, hipStream_t stream,
                                 const omx_program_inspect_record** d_inspected) {
    const char* who = "inspect";
    if (!inspector_) return pl_refuse(who, "the inspector is not configured (omx_program_loudness_bank_inspect_configure)");
    ProgramInspector& in = *inspector_;
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    uint32_t max_frames = 0;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        if (in.h_frames[s] + f > 0xFFFFFFFFull) return pl_refuse(who, "a stream would hold more than 2^32 - 1 frames since its reset");
        in.h_call[s] = (uint32_t)f;  // (host scratch only)
        max_frames = std::max(max_frames, (uint32_t)f);
    }
    const bool any = max_frames != 0;
    if (any && !d_in) return pl_refuse(who, "null pcm");

    last_stream_ = stream;
    if (any) {
        const uint32_t tile = in_tile_frames(in.channels);
        const uint64_t tiles = ((uint64_t)max_frames + tile - 1) / tile;
        in.runs.reserve((size_t)n_streams_ * tiles * (in.channels + 1));
        in.sums.reserve((size_t)n_streams_ * tiles * (2 * in.channels + 3 * in.n_pairs));
        pl_upload_table(in.staging, in.h_call, in.call.ptr, stream);
        InArgs a = inspect_args();
        a.in = d_in;
        a.frames_capacity = frames_capacity;
        a.max_frames = max_frames;
        a.tiles = (uint32_t)tiles;
        launch_in_main(a, stream);
        launch_in_fold(a, stream);
        OMX_HIP(hipGetLastError());
        for (uint32_t s = 0; s < n_streams_; ++s) in.h_frames[s] += in.h_call[s];
    }
    *d_inspected = in.records.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_inspected(uint64_t stream_index, omx_program_inspect_record* dst) {
    if (!inspector_ || stream_index >= n_streams_)
        return pl_refuse("fetch_inspected", "the inspector is not configured, or stream index out of range");
    copy_out(dst, inspector_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_inspect_rule_default(omx_program_inspect_rule* rule) { return in_rule_default(rule); }
int omx_program_inspect_plan(uint32_t channels, omx_program_inspect_info* info) { return in_plan(channels, info); }
int omx_program_inspect_summarize(const omx_program_inspect_rule* rule, const omx_program_inspect_record* record,
                                  omx_program_inspect_summary* summary) {
    return in_summarize(rule, record, summary);
}
int omx_program_loudness_bank_inspect_configure(omx_program_loudness_bank* b, const omx_program_inspect_rule* rule, uint32_t channels,
                                                const uint32_t* pairs, uint32_t n_pairs) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.inspect_configure(rule, channels, pairs, n_pairs); });
}
int omx_program_loudness_bank_inspect_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.inspect_reset(reset_mask); });
}
int omx_program_loudness_bank_inspect(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                      void* stream, const omx_program_inspect_record** d_inspected) {
    if (!b || !d_inspected) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.inspect(d_in, frames_capacity, frames, static_cast<hipStream_t>(stream), d_inspected); });
}
int omx_program_loudness_bank_fetch_inspected(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_inspect_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_inspected(stream_index, dst); });
}

}  // extern "C"
