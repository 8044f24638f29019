// Host side of the programme bank's normalisation (include/omx/program_normalize.h): the rule and the call arguments are checked
// against the host's own values before anything is touched, the per-stream table of an apply call goes up in one upload, every
// launch is on the caller's stream.  Nothing here synchronises except fetch_gains and fetch_applied.
#include "program_gain_device.hpp"
#include "program_loudness.hpp"

namespace omx {

namespace {

bool pn_rule_valid(const omx_program_gain_rule* rule) {
    if (!rule) return false;
    if ((rule->flags & ~OMX_GAIN_LIMIT_PEAK) != 0) return false;
    if (!std::isfinite(rule->target_lufs) || !std::isfinite(rule->min_gain_db) || !std::isfinite(rule->max_gain_db)) return false;
    if ((rule->flags & OMX_GAIN_LIMIT_PEAK) && !std::isfinite(rule->true_peak_ceiling_db)) return false;
    return rule->min_gain_db <= rule->max_gain_db;
}

int bad_rule(const char* who) {
    return pl_refuse(who, "bad gain rule (null, a non-finite field in use, min_gain_db > max_gain_db or an unknown flag)");
}

}  // namespace

int ProgramLoudnessBank::plan_gains(const omx_program_gain_rule* rule, hipStream_t stream, const omx_program_gain_record** d_gains) {
    if (!pn_rule_valid(rule)) return bad_rule("plan_gains");
    if (dirty_) results(stream, nullptr);
    last_stream_ = stream;
    gain_records_.reserve(n_streams_);
    launch_pn_plan(*rule, records_.ptr, gain_records_.ptr, n_streams_, cfg_.floor_db, stream);
    OMX_HIP(hipGetLastError());
    gains_planned_ = n_streams_;
    if (d_gains) *d_gains = gain_records_.ptr;
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::plan_group_gains(const omx_program_gain_rule* rule, const omx_program_interval* members, uint64_t n_members,
                                          const omx_program_group* groups, uint64_t n_groups, hipStream_t stream,
                                          const omx_program_gain_record** d_gains) {
    if (!pn_rule_valid(rule)) return bad_rule("plan_group_gains");
    // measure_groups checks everything else before it touches anything (n_groups == 0: OMX_NONE), then measures on `stream`
    const int rc = measure_groups(members, n_members, groups, n_groups, stream, nullptr);
    if (rc != OMX_PRODUCED) return rc;
    if (dirty_) results(stream, nullptr);  // the member streams' peaks are read from their records
    gain_records_.reserve(n_groups);
    const PgMember* dm = reinterpret_cast<const PgMember*>(group_tables_.ptr);
    const PgGroup* dg = reinterpret_cast<const PgGroup*>(group_tables_.ptr + (size_t)n_members * sizeof(PgMember));
    launch_pn_plan_groups(*rule, group_records_.ptr, records_.ptr, dm, dg, gain_records_.ptr, (uint32_t)n_groups, cfg_.floor_db, stream);
    OMX_HIP(hipGetLastError());
    gains_planned_ = n_groups;
    if (d_gains) *d_gains = gain_records_.ptr;
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::fetch_gains(uint64_t first, uint64_t count, omx_program_gain_record* dst) {
    if (gains_planned_ == 0) return pl_refuse("fetch_gains", "no plan yet (plan_gains / plan_group_gains)");
    if (first > gains_planned_ || count > gains_planned_ - first || (!dst && count != 0))
        return pl_refuse("fetch_gains", "range outside the last plan (or null records)");
    if (count == 0) return OMX_NONE;
    copy_out(dst, gain_records_.ptr + first, (size_t)count * sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out, the gain records and the apply records as they were.
int ProgramLoudnessBank::apply_gains(const float* d_in, float* d_out, uint64_t frames_capacity, const uint32_t* frames, uint32_t channels,
                                     const omx_program_gain_record* d_gains, uint64_t n_gains, const uint32_t* gain_of_stream,
                                     hipStream_t stream, const omx_program_apply_record** d_applied) {
    const char* who = "apply_gains";
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    bool any = false, named = false;
    uint64_t max_n = 0;
    h_apply_calls_.resize(n_streams_);  // (host scratch only: what the device holds is untouched until the upload below)
    for (uint32_t s = 0; s < n_streams_; ++s) {
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        const uint64_t index = gain_of_stream ? gain_of_stream[s] : s;  // (a bank of 2^32 - 1 streams and more does not exist: s is never the unity index)
        if (index != OMX_PROGRAM_UNITY_GAIN && index >= n_gains) return pl_refuse(who, "gain index at or above n_gains");
        any = any || f != 0;
        named = named || index != OMX_PROGRAM_UNITY_GAIN;
        h_apply_calls_[s] = PnStreamCall{f * channels, (uint32_t)index, 0};
        max_n = std::max(max_n, f * channels);
    }
    if (any && (!d_in || !d_out)) return pl_refuse(who, "null pcm");
    if (named && !d_gains) return pl_refuse(who, "null gain records while a stream names one");
    // in place is fine; any other overlap would let a tile read what another has already scaled
    const unsigned __int128 bytes = (unsigned __int128)n_streams_ * frames_capacity * channels * sizeof(float);
    if (any && d_in != d_out && pl_ranges_overlap(d_in, bytes, d_out, bytes))
        return pl_refuse(who, "d_in and d_out overlap without being the same buffer");

    last_stream_ = stream;
    apply_calls_.reserve(n_streams_);
    apply_records_.reserve(n_streams_);
    pl_upload_table(apply_staging_, h_apply_calls_, apply_calls_.ptr, stream);
    PnApplyArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.row = frames_capacity * channels;
    a.calls = apply_calls_.ptr;
    a.gains = d_gains;
    a.applied = apply_records_.ptr;
    a.n_streams = n_streams_;
    a.channels = channels;
    a.floor_db = cfg_.floor_db;
    launch_pn_begin(a, stream);
    if (any) {
        // (tuning library only: OMX_NORMALIZE_STORES=nt stores the scaled PCM of an out-of-place call non-temporally, for the A/B)
        const char* stores = tuning_env("OMX_NORMALIZE_STORES");
        launch_pn_tiles(a, max_n, stores && stores[0] == 'n' && d_in != d_out, stream);
    }
    launch_pn_finish(a, stream);
    OMX_HIP(hipGetLastError());
    applied_ = true;
    if (d_applied) *d_applied = apply_records_.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_applied(uint64_t stream_index, omx_program_apply_record* dst) {
    if (!applied_ || stream_index >= n_streams_) return pl_refuse("fetch_applied", "no apply_gains call yet, or stream index out of range");
    copy_out(dst, apply_records_.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_gain_evaluate(const omx_program_gain_rule* rule, float integrated_lufs, uint64_t gating_above_relative,
                              float max_true_peak_db, float floor_db, omx_program_gain_record* out) {
    if (!out || !pn_rule_valid(rule)) return OMX_ERR_INVALID;
    *out = pn_gain(*rule, integrated_lufs, gating_above_relative, max_true_peak_db, floor_db);
    return OMX_NONE;
}
int omx_program_loudness_bank_plan_gains(omx_program_loudness_bank* b, const omx_program_gain_rule* rule, void* stream,
                                         const omx_program_gain_record** d_gains) {
    if (!b || !d_gains) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.plan_gains(rule, static_cast<hipStream_t>(stream), d_gains); });
}
int omx_program_loudness_bank_plan_group_gains(omx_program_loudness_bank* b, const omx_program_gain_rule* rule,
                                               const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                               uint64_t n_groups, void* stream, const omx_program_gain_record** d_gains) {
    if (!b || !d_gains) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.plan_group_gains(rule, members, n_members, groups, n_groups, static_cast<hipStream_t>(stream), d_gains); });
}
int omx_program_loudness_bank_fetch_gains(omx_program_loudness_bank* b, uint64_t first, uint64_t count, omx_program_gain_record* dst) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_gains(first, count, dst); });
}
int omx_program_loudness_bank_apply_gains(omx_program_loudness_bank* b, const float* d_in, float* d_out, uint64_t frames_capacity,
                                          const uint32_t* frames, uint32_t channels, const omx_program_gain_record* d_gains,
                                          uint64_t n_gains, const uint32_t* gain_of_stream, void* stream,
                                          const omx_program_apply_record** d_applied) {
    if (!b || !d_applied) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.apply_gains(d_in, d_out, frames_capacity, frames, channels, d_gains, n_gains, gain_of_stream,
                                   static_cast<hipStream_t>(stream), d_applied);
    });
}
int omx_program_loudness_bank_fetch_applied(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_apply_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_applied(stream_index, dst); });
}

}  // extern "C"
