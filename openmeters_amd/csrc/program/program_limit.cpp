// Host side of the programme bank's limiter (include/omx/program_limit.h): the rule and every call are checked against the host's
// mirror of the streams (frames taken, frames emitted, flushed) before anything is touched, the per-stream table of a call goes up in
// one upload, every launch is on the caller's stream.  Nothing here synchronises except fetch_limited, limiter_configure and
// limiter_reset's wait for its own upload slot.
#include "program_loudness.hpp"

namespace omx {

namespace {

bool lm_rule_valid(const omx_program_limit_rule* rule) {
    if (!rule) return false;
    if (!std::isfinite(rule->ceiling_db) || rule->ceiling_db < -120.0f || rule->ceiling_db > 20.0f) return false;
    if (rule->attack_frames < 1 || rule->attack_frames > 4096 || rule->release_hold_frames > 16384) return false;
    return rule->flags == 0;
}

}  // namespace

int ProgramLoudnessBank::limiter_configure(const omx_program_limit_rule* rule, uint32_t channels, float sample_rate) {
    if (!lm_rule_valid(rule))
        return pl_refuse("limiter_configure", "bad limit rule (null, ceiling_db not finite or outside [-120, 20], attack_frames outside 1 .. 4096, "
                                              "release_hold_frames above 16384 or a flag set)");
    if (!pl_channels_ok(channels)) return pl_refuse("limiter_configure", "channels outside 1 .. 8");
    const float rate = sanitize_sample_rate(sample_rate);
    if (rate < kPlMinRate) unsupported("programme loudness below 3364 Hz: the K-weighting filter has poles outside the unit circle");
    if (limiter_ && carry_holds_frames(limiter_->h_streams))
        return pl_refuse("limiter_configure", "a stream of the limiter holds frames (reset every stream first)");
    if (limiter_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the old buffers may still be in flight)
    auto lim = limiter_ ? std::move(limiter_) : std::make_unique<ProgramLimiter>();
    lim->rule = *rule;
    lim->channels = channels;
    lim->rate = rate;
    lim->ceiling = (float)std::pow(10.0, (double)rule->ceiling_db / 20.0);
    lim->h_streams.assign(n_streams_, CarryLedger{});
    lim->h_calls.assign(n_streams_, LmStreamCall{});
    const uint32_t A = rule->attack_frames, W = A + 24 + rule->release_hold_frames;
    lim->calls.reserve(n_streams_);
    lim->records.reserve(n_streams_);
    lim->ring_x.reserve((size_t)n_streams_ * (A + kLmHistory) * channels);
    lim->ring_q.reserve((size_t)n_streams_ * (W + A - 2));
    limiter_ = std::move(lim);
    const int rc = limiter_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first apply_limited call may come on another stream)
    return rc;
}

LmArgs ProgramLoudnessBank::limiter_args() const {
    const ProgramLimiter& lim = *limiter_;
    LmArgs a{};
    a.n_streams = n_streams_;
    a.channels = lim.channels;
    a.attack = lim.rule.attack_frames;
    a.window = a.attack + 24 + lim.rule.release_hold_frames;
    a.latency = a.attack + kLmHistory;
    a.q_history = a.window + a.attack - 2;
    a.hold_len = std::min(a.window, kLmHoldMaxWindow);
    const double fs = (double)lim.rate;
    a.delay_len = fs < 96000.0 ? 12u : (fs < 192000.0 ? 24u : 0u);  // TruePeakMeter::new (:107-114)
    a.ceiling = lim.ceiling;
    a.floor_db = cfg_.floor_db;
    a.calls = lim.calls.ptr;
    a.records = lim.records.ptr;
    a.ring_x = lim.ring_x.ptr;
    a.ring_q = lim.ring_q.ptr;
    pl_true_peak_fir(a.fir4, a.fir2);
    return a;
}

int ProgramLoudnessBank::limiter_reset(const uint8_t* reset_mask) {
    if (!limiter_) return pl_refuse("limiter_reset", "the limiter is not configured (omx_program_loudness_bank_limiter_configure)");
    ProgramLimiter& lim = *limiter_;
    carry_reset(lim.h_streams, lim.h_calls, reset_mask, [](const CarryLedger&) { return LmStreamCall{}; });
    pl_upload_table(lim.staging, lim.h_calls, lim.calls.ptr, last_stream_);
    const LmArgs a = limiter_args();
    launch_lm_begin(a, false, last_stream_);
    launch_lm_finish(a, last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out, the records and the limiter's state as they were.
int ProgramLoudnessBank::apply_limited(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, uint64_t out_capacity,
                                       const uint8_t* flush_mask, const omx_program_gain_record* d_gains, uint64_t n_gains,
                                       const uint32_t* gain_of_stream, hipStream_t stream, const omx_program_limit_record** d_limited) {
    const char* who = "apply_limited";
    if (!limiter_) return pl_refuse(who, "the limiter is not configured (omx_program_loudness_bank_limiter_configure)");
    ProgramLimiter& lim = *limiter_;
    if (!pl_capacity_ok(frames_capacity) || !pl_capacity_ok(out_capacity))
        return pl_refuse(who, "frames_capacity or out_capacity beyond 2^32 - 1");
    LmArgs a = limiter_args();
    CarryTotals totals;
    bool named = false;
    std::vector<LmStreamCall>& calls = lim.h_calls;  // (host scratch only: the ledger is committed below, after the last check)
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const CarryLedger& m = lim.h_streams[s];
        CarryStep step;
        const auto emitted = [&](uint64_t n, uint64_t e, bool flush) { return carry_emitted(a.latency, n, e, flush); };
        if (const char* why = carry_step(m, frames, frames_capacity, flush_mask, s, out_capacity, emitted, step)) return pl_refuse(who, why);
        const uint64_t index = gain_of_stream ? gain_of_stream[s] : s;  // (tested behind the shared step: a stream wrong in both ways is refused for its frames)
        if (index != OMX_PROGRAM_UNITY_GAIN && index >= n_gains) return pl_refuse(who, "gain index at or above n_gains");
        LmStreamCall c{};
        c.n_old = m.n;
        c.frames = (uint32_t)step.frames;
        c.emit = (uint32_t)step.emit;
        c.held = (uint32_t)(m.n - m.e);
        c.gain_index = (uint32_t)index;
        c.flags = (step.flush ? kCarryFlagFlush : 0u) | (m.n == 0 && step.frames != 0 ? kLmFlagLatch : 0u);
        c.ring_x = (uint32_t)(m.n % a.latency);
        c.ring_q = (uint32_t)(m.n % a.q_history);
        calls[s] = c;
        totals.take(step);
        named = named || ((c.flags & kLmFlagLatch) && index != OMX_PROGRAM_UNITY_GAIN);
    }
    a.max_frames = totals.max_frames;
    a.max_emit = totals.max_emit;
    if (totals.null_pcm(d_in, d_out)) return pl_refuse(who, "null pcm");
    if (named && !d_gains) return pl_refuse(who, "null gain records while a stream names one");
    if (pl_in_out_overlap(d_in, frames_capacity, d_out, out_capacity, n_streams_, a.channels, a.channels)) return pl_refuse(who, "d_in and d_out overlap");

    carry_commit(lim.h_streams, calls);
    last_stream_ = stream;
    pl_upload_table(lim.staging, calls, lim.calls.ptr, stream);
    a.in = d_in;
    a.out = d_out;
    a.frames_capacity = frames_capacity;
    a.out_capacity = out_capacity;
    a.gains = d_gains;
    a.q_row = a.max_frames;
    a.e_row = a.max_emit;
    a.m_row = a.max_emit + (a.attack - 1) + (a.window - a.hold_len);
    launch_lm_begin(a, true, stream);
    if (totals.any_in) {
        lim.q.reserve((size_t)n_streams_ * a.q_row);
        a.q = lim.q.ptr;
        launch_lm_level(a, stream);
    }
    if (totals.any_out) {
        lim.held_min.reserve((size_t)n_streams_ * a.m_row);
        lim.envelope.reserve((size_t)n_streams_ * a.e_row);
        a.held_min = lim.held_min.ptr;
        a.envelope = lim.envelope.ptr;
        launch_lm_hold(a, stream);
        launch_lm_smooth(a, stream);
        launch_lm_apply(a, stream);
    }
    if (totals.any_in) launch_lm_carry(a, stream);
    launch_lm_finish(a, stream);
    OMX_HIP(hipGetLastError());
    if (d_limited) *d_limited = lim.records.ptr;
    return totals.any_out ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_limited(uint64_t stream_index, omx_program_limit_record* dst) {
    if (!limiter_ || stream_index >= n_streams_)
        return pl_refuse("fetch_limited", "the limiter is not configured, or stream index out of range");
    copy_out(dst, limiter_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_limit_latency(const omx_program_limit_rule* rule, uint32_t* frames) {
    if (!frames || !lm_rule_valid(rule)) return OMX_ERR_INVALID;
    *frames = rule->attack_frames + kLmHistory;
    return OMX_NONE;
}
int omx_program_loudness_bank_limiter_configure(omx_program_loudness_bank* b, const omx_program_limit_rule* rule, uint32_t channels,
                                                float sample_rate) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.limiter_configure(rule, channels, sample_rate); });
}
int omx_program_loudness_bank_limiter_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.limiter_reset(reset_mask); });
}
int omx_program_loudness_bank_apply_limited(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity,
                                            const uint32_t* frames, float* d_out, uint64_t out_capacity, const uint8_t* flush_mask,
                                            const omx_program_gain_record* d_gains, uint64_t n_gains, const uint32_t* gain_of_stream,
                                            void* stream, const omx_program_limit_record** d_limited) {
    if (!b || !d_limited) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.apply_limited(d_in, frames_capacity, frames, d_out, out_capacity, flush_mask, d_gains, n_gains, gain_of_stream,
                                     static_cast<hipStream_t>(stream), d_limited);
    });
}
int omx_program_loudness_bank_fetch_limited(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_limit_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_limited(stream_index, dst); });
}

}  // extern "C"
