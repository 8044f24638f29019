// Host side of the programme bank's convolve stage (include/omx/program_convolve.h): the C ABI of the host-only functions
// (program_convolve_plan.hpp holds them), the tables of a configured set of FIRs, and the calls.  Every call is checked against the
// host's mirror of the streams (frames taken, frames emitted, flushed) before anything is touched, the per-stream table of a call goes
// up in one upload, every launch is on the caller's stream.  Nothing here synchronises except fetch_convolved, convolve_configure and
// convolve_reset's wait for its own upload slot.
#include "program_loudness.hpp"

namespace omx {

namespace {

int cv_refusal(const char* who, int rc, const char* why) {
    pl_refuse(who, why ? why : "refused");
    return rc;
}

}  // namespace

int ProgramLoudnessBank::convolve_configure(uint32_t channels, const omx_program_fir* firs, uint32_t n_firs, const uint32_t* fir_of_channel,
                                            uint32_t delay_frames) {
    const char* who = "convolve_configure";
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (!firs) return pl_refuse(who, "null table");
    if (n_firs == 0 || n_firs > OMX_CONVOLVE_MAX_FIRS) return pl_refuse(who, "n_firs 0 or above OMX_CONVOLVE_MAX_FIRS");
    for (uint32_t k = 0; k < n_firs; ++k) {
        const char* why = nullptr;
        const int rc = cv_check(firs + k, &why);
        if (rc != OMX_NONE) return cv_refusal(who, rc, why);
    }
    // the table as f64, each FIR from a multiple of 8 (the conversion is exact; the kernel converts no tap)
    std::vector<uint32_t> first(n_firs);
    std::vector<double> taps;
    for (uint32_t k = 0; k < n_firs; ++k) {
        first[k] = (uint32_t)taps.size();
        for (uint32_t i = 0; i < firs[k].n_taps; ++i) taps.push_back((double)firs[k].taps[i]);
        taps.resize((taps.size() + 7) / 8 * 8, 0.0);
    }
    std::vector<CvChannel> chan((size_t)n_streams_ * OMX_MAX_CHANNELS, CvChannel{0u, 0u});
    std::vector<uint32_t> longest(n_streams_, 0u);
    std::vector<uint8_t> bypassed(n_streams_, 0);
    uint32_t max_taps = 1;
    for (uint32_t s = 0; s < n_streams_; ++s)
        for (uint32_t c = 0; c < channels; ++c) {
            const uint32_t f = fir_of_channel ? fir_of_channel[(size_t)s * channels + c] : 0u;
            if (f == OMX_CONVOLVE_BYPASS) {
                bypassed[s] = 1;
                continue;
            }
            if (f >= n_firs) return pl_refuse(who, "a FIR index that is neither below n_firs nor OMX_CONVOLVE_BYPASS");
            chan[(size_t)s * OMX_MAX_CHANNELS + c] = CvChannel{first[f], firs[f].n_taps};
            longest[s] = std::max(longest[s], firs[f].n_taps);
            max_taps = std::max(max_taps, firs[f].n_taps);
        }
    if (delay_frames > max_taps - 1) return pl_refuse(who, "delay_frames > max_taps - 1");
    if (convolve_ && carry_holds_frames(convolve_->h_streams)) return pl_refuse(who, "a stream of the stage holds frames (reset every stream first)");
    if (convolve_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the old buffers may still be in flight)

    auto cv = convolve_ ? std::move(convolve_) : std::make_unique<ProgramConvolve>();
    cv->channels = channels;
    cv->delay = delay_frames;
    cv->max_taps = max_taps;
    cv->h_streams.assign(n_streams_, CarryLedger{});
    cv->h_calls.assign(n_streams_, CvStreamCall{});
    cv->h_reach.assign(n_streams_, 0u);
    for (uint32_t s = 0; s < n_streams_; ++s) cv->h_reach[s] = std::max(longest[s], bypassed[s] ? delay_frames + 1 : 1u);
    cv->taps.upload(taps, last_stream_);
    cv->chan.upload(chan, last_stream_);
    cv->calls.reserve(n_streams_);
    cv->records.reserve(n_streams_);
    cv->ring.reserve((size_t)n_streams_ * (max_taps - 1) * channels);
    convolve_ = std::move(cv);
    const int rc = convolve_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first convolve call may come on another stream)
    return rc;
}

CvArgs ProgramLoudnessBank::convolve_args() const {
    const ProgramConvolve& cv = *convolve_;
    CvArgs a{};
    a.n_streams = n_streams_;
    a.channels = cv.channels;
    a.delay = cv.delay;
    a.max_taps = cv.max_taps;
    a.history = cv.max_taps - 1;
    a.floor_db = cfg_.floor_db;
    a.taps = cv.taps.ptr;
    a.chan = cv.chan.ptr;
    a.calls = cv.calls.ptr;
    a.records = cv.records.ptr;
    a.ring = cv.ring.ptr;
    return a;
}

int ProgramLoudnessBank::convolve_reset(const uint8_t* reset_mask) {
    if (!convolve_) return pl_refuse("convolve_reset", "the stage is not configured (omx_program_loudness_bank_convolve_configure)");
    ProgramConvolve& cv = *convolve_;
    carry_reset(cv.h_streams, cv.h_calls, reset_mask, [](const CarryLedger&) { return CvStreamCall{}; });
    pl_upload_table(cv.staging, cv.h_calls, cv.calls.ptr, last_stream_);
    const CvArgs a = convolve_args();
    launch_cv_begin(a, false, last_stream_);
    launch_cv_finish(a, last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out, the records and the stage's state as they were.
int ProgramLoudnessBank::convolve(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, uint64_t out_capacity,
                                  const uint8_t* flush_mask, hipStream_t stream, const omx_program_convolve_record** d_convolved) {
    const char* who = "convolve";
    if (!convolve_) return pl_refuse(who, "the stage is not configured (omx_program_loudness_bank_convolve_configure)");
    ProgramConvolve& cv = *convolve_;
    if (!pl_capacity_ok(frames_capacity) || !pl_capacity_ok(out_capacity))
        return pl_refuse(who, "frames_capacity or out_capacity beyond 2^32 - 1");
    CvArgs a = convolve_args();
    CarryTotals totals;
    std::vector<CvStreamCall>& calls = cv.h_calls;  // (host scratch only: the ledger is committed below, after the last check)
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const CarryLedger& m = cv.h_streams[s];
        CarryStep step;
        const auto emitted = [&](uint64_t n, uint64_t e, bool flush) { return carry_emitted(cv.delay, n, e, flush); };
        if (const char* why = carry_step(m, frames, frames_capacity, flush_mask, s, out_capacity, emitted, step)) return pl_refuse(who, why);
        CvStreamCall c{};
        c.n_old = m.n;
        c.e_old = m.e;
        c.rel_e = (int64_t)(m.e + cv.delay) - (int64_t)m.n;
        c.frames = (uint32_t)step.frames;
        c.emit = (uint32_t)step.emit;
        c.ring = a.history ? (uint32_t)(m.n % a.history) : 0u;
        c.flags = step.flush ? kCarryFlagFlush : 0u;
        c.reach = cv.h_reach[s];
        calls[s] = c;
        totals.take(step);
    }
    a.max_frames = totals.max_frames;
    a.max_emit = totals.max_emit;
    if (totals.null_pcm(d_in, d_out)) return pl_refuse(who, "null pcm");
    if (pl_in_out_overlap(d_in, frames_capacity, d_out, out_capacity, n_streams_, a.channels, a.channels)) return pl_refuse(who, "d_in and d_out overlap");

    carry_commit(cv.h_streams, calls);
    last_stream_ = stream;
    pl_upload_table(cv.staging, calls, cv.calls.ptr, stream);
    a.in = d_in;
    a.out = d_out;
    a.frames_capacity = frames_capacity;
    a.out_capacity = out_capacity;
    launch_cv_begin(a, true, stream);
    if (totals.any_out) launch_cv_main(a, stream);
    if (totals.any_in) launch_cv_carry(a, stream);
    launch_cv_finish(a, stream);
    OMX_HIP(hipGetLastError());
    if (d_convolved) *d_convolved = cv.records.ptr;
    return totals.any_out ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_convolved(uint64_t stream_index, omx_program_convolve_record* dst) {
    if (!convolve_ || stream_index >= n_streams_)
        return pl_refuse("fetch_convolved", "the stage is not configured, or stream index out of range");
    copy_out(dst, convolve_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_convolve_plan(uint32_t channels, uint32_t max_taps, omx_program_convolve_info* info) {
    const char* why = nullptr;
    const int rc = cv_plan(channels, max_taps, info, &why);
    return rc == OMX_NONE ? rc : cv_refusal("convolve plan", rc, why);
}
int omx_program_convolve_frames(uint32_t delay_frames, uint64_t frames_in_before, uint64_t frames_out_before, uint64_t frames,
                                uint32_t flush, uint64_t* frames_out) {
    const char* why = nullptr;
    const int rc = cv_frames(delay_frames, frames_in_before, frames_out_before, frames, flush, frames_out, &why);
    return rc == OMX_NONE ? rc : cv_refusal("convolve frames", rc, why);
}
int omx_program_convolve_check(const omx_program_fir* fir) {
    const char* why = nullptr;
    const int rc = cv_check(fir, &why);
    return rc == OMX_NONE ? rc : cv_refusal("convolve check", rc, why);
}
int omx_program_convolve_design(const omx_program_convolve_spec* spec, double sample_rate, float* taps_out, uint32_t n_floats) {
    return guarded([&] {
        const char* why = nullptr;
        const int rc = cv_design(spec, sample_rate, taps_out, n_floats, &why);
        return rc == OMX_NONE ? rc : cv_refusal("convolve design", rc, why);
    });
}
int omx_program_convolve_response(const omx_program_fir* fir, double sample_rate, double frequency_hz, double* magnitude_db,
                                  double* phase_rad) {
    const char* why = nullptr;
    const int rc = cv_response(fir, sample_rate, frequency_hz, magnitude_db, phase_rad, &why);
    return rc == OMX_NONE ? rc : cv_refusal("convolve response", rc, why);
}
int omx_program_loudness_bank_convolve_configure(omx_program_loudness_bank* b, uint32_t channels, const omx_program_fir* firs,
                                                 uint32_t n_firs, const uint32_t* fir_of_channel, uint32_t delay_frames) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.convolve_configure(channels, firs, n_firs, fir_of_channel, delay_frames); });
}
int omx_program_loudness_bank_convolve_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.convolve_reset(reset_mask); });
}
int omx_program_loudness_bank_convolve(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                       float* d_out, uint64_t out_capacity, const uint8_t* flush_mask, void* stream,
                                       const omx_program_convolve_record** d_convolved) {
    if (!b || !d_convolved) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.convolve(d_in, frames_capacity, frames, d_out, out_capacity, flush_mask, static_cast<hipStream_t>(stream), d_convolved);
    });
}
int omx_program_loudness_bank_fetch_convolved(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_convolve_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_convolved(stream_index, dst); });
}

}  // extern "C"
