// Host side of the programme bank's long-term spectrum (include/omx/program_spectrum.h): the C ABI of the host-only functions
// (program_spectrum_plan.hpp) and the calls.  Every call is checked before anything is touched; the host mirrors every count of a
// stream, so a call's table goes up in one upload and every launch is on the caller's stream.  Nothing here synchronises except
// fetch_spectrum and spectrum_configure.
#include "program_loudness.hpp"

namespace omx {

namespace {

int sp_refusal(const char* who, int rc, const char* why) {
    pl_refuse(who, why ? why : "refused");
    return rc;
}

const char* kSpNotConfigured = "the spectrum stage is not configured (omx_program_loudness_bank_spectrum_configure)";

// a host-only function of the header behind the C ABI: nothing unwinds across it (summarize and match allocate)
template <class F>
int sp_host(const char* who, F&& body) {
    const char* why = nullptr;
    int rc;
    try {
        rc = body(&why);
    } catch (const std::exception&) {
        rc = OMX_ERR_BACKEND;
        why = "out of memory";
    }
    return rc == OMX_NONE ? rc : sp_refusal(who, rc, why);
}

}  // namespace

int ProgramLoudnessBank::spectrum_configure(const omx_program_spectrum_rule* rule, uint32_t channels) {
    const char* who = "spectrum_configure";
    if (!sp_rule_ok(rule)) return pl_refuse(who, kSpBadRule);
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (spectrum_)
        for (const uint64_t n : spectrum_->h_frames)
            if (n != 0) return pl_refuse(who, "a stream of the spectrum stage holds frames (reset every stream first)");
    if (spectrum_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the old buffers may still be in flight)
    auto sp = spectrum_ ? std::move(spectrum_) : std::make_unique<ProgramSpectrum>();
    const uint32_t n = rule->fft_size, bins = n / 2 + 1;
    sp->rule = *rule;
    sp->channels = channels;
    sp->h_frames.assign(n_streams_, 0);
    sp->h_taken.assign(n_streams_, 0);
    sp->h_carried.assign(n_streams_, 0);
    sp->h_parity.assign(n_streams_, 0);
    sp->h_finished.assign(n_streams_, 0);
    sp->h_call.assign(n_streams_, SpCall{});
    sp->call.reserve(n_streams_);
    sp->records.reserve(n_streams_);
    const size_t per = (size_t)n_streams_ * channels * bins;
    sp->sums.reserve(per);
    sp->closed.reserve(per);
    sp->open.reserve(per);
    sp->carry.reserve((size_t)2 * n_streams_ * n * channels);
    std::vector<float> window(n);
    for (uint32_t i = 0; i < n; ++i) window[i] = sp_window_at(n, i);
    sp->window.upload(window, last_stream_);
    sp->tw256.upload(twiddle_table(256, 256), last_stream_);
    sp->tw_half.upload(twiddle_table(n / 2, n / 2), last_stream_);
    sp->tw_full.upload(twiddle_table(n, n / 2), last_stream_);
    spectrum_ = std::move(sp);
    const int rc = spectrum_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first spectrum call may come on another stream)
    return rc;
}

SpArgs ProgramLoudnessBank::spectrum_args() const {
    const ProgramSpectrum& sp = *spectrum_;
    SpArgs a{};
    a.n_streams = n_streams_;
    a.channels = sp.channels;
    a.fft_size = sp.rule.fft_size;
    a.calls = sp.call.ptr;
    a.records = sp.records.ptr;
    a.sums = sp.sums.ptr;
    a.closed = sp.closed.ptr;
    a.open = sp.open.ptr;
    a.rows = sp.rows.ptr;
    a.carry = sp.carry.ptr;
    a.window = sp.window.ptr;
    a.tw256 = sp.tw256.ptr;
    a.tw_half = sp.tw_half.ptr;
    a.tw_full = sp.tw_full.ptr;
    return a;
}

int ProgramLoudnessBank::spectrum_reset(const uint8_t* reset_mask) {
    if (!spectrum_) return pl_refuse("spectrum_reset", kSpNotConfigured);
    ProgramSpectrum& sp = *spectrum_;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const bool clear = !reset_mask || reset_mask[s];
        if (clear) {
            sp.h_frames[s] = sp.h_taken[s] = 0;
            sp.h_carried[s] = 0;
            sp.h_finished[s] = 0;
        }
        sp.h_call[s] = SpCall{};
        sp.h_call[s].frames = clear ? 1u : 0u;
    }
    pl_upload_table(sp.staging, sp.h_call, sp.call.ptr, last_stream_);
    launch_sp_reset(spectrum_args(), last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves the records, the sums and the host's mirror as they were.
int ProgramLoudnessBank::spectrum(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, const uint8_t* finish_mask,
                                  hipStream_t stream, const omx_program_spectrum_record** d_records, const double** d_sums) {
    const char* who = "spectrum";
    if (!spectrum_) return pl_refuse(who, kSpNotConfigured);
    ProgramSpectrum& sp = *spectrum_;
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    const uint32_t n = sp.rule.fft_size, hop = n / 2, ch = sp.channels;
    bool any = false, brings = false;
    uint64_t max_rows = 0, max_move = 0;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        if (sp.h_frames[s] + f > 0xFFFFFFFFull) return pl_refuse(who, "a stream would hold more than 2^32 - 1 frames since its reset");
        if (f && sp.h_finished[s]) return pl_refuse(who, "frames for a stream that is finished (spectrum_reset lets it start over)");
        const bool done = sp.h_finished[s] != 0, finish = finish_mask && finish_mask[s] && !done;
        const uint64_t held = sp.h_frames[s] + f, k0 = sp.h_taken[s];
        const uint64_t k1 = done ? k0 : sp_transforms_of(held, finish, n), k_next = sp_transforms_of(held, false, n);
        SpCall c{};  // (host scratch only until the call is accepted)
        c.frames = (uint32_t)f;
        c.carried = sp.h_carried[s];
        c.k0 = (uint32_t)k0;
        c.nk = (uint32_t)(k1 - k0);
        c.shift = finish || done ? 0u : (uint32_t)((k_next - k0) * hop);
        c.keep = finish || done ? 0u : (uint32_t)(held - k_next * hop);
        c.parity = sp.h_parity[s];
        c.finish = finish ? 1u : 0u;
        sp.h_call[s] = c;
        any = any || f != 0 || finish;
        brings = brings || f != 0;
        max_rows = std::max(max_rows, sp_runs_touched(k0, k1));
        if (!finish && !done) max_move = std::max<uint64_t>(max_move, (uint64_t)(c.shift ? c.keep : c.keep - c.carried) * ch);
    }
    if (brings && !d_in) return pl_refuse(who, "null pcm");

    last_stream_ = stream;
    if (any) {
        sp.rows.reserve((size_t)n_streams_ * ch * max_rows * (hop + 1));
        pl_upload_table(sp.staging, sp.h_call, sp.call.ptr, stream);
        SpArgs a = spectrum_args();
        a.in = d_in;
        a.frames_capacity = frames_capacity;
        a.max_rows = (uint32_t)max_rows;
        a.max_units = (uint32_t)max_rows * ch;
        a.max_move = (uint32_t)max_move;
        launch_sp_begin(a, stream);
        launch_sp_transform(a, stream);
        launch_sp_chain(a, stream);
        launch_sp_carry(a, stream);
        OMX_HIP(hipGetLastError());
        for (uint32_t s = 0; s < n_streams_; ++s) {
            const SpCall& c = sp.h_call[s];
            sp.h_frames[s] += c.frames;
            sp.h_taken[s] += c.nk;
            sp.h_carried[s] = c.keep;
            if (c.shift) sp.h_parity[s] ^= 1u;
            if (c.finish) sp.h_finished[s] = 1;
        }
    }
    *d_records = sp.records.ptr;
    *d_sums = sp.sums.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_spectrum(uint64_t stream_index, omx_program_spectrum_record* record, double* sums) {
    if (!spectrum_) return pl_refuse("fetch_spectrum", kSpNotConfigured);
    if (stream_index >= n_streams_) return pl_refuse("fetch_spectrum", "stream index out of range");
    const ProgramSpectrum& sp = *spectrum_;
    const size_t per = (size_t)sp.channels * (sp.rule.fft_size / 2 + 1);
    copy_out(record, sp.records.ptr + stream_index, sizeof(*record), false, last_stream_);
    copy_out(sums, sp.sums.ptr + stream_index * per, per * sizeof(double), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_spectrum_rule_default(omx_program_spectrum_rule* rule) {
    return sp_host("spectrum rule_default", [&](const char** why) { return sp_rule_default(rule, why); });
}
int omx_program_spectrum_qc_default(omx_program_spectrum_qc* qc) {
    return sp_host("spectrum qc_default", [&](const char** why) { return sp_qc_default(qc, why); });
}
int omx_program_spectrum_match_spec_default(double sample_rate, omx_program_spectrum_match_spec* spec) {
    return sp_host("spectrum match_spec_default", [&](const char** why) { return sp_match_spec_default(sample_rate, spec, why); });
}
int omx_program_spectrum_plan(const omx_program_spectrum_rule* rule, uint32_t channels, uint64_t n_streams, uint64_t frames,
                              omx_program_spectrum_info* info) {
    return sp_host("spectrum plan", [&](const char** why) { return sp_plan(rule, channels, n_streams, frames, info, why); });
}
int omx_program_spectrum_window(uint32_t fft_size, float* window) {
    return sp_host("spectrum window", [&](const char** why) { return sp_window(fft_size, window, why); });
}
int omx_program_spectrum_transforms(uint64_t frames, uint32_t finished, uint32_t fft_size, uint64_t* count) {
    return sp_host("spectrum transforms", [&](const char** why) { return sp_transforms(frames, finished, fft_size, count, why); });
}
int omx_program_spectrum_density(const omx_program_spectrum_record* record, const double* sums, uint32_t channel, double* density) {
    return sp_host("spectrum density", [&](const char** why) { return sp_density(record, sums, channel, density, why); });
}
int omx_program_spectrum_bands(const double* density, uint32_t fft_size, double sample_rate, uint32_t fraction, double* centre_hz,
                               double* level_db, uint32_t* n) {
    return sp_host("spectrum bands",
                   [&](const char** why) { return sp_bands(density, fft_size, sample_rate, fraction, centre_hz, level_db, n, why); });
}
int omx_program_spectrum_summarize(const omx_program_spectrum_qc* qc, const double* density, uint32_t fft_size, double sample_rate,
                                   omx_program_spectrum_summary* summary) {
    return sp_host("spectrum summarize", [&](const char** why) { return sp_summarize(qc, density, fft_size, sample_rate, summary, why); });
}
int omx_program_spectrum_match(const double* density_source, const double* density_target, uint32_t fft_size, double sample_rate,
                               const omx_program_spectrum_match_spec* spec, float* taps, uint32_t n_taps) {
    return sp_host("spectrum match", [&](const char** why) {
        return sp_match(density_source, density_target, fft_size, sample_rate, spec, taps, n_taps, why);
    });
}

int omx_program_loudness_bank_spectrum_configure(omx_program_loudness_bank* b, const omx_program_spectrum_rule* rule, uint32_t channels) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.spectrum_configure(rule, channels); });
}
int omx_program_loudness_bank_spectrum_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.spectrum_reset(reset_mask); });
}
int omx_program_loudness_bank_spectrum(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                       const uint8_t* finish_mask, void* stream, const omx_program_spectrum_record** d_records,
                                       const double** d_sums) {
    if (!b || !d_records || !d_sums) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.spectrum(d_in, frames_capacity, frames, finish_mask, static_cast<hipStream_t>(stream), d_records, d_sums);
    });
}
int omx_program_loudness_bank_fetch_spectrum(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_spectrum_record* record,
                                             double* sums) {
    if (!b || !record || !sums) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_spectrum(stream_index, record, sums); });
}

}  // extern "C"
