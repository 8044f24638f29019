// Host side of the programme bank's sample-rate conversion (include/omx/program_resample.h): the plan, the tap table (f64, every step
// its own operation: the library is built with -ffp-contract=off), and the calls.  The rule and every call are checked against the
// host's mirror of the streams (frames taken, frames emitted, flushed) before anything is touched, the per-stream table of a call
// goes up in one upload, every launch is on the caller's stream.  Nothing here synchronises except fetch_resampled,
// resampler_configure and resampler_reset's wait for its own upload slot.
#include <numeric>

#include "program_loudness.hpp"

namespace omx {

namespace {

double rs_i0(double v) {  // the power series, OMX_RESAMPLE_I0_TERMS terms behind the leading 1
    const double y = v * 0.5;
    double t = 1.0, s = 1.0;
    for (uint32_t i = 1; i <= OMX_RESAMPLE_I0_TERMS; ++i) {
        t = t * (y / (double)i);
        s = s + t * t;
    }
    return s;
}

}  // namespace

int rs_plan(const omx_program_resample_rule* rule, omx_program_resample_info* info) {
    const char* who = "resample plan";
    if (!rule || !info) return pl_refuse(who, "null rule or info");
    if (rule->rate_in == 0 || rule->rate_out == 0 || rule->rate_in == rule->rate_out) return pl_refuse(who, "a rate of 0, or rate_in == rate_out");
    if (rule->half_width < 8 || rule->half_width > 64 || (rule->half_width & 1u)) return pl_refuse(who, "half_width odd or outside 8 .. 64");
    if (!std::isfinite(rule->beta) || rule->beta < 0.0f || rule->beta > 20.0f) return pl_refuse(who, "beta not finite or outside [0, 20]");
    if (!(rule->cutoff > 0.5f && rule->cutoff <= 1.0f)) return pl_refuse(who, "cutoff not in (0.5, 1]");
    if (rule->flags != 0) return pl_refuse(who, "a flag set");
    const auto refuse_unsupported = [](const char* why) {
        set_last_error(std::string("unsupported configuration for the HIP path: resample plan: ") + why);
        return (int)OMX_ERR_UNSUPPORTED;
    };
    if (rule->rate_in < OMX_RESAMPLE_MIN_RATE || rule->rate_in > OMX_RESAMPLE_MAX_RATE || rule->rate_out < OMX_RESAMPLE_MIN_RATE ||
        rule->rate_out > OMX_RESAMPLE_MAX_RATE)
        return refuse_unsupported("a rate outside 3364 .. 768000 Hz (the rates process accepts)");
    const uint32_t g = std::gcd(rule->rate_in, rule->rate_out);
    const uint32_t L = rule->rate_out / g, M = rule->rate_in / g;
    if (L > OMX_RESAMPLE_MAX_FACTOR || M > OMX_RESAMPLE_MAX_FACTOR) return refuse_unsupported("L or M above 1024");
    const uint64_t Z = rule->half_width;
    const uint64_t H = L >= M ? Z : 2 * ((Z * M + 2 * (uint64_t)L - 1) / (2 * (uint64_t)L));
    if (H > OMX_RESAMPLE_MAX_HALF_WIDTH) return refuse_unsupported("H above 512");
    omx_program_resample_info out{};
    out.L = L;
    out.M = M;
    out.taps = (uint32_t)(2 * H);
    out.latency_frames = (uint32_t)H;
    out.table_floats = (uint64_t)L * out.taps;
    uint32_t tile = kRsThreads;  // the longest tile whose reach fits the staging
    while (tile > 1 && ((uint64_t)(tile - 1) * M) / L + 1 + out.taps > kRsStageFrames) --tile;
    out.tile_frames = tile;
    *info = out;
    return OMX_NONE;
}

void rs_build_taps(const omx_program_resample_rule& rule, const omx_program_resample_info& info, float* dst) {
    const uint32_t L = info.L, M = info.M, T = info.taps, H = info.latency_frames;
    const double fc = (double)rule.cutoff * (L < M ? (double)L / (double)M : 1.0);
    const double beta = (double)rule.beta, i0_beta = rs_i0(beta);
    std::vector<double> row(T);
    for (uint32_t p = 0; p < L; ++p) {
        double sum = 0.0;
        for (uint32_t k = 0; k < T; ++k) {
            const double d = (double)((int64_t)k - (int64_t)H + 1) - (double)p / (double)L;
            double h = 0.0;
            if (std::fabs(d) < (double)H) {
                const double r = d / (double)H;
                const double u = fc * d;
                const double a = M_PI * u;
                const double sinc = u == 0.0 ? 1.0 : std::sin(a) / a;
                h = fc * sinc * rs_i0(beta * std::sqrt(1.0 - r * r)) / i0_beta;
            }
            row[k] = h;
            sum = sum + h;
        }
        for (uint32_t k = 0; k < T; ++k) dst[(size_t)p * T + k] = (float)(row[k] / sum);
    }
}

uint64_t rs_emitted(const omx_program_resample_info& info, uint64_t n, uint64_t e, bool flush) {
    const unsigned __int128 L = info.L, M = info.M;
    const uint64_t H = info.latency_frames;
    if (flush) return (uint64_t)(((unsigned __int128)n * L + M - 1) / M);
    const uint64_t ready = n > H ? (uint64_t)(((unsigned __int128)(n - H) * L + M - 1) / M) : 0;
    return std::max(e, ready);
}

int ProgramLoudnessBank::resampler_configure(const omx_program_resample_rule* rule, uint32_t channels) {
    const char* who = "resampler_configure";
    omx_program_resample_info info{};
    const int planned = rs_plan(rule, &info);
    if (planned != OMX_NONE) return planned;
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (resampler_ && carry_holds_frames(resampler_->h_streams)) return pl_refuse(who, "a stream of the resampler holds frames (reset every stream first)");
    if (resampler_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the old buffers may still be in flight)
    auto rs = resampler_ ? std::move(resampler_) : std::make_unique<ProgramResampler>();
    rs->rule = *rule;
    rs->info = info;
    rs->channels = channels;
    rs->h_streams.assign(n_streams_, CarryLedger{});
    rs->h_calls.assign(n_streams_, RsStreamCall{});
    std::vector<float> taps(info.table_floats);
    rs_build_taps(*rule, info, taps.data());
    std::vector<float> by_tap(taps.size());  // the kernel's order, [T / 4][L][4] (program_resample_kernels.hip says why)
    for (uint32_t p = 0; p < info.L; ++p)
        for (uint32_t k = 0; k < info.taps; ++k) by_tap[((size_t)(k / 4) * info.L + p) * 4 + k % 4] = taps[(size_t)p * info.taps + k];
    rs->table.upload(by_tap, last_stream_);
    rs->calls.reserve(n_streams_);
    rs->records.reserve(n_streams_);
    rs->ring.reserve((size_t)n_streams_ * (info.taps - 1) * channels);
    resampler_ = std::move(rs);
    const int rc = resampler_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first resample call may come on another stream)
    return rc;
}

RsArgs ProgramLoudnessBank::resampler_args() const {
    const ProgramResampler& rs = *resampler_;
    RsArgs a{};
    a.n_streams = n_streams_;
    a.channels = rs.channels;
    a.L = rs.info.L;
    a.M = rs.info.M;
    a.taps = rs.info.taps;
    a.half = rs.info.latency_frames;
    a.tile = rs.info.tile_frames;
    a.history = rs.info.taps - 1;
    a.floor_db = cfg_.floor_db;
    a.table = rs.table.ptr;
    a.calls = rs.calls.ptr;
    a.records = rs.records.ptr;
    a.ring = rs.ring.ptr;
    return a;
}

int ProgramLoudnessBank::resampler_reset(const uint8_t* reset_mask) {
    if (!resampler_) return pl_refuse("resampler_reset", "the resampler is not configured (omx_program_loudness_bank_resampler_configure)");
    ProgramResampler& rs = *resampler_;
    carry_reset(rs.h_streams, rs.h_calls, reset_mask, [](const CarryLedger&) { return RsStreamCall{}; });
    pl_upload_table(rs.staging, rs.h_calls, rs.calls.ptr, last_stream_);
    const RsArgs a = resampler_args();
    launch_rs_begin(a, false, last_stream_);
    launch_rs_finish(a, last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out, the records and the resampler's state as they were.
int ProgramLoudnessBank::resample(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, uint64_t out_capacity,
                                  const uint8_t* flush_mask, hipStream_t stream, const omx_program_resample_record** d_resampled) {
    const char* who = "resample";
    if (!resampler_) return pl_refuse(who, "the resampler is not configured (omx_program_loudness_bank_resampler_configure)");
    ProgramResampler& rs = *resampler_;
    if (!pl_capacity_ok(frames_capacity) || !pl_capacity_ok(out_capacity))
        return pl_refuse(who, "frames_capacity or out_capacity beyond 2^32 - 1");
    RsArgs a = resampler_args();
    CarryTotals totals;
    std::vector<RsStreamCall>& calls = rs.h_calls;  // (host scratch only: the ledger is committed below, after the last check)
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const CarryLedger& m = rs.h_streams[s];
        CarryStep step;
        const auto emitted = [&](uint64_t n, uint64_t e, bool flush) { return rs_emitted(rs.info, n, e, flush); };
        if (const char* why = carry_step(m, frames, frames_capacity, flush_mask, s, out_capacity, emitted, step)) return pl_refuse(who, why);
        const unsigned __int128 pos = (unsigned __int128)m.e * a.M;
        RsStreamCall c{};
        c.n_old = m.n;
        c.e_old = m.e;
        c.rel_e = (int64_t)(uint64_t)(pos / a.L) - (int64_t)m.n;
        c.phase_e = (uint32_t)(pos % a.L);
        c.frames = (uint32_t)step.frames;
        c.emit = (uint32_t)step.emit;
        c.ring = (uint32_t)(m.n % a.history);
        c.flags = step.flush ? kCarryFlagFlush : 0u;
        calls[s] = c;
        totals.take(step);
    }
    a.max_frames = totals.max_frames;
    a.max_emit = totals.max_emit;
    if (totals.null_pcm(d_in, d_out)) return pl_refuse(who, "null pcm");
    if (((uint64_t)a.max_emit + a.tile - 1) / a.tile * kRsThreads > 0xFFFFFFFFull) unsupported("programme resampler: call too long for one launch");
    if (pl_in_out_overlap(d_in, frames_capacity, d_out, out_capacity, n_streams_, a.channels, a.channels)) return pl_refuse(who, "d_in and d_out overlap");

    carry_commit(rs.h_streams, calls);
    last_stream_ = stream;
    pl_upload_table(rs.staging, calls, rs.calls.ptr, stream);
    a.in = d_in;
    a.out = d_out;
    a.frames_capacity = frames_capacity;
    a.out_capacity = out_capacity;
    launch_rs_begin(a, true, stream);
    if (totals.any_out) launch_rs_main(a, stream);
    if (totals.any_in) launch_rs_carry(a, stream);
    launch_rs_finish(a, stream);
    OMX_HIP(hipGetLastError());
    if (d_resampled) *d_resampled = rs.records.ptr;
    return totals.any_out ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_resampled(uint64_t stream_index, omx_program_resample_record* dst) {
    if (!resampler_ || stream_index >= n_streams_)
        return pl_refuse("fetch_resampled", "the resampler is not configured, or stream index out of range");
    copy_out(dst, resampler_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_resample_plan(const omx_program_resample_rule* rule, omx_program_resample_info* info) { return rs_plan(rule, info); }
int omx_program_resample_taps(const omx_program_resample_rule* rule, float* dst, uint64_t n_floats) {
    omx_program_resample_info info{};
    const int planned = rs_plan(rule, &info);
    if (planned != OMX_NONE) return planned;
    if (!dst || n_floats != info.table_floats) return OMX_ERR_INVALID;
    return guarded([&] {
        rs_build_taps(*rule, info, dst);
        return (int)OMX_NONE;
    });
}
int omx_program_resample_frames(const omx_program_resample_rule* rule, uint64_t frames_in_before, uint64_t frames_out_before, uint64_t frames,
                                uint32_t flush, uint64_t* frames_out) {
    omx_program_resample_info info{};
    const int planned = rs_plan(rule, &info);
    if (planned != OMX_NONE) return planned;
    if (!frames_out || frames_in_before > (1ull << 63) || frames > (1ull << 63) - frames_in_before) return OMX_ERR_INVALID;
    *frames_out = rs_emitted(info, frames_in_before + frames, frames_out_before, flush != 0) - frames_out_before;
    return OMX_NONE;
}
int omx_program_loudness_bank_resampler_configure(omx_program_loudness_bank* b, const omx_program_resample_rule* rule, uint32_t channels) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.resampler_configure(rule, channels); });
}
int omx_program_loudness_bank_resampler_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.resampler_reset(reset_mask); });
}
int omx_program_loudness_bank_resample(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                       float* d_out, uint64_t out_capacity, const uint8_t* flush_mask, void* stream,
                                       const omx_program_resample_record** d_resampled) {
    if (!b || !d_resampled) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.resample(d_in, frames_capacity, frames, d_out, out_capacity, flush_mask, static_cast<hipStream_t>(stream), d_resampled);
    });
}
int omx_program_loudness_bank_fetch_resampled(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_resample_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_resampled(stream_index, dst); });
}

}  // extern "C"
