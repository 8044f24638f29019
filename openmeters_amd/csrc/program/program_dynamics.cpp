// Host side of the programme bank's dynamics stage (include/omx/program_dynamics.h): the C ABI of the host-only functions
// (program_dynamics_plan.hpp holds them), the tables of a configured set of curves, and the calls.  Every call is checked against the
// host's mirror of the streams (frames taken, frames emitted, flushed) before anything is touched, the per-stream table of a call goes
// up in one upload, every launch is on the caller's stream.  Nothing here synchronises except fetch_dynamics, dynamics_configure and
// dynamics_reset's wait for its own upload slot.
#include "program_loudness.hpp"

namespace omx {

namespace {

int dy_refusal(const char* who, int rc, const char* why) {
    pl_refuse(who, why ? why : "refused");
    return rc;
}

// what a stream's curve fixes of every call's table entry
DyStreamCall dy_call_of(const ProgramDynamics::Stream& m) {
    DyStreamCall c{};
    c.step = m.step;
    c.curve = m.curve;
    c.curve_index = m.curve_index;
    c.mask = m.mask;
    c.attack = m.attack;
    c.window = m.attack + m.hold;
    return c;
}

}  // namespace

int ProgramLoudnessBank::dynamics_configure(uint32_t channels, const omx_program_dynamics_curve* curves, uint32_t n_curves,
                                            const uint32_t* curve_of_stream) {
    const char* who = "dynamics_configure";
    if (!pl_channels_ok(channels)) return pl_refuse(who, "channels outside 1 .. 8");
    if (!curves) return pl_refuse(who, "null table");
    if (n_curves == 0 || n_curves > OMX_DYNAMICS_MAX_CURVES) return pl_refuse(who, "n_curves 0 or above OMX_DYNAMICS_MAX_CURVES");
    uint32_t max_attack = 1;
    for (uint32_t k = 0; k < n_curves; ++k) {
        const char* why = nullptr;
        const int rc = dy_check(curves + k, &why);
        if (rc != OMX_NONE) return dy_refusal(who, rc, why);
        if (curves[k].detector_mask >> channels) return pl_refuse(who, "a detector_mask with a bit at or above channels");
        max_attack = std::max(max_attack, curves[k].attack_frames);
    }
    for (uint32_t s = 0; curve_of_stream && s < n_streams_; ++s)
        if (curve_of_stream[s] != OMX_DYNAMICS_BYPASS && curve_of_stream[s] >= n_curves)
            return pl_refuse(who, "a curve index that is neither below n_curves nor OMX_DYNAMICS_BYPASS");
    if (dynamics_ && carry_holds_frames(dynamics_->h_streams)) return pl_refuse(who, "a stream of the stage holds frames (reset every stream first)");
    if (dynamics_) OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the old buffers may still be in flight)

    auto dy = dynamics_ ? std::move(dynamics_) : std::make_unique<ProgramDynamics>();
    dy->channels = channels;
    dy->n_curves = n_curves;
    dy->max_attack = max_attack;
    dy->h_streams.assign(n_streams_, ProgramDynamics::Stream{});
    dy->h_calls.assign(n_streams_, DyStreamCall{});
    uint32_t max_history = 1;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        ProgramDynamics::Stream& m = dy->h_streams[s];
        const uint32_t k = curve_of_stream ? curve_of_stream[s] : 0u;
        m.curve_index = k;
        if (k == OMX_DYNAMICS_BYPASS) {  // the row of zeros under the longest attack: E is 0 everywhere, every frame is copied
            m.curve = n_curves;
            m.mask = 1;
            m.attack = max_attack;
            m.hold = 0;
            m.step = OMX_DYNAMICS_MAX_STEP;
        } else {
            m.curve = k;
            m.mask = curves[k].detector_mask;
            m.attack = curves[k].attack_frames;
            m.hold = curves[k].hold_frames;
            m.step = curves[k].release_step;
        }
        max_history = std::max(max_history, m.attack + m.hold - 1);
    }
    dy->max_latency = std::max(max_attack - 1, 1u);
    dy->max_history = max_history;
    std::vector<int32_t> table((size_t)(n_curves + 1) * kDyCurveRow, 0);
    for (uint32_t k = 0; k < n_curves; ++k) std::copy(curves[k].T, curves[k].T + OMX_DYNAMICS_CURVE_POINTS, table.begin() + (size_t)k * kDyCurveRow);
    dy->curves.upload(table, last_stream_);
    dy->log_table.upload(std::vector<int32_t>(kDyLog, kDyLog + OMX_DYNAMICS_TABLE_ENTRIES), last_stream_);
    dy->exp_table.upload(std::vector<unsigned long long>(kDyExp, kDyExp + OMX_DYNAMICS_TABLE_ENTRIES), last_stream_);
    dy->calls.reserve(n_streams_);
    dy->records.reserve(n_streams_);
    dy->carry.reserve(n_streams_);
    dy->ring_x.reserve((size_t)n_streams_ * dy->max_latency * channels);
    dy->ring_r.reserve((size_t)n_streams_ * dy->max_latency);
    dy->ring_g.reserve((size_t)n_streams_ * dy->max_history);
    dynamics_ = std::move(dy);
    const int rc = dynamics_reset(nullptr);
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first dynamics call may come on another stream)
    return rc;
}

DyArgs ProgramLoudnessBank::dynamics_args() const {
    const ProgramDynamics& dy = *dynamics_;
    DyArgs a{};
    a.n_streams = n_streams_;
    a.channels = dy.channels;
    a.max_latency = dy.max_latency;
    a.max_history = dy.max_history;
    a.max_attack = dy.max_attack;
    a.floor_db = cfg_.floor_db;
    a.calls = dy.calls.ptr;
    a.records = dy.records.ptr;
    a.curves = dy.curves.ptr;
    a.log_table = dy.log_table.ptr;
    a.exp_table = dy.exp_table.ptr;
    a.carry = dy.carry.ptr;
    a.ring_x = dy.ring_x.ptr;
    a.ring_g = dy.ring_g.ptr;
    a.ring_r = dy.ring_r.ptr;
    return a;
}

int ProgramLoudnessBank::dynamics_reset(const uint8_t* reset_mask) {
    if (!dynamics_) return pl_refuse("dynamics_reset", "the stage is not configured (omx_program_loudness_bank_dynamics_configure)");
    ProgramDynamics& dy = *dynamics_;
    carry_reset(dy.h_streams, dy.h_calls, reset_mask, dy_call_of);
    pl_upload_table(dy.staging, dy.h_calls, dy.calls.ptr, last_stream_);
    const DyArgs a = dynamics_args();
    launch_dy_begin(a, false, last_stream_);
    launch_dy_finish(a, last_stream_);
    OMX_HIP(hipGetLastError());
    return OMX_NONE;
}

// Everything is checked before anything is touched: a refused call leaves d_out, the trace, the records and the stage's state as they were.
int ProgramLoudnessBank::dynamics(const float* d_in, const float* d_key, uint64_t frames_capacity, const uint32_t* frames, float* d_out,
                                  float* d_gain_db, uint64_t out_capacity, const uint8_t* flush_mask, hipStream_t stream,
                                  const omx_program_dynamics_record** d_records) {
    const char* who = "dynamics";
    if (!dynamics_) return pl_refuse(who, "the stage is not configured (omx_program_loudness_bank_dynamics_configure)");
    ProgramDynamics& dy = *dynamics_;
    if (!pl_capacity_ok(frames_capacity) || !pl_capacity_ok(out_capacity))
        return pl_refuse(who, "frames_capacity or out_capacity beyond 2^32 - 1");
    DyArgs a = dynamics_args();
    CarryTotals totals;
    bool any_scan = false;
    uint64_t max_hold = 0;
    std::vector<DyStreamCall>& calls = dy.h_calls;  // (host scratch only: the ledger is committed below, after the last check)
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const ProgramDynamics::Stream& m = dy.h_streams[s];
        const uint32_t latency = m.attack - 1;
        CarryStep step;
        const auto emitted = [&](uint64_t n, uint64_t e, bool flush) { return carry_emitted(latency, n, e, flush); };
        if (const char* why = carry_step(m, frames, frames_capacity, flush_mask, s, out_capacity, emitted, step)) return pl_refuse(who, why);
        const uint64_t scan = m.flushed ? 0 : step.frames + (step.flush ? latency : 0);
        if (scan > 0xFFFFFFFFull) return pl_refuse(who, "frames_capacity or out_capacity beyond 2^32 - 1");
        DyStreamCall c = dy_call_of(m);
        c.n_old = m.n;
        c.frames = (uint32_t)step.frames;
        c.emit = (uint32_t)step.emit;
        c.held = (uint32_t)(m.n - m.e);
        c.scan = (uint32_t)scan;
        c.flags = step.flush ? kCarryFlagFlush : 0u;
        c.ring_x = latency ? (uint32_t)(m.n % latency) : 0u;
        c.ring_g = c.window > 1 ? (uint32_t)(m.n % (c.window - 1)) : 0u;
        calls[s] = c;
        totals.take(step);
        any_scan = any_scan || scan != 0;
        a.max_scan = std::max(a.max_scan, c.scan);
        if (scan != 0) max_hold = std::max<uint64_t>(max_hold, scan + (c.window - std::min(c.window, kDyHoldMaxWindow)));
    }
    a.max_frames = totals.max_frames;
    a.max_emit = totals.max_emit;
    if (totals.null_pcm(d_in, d_out)) return pl_refuse(who, "null pcm");
    // out of place, for the key and the trace as well: neither output may share a byte with either input, nor with the other output
    const uint32_t C = a.channels;
    const auto hits_input = [&](const float* p, uint32_t frame_floats) {
        return pl_in_out_overlap(d_in, frames_capacity, p, out_capacity, n_streams_, C, frame_floats) ||
               pl_in_out_overlap(d_key, frames_capacity, p, out_capacity, n_streams_, C, frame_floats);
    };
    if (hits_input(d_out, C)) return pl_refuse(who, "d_out overlaps d_in or d_key");
    if (hits_input(d_gain_db, 1)) return pl_refuse(who, "d_gain_db overlaps d_in or d_key");
    const unsigned __int128 trace_bytes = (unsigned __int128)n_streams_ * sizeof(float) * out_capacity;
    if (d_out && d_gain_db && pl_ranges_overlap(d_out, trace_bytes * C, d_gain_db, trace_bytes)) return pl_refuse(who, "d_out and d_gain_db overlap");
    // the largest grid of the call is the apply pass's or the hold pass's: refused here, in front of the first change
    const uint64_t most_tiles = std::max<uint64_t>((a.max_emit + (uint64_t)kDySmoothTile - 1) / kDySmoothTile, (max_hold + kDyHoldTile - 1) / kDyHoldTile);
    if (max_hold > 0xFFFFFFFFull || most_tiles * n_streams_ > 0x7FFFFFFFull) unsupported("programme dynamics: call too long for one launch");

    carry_commit(dy.h_streams, calls);
    last_stream_ = stream;
    pl_upload_table(dy.staging, calls, dy.calls.ptr, stream);
    a.in = d_in;
    a.key = d_key ? d_key : d_in;
    a.out = d_out;
    a.gain_db = d_gain_db;
    a.frames_capacity = frames_capacity;
    a.out_capacity = out_capacity;
    a.g_row = a.max_frames;
    a.m_row = (uint32_t)max_hold;
    a.r_row = (a.max_scan + 1u) & ~1u;
    a.t_row = (a.max_scan + kDyReleaseTile - 1) / kDyReleaseTile;
    launch_dy_begin(a, true, stream);
    if (totals.any_in) {
        dy.gt.reserve((size_t)n_streams_ * a.g_row);
        a.gt = dy.gt.ptr;
        launch_dy_level(a, stream);
    }
    if (any_scan) {
        dy.held_min.reserve((size_t)n_streams_ * a.m_row);
        dy.r_local.reserve((size_t)n_streams_ * a.r_row);
        dy.tile_agg.reserve((size_t)n_streams_ * a.t_row);
        dy.tile_carry.reserve((size_t)n_streams_ * a.t_row);
        a.held_min = dy.held_min.ptr;
        a.r_local = dy.r_local.ptr;
        a.tile_agg = dy.tile_agg.ptr;
        a.tile_carry = dy.tile_carry.ptr;
        launch_dy_hold(a, stream);
        launch_dy_release(a, stream);
        launch_dy_chain(a, stream);
    }
    if (totals.any_out) launch_dy_apply(a, stream);
    if (totals.any_in) launch_dy_carry(a, stream);
    launch_dy_finish(a, stream);
    OMX_HIP(hipGetLastError());
    if (d_records) *d_records = dy.records.ptr;
    return totals.any_out ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_dynamics(uint64_t stream_index, omx_program_dynamics_record* dst) {
    if (!dynamics_ || stream_index >= n_streams_)
        return pl_refuse("fetch_dynamics", "the stage is not configured, or stream index out of range");
    copy_out(dst, dynamics_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_dynamics_plan(uint32_t channels, omx_program_dynamics_info* info) {
    const char* why = nullptr;
    const int rc = dy_plan(channels, info, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics plan", rc, why);
}
int omx_program_dynamics_tables(int32_t* log_out, uint64_t* exp_out) {
    if (log_out) std::copy(kDyLog, kDyLog + OMX_DYNAMICS_TABLE_ENTRIES, log_out);
    if (exp_out) std::copy(kDyExp, kDyExp + OMX_DYNAMICS_TABLE_ENTRIES, exp_out);
    return OMX_NONE;
}
int omx_program_dynamics_check(const omx_program_dynamics_curve* curve) {
    const char* why = nullptr;
    const int rc = dy_check(curve, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics check", rc, why);
}
int omx_program_dynamics_latency(const omx_program_dynamics_curve* curve, uint32_t* frames) {
    const char* why = nullptr;
    const int rc = dy_latency(curve, frames, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics latency", rc, why);
}
int omx_program_dynamics_design(const omx_program_dynamics_spec* spec, omx_program_dynamics_curve* curve) {
    const char* why = nullptr;
    const int rc = dy_design(spec, curve, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics design", rc, why);
}
int omx_program_dynamics_from_points(const omx_program_dynamics_point* points, uint32_t n, omx_program_dynamics_curve* curve) {
    const char* why = nullptr;
    const int rc = dy_from_points(points, n, curve, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics points", rc, why);
}
int omx_program_dynamics_gain_db(const omx_program_dynamics_curve* curve, double level_db, double* gain_db) {
    const char* why = nullptr;
    const int rc = dy_gain_db(curve, level_db, gain_db, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics gain", rc, why);
}
int omx_program_dynamics_time(double sample_rate, double attack_ms, double hold_ms, double release_db_per_s, uint32_t* attack_frames,
                              uint32_t* hold_frames, int64_t* release_step) {
    const char* why = nullptr;
    const int rc = dy_time(sample_rate, attack_ms, hold_ms, release_db_per_s, attack_frames, hold_frames, release_step, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics time", rc, why);
}
int omx_program_dynamics_frames(uint32_t latency_frames, uint64_t frames_in_before, uint64_t frames_out_before, uint64_t frames,
                                uint32_t flush, uint64_t* frames_out) {
    const char* why = nullptr;
    const int rc = dy_frames(latency_frames, frames_in_before, frames_out_before, frames, flush, frames_out, &why);
    return rc == OMX_NONE ? rc : dy_refusal("dynamics frames", rc, why);
}

int omx_program_loudness_bank_dynamics_configure(omx_program_loudness_bank* b, uint32_t channels, const omx_program_dynamics_curve* curves,
                                                 uint32_t n_curves, const uint32_t* curve_of_stream) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.dynamics_configure(channels, curves, n_curves, curve_of_stream); });
}
int omx_program_loudness_bank_dynamics_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.dynamics_reset(reset_mask); });
}
int omx_program_loudness_bank_dynamics(omx_program_loudness_bank* b, const float* d_in, const float* d_key, uint64_t frames_capacity,
                                       const uint32_t* frames, float* d_out, float* d_gain_db, uint64_t out_capacity,
                                       const uint8_t* flush_mask, void* stream, const omx_program_dynamics_record** d_records) {
    if (!b || !d_records) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.dynamics(d_in, d_key, frames_capacity, frames, d_out, d_gain_db, out_capacity, flush_mask,
                                static_cast<hipStream_t>(stream), d_records);
    });
}
int omx_program_loudness_bank_fetch_dynamics(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_dynamics_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_dynamics(stream_index, dst); });
}

}  // extern "C"
