// Host side of the programme loudness bank: handle, per-stream counters (every count of a stream follows from the call arguments, so
// the host keeps them and the device never has to report back), per-rate tables, launches on the caller's stream.  Nothing here
// synchronises except fetch / fetch_segments and the (re)building of the per-rate tables.
#include "program_loudness.hpp"

#include "../loudness.hpp"  // k_weighting_coefficients (loudness/processor.rs:22-55): a pure host function

namespace omx {

namespace {

double channel_weight(uint8_t position) {  // loudness/processor.rs:174-183
    switch (position) {
        case OMX_POS_LOW_FREQUENCY: return 0.0;
        case OMX_POS_REAR_LEFT:
        case OMX_POS_REAR_RIGHT:
        case OMX_POS_SIDE_LEFT:
        case OMX_POS_SIDE_RIGHT: return 1.41;
        default: return 1.0;
    }
}

// double-double arithmetic for the host tables: the zero-input recurrence of the K-weighting filter has entries that cancel by many
// orders of magnitude over a work item (loudness.cpp explains the numerics); the tables are rounded once, at the end
struct DD {
    double h, l;
};
DD two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
DD dd_add(DD a, DD b) {
    DD s = two_sum(a.h, b.h);
    const DD t = two_sum(a.l, b.l);
    s.l += t.h;
    s = {s.h + s.l, s.l - ((s.h + s.l) - s.h)};
    s.l += t.l;
    return {s.h + s.l, s.l - ((s.h + s.l) - s.h)};
}
DD dd_mul_d(DD a, double b) {
    const double p = a.h * b, e = std::fma(a.h, b, -p) + a.l * b;
    return {p + e, e - ((p + e) - p)};
}
void zero_input_step(DD (&g)[4], const double a[5]) {  // y = g0; g0' = g1 - a1 y; g1' = g2 - a2 y; g2' = g3 - a3 y; g3' = -a4 y
    const DD y = g[0];
    g[0] = dd_add(g[1], dd_mul_d(y, -a[1]));
    g[1] = dd_add(g[2], dd_mul_d(y, -a[2]));
    g[2] = dd_add(g[3], dd_mul_d(y, -a[3]));
    g[3] = dd_mul_d(y, -a[4]);
}

}  // namespace

ProgramLoudnessBank::ProgramLoudnessBank(const omx_loudness_config& cfg, uint32_t n_streams, uint32_t capacity_seconds, bool bounded)
    : n_streams_(n_streams), capacity_(bounded ? 0 : (uint64_t)capacity_seconds * 10), bounded_(bounded) {
    cfg_ = cfg;
    const size_t slots = (size_t)n_streams * kPlSlots;
    state_.reserve(slots * 4);
    part_.reserve(slots);
    segments_.reserve((size_t)n_streams * capacity_);
    tp_max_.upload(std::vector<float>(n_streams, cfg.floor_db), nullptr);
    calls_.reserve(n_streams);
    meta_.reserve(n_streams);
    records_.reserve(n_streams);
    OMX_HIP(hipMemset(state_.ptr, 0, slots * 4 * sizeof(double)));
    OMX_HIP(hipMemset(part_.ptr, 0, slots * sizeof(double)));
    h_meta_.assign(n_streams, PlStreamMeta{0, 0, 0});
    h_calls_.assign(n_streams, PlStreamCall{});
    if (bounded_) bounded_init();
}

void ProgramLoudnessBank::set_rate(float rate) {
    rate_ = rate;
    k_weighting_coefficients((double)rate, b_, a_);
    seg_ = ((uint32_t)rate + 5u) / 10u;
}

// Zero-state weights W[k][i] = (A^(L-1-k) B)_i (B_i = b_i - a_i b_0) and the zero-input transition A^L as high + low parts, L = the
// work item length of the time-parallel form
void ProgramLoudnessBank::host_tables(hipStream_t stream) {
    const uint32_t L = std::min(kPlChunkFrames, seg_);
    if (tables_rate_ == rate_ && tables_chunk_ == L) return;
    const uint32_t padded = (L + kPlTile - 1) / kPlTile * kPlTile;  // the pass reads whole tiles of weights
    std::vector<double> W((size_t)padded * 4, 0.0);
    DD g[4];
    for (int i = 0; i < 4; ++i) g[i] = dd_add(DD{b_[i + 1], 0.0}, dd_mul_d(DD{b_[0], 0.0}, -a_[i + 1]));
    for (uint32_t n = 0; n < L; ++n) {
        const uint32_t k = L - 1 - n;
        for (int i = 0; i < 4; ++i) W[(size_t)k * 4 + i] = g[i].h;
        zero_input_step(g, a_);
    }
    std::vector<double> T(32, 0.0);
    for (int m = 0; m < 4; ++m) {  // column m: the state that started as unit vector m
        DD f[4];
        for (int k = 0; k < 4; ++k) f[k] = {k == m ? 1.0 : 0.0, 0.0};
        for (uint32_t n = 0; n < L; ++n) zero_input_step(f, a_);
        for (int k = 0; k < 4; ++k) {
            T[(size_t)k * 4 + m] = f[k].h;
            T[16 + (size_t)k * 4 + m] = f[k].l;
        }
    }
    zs_weights_.upload(W, stream);
    transition_.upload(T, stream);
    tables_rate_ = rate_;
    tables_chunk_ = L;
}

int ProgramLoudnessBank::reset(const uint8_t* reset_mask) {
    std::vector<uint8_t> all;
    if (!reset_mask) {
        all.assign(n_streams_, 1);
        reset_mask = all.data();
    }
    const uint8_t positions[OMX_MAX_CHANNELS] = {0, 0, 0, 0, 0, 0, 0, 0};
    // a call without frames: only the flagged streams change
    std::vector<uint32_t> none(n_streams_, 0);
    return process(nullptr, 0, none.data(), reset_mask, channels_ ? channels_ : 1, rate_ != 0.0f ? rate_ : cfg_.sample_rate, positions, last_stream_);
}

int ProgramLoudnessBank::process(const float* d_pcm, uint64_t frames_capacity, const uint32_t* frames, const uint8_t* reset_mask,
                                 uint32_t channels_in, float sample_rate, const uint8_t positions[OMX_MAX_CHANNELS], hipStream_t stream) {
    const char* who = "process";
    const uint32_t seg_before = seg_, channels_before = channels_;  // the layout the peak timeline's stored keys were written with
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    // (a clamped count with the caller's stride would read the wrong samples)
    if (!pl_channels_ok(channels_in)) return pl_refuse(who, "channels outside 1 .. 8");
    const uint32_t channels = channels_in;
    const float rate = sanitize_sample_rate(sample_rate);
    if (rate < kPlMinRate) unsupported("programme loudness below 3364 Hz: the K-weighting filter has poles outside the unit circle");
    bool any = false, any_reset = false;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        any = any || f != 0;
        any_reset = any_reset || (reset_mask && reset_mask[s]);
    }
    if (any && !d_pcm) return pl_refuse(who, "null pcm");
    if (rate != rate_ || channels != channels_) {
        // a programme cannot change its rate or layout: refused unless every stream that has taken samples starts over in this call
        for (uint32_t s = 0; s < n_streams_; ++s)
            if (h_meta_[s].frames != 0 && !(reset_mask && reset_mask[s]))
                return pl_refuse(who, "sample rate / channel count changed while a programme is running (reset it in the same call)");
        if (any || rate_ == 0.0f) {  // (a bare reset keeps the rate the next call may confirm or change)
            set_rate(rate);
            channels_ = channels;
        }
    }
    last_stream_ = stream;
    if (!any && !any_reset) return OMX_NONE;

    uint32_t max_frames = 0, max_new = 0;
    bool taken = false;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        PlStreamMeta& m = h_meta_[s];
        PlStreamCall& c = h_calls_[s];
        c.reset = (reset_mask && reset_mask[s]) ? 1u : 0u;
        if (c.reset && peak_timeline_on_ && m.frames != 0) {  // the peak segments the stream has stored go back to zero (measure_peaks)
            const uint64_t row = (uint64_t)channels_before * kPtKinds;
            const uint64_t at = (uint64_t)s * (capacity_ + 1) * row, n = std::min<uint64_t>((m.frames + seg_before - 1) / seg_before, capacity_ + 1) * row;
            for (uint64_t e = 0; e < n; e += kPtClearChunk) h_pt_clear_.push_back(PtClearItem{at + e, (uint32_t)std::min<uint64_t>(kPtClearChunk, n - e), 0u});
        }
        if (c.reset) m = PlStreamMeta{0, 0, 0};
        const uint64_t room = bounded_ ? ~0ull : capacity_ * seg_ - m.frames;  // a full stream takes no more samples; a bounded one never fills
        const uint64_t want = any ? (frames ? frames[s] : frames_capacity) : 0;
        c.frames = (uint32_t)std::min<uint64_t>(want, room);
        c.phase = seg_ ? (uint32_t)(m.frames % seg_) : 0u;
        c.n_new = seg_ ? (uint32_t)(((uint64_t)c.phase + c.frames) / seg_) : 0u;
        c.seg_base = bounded_ ? 0 : m.segments;  // bounded: the commit writes row s of the call's own scratch
        m.frames += c.frames;
        m.segments += c.n_new;
        if (!bounded_ && seg_ && m.segments >= capacity_) m.overflow = 1;
        max_frames = std::max(max_frames, c.frames);
        max_new = std::max(max_new, c.n_new);
        taken = taken || c.frames != 0;
    }
    pl_upload_table(call_staging_, h_calls_, calls_.ptr, stream);
    dirty_ = true;

    PlArgs a{};
    a.pcm = d_pcm;
    a.frames_capacity = frames_capacity;
    a.n_streams = n_streams_;
    a.channels = channels;
    a.slot_shift = channels == 1 ? 0u : (channels == 2 ? 1u : (channels <= 4 ? 2u : 3u));
    a.seg = seg_;
    a.max_new = max_new;
    for (int i = 0; i < 5; ++i) {
        a.b[i] = b_[i];
        a.a[i] = a_[i];
    }
    for (int i = 0; i < OMX_MAX_CHANNELS; ++i) a.weights[i] = channel_weight(positions[i]);
    a.calls = calls_.ptr;
    a.state = state_.ptr;
    a.part = part_.ptr;
    a.segments = segments_.ptr;
    a.capacity = capacity_;
    if (any_reset) launch_pl_reset(a, tp_max_.ptr, cfg_.floor_db, stream);
    if (bounded_) {
        fresh_.reserve((size_t)n_streams_ * std::max<uint32_t>(max_new, 1));
        a.segments = fresh_.ptr;
        a.capacity = max_new;
    }
    if (!taken) {
        if (bounded_ && any_reset) bounded_fold(0, stream);
        if (peaks_on_ && any_reset) measure_peaks(d_pcm, frames_capacity, 0, stream);  // (the flagged streams' peaks are cleared by the fold)
        OMX_HIP(hipGetLastError());
        return OMX_NONE;
    }
    chan_sums_.reserve((size_t)n_streams_ * kPlSlots * std::max<uint32_t>(max_new, 1));
    a.chan_sums = chan_sums_.ptr;
    // Which evaluation order (OMX_OPT_KERNEL_FORM pins one).  The reference-order pass runs one wavefront per 64 (stream, channel)
    // slots however long the call is; the time-parallel pass reads the PCM twice but fills the card when the call is long.
    const uint32_t item = std::min(kPlChunkFrames, seg_);
    const uint64_t waves = ((uint64_t)n_streams_ << a.slot_shift) / 64 + 1;
    const bool by_shape = max_frames >= 4 * item && waves * 4 < 2048;
    // above kPlTimeParallelMaxRate the time-parallel pass cannot hold the parity bar (program_loudness.hpp): the reference order runs,
    // also for a pinned form 2, and last_form() says so
    const bool time_parallel = rate_ <= kPlTimeParallelMaxRate && (form_ == 2 || (form_ == 0 && by_shape));
    if (time_parallel) {
        host_tables(stream);
        a.chunk = item;
        a.n_chunks = (max_frames + item - 1) / item;
        const size_t items = (size_t)n_streams_ * kPlSlots * a.n_chunks;
        starts_.reserve(items * 4);
        partials_.reserve(items * 2);
        a.starts = starts_.ptr;
        a.partials = partials_.ptr;
        a.zs_weights = zs_weights_.ptr;
        a.transition = transition_.ptr;
        launch_pl_time_parallel(a, stream);
        last_form_ = 2;
    } else {
        a.chunk = max_frames;
        a.n_chunks = 1;
        a.starts = state_.ptr;
        launch_pl_reference_order(a, stream);
        last_form_ = 1;
    }
    launch_pl_commit(a, stream);
    if (bounded_ && (max_new != 0 || any_reset)) bounded_fold(max_new, stream);
    if (peaks_on_) measure_peaks(d_pcm, frames_capacity, max_frames, stream);
    OMX_HIP(hipGetLastError());
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::note_snapshots(const omx_loudness_snapshot* d_snapshots, uint64_t n_blocks, const uint32_t* d_n_blocks,
                                        hipStream_t stream) {
    last_stream_ = stream;
    if (n_blocks == 0) return OMX_NONE;
    launch_pl_true_peak_fold(d_snapshots, n_blocks, d_n_blocks, n_streams_, tp_max_.ptr, stream);
    OMX_HIP(hipGetLastError());
    dirty_ = true;
    return OMX_NONE;
}

PlResultArgs ProgramLoudnessBank::result_args() const {
    PlResultArgs r{};
    r.segments = segments_.ptr;
    r.capacity = capacity_;
    r.meta = meta_.ptr;
    r.tp_max = tp_max_.ptr;
    r.peaks = peaks_on_ ? peak_records_.ptr : nullptr;
    r.records = records_.ptr;
    r.n_streams = n_streams_;
    r.floor_db = cfg_.floor_db;
    r.absolute_gate = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    return r;
}

int ProgramLoudnessBank::results(hipStream_t stream, const omx_program_loudness_record** d_records) {
    last_stream_ = stream;
    pl_upload_table(meta_staging_, h_meta_, meta_.ptr, stream);
    if (bounded_) bounded_results(stream);
    else launch_pl_results(result_args(), stream);
    OMX_HIP(hipGetLastError());
    dirty_ = false;
    if (d_records) *d_records = records_.ptr;
    return OMX_NONE;
}

int ProgramLoudnessBank::fetch(uint64_t stream_index, omx_program_loudness_record* dst) {
    if (stream_index >= n_streams_) return pl_refuse("fetch", "stream index out of range");
    if (dirty_) results(last_stream_, nullptr);
    copy_out(dst, records_.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

int ProgramLoudnessBank::fetch_segments(uint64_t stream_index, uint64_t first, uint64_t count, double* dst) {
    if (bounded_) return bounded_refusal("fetch_segments");
    if (stream_index >= n_streams_ || first > h_meta_[stream_index].segments || count > h_meta_[stream_index].segments - first)
        return pl_refuse("fetch_segments", "range outside the stored segments");
    if (count == 0) return OMX_NONE;
    copy_out(dst, segments_.ptr + stream_index * capacity_ + first, count * sizeof(double), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

// ---------------------------------------------------------------- C ABI (include/omx/program_loudness.h)
using namespace omx;

extern "C" {

int omx_program_loudness_bank_create(const omx_loudness_config* cfg, uint32_t n_streams, uint32_t channels, uint32_t capacity_seconds,
                                     omx_program_loudness_bank** out) {
    (void)channels;  // taken from each call; state is sized for OMX_MAX_CHANNELS
    if (!cfg || !out || n_streams == 0 || capacity_seconds == 0) return OMX_ERR_INVALID;
    const int rc = device_ready();
    if (rc != OMX_NONE) return rc;
    return guarded([&] {
        *out = new omx_program_loudness_bank(*cfg, n_streams, capacity_seconds);
        return (int)OMX_NONE;
    });
}
void omx_program_loudness_bank_destroy(omx_program_loudness_bank* b) { delete b; }
int omx_program_loudness_bank_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.reset(reset_mask); });
}
int omx_program_loudness_bank_process(omx_program_loudness_bank* b, const float* d_pcm, uint64_t frames_capacity, const uint32_t* frames,
                                      const uint8_t* reset_mask, uint32_t channels, float sample_rate,
                                      const uint8_t positions[OMX_MAX_CHANNELS], void* stream) {
    if (!b || !positions) return OMX_ERR_INVALID;
    return guarded([&] {
        return b->impl.process(d_pcm, frames_capacity, frames, reset_mask, channels, sample_rate, positions, static_cast<hipStream_t>(stream));
    });
}
int omx_program_loudness_bank_note_snapshots(omx_program_loudness_bank* b, const omx_loudness_snapshot* d_snapshots, uint64_t n_blocks,
                                             const uint32_t* d_n_blocks, void* stream) {
    if (!b || !d_snapshots) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.note_snapshots(d_snapshots, n_blocks, d_n_blocks, static_cast<hipStream_t>(stream)); });
}
int omx_program_loudness_bank_results(omx_program_loudness_bank* b, void* stream, const omx_program_loudness_record** d_records) {
    if (!b || !d_records) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.results(static_cast<hipStream_t>(stream), d_records); });
}
int omx_program_loudness_bank_fetch(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_loudness_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch(stream_index, dst); });
}
int omx_program_loudness_bank_fetch_segments(omx_program_loudness_bank* b, uint64_t stream_index, uint64_t first, uint64_t count,
                                             double* dst) {
    if (!b || (!dst && count != 0)) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_segments(stream_index, first, count, dst); });
}
int omx_program_loudness_bank_set_option(omx_program_loudness_bank* b, uint32_t option, uint64_t value) {
    if (!b || option != OMX_OPT_KERNEL_FORM || value > 2) return OMX_ERR_INVALID;
    b->impl.form((int)value);
    return OMX_NONE;
}
int omx_debug_program_loudness_bank_last_form(const omx_program_loudness_bank* b) { return b ? b->impl.last_form() : OMX_ERR_INVALID; }

}  // extern "C"
