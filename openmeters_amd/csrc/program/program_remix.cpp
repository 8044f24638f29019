// Host side of the programme bank's channel remix (include/omx/program_remix.h): the two presets (plain f32 arithmetic, every step
// its own operation: the library is built with -ffp-contract=off), the compaction of a matrix into the term lists the kernel walks,
// and the calls.  Every call is checked before anything is touched, the per-stream table of a call goes up in one upload, every
// launch is on the caller's stream.  Nothing here synchronises except fetch_remixed and remix_configure.
#include "program_loudness.hpp"

namespace omx {

namespace {

bool rm_level_ok(float v) { return std::isfinite(v) && v >= 0.0f && v <= 2.0f; }

// The term lists of one matrix [channels_out][channels_in]: the non-zero coefficients of every row, input channels in increasing order
RmMatrix rm_compact(const float* m, uint32_t channels_in, uint32_t channels_out) {
    RmMatrix out{};
    uint32_t n = 0;
    for (uint32_t o = 0; o < channels_out; ++o) {
        out.start[o] = n;
        for (uint32_t i = 0; i < channels_in; ++i) {
            const float c = m[o * channels_in + i];
            if (c == 0.0f) continue;  // (either sign)
            out.term[n].in = i;
            out.term[n].coef = c;
            ++n;
        }
    }
    for (uint32_t o = channels_out; o <= OMX_MAX_CHANNELS; ++o) out.start[o] = n;
    out.terms = n;
    return out;
}

}  // namespace

int rm_plan(uint32_t channels_in, uint32_t channels_out, omx_program_remix_info* info) {
    if (!info) return pl_refuse("remix plan", "null info");
    if (!pl_channels_ok(channels_in) || !pl_channels_ok(channels_out)) return pl_refuse("remix plan", "a channel count outside 1 .. 8");
    omx_program_remix_info out{};
    out.tile_frames = kRmThreads * rm_frames_per_thread(channels_in, channels_out);
    out.channels_in = channels_in;
    out.channels_out = channels_out;
    *info = out;
    return OMX_NONE;
}

int rm_downmix(const omx_program_downmix_rule* rule, uint32_t channels_in, const uint8_t* positions_in, float* matrix, uint32_t* channels_out,
               uint8_t* positions_out) {
    const char* who = "remix downmix";
    if (!rule || !positions_in || !matrix || !channels_out || !positions_out) return pl_refuse(who, "null pointer");
    if (!pl_channels_ok(channels_in)) return pl_refuse(who, "channels_in outside 1 .. 8");
    if (rule->kind != OMX_REMIX_KIND_STEREO && rule->kind != OMX_REMIX_KIND_MONO) return pl_refuse(who, "unknown kind");
    if (rule->flags & ~OMX_REMIX_NORMALIZE) return pl_refuse(who, "unknown flag");
    if (!rm_level_ok(rule->center_level) || !rm_level_ok(rule->surround_level) || !rm_level_ok(rule->lfe_level))
        return pl_refuse(who, "a level that is not finite or lies outside [0, 2]");
    const float c = rule->center_level, s = rule->surround_level, l = rule->lfe_level;
    float wl[OMX_MAX_CHANNELS], wr[OMX_MAX_CHANNELS];
    for (uint32_t i = 0; i < channels_in; ++i) {
        float a = 0.0f, b = 0.0f;
        switch (positions_in[i]) {
            case OMX_POS_FRONT_LEFT: a = 1.0f; break;
            case OMX_POS_FRONT_RIGHT: b = 1.0f; break;
            case OMX_POS_FRONT_CENTER:
            case OMX_POS_MONO: a = c, b = c; break;
            case OMX_POS_LOW_FREQUENCY: a = l, b = l; break;
            case OMX_POS_REAR_LEFT:
            case OMX_POS_SIDE_LEFT: a = s; break;
            case OMX_POS_REAR_RIGHT:
            case OMX_POS_SIDE_RIGHT: b = s; break;
            default: break;  // UNKNOWN, AUX
        }
        wl[i] = a;
        wr[i] = b;
    }
    if (rule->flags & OMX_REMIX_NORMALIZE) {
        float sl = 0.0f, sr = 0.0f;
        for (uint32_t i = 0; i < channels_in; ++i) sl = sl + std::fabs(wl[i]);
        for (uint32_t i = 0; i < channels_in; ++i) sr = sr + std::fabs(wr[i]);
        const float n = sl > sr ? sl : sr;
        if (n > 1.0f)
            for (uint32_t i = 0; i < channels_in; ++i) {
                wl[i] = wl[i] / n;
                wr[i] = wr[i] / n;
            }
    }
    for (uint32_t i = 0; i < OMX_MAX_CHANNELS; ++i) positions_out[i] = OMX_POS_UNKNOWN;
    if (rule->kind == OMX_REMIX_KIND_STEREO) {
        for (uint32_t i = 0; i < channels_in; ++i) {
            matrix[i] = wl[i];
            matrix[channels_in + i] = wr[i];
        }
        *channels_out = 2;
        positions_out[0] = OMX_POS_FRONT_LEFT;
        positions_out[1] = OMX_POS_FRONT_RIGHT;
    } else {
        for (uint32_t i = 0; i < channels_in; ++i) {
            const float sum = wl[i] + wr[i];
            matrix[i] = 0.5f * sum;
        }
        *channels_out = 1;
        positions_out[0] = OMX_POS_MONO;
    }
    return OMX_NONE;
}

int rm_select(uint32_t channels_in, const uint8_t* positions_in, uint32_t channels_out, const uint8_t* positions_out, float* matrix,
              uint32_t* missing_mask) {
    const char* who = "remix select";
    if (!positions_in || !positions_out || !matrix || !missing_mask) return pl_refuse(who, "null pointer");
    if (!pl_channels_ok(channels_in) || !pl_channels_ok(channels_out)) return pl_refuse(who, "a channel count outside 1 .. 8");
    uint32_t missing = 0;
    for (uint32_t o = 0; o < channels_out; ++o) {
        bool found = false;
        for (uint32_t i = 0; i < channels_in; ++i) {
            const bool here = !found && positions_in[i] == positions_out[o];
            matrix[o * channels_in + i] = here ? 1.0f : 0.0f;
            found = found || here;
        }
        if (!found) missing |= 1u << o;
    }
    *missing_mask = missing;
    return OMX_NONE;
}

int ProgramLoudnessBank::remix_configure(uint32_t channels_in, uint32_t channels_out, const float* matrices, uint32_t n_matrices) {
    const char* who = "remix_configure";
    if (!pl_channels_ok(channels_in) || !pl_channels_ok(channels_out)) return pl_refuse(who, "a channel count outside 1 .. 8");
    if (!matrices) return pl_refuse(who, "null table");
    if (n_matrices == 0 || n_matrices > OMX_REMIX_MAX_MATRICES) return pl_refuse(who, "n_matrices 0 or above OMX_REMIX_MAX_MATRICES");
    const size_t per = (size_t)channels_in * channels_out;
    for (size_t i = 0; i < per * n_matrices; ++i)
        if (!std::isfinite(matrices[i])) return pl_refuse(who, "a coefficient that is not finite");
    std::vector<RmMatrix> compact(n_matrices);
    std::vector<uint32_t> terms(n_matrices);
    for (uint32_t k = 0; k < n_matrices; ++k) {
        compact[k] = rm_compact(matrices + per * k, channels_in, channels_out);
        terms[k] = compact[k].terms;
    }
    // A remix call enqueued on ANY stream may still read the table and the records that go now: wait for the whole device.
    if (remix_) OMX_HIP(hipDeviceSynchronize());
    auto rm = std::make_unique<ProgramRemix>();
    rm->channels_in = channels_in;
    rm->channels_out = channels_out;
    rm->n_matrices = n_matrices;
    rm->h_terms = std::move(terms);
    rm->h_calls.assign(n_streams_, RmStreamCall{});
    rm->matrices.upload(compact, last_stream_);
    rm->calls.reserve(n_streams_);
    rm->records.reserve(n_streams_);
    remix_ = std::move(rm);  // (the earlier buffers are released here, behind the wait above)
    // the records of a call that brought nothing, so that fetch_remixed has something to say before the first call
    for (uint32_t s = 0; s < n_streams_; ++s) remix_->h_calls[s] = RmStreamCall{0, 0, remix_->h_terms[0], 0};
    pl_upload_table(remix_->staging, remix_->h_calls, remix_->calls.ptr, last_stream_);
    const RmArgs a = remix_args();
    launch_rm_begin(a, last_stream_);
    OMX_HIP(hipGetLastError());
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first remix call may come on another stream)
    return OMX_NONE;
}

RmArgs ProgramLoudnessBank::remix_args() const {
    const ProgramRemix& rm = *remix_;
    RmArgs a{};
    a.n_streams = n_streams_;
    a.channels_in = rm.channels_in;
    a.channels_out = rm.channels_out;
    a.floor_db = cfg_.floor_db;
    a.matrices = rm.matrices.ptr;
    a.calls = rm.calls.ptr;
    a.records = rm.records.ptr;
    return a;
}

// Everything is checked before anything is touched: a refused call leaves d_out and the records as they were.
int ProgramLoudnessBank::remix(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, const uint32_t* matrix_of_stream,
                               hipStream_t stream, const omx_program_remix_record** d_remixed) {
    const char* who = "remix";
    if (!remix_) return pl_refuse(who, "the remix is not configured (omx_program_loudness_bank_remix_configure)");
    ProgramRemix& rm = *remix_;
    if (!pl_capacity_ok(frames_capacity)) return pl_refuse(who, "frames_capacity beyond 2^32 - 1");
    RmArgs a = remix_args();
    std::vector<RmStreamCall>& calls = rm.h_calls;  // (host scratch only)
    for (uint32_t s = 0; s < n_streams_; ++s) {
        uint64_t f;
        if (!pl_stream_frames(who, frames, frames_capacity, s, f)) return OMX_ERR_INVALID;
        const uint32_t m = matrix_of_stream ? matrix_of_stream[s] : 0u;
        if (m >= rm.n_matrices) return pl_refuse(who, "matrix index out of range");
        calls[s] = RmStreamCall{(uint32_t)f, m, rm.h_terms[m], 0};
        a.max_frames = std::max(a.max_frames, (uint32_t)f);
    }
    const bool any = a.max_frames != 0;
    if (any && (!d_in || !d_out)) return pl_refuse(who, "null pcm");
    // out of place only: a tile would read what another has already written
    const unsigned __int128 row_bytes = (unsigned __int128)n_streams_ * frames_capacity * sizeof(float);
    if (d_in && d_out && pl_ranges_overlap(d_in, row_bytes * a.channels_in, d_out, row_bytes * a.channels_out))
        return pl_refuse(who, "d_in and d_out overlap");

    last_stream_ = stream;
    pl_upload_table(rm.staging, calls, rm.calls.ptr, stream);
    a.in = d_in;
    a.out = d_out;
    a.frames_capacity = frames_capacity;
    launch_rm_begin(a, stream);
    if (any) launch_rm_main(a, stream);
    launch_rm_finish(a, stream);
    OMX_HIP(hipGetLastError());
    if (d_remixed) *d_remixed = rm.records.ptr;
    return any ? OMX_PRODUCED : OMX_NONE;
}

int ProgramLoudnessBank::fetch_remixed(uint64_t stream_index, omx_program_remix_record* dst) {
    if (!remix_ || stream_index >= n_streams_) return pl_refuse("fetch_remixed", "the remix is not configured, or stream index out of range");
    copy_out(dst, remix_->records.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_remix_plan(uint32_t channels_in, uint32_t channels_out, omx_program_remix_info* info) {
    return rm_plan(channels_in, channels_out, info);
}
int omx_program_remix_downmix(const omx_program_downmix_rule* rule, uint32_t channels_in, const uint8_t positions_in[OMX_MAX_CHANNELS],
                              float* matrix, uint32_t* channels_out, uint8_t positions_out[OMX_MAX_CHANNELS]) {
    return rm_downmix(rule, channels_in, positions_in, matrix, channels_out, positions_out);
}
int omx_program_remix_select(uint32_t channels_in, const uint8_t positions_in[OMX_MAX_CHANNELS], uint32_t channels_out,
                             const uint8_t positions_out[OMX_MAX_CHANNELS], float* matrix, uint32_t* missing_mask) {
    return rm_select(channels_in, positions_in, channels_out, positions_out, matrix, missing_mask);
}
int omx_program_loudness_bank_remix_configure(omx_program_loudness_bank* b, uint32_t channels_in, uint32_t channels_out, const float* matrices,
                                              uint32_t n_matrices) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.remix_configure(channels_in, channels_out, matrices, n_matrices); });
}
int omx_program_loudness_bank_remix(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                    float* d_out, const uint32_t* matrix_of_stream, void* stream,
                                    const omx_program_remix_record** d_remixed) {
    if (!b || !d_remixed) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.remix(d_in, frames_capacity, frames, d_out, matrix_of_stream, static_cast<hipStream_t>(stream), d_remixed); });
}
int omx_program_loudness_bank_fetch_remixed(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_remix_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_remixed(stream_index, dst); });
}

}  // extern "C"
