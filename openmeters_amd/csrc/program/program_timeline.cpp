// Host side of the programme bank's timeline and intervals (include/omx/program_timeline.h): validation against the host's own
// counters (h_meta_: the device is never read), scratch that grows on first use, launches on the caller's stream.  Nothing here
// synchronises except the two fetch forms.
#include "program_loudness.hpp"

namespace omx {

// Rows j = first + i * stride, i < count, of the streams [stream_base, stream_base + n_streams) into d_rows [n_streams][count].
// The arguments are checked before anything is touched: a refused call leaves the bank and every earlier result as they were.
int ProgramLoudnessBank::timeline_rows(uint32_t stream_base, uint32_t n_streams, uint64_t first, uint64_t stride, uint64_t count,
                                       omx_program_timeline_row* d_rows, hipStream_t stream) {
    if (count == 0) return OMX_NONE;
    const char* who = "timeline";
    if (!d_rows) return pl_refuse(who, "null rows");
    if (stride == 0) return pl_refuse(who, "stride 0");
    // the last j in 64 bits, the launch grid and the row index in 32
    if ((count - 1) > (~0ull - first) / stride || count > 0x7FFFFFFFull - kTlThreads || count * n_streams > 0xFFFFFFFFull)
        return pl_refuse(who, "first + (count - 1) * stride or n_streams * count out of range");
    // refused before anything is touched, not left to fail at the launch
    if (n_streams > kTlMaxStreams) return pl_refuse(who, "more than 65535 streams in one call (use fetch_timeline per stream)");
    const uint64_t last = first + (count - 1) * stride;
    uint64_t pitch = 1;  // 1 + the largest j that exists and is asked for
    for (uint32_t s = stream_base; s < stream_base + n_streams; ++s) pitch = std::max(pitch, std::min<uint64_t>(h_meta_[s].segments, last + 1));
    if (pitch > 0x7FFFFFFFull) unsupported("programme loudness timeline: more than 2^31 - 1 segments in a stream");
    last_stream_ = stream;
    pl_upload_table(meta_staging_, h_meta_, meta_.ptr, stream);
    // scratch: 20 bytes per block up to the last j asked for, grow-only, kept until the bank goes; every call redoes the scan from k = 0
    tl_gated_.reserve((size_t)n_streams * pitch);
    tl_threshold_.reserve((size_t)n_streams * pitch);
    tl_above_.reserve((size_t)n_streams * pitch);
    TlArgs a{};
    a.segments = segments_.ptr;
    a.capacity = capacity_;
    a.meta = meta_.ptr;
    a.first = first;
    a.stride = stride;
    a.count = (uint32_t)count;
    a.pitch = (uint32_t)pitch;
    a.n_streams = n_streams;
    a.stream_base = stream_base;
    a.floor_db = cfg_.floor_db;
    a.absolute_gate = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    a.gated = tl_gated_.ptr;
    a.threshold = tl_threshold_.ptr;
    a.above = tl_above_.ptr;
    a.rows = d_rows;
    launch_tl_scan(a, stream);
    launch_tl_rows(a, stream);
    OMX_HIP(hipGetLastError());
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::timeline(uint64_t first, uint64_t stride, uint64_t count, omx_program_timeline_row* d_rows, hipStream_t stream) {
    if (bounded_) return bounded_refusal("timeline");
    return timeline_rows(0, n_streams_, first, stride, count, d_rows, stream);
}

int ProgramLoudnessBank::fetch_timeline(uint64_t stream_index, uint64_t first, uint64_t stride, uint64_t count, omx_program_timeline_row* dst) {
    if (bounded_) return bounded_refusal("fetch_timeline");
    const char* who = "fetch_timeline";
    if (stream_index >= n_streams_) return pl_refuse(who, "stream index out of range");
    if (count == 0) return OMX_NONE;
    if (!dst || stride == 0 || count > 0x7FFFFFFFull - kTlThreads) return pl_refuse(who, "null rows, stride 0 or count out of range");
    if ((count - 1) > (~0ull - first) / stride) return pl_refuse(who, "first + (count - 1) * stride out of range");
    tl_rows_.reserve(count);
    const int rc = timeline_rows((uint32_t)stream_index, 1, first, stride, count, tl_rows_.ptr, last_stream_);
    if (rc < 0) return rc;
    copy_out(dst, tl_rows_.ptr, count * sizeof(*dst), false, last_stream_);
    return rc;
}

int ProgramLoudnessBank::measure_intervals(const omx_program_interval* intervals, uint64_t n, hipStream_t stream,
                                           const omx_program_loudness_record** d_records) {
    if (bounded_) return bounded_refusal("measure_intervals");
    if (n == 0) return OMX_NONE;
    const char* who = "measure_intervals";
    if (!intervals || n > 0x7FFFFFFFull) return pl_refuse(who, "null intervals (or more than 2^31 - 1)");
    for (uint64_t i = 0; i < n; ++i) {
        const omx_program_interval& in = intervals[i];
        if (in.stream >= n_streams_ || in.first_segment > h_meta_[in.stream].segments ||
            in.segment_count > h_meta_[in.stream].segments - in.first_segment)
            return pl_refuse(who, "stream index out of range or interval outside the stored segments");
    }
    h_interval_descs_.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        const omx_program_interval& in = intervals[i];
        h_interval_descs_[i] = PlIntervalDesc{(uint64_t)in.stream * capacity_ + in.first_segment, in.segment_count * seg_, (uint32_t)in.segment_count, 0u};
    }
    last_stream_ = stream;
    interval_descs_.reserve(n);
    interval_records_.reserve(n);
    pl_upload_table(interval_staging_, h_interval_descs_, interval_descs_.ptr, stream);
    PlResultArgs r = result_args();
    r.records = interval_records_.ptr;
    launch_pl_intervals(r, interval_descs_.ptr, (uint32_t)n, stream);
    OMX_HIP(hipGetLastError());
    if (d_records) *d_records = interval_records_.ptr;
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::fetch_intervals(const omx_program_interval* intervals, uint64_t n, omx_program_loudness_record* dst) {
    if (bounded_) return bounded_refusal("fetch_intervals");
    if (n == 0) return OMX_NONE;
    if (!dst) return pl_refuse("fetch_intervals", "null records");
    const int rc = measure_intervals(intervals, n, last_stream_, nullptr);
    if (rc < 0) return rc;
    copy_out(dst, interval_records_.ptr, (size_t)n * sizeof(*dst), false, last_stream_);
    return rc;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_loudness_bank_timeline(omx_program_loudness_bank* b, uint64_t first, uint64_t stride, uint64_t count,
                                       omx_program_timeline_row* d_rows, void* stream) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.timeline(first, stride, count, d_rows, static_cast<hipStream_t>(stream)); });
}
int omx_program_loudness_bank_fetch_timeline(omx_program_loudness_bank* b, uint64_t stream_index, uint64_t first, uint64_t stride,
                                             uint64_t count, omx_program_timeline_row* dst) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_timeline(stream_index, first, stride, count, dst); });
}
int omx_program_loudness_bank_measure_intervals(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                                void* stream, const omx_program_loudness_record** d_records) {
    if (!b || !d_records) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.measure_intervals(intervals, n, static_cast<hipStream_t>(stream), d_records); });
}
int omx_program_loudness_bank_fetch_intervals(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                              omx_program_loudness_record* dst) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_intervals(intervals, n, dst); });
}

}  // extern "C"
