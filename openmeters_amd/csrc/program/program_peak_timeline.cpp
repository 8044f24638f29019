// Host side of the programme bank's peak timeline (include/omx/program_peak_timeline.h): the switch, the keys' storage, validation
// against the host's own counters (h_meta_: the device is never read), one small table per part call, launches on the caller's
// stream.  Nothing here synchronises except the fetch forms and the switch.  Every refusal reads "program loudness peak timeline: ...".
#include "program_loudness.hpp"

namespace omx {

namespace {

const char* const kWho = "peak timeline";
const char* const kOff = "the timeline is off (omx_program_loudness_bank_set_peak_timeline)";

}  // namespace

int ProgramLoudnessBank::set_peak_timeline(bool on) {
    if (bounded_) {
        set_last_error("program loudness peak timeline: the bank has bounded storage and keeps no segments");
        return OMX_ERR_UNSUPPORTED;
    }
    if (!peaks_on_) return pl_refuse(kWho, "peaks are off (omx_program_loudness_bank_set_peaks first)");
    for (uint32_t s = 0; s < n_streams_; ++s)
        if (h_meta_[s].frames != 0) return pl_refuse(kWho, "a stream holds samples (reset every stream first)");
    if (!on) peak_timeline_off();
    peak_timeline_on_ = on;
    return OMX_NONE;
}

void ProgramLoudnessBank::peak_timeline_off() {
    if (!peak_timeline_on_) return;
    OMX_HIP(hipStreamSynchronize(last_stream_));  // (a pass that reads the keys may still be in flight)
    pt_keys_.release();
    pt_clear_.release();
    pt_rows_.release();
    pt_tables_.release();
    pt_records_.release();
    peak_timeline_on_ = false;
}

// In front of the peak pass of a call, on its stream: the stored keys of the streams the call resets go back to zero (in the layout
// they were written with: the rate and the channel count of before the call), and a call that brings frames makes sure the keys exist.
unsigned long long* ProgramLoudnessBank::peak_timeline_keys(bool frames_taken, hipStream_t stream) {
    if (!h_pt_clear_.empty() && pt_keys_.ptr) {
        pt_clear_.reserve(h_pt_clear_.size());
        pl_upload_table(pt_clear_staging_, h_pt_clear_, pt_clear_.ptr, stream);
        launch_pt_clear(pt_keys_.ptr, pt_clear_.ptr, h_pt_clear_.size(), stream);
    }
    h_pt_clear_.clear();
    if (!frames_taken) return pt_keys_.ptr;
    const size_t need = (size_t)n_streams_ * (capacity_ + 1) * channels_ * kPtKinds;
    if (need > pt_keys_.count) {
        // grow-only.  A larger layout means more channels, which a bank takes on only when every stream that held samples is reset
        // in this call: nothing stored is lost, and the new buffer starts cleared.
        pt_keys_.reserve(need);
        OMX_HIP(hipMemsetAsync(pt_keys_.ptr, 0, need * sizeof(unsigned long long), stream));
    }
    return pt_keys_.ptr;
}

// What refuses a rows call of n_streams streams (0: nothing does).  Everything is checked before anything is touched or grown.
int ProgramLoudnessBank::peak_rows_refusal(uint32_t n_streams, uint64_t first, uint64_t stride, uint64_t count, const void* rows) const {
    if (!rows) return pl_refuse(kWho, "null rows");
    if (stride == 0) return pl_refuse(kWho, "stride 0");
    if (stride > 0xFFFFFFFFull / std::max(seg_, 1u)) return pl_refuse(kWho, "stride * segment length beyond 2^32 - 1 frames");
    if ((count - 1) > (~0ull - first) / stride || count > 0x7FFFFFFFull - kPtThreads || count * n_streams > 0xFFFFFFFFull)
        return pl_refuse(kWho, "first + (count - 1) * stride, count (beyond 2^31 - 257) or n_streams * count out of range");
    if (n_streams > kPtMaxStreams) return pl_refuse(kWho, "more than 65535 streams in one call (use fetch_peak_rows per stream)");
    return 0;
}

// Rows of the streams [stream_base, stream_base + n_streams) into d_rows [n_streams][count]; the call has been checked.
void ProgramLoudnessBank::peak_rows_of(uint32_t stream_base, uint32_t n_streams, uint64_t first, uint64_t stride, uint64_t count,
                                       omx_program_peak_row* d_rows, hipStream_t stream) {
    last_stream_ = stream;
    pl_upload_table(meta_staging_, h_meta_, meta_.ptr, stream);
    PtRowArgs a{};
    a.keys = pt_keys_.ptr;  // (null until a call brings frames: no stream has a segment then, and none is read)
    a.rows_capacity = capacity_ + 1;
    a.meta = meta_.ptr;
    a.first = first;
    a.stride = stride;
    a.count = (uint32_t)count;
    a.n_streams = n_streams;
    a.stream_base = stream_base;
    a.channels = std::max(channels_, 1u);
    a.seg = std::max(seg_, 1u);  // (no programme yet: no stream has a segment, every row is invalid)
    a.rows = d_rows;
    launch_pt_rows(a, stream);
    OMX_HIP(hipGetLastError());
}

int ProgramLoudnessBank::peak_rows(uint64_t first, uint64_t stride, uint64_t count, omx_program_peak_row* d_rows, hipStream_t stream) {
    if (!peak_timeline_on_) return pl_refuse(kWho, kOff);
    if (count == 0) return OMX_NONE;
    if (const int rc = peak_rows_refusal(n_streams_, first, stride, count, d_rows)) return rc;
    peak_rows_of(0, n_streams_, first, stride, count, d_rows, stream);
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::fetch_peak_rows(uint64_t stream_index, uint64_t first, uint64_t stride, uint64_t count, omx_program_peak_row* dst) {
    if (!peak_timeline_on_) return pl_refuse(kWho, kOff);
    if (stream_index >= n_streams_) return pl_refuse(kWho, "stream index out of range");
    if (count == 0) return OMX_NONE;
    if (const int rc = peak_rows_refusal(1, first, stride, count, dst)) return rc;
    pt_rows_.reserve(count);
    peak_rows_of((uint32_t)stream_index, 1, first, stride, count, pt_rows_.ptr, last_stream_);
    copy_out(dst, pt_rows_.ptr, count * sizeof(*dst), false, last_stream_);
    return OMX_PRODUCED;
}

// Intervals (groups == null: every member is a part of its own) and groups: the tables resolved against h_meta_, one upload, one
// workgroup per part.  Everything is checked before anything on the device is touched.  for_gains: the call is plan_part_gains',
// which measures the groups' loudness next, so the one refusal measure_groups has beyond these (the gating blocks of a group) is made
// here, in this header's words and in front of the first launch.
int ProgramLoudnessBank::part_peaks(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups, uint64_t n_groups,
                                    hipStream_t stream, const omx_program_part_peak** d_peaks, bool for_gains) {
    if (!peak_timeline_on_) return pl_refuse(kWho, kOff);
    const uint64_t n_parts = groups ? n_groups : n_members;
    if (n_parts == 0) return OMX_NONE;
    if ((!members && n_members > 0) || n_parts > 0x7FFFFFFFull || n_members > 0x7FFFFFFFull)
        return pl_refuse(kWho, "null members or groups (or more than 2^31 - 1 of them)");
    const size_t parts_at = (size_t)n_members * sizeof(PtMember);
    h_pt_tables_.resize(parts_at + (size_t)n_parts * sizeof(PtPart));
    PtMember* hm = reinterpret_cast<PtMember*>(h_pt_tables_.data());
    PtPart* hp = reinterpret_cast<PtPart*>(h_pt_tables_.data() + parts_at);
    h_pt_before_.assign(2 * ((size_t)n_members + 1), 0);  // segments and gating blocks in front of member i
    uint64_t* seg_before = h_pt_before_.data();
    uint64_t* g_before = seg_before + n_members + 1;
    for (uint64_t i = 0; i < n_members; ++i) {
        const omx_program_interval& in = members[i];
        if (in.stream >= n_streams_ || in.first_segment > h_meta_[in.stream].segments ||
            (in.segment_count != OMX_PROGRAM_TO_END && in.segment_count > h_meta_[in.stream].segments - in.first_segment))
            return pl_refuse(kWho, "stream index out of range or interval outside the stored segments");
        const uint64_t n = in.segment_count == OMX_PROGRAM_TO_END ? h_meta_[in.stream].segments - in.first_segment : in.segment_count;
        hm[i] = PtMember{in.first_segment, n, in.stream, 0u};
        seg_before[i + 1] = seg_before[i] + n;
        g_before[i + 1] = g_before[i] + (n >= 4 ? n - 3 : 0);
        if (!groups) hp[i] = PtPart{(uint32_t)i, 1u, n * seg_};
    }
    for (uint64_t k = 0; groups && k < n_groups; ++k) {
        const omx_program_group& g = groups[k];
        if (g.first_member > n_members || g.member_count > n_members - g.first_member) return pl_refuse(kWho, "group range outside the member table");
        if (for_gains && g_before[g.first_member + g.member_count] - g_before[g.first_member] > 0xFFFFFFFFull)
            return pl_refuse(kWho, "more than 2^32 - 1 gating blocks in a group");
        hp[k] = PtPart{(uint32_t)g.first_member, (uint32_t)g.member_count, (seg_before[g.first_member + g.member_count] - seg_before[g.first_member]) * seg_};
    }
    last_stream_ = stream;
    pt_tables_.reserve(h_pt_tables_.size());
    pt_records_.reserve(n_parts);
    pt_staging_.upload(h_pt_tables_.data(), h_pt_tables_.size(), pt_tables_.ptr, stream);
    PtPartArgs a{};
    a.keys = pt_keys_.ptr;  // (null until a call brings frames: every member is empty then, and nothing is read)
    a.rows_capacity = capacity_ + 1;
    a.members = reinterpret_cast<const PtMember*>(pt_tables_.ptr);
    a.parts = reinterpret_cast<const PtPart*>(pt_tables_.ptr + parts_at);
    a.records = pt_records_.ptr;
    a.channels = std::max(channels_, 1u);
    a.seg = seg_;
    a.floor_db = cfg_.floor_db;
    launch_pt_parts(a, (uint32_t)n_parts, stream);
    OMX_HIP(hipGetLastError());
    if (d_peaks) *d_peaks = pt_records_.ptr;
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::measure_interval_peaks(const omx_program_interval* intervals, uint64_t n, hipStream_t stream,
                                                const omx_program_part_peak** d_peaks) {
    return part_peaks(intervals, n, nullptr, 0, stream, d_peaks, false);
}

int ProgramLoudnessBank::fetch_interval_peaks(const omx_program_interval* intervals, uint64_t n, omx_program_part_peak* dst) {
    if (!peak_timeline_on_) return pl_refuse(kWho, kOff);
    if (n == 0) return OMX_NONE;
    if (!dst) return pl_refuse(kWho, "null records");
    const int rc = part_peaks(intervals, n, nullptr, 0, last_stream_, nullptr, false);
    if (rc < 0) return rc;
    copy_out(dst, pt_records_.ptr, (size_t)n * sizeof(*dst), false, last_stream_);
    return rc;
}

int ProgramLoudnessBank::measure_group_peaks(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                             uint64_t n_groups, hipStream_t stream, const omx_program_part_peak** d_peaks) {
    if (!peak_timeline_on_) return pl_refuse(kWho, kOff);
    if (n_groups == 0) return OMX_NONE;
    if (!groups) return pl_refuse(kWho, "null members or groups (or more than 2^31 - 1 of them)");
    return part_peaks(members, n_members, groups, n_groups, stream, d_peaks, false);
}

int ProgramLoudnessBank::fetch_group_peaks(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                           uint64_t n_groups, omx_program_part_peak* dst) {
    if (!peak_timeline_on_) return pl_refuse(kWho, kOff);
    if (n_groups == 0) return OMX_NONE;
    if (!dst) return pl_refuse(kWho, "null records");
    const int rc = measure_group_peaks(members, n_members, groups, n_groups, last_stream_, nullptr);
    if (rc < 0) return rc;
    copy_out(dst, pt_records_.ptr, (size_t)n_groups * sizeof(*dst), false, last_stream_);
    return rc;
}

int ProgramLoudnessBank::plan_part_gains(const omx_program_gain_rule* rule, const omx_program_interval* members, uint64_t n_members,
                                         const omx_program_group* groups, uint64_t n_groups, hipStream_t stream,
                                         const omx_program_gain_record** d_gains) {
    omx_program_gain_record probe;
    if (omx_program_gain_evaluate(rule, 0.0f, 0, 0.0f, 0.0f, &probe) != OMX_NONE)
        return pl_refuse(kWho, "bad gain rule (null, a non-finite field in use, min_gain_db > max_gain_db or an unknown flag)");
    // the peaks first: they make every check measure_groups makes on a bank with stored segments, so it refuses nothing after them
    if (!peak_timeline_on_) return pl_refuse(kWho, kOff);
    if (n_groups == 0) return OMX_NONE;
    if (!groups) return pl_refuse(kWho, "null members or groups (or more than 2^31 - 1 of them)");
    int rc = part_peaks(members, n_members, groups, n_groups, stream, nullptr, true);
    if (rc != OMX_PRODUCED) return rc;
    rc = measure_groups(members, n_members, groups, n_groups, stream, nullptr);
    if (rc != OMX_PRODUCED) return rc;
    gain_records_.reserve(n_groups);
    launch_pt_plan(*rule, group_records_.ptr, pt_records_.ptr, gain_records_.ptr, (uint32_t)n_groups, cfg_.floor_db, stream);
    OMX_HIP(hipGetLastError());
    gains_planned_ = n_groups;
    if (d_gains) *d_gains = gain_records_.ptr;
    return OMX_PRODUCED;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_loudness_bank_set_peak_timeline(omx_program_loudness_bank* b, uint32_t on) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.set_peak_timeline(on != 0); });
}
int omx_program_loudness_bank_peak_rows(omx_program_loudness_bank* b, uint64_t first, uint64_t stride, uint64_t count,
                                        omx_program_peak_row* d_rows, void* stream) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.peak_rows(first, stride, count, d_rows, static_cast<hipStream_t>(stream)); });
}
int omx_program_loudness_bank_fetch_peak_rows(omx_program_loudness_bank* b, uint64_t stream_index, uint64_t first, uint64_t stride,
                                              uint64_t count, omx_program_peak_row* dst) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_peak_rows(stream_index, first, stride, count, dst); });
}
int omx_program_loudness_bank_measure_interval_peaks(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                                     void* stream, const omx_program_part_peak** d_peaks) {
    if (!b) return OMX_ERR_INVALID;
    if (!d_peaks) return pl_refuse(kWho, "null d_peaks");
    return guarded([&] { return b->impl.measure_interval_peaks(intervals, n, static_cast<hipStream_t>(stream), d_peaks); });
}
int omx_program_loudness_bank_fetch_interval_peaks(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                                   omx_program_part_peak* dst) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_interval_peaks(intervals, n, dst); });
}
int omx_program_loudness_bank_measure_group_peaks(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                                  const omx_program_group* groups, uint64_t n_groups, void* stream,
                                                  const omx_program_part_peak** d_peaks) {
    if (!b) return OMX_ERR_INVALID;
    if (!d_peaks) return pl_refuse(kWho, "null d_peaks");
    return guarded([&] { return b->impl.measure_group_peaks(members, n_members, groups, n_groups, static_cast<hipStream_t>(stream), d_peaks); });
}
int omx_program_loudness_bank_fetch_group_peaks(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                                const omx_program_group* groups, uint64_t n_groups, omx_program_part_peak* dst) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_group_peaks(members, n_members, groups, n_groups, dst); });
}
int omx_program_loudness_bank_plan_part_gains(omx_program_loudness_bank* b, const omx_program_gain_rule* rule,
                                              const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                              uint64_t n_groups, void* stream, const omx_program_gain_record** d_gains) {
    if (!b) return OMX_ERR_INVALID;
    if (!d_gains) return pl_refuse(kWho, "null d_gains");
    return guarded([&] { return b->impl.plan_part_gains(rule, members, n_members, groups, n_groups, static_cast<hipStream_t>(stream), d_gains); });
}

}  // extern "C"
