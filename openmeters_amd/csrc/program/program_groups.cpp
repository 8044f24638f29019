// Host side of the programme bank's groups (include/omx/program_groups.h): validation against the host's own counters (h_meta_: the
// device is never read), the resolved member and group tables of the call in one upload, scratch that grows on first use, one launch
// on the caller's stream.  Nothing here synchronises except fetch_groups.
#include "program_loudness.hpp"

namespace omx {

// Everything is checked before anything is touched: a refused call leaves the bank and every earlier result as they were.
int ProgramLoudnessBank::measure_groups(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                        uint64_t n_groups, hipStream_t stream, const omx_program_loudness_record** d_records) {
    if (n_groups == 0) return OMX_NONE;
    const char* who = "measure_groups";
    if (!groups || (!members && n_members > 0) || n_groups > 0x7FFFFFFFull || n_members > 0x7FFFFFFFull)
        return pl_refuse(who, "null members or groups (or more than 2^31 - 1 of them)");
    // ---- the members, resolved; before[m] of member m in 64 bits for the groups' own counts
    const size_t groups_at = (size_t)n_members * sizeof(PgMember);
    h_group_tables_.resize(groups_at + (size_t)n_groups * sizeof(PgGroup));
    PgMember* hm = reinterpret_cast<PgMember*>(h_group_tables_.data());
    PgGroup* hg = reinterpret_cast<PgGroup*>(h_group_tables_.data() + groups_at);
    std::vector<uint64_t> seg_before(n_members + 1, 0), g_before(n_members + 1, 0), s_before(n_members + 1, 0);
    bool partial = false;
    // (tuning library only: OMX_GROUPS_STAGING=0 forms the short-term blocks anew in every walk, for the A/B)
    const char* staging_env = tuning_env("OMX_GROUPS_STAGING");
    const bool staging = !bounded_ && !(staging_env && staging_env[0] == '0');
    uint64_t staged = 0;
    for (uint64_t i = 0; i < n_members; ++i) {
        const omx_program_interval& in = members[i];
        if (in.stream >= n_streams_ || in.first_segment > h_meta_[in.stream].segments ||
            (in.segment_count != OMX_PROGRAM_TO_END && in.segment_count > h_meta_[in.stream].segments - in.first_segment))
            return pl_refuse(who, "stream index out of range or member outside the stored segments");
        const uint64_t segments = h_meta_[in.stream].segments;
        const uint64_t n = in.segment_count == OMX_PROGRAM_TO_END ? segments - in.first_segment : in.segment_count;
        partial = partial || in.first_segment != 0 || n != segments;
        hm[i] = PgMember{(uint64_t)in.stream * capacity_ + in.first_segment, (uint32_t)n, (uint32_t)g_before[i], (uint32_t)s_before[i], in.stream};
        seg_before[i + 1] = seg_before[i] + n;
        g_before[i + 1] = g_before[i] + (n >= 4 ? n - 3 : 0);
        s_before[i + 1] = s_before[i] + (n >= 30 ? n - 29 : 0);
    }
    for (uint64_t k = 0; k < n_groups; ++k) {
        const omx_program_group& g = groups[k];
        if (g.first_member > n_members || g.member_count > n_members - g.first_member) return pl_refuse(who, "group range outside the member table");
        const uint64_t lo = g.first_member, hi = g.first_member + g.member_count;
        if (g_before[hi] - g_before[lo] > 0xFFFFFFFFull) return pl_refuse(who, "more than 2^32 - 1 gating blocks in a group");
        const uint64_t segments = seg_before[hi] - seg_before[lo];
        const uint64_t st_blocks = s_before[hi] - s_before[lo];
        const bool stage = staging && st_blocks >= kPgStageMin && staged + st_blocks <= kPgStageMax;
        hg[k] = PgGroup{(uint32_t)lo, (uint32_t)g.member_count, segments * seg_, segments, g_before[hi] - g_before[lo], st_blocks,
                        stage ? staged : kPgNoStage};
        if (stage) staged += st_blocks;
    }
    if (bounded_ && partial) {
        set_last_error("program loudness measure_groups: the bank has bounded storage and keeps no segments: every member must be a whole stream");
        return OMX_ERR_UNSUPPORTED;
    }

    last_stream_ = stream;
    group_tables_.reserve(h_group_tables_.size());
    group_records_.reserve(n_groups);
    group_stage_.reserve(staged);
    group_staging_.upload(h_group_tables_.data(), h_group_tables_.size(), group_tables_.ptr, stream);
    const PgMember* dm = reinterpret_cast<const PgMember*>(group_tables_.ptr);
    const PgGroup* dg = reinterpret_cast<const PgGroup*>(group_tables_.ptr + groups_at);
    if (bounded_) {
        PgBoundedArgs a{};
        a.hist = hist_.ptr;
        a.running = running_.ptr;
        a.members = dm;
        a.groups = dg;
        a.records = group_records_.ptr;
        a.floor_db = cfg_.floor_db;
        launch_pg_bounded(a, (uint32_t)n_groups, stream);
    } else {
        PlResultArgs r = result_args();
        r.records = group_records_.ptr;
        launch_pg_stored(r, dm, dg, group_stage_.ptr, (uint32_t)n_groups, stream);
    }
    OMX_HIP(hipGetLastError());
    if (d_records) *d_records = group_records_.ptr;
    return OMX_PRODUCED;
}

int ProgramLoudnessBank::fetch_groups(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                      uint64_t n_groups, omx_program_loudness_record* dst) {
    if (n_groups == 0) return OMX_NONE;
    if (!dst) return pl_refuse("fetch_groups", "null records");
    const int rc = measure_groups(members, n_members, groups, n_groups, last_stream_, nullptr);
    if (rc < 0) return rc;
    copy_out(dst, group_records_.ptr, (size_t)n_groups * sizeof(*dst), false, last_stream_);
    return rc;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_loudness_bank_measure_groups(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                             const omx_program_group* groups, uint64_t n_groups, void* stream,
                                             const omx_program_loudness_record** d_records) {
    if (!b || !d_records) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.measure_groups(members, n_members, groups, n_groups, static_cast<hipStream_t>(stream), d_records); });
}
int omx_program_loudness_bank_fetch_groups(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                           const omx_program_group* groups, uint64_t n_groups, omx_program_loudness_record* dst) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_groups(members, n_members, groups, n_groups, dst); });
}

}  // extern "C"
