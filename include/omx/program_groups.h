/* Programme loudness bank, groups: several programmes, or parts of programmes, measured as ONE programme: the album loudness of
 * twelve tracks, a series across its episodes, a programme without its ad breaks, a reel assembled from spots (what libebur128
 * offers as ebur128_loudness_global_multiple / ebur128_loudness_range_multiple).
 *
 * The figure cannot be made from the members' own records: the relative gate of the whole differs from every member's (a quiet track
 * passes its own gate and fails the album's), and the loudness range needs two order statistics over the union of all short-term
 * blocks.  The bank holds every segment energy (or histogram) in device memory, so the group record is made there and 168 bytes per
 * group cross to the host.
 *
 * Additive: this header adds two functions, one structure and one constant; nothing declared in program_loudness.h, program_peaks.h,
 * program_timeline.h or program_histogram.h changes and OMX_ABI_VERSION stays as it is.  A bank that never calls one of them launches
 * and allocates nothing more.
 *
 * MEMBERS AND GROUPS
 *   A member is an omx_program_interval (program_timeline.h): segments [first_segment, first_segment + segment_count) of one stream.
 *   segment_count == OMX_PROGRAM_TO_END means "up to the stream's last stored segment" (as the host's counters stand at the call).
 *   A group is a contiguous range [first_member, first_member + member_count) of the member table.  Ranges of different groups may
 *   overlap ("disc 1", "disc 2" and "the box set" share members).  A stream or part may appear more than once in a group and counts
 *   that many times.  member_count == 0 is allowed.
 *
 * DEFINITIONS, STORED MODE ("Groups"; tests/program_groups_ref.py restates them), on top of those of
 * program_loudness.h and program_timeline.h.
 *   Member m, with a_m = first_segment, n_m = its resolved segment_count and s_m = its stream, contributes its own gating blocks
 *   g_m[k], k = 3 .. n_m - 1, and short-term blocks st_m[k], k = 29 .. n_m - 1, both formed from e[s_m][a_m .. a_m + n_m) with the
 *   result pass's own expressions, oldest segment first (exactly the blocks of the INTERVAL RECORD of that member).  No block spans
 *   two members.
 *   G and ST are the concatenations of these blocks in member order.  The group record is the record of program_loudness.h with G
 *   and ST in place of the stream's gating and short-term blocks:
 *     the absolute gate;  relative_threshold_energy = 0.1 * mean(G above the absolute gate);
 *     integrated_energy = mean of G above both gates;  all four counts above the gates;
 *     loudness range = the nearest-rank elements floor((n - 1) * 0.10 + 0.5) and floor((n - 1) * 0.95 + 0.5) of the sorted ST above
 *       both gates (factor 0.01), n their number;
 *     max_momentary_energy / max_short_term_energy = the maximum over G / ST.
 *   The remaining fields:
 *     segments = sum of n_m;  frames = segments * the segment length in frames;  gating_blocks = |G|;  short_term_blocks = |ST|
 *     momentary_* / short_term_* (the latest blocks) = those of the LAST member: its last block, 0 / the floor when it has fewer than
 *       4 / 30 segments or the group is empty
 *     max_true_peak_db = the floor, as for an interval (program_peak_timeline.h measures the peaks of a group);  overflow = 0
 *   An empty group, or one with no passing block, has integrated = the floor and range = 0.
 *   SUMMATION ORDER.  Block i of G (and of ST), counted from 0 over the concatenation, goes to lane i mod 256; each lane adds its
 *   blocks in ascending i; then the binary tree of the result pass runs.  So a group of ONE member has the bytes of
 *   omx_program_loudness_bank_fetch_intervals of that member in every field, and a group of one whole stream the bytes of
 *   omx_program_loudness_bank_fetch in every field but frames, overflow and max_true_peak_db.  Counts, both range energies and both
 *   maxima do not depend on the order of the members; the means do, within rounding.
 *
 * DEFINITIONS, BOUNDED MODE (a bank made by omx_program_loudness_bank_create_bounded, program_histogram.h)
 *   Every member must be a whole stream: first_segment == 0 and segment_count == OMX_PROGRAM_TO_END or segments[stream]; anything
 *   else is OMX_ERR_UNSUPPORTED (the histograms have no time axis).
 *   Group histogram: count[i] = sum over the members of count_m[i]; sum[i] = the members' sum_m[i] added in member order, in f64
 *   without fused multiply-add, starting from 0.  The record is made from that histogram by the definitions of program_histogram.h
 *   (literally ascending i, by the code of the per-stream result pass).  Maxima: the maximum over the members.  Latest blocks: the
 *   last member's.  segments, gating_blocks and short_term_blocks: the sums of the members' counts; frames = segments * the segment
 *   length; max_true_peak_db = the floor; overflow = 0.
 *   A group of one stream has the bytes of omx_program_loudness_bank_fetch of that stream but for frames and max_true_peak_db. */
#ifndef OMX_PROGRAM_GROUPS_H
#define OMX_PROGRAM_GROUPS_H

#include "program_timeline.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_PROGRAM_TO_END UINT64_MAX   /* as a member's segment_count: up to the stream's last stored segment */

typedef struct omx_program_group {
    uint64_t first_member;
    uint64_t member_count;
} omx_program_group;                    /* 16 bytes: members[first_member .. first_member + member_count) */

/* members: host array [n_members]; groups: host array [n_groups].  *d_records: device array [n_groups], one record per group, written
 * on `stream`, valid until the next call on the bank.
 * OMX_ERR_INVALID, with nothing changed: a stream index out of range; first_segment > segments[stream]; first_segment +
 * segment_count > segments[stream] for a count other than OMX_PROGRAM_TO_END; a group range outside members[0 .. n_members); null
 * members with n_members > 0; null groups with n_groups > 0; a null d_records; more than 2^31 - 1 groups or members; a group with
 * more than 2^32 - 1 gating blocks.
 * OMX_ERR_UNSUPPORTED, with nothing changed: on a bounded bank, a member that is not a whole stream.
 * n_groups == 0: OMX_NONE, nothing is measured.  Otherwise OMX_PRODUCED. */
int omx_program_loudness_bank_measure_groups(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                             const omx_program_group* groups, uint64_t n_groups, void* stream,
                                             const omx_program_loudness_record** d_records);
/* Measures, copies to dst [n_groups] (host) and synchronises.  Also OMX_ERR_INVALID: a null dst. */
int omx_program_loudness_bank_fetch_groups(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                           const omx_program_group* groups, uint64_t n_groups, omx_program_loudness_record* dst);
/* A refused call changes nothing: neither the bank's state nor what an earlier call returned. */

#ifdef __cplusplus
}
#endif
#endif
