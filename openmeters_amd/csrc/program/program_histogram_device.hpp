// Device side of the result pass over histograms (include/omx/program_histogram.h), shared by the per-stream kernel
// (program_histogram_kernels.hip) and the bounded group kernel (program_groups_kernels.hip): from 2 x 1000 bins in LDS to the record.
// Lane 0 (gating) and lane 64 (short-term) add the bins in ascending bin order as the definition says; the bin means and gate
// decisions are made in parallel in between.  The caller fills cnt[] / sum[] and synchronises; one lane supplies the rest of the record.
// Include from .hip files only.
#pragma once
#include "program_result_device.hpp"  // ms_to_lufs

namespace omx {

struct PhResultLds {
    unsigned long long cnt[2][kPhBins];  // [0]: gating, [1]: short-term
    double sum[2][kPhBins];
    uint8_t pass[2][kPhBins];
    double threshold[2], pass_sum[2], lra_e[2];
    unsigned long long abs_cnt[2], pass_cnt[2];
};

struct PhRecordTail {  // what the record holds besides the figures made from the bins
    PhRunning run;
    uint64_t frames, segments, gating_blocks, short_term_blocks;
    float max_true_peak_db;
};

// l.cnt / l.sum are filled and a barrier has passed.  `tail()` is called by lane 0 alone.
template <class Tail>
__device__ __forceinline__ void ph_result_from_bins(PhResultLds& l, float floor_db, omx_program_loudness_record* out, Tail&& tail) {
    const uint32_t tid = threadIdx.x;
    const bool adder = tid == 0 || tid == 64;  // one lane per histogram, in two wavefronts
    const uint32_t which = tid >> 6;
    if (adder) {
        unsigned long long c = 0;
        double z = 0.0;
        for (uint32_t i = 0; i < kPhBins; ++i) {  // ascending i (an empty bin adds 0.0: the same bits)
            c += l.cnt[which][i];
            z += l.sum[which][i];
        }
        l.abs_cnt[which] = c;
        l.threshold[which] = c ? (which ? 0.01 : 0.1) * (z / (double)c) : 0.0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < kPhBins; i += kPhThreads) {
#pragma unroll
        for (uint32_t w = 0; w < 2; ++w) l.pass[w][i] = l.cnt[w][i] != 0 && l.sum[w][i] / (double)l.cnt[w][i] > l.threshold[w];
    }
    __syncthreads();
    if (adder) {
        unsigned long long c = 0;
        double z = 0.0;
        for (uint32_t i = 0; i < kPhBins; ++i) {
            if (!l.pass[which][i]) continue;
            c += l.cnt[which][i];
            z += l.sum[which][i];
        }
        l.pass_cnt[which] = c;
        l.pass_sum[which] = z;
        if (which == 1) {
            double lo_e = 0.0, hi_e = 0.0;
            if (c) {
                const double n = (double)c;
                const unsigned long long r_lo = (unsigned long long)floor((n - 1.0) * 0.10 + 0.5), r_hi = (unsigned long long)floor((n - 1.0) * 0.95 + 0.5);
                unsigned long long below = 0;
                bool have_lo = false, have_hi = false;
                for (uint32_t i = 0; i < kPhBins && !have_hi; ++i) {
                    if (!l.pass[1][i]) continue;
                    const unsigned long long upto = below + l.cnt[1][i];
                    if (!have_lo && r_lo < upto) {
                        lo_e = l.sum[1][i] / (double)l.cnt[1][i];
                        have_lo = true;
                    }
                    if (r_hi < upto) {
                        hi_e = l.sum[1][i] / (double)l.cnt[1][i];
                        have_hi = true;
                    }
                    below = upto;
                }
            }
            l.lra_e[0] = lo_e;
            l.lra_e[1] = hi_e;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const PhRecordTail t = tail();
        const float floor = floor_db;
        omx_program_loudness_record r{};
        r.integrated_energy = l.pass_cnt[0] ? l.pass_sum[0] / (double)l.pass_cnt[0] : 0.0;
        r.relative_threshold_energy = l.threshold[0];
        r.lra_low_energy = l.lra_e[0];
        r.lra_high_energy = l.lra_e[1];
        r.momentary_energy = t.run.momentary;
        r.short_term_energy = t.run.short_term;
        r.max_momentary_energy = t.run.max_momentary;
        r.max_short_term_energy = t.run.max_short_term;
        r.frames = t.frames;
        r.segments = t.segments;
        r.gating_blocks = t.gating_blocks;
        r.gating_above_absolute = l.abs_cnt[0];
        r.gating_above_relative = l.pass_cnt[0];
        r.short_term_blocks = t.short_term_blocks;
        r.short_term_above_absolute = l.abs_cnt[1];
        r.short_term_above_relative = l.pass_cnt[1];
        r.integrated_lufs = ms_to_lufs(r.integrated_energy, floor);
        r.relative_threshold_lufs = ms_to_lufs(r.relative_threshold_energy, floor);
        r.loudness_range_lu = l.pass_cnt[1] ? (float)(fma(log10(l.lra_e[1]), 10.0, -0.691) - fma(log10(l.lra_e[0]), 10.0, -0.691)) : 0.0f;
        r.momentary_lufs = ms_to_lufs(r.momentary_energy, floor);
        r.short_term_lufs = ms_to_lufs(r.short_term_energy, floor);
        r.max_momentary_lufs = ms_to_lufs(r.max_momentary_energy, floor);
        r.max_short_term_lufs = ms_to_lufs(r.max_short_term_energy, floor);
        r.max_true_peak_db = t.max_true_peak_db;
        r.overflow = 0;
        *out = r;
    }
}

}  // namespace omx
