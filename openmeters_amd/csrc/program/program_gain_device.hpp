// The normalisation gain of include/omx/program_normalize.h, steps 1 - 7 of its definition, as ONE function for the host
// (omx_program_gain_evaluate) and the device (the two plan kernels of program_normalize_kernels.hip): they cannot drift apart.
// Every step is f64 on f32 inputs; the library is built with -ffp-contract=off, so no step is fused on either side.  pow is the only
// call whose f64 result may differ between the host's and the device's library.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../../include/omx/program_normalize.h"

namespace omx {

// the rule has been validated (pn_rule_valid, program_normalize.cpp)
__host__ __device__ inline omx_program_gain_record pn_gain(const omx_program_gain_rule& rule, float integrated_lufs, uint64_t gating_above_relative,
                                                           float max_true_peak_db, float floor_db) {
    omx_program_gain_record r;
    const bool peak_known = max_true_peak_db > floor_db;
    r.source_lufs = integrated_lufs;
    r.source_peak_db = max_true_peak_db;
    r.peak_known = peak_known ? 1u : 0u;
    if (gating_above_relative == 0) {
        r.gain_db = 0.0f;
        r.gain = 1.0f;
        r.predicted_lufs = integrated_lufs;
        r.predicted_peak_db = max_true_peak_db;
        r.limited_by = OMX_GAIN_BY_NO_MEASUREMENT;
        return r;
    }
    double g = (double)rule.target_lufs - (double)integrated_lufs;
    uint32_t by = OMX_GAIN_BY_TARGET;
    if ((rule.flags & OMX_GAIN_LIMIT_PEAK) && peak_known) {
        const double pg = (double)rule.true_peak_ceiling_db - (double)max_true_peak_db;
        if (pg < g) {
            g = pg;
            by = OMX_GAIN_BY_PEAK;
        }
    }
    if (g > (double)rule.max_gain_db) {
        g = (double)rule.max_gain_db;
        by = OMX_GAIN_BY_MAX_GAIN;
    }
    if (g < (double)rule.min_gain_db) {  // after the peak limit on purpose: the minimum clamp wins
        g = (double)rule.min_gain_db;
        by = OMX_GAIN_BY_MIN_GAIN;
    }
    r.gain_db = (float)g;
    r.gain = (float)pow(10.0, (double)r.gain_db / 20.0);
    r.predicted_lufs = (float)((double)integrated_lufs + (double)r.gain_db);
    r.predicted_peak_db = peak_known ? (float)((double)max_true_peak_db + (double)r.gain_db) : floor_db;
    r.limited_by = by;
    return r;
}

}  // namespace omx
