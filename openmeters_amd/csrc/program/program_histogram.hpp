// Bounded storage of the programme loudness bank (include/omx/program_histogram.h): per stream a histogram of the gating blocks and
// one of the short-term blocks, the newest 29 segment energies and the running maxima instead of every segment energy.
// program_histogram_kernels.hip holds the fold (after the commit of a process call) and the result pass over the histograms.
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_histogram.h"
#include "../../../include/omx/program_peaks.h"

namespace omx {

struct PlStreamCall;
struct PlStreamMeta;

constexpr uint32_t kPhBins = OMX_PROGRAM_HISTOGRAM_BINS;
constexpr uint32_t kPhTail = OMX_PROGRAM_HISTOGRAM_TAIL;
constexpr uint32_t kPhThreads = 256;  // lane t of a stream's workgroup owns the bins t, t + 256, t + 512, t + 768
constexpr uint32_t kPhTile = 1024;    // new segments per LDS tile of the fold

void ph_boundaries(double dst[kPhBins + 1]);  // B[i] = pow(10, (-70 + 0.691 + i / 10.0) / 10)

struct PhRunning {  // what a bounded stream keeps besides its histogram: the latest blocks and the largest ones
    double momentary, short_term, max_momentary, max_short_term;
};

struct PhFoldArgs {
    const PlStreamCall* calls;   // [n_streams]: n_new and reset of this call
    const double* fresh;         // [n_streams][max_new]: the segment energies that completed in this call (the commit's output)
    uint32_t max_new;
    const double* boundaries;    // [kPhBins + 1]
    omx_program_histogram* hist; // [n_streams]
    PhRunning* running;          // [n_streams]
};
void launch_ph_fold(const PhFoldArgs& a, uint32_t n_streams, hipStream_t stream);

struct PhResultArgs {
    const omx_program_histogram* hist;
    const PhRunning* running;
    const PlStreamMeta* meta;
    const float* tp_max;
    const omx_program_peak_record* peaks;  // null with peaks off; else max_true_peak_db = the larger of tp_max and the measured one
    omx_program_loudness_record* records;
    uint32_t n_streams;
    float floor_db;
};
void launch_ph_results(const PhResultArgs& a, hipStream_t stream);

}  // namespace omx
