// Host side of the programme bank's bounded storage (include/omx/program_histogram.h): the boundaries, the per-stream histograms and
// running values, the fold behind the commit of a process call and the result pass over the histograms.  Nothing here synchronises
// except fetch_histogram and the one upload of the boundaries at creation.
#include "program_loudness.hpp"

namespace omx {

void ph_boundaries(double dst[kPhBins + 1]) {
    for (uint32_t i = 0; i <= kPhBins; ++i) dst[i] = std::pow(10.0, (-70.0 + 0.691 + (double)i / 10.0) / 10.0);
}

void ProgramLoudnessBank::bounded_init() {
    std::vector<double> b(kPhBins + 1);
    ph_boundaries(b.data());
    boundaries_.upload(b, nullptr);
    hist_.reserve(n_streams_);
    running_.reserve(n_streams_);
    OMX_HIP(hipMemset(hist_.ptr, 0, (size_t)n_streams_ * sizeof(omx_program_histogram)));
    OMX_HIP(hipMemset(running_.ptr, 0, (size_t)n_streams_ * sizeof(PhRunning)));
}

// behind the commit (which left the call's new segment energies in fresh_): calls_ holds n_new and reset of every stream
void ProgramLoudnessBank::bounded_fold(uint32_t max_new, hipStream_t stream) {
    PhFoldArgs f{};
    f.calls = calls_.ptr;
    f.fresh = fresh_.ptr;
    f.max_new = max_new;
    f.boundaries = boundaries_.ptr;
    f.hist = hist_.ptr;
    f.running = running_.ptr;
    launch_ph_fold(f, n_streams_, stream);
}

void ProgramLoudnessBank::bounded_results(hipStream_t stream) {
    PhResultArgs r{};
    r.hist = hist_.ptr;
    r.running = running_.ptr;
    r.meta = meta_.ptr;
    r.tp_max = tp_max_.ptr;
    r.peaks = peaks_on_ ? peak_records_.ptr : nullptr;
    r.records = records_.ptr;
    r.n_streams = n_streams_;
    r.floor_db = cfg_.floor_db;
    launch_ph_results(r, stream);
}

int ProgramLoudnessBank::bounded_refusal(const char* what) const {
    set_last_error(std::string("program loudness ") + what + ": the bank has bounded storage and keeps no segments");
    return OMX_ERR_UNSUPPORTED;
}

int ProgramLoudnessBank::fetch_histogram(uint64_t stream_index, omx_program_histogram* dst) {
    if (!bounded_) return pl_refuse("fetch_histogram", "the bank stores segments, not histograms");
    if (stream_index >= n_streams_) return pl_refuse("fetch_histogram", "stream index out of range");
    copy_out(dst, hist_.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_histogram_boundaries(double dst[OMX_PROGRAM_HISTOGRAM_BINS + 1]) {
    if (!dst) return OMX_ERR_INVALID;
    ph_boundaries(dst);
    return OMX_NONE;
}
int omx_program_loudness_bank_create_bounded(const omx_loudness_config* cfg, uint32_t n_streams, uint32_t channels,
                                             omx_program_loudness_bank** out) {
    (void)channels;  // taken from each call, as in omx_program_loudness_bank_create
    if (!cfg || !out || n_streams == 0) return OMX_ERR_INVALID;
    const int rc = device_ready();
    if (rc != OMX_NONE) return rc;
    return guarded([&] {
        *out = new omx_program_loudness_bank(*cfg, n_streams, 0, true);
        return (int)OMX_NONE;
    });
}
int omx_program_loudness_bank_is_bounded(const omx_program_loudness_bank* b) { return b ? (b->impl.bounded() ? 1 : 0) : OMX_ERR_INVALID; }
int omx_program_loudness_bank_fetch_histogram(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_histogram* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_histogram(stream_index, dst); });
}

}  // extern "C"
