// Host side of the programme bank's peaks (include/omx/program_peaks.h): the switch, the two launches behind the segment pass of a
// process call, the hand-out of the records.  Nothing here synchronises except fetch_peaks and set_peaks.
#include "program_loudness.hpp"

namespace omx {

namespace {

constexpr size_t kTruePeakTaps = 48;  // loudness/processor.rs:75

float true_peak_coefficient(size_t j, size_t factor) {  // :79-84
    const double offset = (double)j - (double)kTruePeakTaps * 0.5;
    const double window = 0.5 * (1.0 - std::cos(2.0 * M_PI * (double)j / (double)kTruePeakTaps));
    const double x = offset * M_PI / (double)factor;
    return (float)(window * std::sin(x) / x);
}

}  // namespace

int ProgramLoudnessBank::set_peaks(bool on) {
    for (uint32_t s = 0; s < n_streams_; ++s)
        if (h_meta_[s].frames != 0) {
            set_last_error("program loudness set_peaks: a stream holds samples (reset every stream first)");
            return OMX_ERR_INVALID;
        }
    if (on) {
        peak_records_.reserve(n_streams_);
        peak_delay_.reserve((size_t)n_streams_ * kPlSlots * kPkMaxDelay);
        launch_pk_clear(peak_records_.ptr, peak_delay_.ptr, n_streams_, cfg_.floor_db, last_stream_);
        OMX_HIP(hipGetLastError());
        OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first process call may come on another stream)
    } else {
        OMX_HIP(hipStreamSynchronize(last_stream_));  // (a result pass that reads the records may still be in flight)
        peak_records_.release();
        peak_delay_.release();
        peak_partials_.release();
    }
    peaks_on_ = on;
    dirty_ = true;
    return OMX_NONE;
}

// Behind the segment pass of a call, on the same stream: h_calls_ is on the device already.  max_frames = 0: a call that only resets.
void ProgramLoudnessBank::measure_peaks(const float* d_pcm, uint64_t frames_capacity, uint32_t max_frames, hipStream_t stream) {
    PkArgs p{};
    p.pcm = d_pcm;
    p.frames_capacity = frames_capacity;
    p.n_streams = n_streams_;
    p.channels = channels_;
    p.n_tiles = (max_frames + kPkTile - 1) / kPkTile;
    const double fs = (double)rate_;
    p.delay_len = fs < 96000.0 ? 12u : (fs < 192000.0 ? 24u : 0u);  // TruePeakMeter::new (:107-114)
    p.floor_db = cfg_.floor_db;
    p.calls = calls_.ptr;
    p.delay = peak_delay_.ptr;
    p.records = peak_records_.ptr;
    for (size_t tap = 0; tap < 12; ++tap)
        for (size_t phase = 0; phase < 3; ++phase) p.fir4[tap][phase] = true_peak_coefficient(tap * 4 + phase + 1, 4);
    for (size_t tap = 0; tap < 24; ++tap) p.fir2[tap] = true_peak_coefficient(tap * 2 + 1, 2);
    if (p.n_tiles != 0) {
        peak_partials_.reserve((size_t)n_streams_ * channels_ * p.n_tiles);
        p.partials = peak_partials_.ptr;
        launch_pk_tiles(p, stream);
    }
    launch_pk_fold(p, stream);
}

int ProgramLoudnessBank::peaks(hipStream_t stream, const omx_program_peak_record** d_records) {
    if (!peaks_on_) {
        set_last_error("program loudness peaks: peaks are off (omx_program_loudness_bank_set_peaks)");
        return OMX_ERR_INVALID;
    }
    last_stream_ = stream;
    *d_records = peak_records_.ptr;
    return OMX_NONE;
}

int ProgramLoudnessBank::fetch_peaks(uint64_t stream_index, omx_program_peak_record* dst) {
    if (!peaks_on_) {
        set_last_error("program loudness fetch_peaks: peaks are off (omx_program_loudness_bank_set_peaks)");
        return OMX_ERR_INVALID;
    }
    if (stream_index >= n_streams_) {
        set_last_error("program loudness fetch_peaks: stream index out of range");
        return OMX_ERR_INVALID;
    }
    copy_out(dst, peak_records_.ptr + stream_index, sizeof(*dst), false, last_stream_);
    return OMX_NONE;
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_program_loudness_bank_set_peaks(omx_program_loudness_bank* b, uint32_t on) {
    if (!b) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.set_peaks(on != 0); });
}
int omx_program_loudness_bank_peaks(omx_program_loudness_bank* b, void* stream, const omx_program_peak_record** d_records) {
    if (!b || !d_records) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.peaks(static_cast<hipStream_t>(stream), d_records); });
}
int omx_program_loudness_bank_fetch_peaks(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_peak_record* dst) {
    if (!b || !dst) return OMX_ERR_INVALID;
    return guarded([&] { return b->impl.fetch_peaks(stream_index, dst); });
}

}  // extern "C"
