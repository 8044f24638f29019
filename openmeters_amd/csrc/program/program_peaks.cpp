// Host side of the programme bank's peaks (include/omx/program_peaks.h): the switch, the two launches behind the segment pass of a
// process call, the hand-out of the records.  Nothing here synchronises except fetch_peaks and set_peaks.
#include "program_loudness.hpp"

namespace omx {

int ProgramLoudnessBank::set_peaks(bool on) {
    for (uint32_t s = 0; s < n_streams_; ++s)
        if (h_meta_[s].frames != 0) return pl_refuse("set_peaks", "a stream holds samples (reset every stream first)");
    if (on) {
        peak_records_.reserve(n_streams_);
        peak_delay_.reserve((size_t)n_streams_ * kPlSlots * kPkMaxDelay);
        launch_pk_clear(peak_records_.ptr, peak_delay_.ptr, n_streams_, cfg_.floor_db, last_stream_);
        OMX_HIP(hipGetLastError());
        OMX_HIP(hipStreamSynchronize(last_stream_));  // (the first process call may come on another stream)
    } else {
        peak_timeline_off();  // (the peak timeline lives on the peak pass: off with it)
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
    pl_true_peak_fir(p.fir4, p.fir2);
    if (peak_timeline_on_) {  // (in front of the tile pass: the keys of a reset stream are cleared before the call's frames merge in)
        p.tl_keys = peak_timeline_keys(p.n_tiles != 0, stream);
        p.tl_rows = capacity_ + 1;
        p.seg = seg_;
    }
    if (p.n_tiles != 0) {
        peak_partials_.reserve((size_t)n_streams_ * channels_ * p.n_tiles);
        p.partials = peak_partials_.ptr;
        launch_pk_tiles(p, stream);
    }
    launch_pk_fold(p, stream);
}

int ProgramLoudnessBank::peaks(hipStream_t stream, const omx_program_peak_record** d_records) {
    if (!peaks_on_) return pl_refuse("peaks", "peaks are off (omx_program_loudness_bank_set_peaks)");
    last_stream_ = stream;
    *d_records = peak_records_.ptr;
    return OMX_NONE;
}

int ProgramLoudnessBank::fetch_peaks(uint64_t stream_index, omx_program_peak_record* dst) {
    if (!peaks_on_) return pl_refuse("fetch_peaks", "peaks are off (omx_program_loudness_bank_set_peaks)");
    if (stream_index >= n_streams_) return pl_refuse("fetch_peaks", "stream index out of range");
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
