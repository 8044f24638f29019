// ProgramLoudnessBank: the EBU R 128 programme figures (gated integrated loudness, loudness range, maxima) for S streams.
// include/omx/program_loudness.h states the definitions; program_loudness_kernels.hip holds the kernels.
// Self-contained: shares no state and no kernel with LoudnessBank (its copy of the K-weighting step is a later consolidation).
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_loudness.h"
#include "program_stage.hpp"
#include "program_peaks.hpp"
#include "program_timeline.hpp"
#include "program_histogram.hpp"
#include "program_groups.hpp"
#include "program_normalize.hpp"
#include "program_limit.hpp"
#include "program_pcm.hpp"
#include "program_resample.hpp"
#include "program_remix.hpp"
#include "program_inspect.hpp"
#include "program_edit.hpp"
#include "program_peak_timeline.hpp"
#include "program_filter.hpp"
#include "program_mix.hpp"
#include "program_convolve.hpp"
#include "program_dynamics.hpp"
#include "program_spectrum.hpp"

namespace omx {

constexpr uint32_t kPlTile = 32;          // frames per LDS tile of the segment pass
constexpr uint32_t kPlChunkFrames = 1024;  // frames per work item of the time-parallel form (never more than one segment)
constexpr uint32_t kPlSlots = OMX_MAX_CHANNELS;  // state is laid out [stream][8 channel slots] whatever the channel count
// Lowest rate: the K-weighting shelf sits at 1681.97 Hz and its bilinear transform has poles outside the unit circle for every rate
// from there to twice that (3363.95 Hz; largest pole radius 1.98 at 2 kHz, 1.0006 at 3363 Hz, 0.99997 at 3364 Hz:
// tests/test_cpu_program_loudness_inputs.py); below 1682 Hz the shelf lies above the rate itself
constexpr float kPlMinRate = 3364.0f;
// Highest rate of the time-parallel form.  A work item starts from a state rounded to f64, and the zero-input response amplifies that
// rounding by up to |A^L| before the poles let it decay: 2.1e6 at 384 kHz, 1.1e7 at 768 kHz (L = 1024).  A CPU model of the form with an
// exact scan leaves 5e-6 dB on a 5 Hz sine at 0.5 under noise at -60 dBFS at 384 kHz and 8e-5 dB at 768 kHz, against a bar of 1e-4 dB:
// above 384 kHz the reference order runs whatever form is asked for.
constexpr float kPlTimeParallelMaxRate = 384000.0f;

// What one call does to one stream: made on the host (every count of a stream follows from the call arguments), uploaded per call.
struct PlStreamCall {
    uint32_t frames;    // frames taken in this call (after the capacity clamp)
    uint32_t phase;     // frames already in the open segment when the call starts
    uint32_t n_new;     // segments that complete in this call
    uint32_t reset;     // state cleared before the samples are taken
    uint64_t seg_base;  // segments stored before the call
};
struct PlStreamMeta {  // the host's counters of a stream, for the result pass
    uint64_t frames;
    uint32_t segments, overflow;
};

struct PlArgs {
    const float* pcm;  // [n_streams][frames_capacity][channels]
    uint64_t frames_capacity;
    uint32_t n_streams, channels, slot_shift;  // lane = (stream << slot_shift) + channel
    uint32_t seg;       // frames per segment
    uint32_t chunk;     // frames per work item: the whole call (reference order) or kPlChunkFrames (time-parallel, <= seg)
    uint32_t n_chunks;  // work items per stream
    uint32_t max_new;   // row length of chan_sums
    double b[5], a[5];
    double weights[OMX_MAX_CHANNELS];
    const PlStreamCall* calls;  // [n_streams]
    double* state;      // [n_streams][8][4] K-weighting TDF-II state
    double* starts;     // [n_streams][8][n_chunks][4] start state of every work item (reference order: `state` itself)
    double* part;       // [n_streams][8] weighted energy sum of the open segment
    double* chan_sums;  // [n_streams][8][max_new] weighted energy sums of the segments completed in this call
    double* partials;   // time-parallel: [n_streams][8][n_chunks][2] sums before / after the segment boundary inside a work item
    const double* zs_weights;   // [chunk][4]: weight of sample k of a work item on its zero-state end state
    const double* transition;   // [2][4][4]: zero-input transition over `chunk` frames, high parts then low parts
    double* segments;   // [n_streams][capacity] stored segment energies
    uint64_t capacity;
};
void launch_pl_reset(const PlArgs& a, float* tp_max, float floor_db, hipStream_t stream);
void launch_pl_reference_order(const PlArgs& a, hipStream_t stream);
void launch_pl_time_parallel(const PlArgs& a, hipStream_t stream);
void launch_pl_commit(const PlArgs& a, hipStream_t stream);

struct PlResultArgs {
    const double* segments;
    uint64_t capacity;
    const PlStreamMeta* meta;
    const float* tp_max;
    const omx_program_peak_record* peaks;  // null with peaks off; else max_true_peak_db = the larger of tp_max and the measured one
    omx_program_loudness_record* records;
    uint32_t n_streams;
    float floor_db;
    double absolute_gate;  // energy of -70 LUFS
};
void launch_pl_results(const PlResultArgs& a, hipStream_t stream);
void launch_pl_true_peak_fold(const omx_loudness_snapshot* snapshots, uint64_t n_blocks, const uint32_t* d_n_blocks, uint32_t n_streams,
                              float* tp_max, hipStream_t stream);

class ProgramLoudnessBank {
public:
    // bounded: histogram storage (include/omx/program_histogram.h); capacity_seconds is not used then
    ProgramLoudnessBank(const omx_loudness_config& cfg, uint32_t n_streams, uint32_t capacity_seconds, bool bounded = false);
    int reset(const uint8_t* reset_mask);
    int process(const float* d_pcm, uint64_t frames_capacity, const uint32_t* frames, const uint8_t* reset_mask, uint32_t channels,
                float sample_rate, const uint8_t positions[OMX_MAX_CHANNELS], hipStream_t stream);
    int note_snapshots(const omx_loudness_snapshot* d_snapshots, uint64_t n_blocks, const uint32_t* d_n_blocks, hipStream_t stream);
    int results(hipStream_t stream, const omx_program_loudness_record** d_records);
    int fetch(uint64_t stream_index, omx_program_loudness_record* dst);
    int fetch_segments(uint64_t stream_index, uint64_t first, uint64_t count, double* dst);
    // include/omx/program_peaks.h (program_peaks.cpp)
    int set_peaks(bool on);
    int peaks(hipStream_t stream, const omx_program_peak_record** d_records);
    int fetch_peaks(uint64_t stream_index, omx_program_peak_record* dst);
    // include/omx/program_timeline.h (program_timeline.cpp)
    int timeline(uint64_t first, uint64_t stride, uint64_t count, omx_program_timeline_row* d_rows, hipStream_t stream);
    int fetch_timeline(uint64_t stream_index, uint64_t first, uint64_t stride, uint64_t count, omx_program_timeline_row* dst);
    int measure_intervals(const omx_program_interval* intervals, uint64_t n, hipStream_t stream, const omx_program_loudness_record** d_records);
    int fetch_intervals(const omx_program_interval* intervals, uint64_t n, omx_program_loudness_record* dst);
    // include/omx/program_histogram.h (program_histogram.cpp)
    bool bounded() const { return bounded_; }
    int fetch_histogram(uint64_t stream_index, omx_program_histogram* dst);
    // include/omx/program_groups.h (program_groups.cpp)
    int measure_groups(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups, uint64_t n_groups,
                       hipStream_t stream, const omx_program_loudness_record** d_records);
    int fetch_groups(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups, uint64_t n_groups,
                     omx_program_loudness_record* dst);
    // include/omx/program_normalize.h (program_normalize.cpp)
    int plan_gains(const omx_program_gain_rule* rule, hipStream_t stream, const omx_program_gain_record** d_gains);
    int plan_group_gains(const omx_program_gain_rule* rule, const omx_program_interval* members, uint64_t n_members,
                         const omx_program_group* groups, uint64_t n_groups, hipStream_t stream, const omx_program_gain_record** d_gains);
    int fetch_gains(uint64_t first, uint64_t count, omx_program_gain_record* dst);
    int apply_gains(const float* d_in, float* d_out, uint64_t frames_capacity, const uint32_t* frames, uint32_t channels,
                    const omx_program_gain_record* d_gains, uint64_t n_gains, const uint32_t* gain_of_stream, hipStream_t stream,
                    const omx_program_apply_record** d_applied);
    int fetch_applied(uint64_t stream_index, omx_program_apply_record* dst);
    // include/omx/program_limit.h (program_limit.cpp)
    int limiter_configure(const omx_program_limit_rule* rule, uint32_t channels, float sample_rate);
    int limiter_reset(const uint8_t* reset_mask);
    int apply_limited(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, uint64_t out_capacity,
                      const uint8_t* flush_mask, const omx_program_gain_record* d_gains, uint64_t n_gains, const uint32_t* gain_of_stream,
                      hipStream_t stream, const omx_program_limit_record** d_limited);
    int fetch_limited(uint64_t stream_index, omx_program_limit_record* dst);
    // include/omx/program_pcm.h (program_pcm.cpp)
    int import_pcm(const void* d_in, uint32_t format, float* d_out, uint64_t frames_capacity, const uint32_t* frames, uint32_t channels,
                   hipStream_t stream);
    int export_configure(const omx_program_export_rule* rule, uint32_t channels);
    int export_reset(const uint8_t* reset_mask);
    int export_pcm(const float* d_in, void* d_out, uint64_t frames_capacity, const uint32_t* frames, hipStream_t stream,
                   const omx_program_export_record** d_exported);
    int fetch_exported(uint64_t stream_index, omx_program_export_record* dst);
    // include/omx/program_resample.h (program_resample.cpp)
    int resampler_configure(const omx_program_resample_rule* rule, uint32_t channels);
    int resampler_reset(const uint8_t* reset_mask);
    int resample(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, uint64_t out_capacity,
                 const uint8_t* flush_mask, hipStream_t stream, const omx_program_resample_record** d_resampled);
    int fetch_resampled(uint64_t stream_index, omx_program_resample_record* dst);
    // include/omx/program_remix.h (program_remix.cpp)
    int remix_configure(uint32_t channels_in, uint32_t channels_out, const float* matrices, uint32_t n_matrices);
    int remix(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, const uint32_t* matrix_of_stream,
              hipStream_t stream, const omx_program_remix_record** d_remixed);
    int fetch_remixed(uint64_t stream_index, omx_program_remix_record* dst);
    // include/omx/program_inspect.h (program_inspect.cpp)
    int inspect_configure(const omx_program_inspect_rule* rule, uint32_t channels, const uint32_t* pairs, uint32_t n_pairs);
    int inspect_reset(const uint8_t* reset_mask);
    int inspect(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, hipStream_t stream,
                const omx_program_inspect_record** d_inspected);
    int fetch_inspected(uint64_t stream_index, omx_program_inspect_record* dst);
    // include/omx/program_edit.h (program_edit.cpp)
    int edit_configure(uint32_t channels, uint32_t max_outputs);
    int edit(const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in, const omx_program_edit_clip* clips, uint64_t n_clips,
             float* d_out, uint64_t out_capacity, uint32_t n_out, const uint64_t* out_first, const uint32_t* out_frames, hipStream_t stream,
             const omx_program_edit_record** d_edited);
    int fetch_edited(uint64_t output_index, omx_program_edit_record* dst);
    // include/omx/program_peak_timeline.h (program_peak_timeline.cpp)
    int set_peak_timeline(bool on);
    int peak_rows(uint64_t first, uint64_t stride, uint64_t count, omx_program_peak_row* d_rows, hipStream_t stream);
    int fetch_peak_rows(uint64_t stream_index, uint64_t first, uint64_t stride, uint64_t count, omx_program_peak_row* dst);
    int measure_interval_peaks(const omx_program_interval* intervals, uint64_t n, hipStream_t stream, const omx_program_part_peak** d_peaks);
    int fetch_interval_peaks(const omx_program_interval* intervals, uint64_t n, omx_program_part_peak* dst);
    int measure_group_peaks(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups, uint64_t n_groups,
                            hipStream_t stream, const omx_program_part_peak** d_peaks);
    int fetch_group_peaks(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups, uint64_t n_groups,
                          omx_program_part_peak* dst);
    int plan_part_gains(const omx_program_gain_rule* rule, const omx_program_interval* members, uint64_t n_members,
                        const omx_program_group* groups, uint64_t n_groups, hipStream_t stream, const omx_program_gain_record** d_gains);
    // include/omx/program_filter.h (program_filter.cpp)
    int filter_configure(uint32_t channels, double sample_rate, const omx_program_filter* filters, uint32_t n_filters,
                         const uint32_t* filter_of_channel);
    int filter_reset(const uint8_t* reset_mask);
    int filter(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, hipStream_t stream,
               const omx_program_filter_record** d_filtered);
    int fetch_filtered(uint64_t stream_index, omx_program_filter_record* dst);
    int filter_set_form(uint32_t form);
    int filter_last_form() const { return filter_last_form_; }
    // include/omx/program_mix.h (program_mix.cpp)
    int mix_configure(uint32_t channels, uint32_t max_buses);
    int mix(const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in, const omx_program_mix_send* sends, uint64_t n_sends,
            float* d_out, uint64_t out_capacity, uint32_t n_out, const uint64_t* out_first, const uint32_t* out_frames, hipStream_t stream,
            const omx_program_mix_record** d_mixed);
    int fetch_mixed(uint64_t bus, omx_program_mix_record* dst);
    // include/omx/program_convolve.h (program_convolve.cpp)
    int convolve_configure(uint32_t channels, const omx_program_fir* firs, uint32_t n_firs, const uint32_t* fir_of_channel,
                           uint32_t delay_frames);
    int convolve_reset(const uint8_t* reset_mask);
    int convolve(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, float* d_out, uint64_t out_capacity,
                 const uint8_t* flush_mask, hipStream_t stream, const omx_program_convolve_record** d_convolved);
    int fetch_convolved(uint64_t stream_index, omx_program_convolve_record* dst);
    // include/omx/program_dynamics.h (program_dynamics.cpp)
    int dynamics_configure(uint32_t channels, const omx_program_dynamics_curve* curves, uint32_t n_curves, const uint32_t* curve_of_stream);
    int dynamics_reset(const uint8_t* reset_mask);
    int dynamics(const float* d_in, const float* d_key, uint64_t frames_capacity, const uint32_t* frames, float* d_out, float* d_gain_db,
                 uint64_t out_capacity, const uint8_t* flush_mask, hipStream_t stream, const omx_program_dynamics_record** d_records);
    int fetch_dynamics(uint64_t stream_index, omx_program_dynamics_record* dst);
    // include/omx/program_spectrum.h (program_spectrum.cpp)
    int spectrum_configure(const omx_program_spectrum_rule* rule, uint32_t channels);
    int spectrum_reset(const uint8_t* reset_mask);
    int spectrum(const float* d_in, uint64_t frames_capacity, const uint32_t* frames, const uint8_t* finish_mask, hipStream_t stream,
                 const omx_program_spectrum_record** d_records, const double** d_sums);
    int fetch_spectrum(uint64_t stream_index, omx_program_spectrum_record* record, double* sums);
    void form(int f) { form_ = f; }
    int last_form() const { return last_form_; }

private:
    void set_rate(float rate);
    void host_tables(hipStream_t stream);
    PlResultArgs result_args() const;
    int timeline_rows(uint32_t stream_base, uint32_t n_streams, uint64_t first, uint64_t stride, uint64_t count, omx_program_timeline_row* d_rows,
                      hipStream_t stream);
    void measure_peaks(const float* d_pcm, uint64_t frames_capacity, uint32_t max_frames, hipStream_t stream);
    void bounded_init();
    void bounded_fold(uint32_t max_new, hipStream_t stream);
    void bounded_results(hipStream_t stream);
    int bounded_refusal(const char* what) const;  // OMX_ERR_UNSUPPORTED for what needs the stored segments

    omx_loudness_config cfg_{};
    uint32_t n_streams_;
    uint64_t capacity_;     // segments per stream
    float rate_ = 0.0f;     // sanitised rate of the running programmes (0: none yet)
    uint32_t channels_ = 0;
    uint32_t seg_ = 0;
    double b_[5], a_[5];
    std::vector<PlStreamMeta> h_meta_;
    std::vector<PlStreamCall> h_calls_;
    DeviceBuffer<double> state_, part_, segments_, chan_sums_, partials_, starts_, zs_weights_, transition_;
    DeviceBuffer<float> tp_max_;
    DeviceBuffer<PlStreamCall> calls_;
    DeviceBuffer<PlStreamMeta> meta_;
    DeviceBuffer<omx_program_loudness_record> records_;
    BlobStaging call_staging_, meta_staging_;
    float tables_rate_ = 0.0f;
    uint32_t tables_chunk_ = 0;
    bool dirty_ = true;
    int form_ = 0, last_form_ = 0;
    hipStream_t last_stream_ = nullptr;
    // peaks: nothing is allocated or launched while they are off
    bool peaks_on_ = false;
    DeviceBuffer<omx_program_peak_record> peak_records_;
    DeviceBuffer<float> peak_delay_;
    DeviceBuffer<PkPartial> peak_partials_;
    // peak timeline: nothing is allocated or launched while it is off
    void peak_timeline_off();
    unsigned long long* peak_timeline_keys(bool frames_taken, hipStream_t stream);
    int peak_rows_refusal(uint32_t n_streams, uint64_t first, uint64_t stride, uint64_t count, const void* rows) const;
    void peak_rows_of(uint32_t stream_base, uint32_t n_streams, uint64_t first, uint64_t stride, uint64_t count, omx_program_peak_row* d_rows,
                      hipStream_t stream);
    int part_peaks(const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups, uint64_t n_groups,
                   hipStream_t stream, const omx_program_part_peak** d_peaks, bool for_gains);
    bool peak_timeline_on_ = false;
    DeviceBuffer<unsigned long long> pt_keys_;  // [n_streams][capacity_ + 1][channels_][2], reserved by the first call that brings frames
    std::vector<PtClearItem> h_pt_clear_;       // the current call: the stored keys of the streams it resets, in runs of at most
    DeviceBuffer<PtClearItem> pt_clear_;        // kPtClearChunk, in the layout of before the call (its rate and channel count)
    BlobStaging pt_clear_staging_;
    DeviceBuffer<omx_program_peak_row> pt_rows_;  // fetch_peak_rows' device rows
    DeviceBuffer<uint8_t> pt_tables_;             // [PtMember x n_members][PtPart x n_parts] of the current call
    DeviceBuffer<omx_program_part_peak> pt_records_;
    std::vector<uint8_t> h_pt_tables_;
    std::vector<uint64_t> h_pt_before_;           // part_peaks' running sums over the member table
    BlobStaging pt_staging_;
    // timeline and intervals: nothing is allocated or launched until one of their functions is called
    DeviceBuffer<double> tl_gated_, tl_threshold_;
    DeviceBuffer<uint32_t> tl_above_;
    DeviceBuffer<omx_program_timeline_row> tl_rows_;  // fetch_timeline's device rows
    DeviceBuffer<PlIntervalDesc> interval_descs_;
    DeviceBuffer<omx_program_loudness_record> interval_records_;
    std::vector<PlIntervalDesc> h_interval_descs_;
    BlobStaging interval_staging_;
    // bounded storage: nothing is allocated or launched unless the bank was created bounded
    bool bounded_ = false;
    DeviceBuffer<omx_program_histogram> hist_;
    DeviceBuffer<PhRunning> running_;
    DeviceBuffer<double> fresh_, boundaries_;  // fresh_: [n_streams][max_new] segments of the current call, grown on demand
    // groups: nothing is allocated or launched until measure_groups / fetch_groups is called; grow-only, kept until the bank goes
    DeviceBuffer<uint8_t> group_tables_;  // [PgMember x n_members][PgGroup x n_groups] of the current call
    DeviceBuffer<omx_program_loudness_record> group_records_;
    DeviceBuffer<double> group_stage_;    // staged short-term blocks of the call's long groups (program_groups.hpp)
    std::vector<uint8_t> h_group_tables_;
    BlobStaging group_staging_;
    // normalisation: nothing is allocated or launched until a plan_* / apply_gains call; grow-only, kept until the bank goes
    DeviceBuffer<omx_program_gain_record> gain_records_;  // the last plan's records
    uint64_t gains_planned_ = 0;                          // how many of them (0: no plan yet)
    DeviceBuffer<PnStreamCall> apply_calls_;
    DeviceBuffer<omx_program_apply_record> apply_records_;
    std::vector<PnStreamCall> h_apply_calls_;
    BlobStaging apply_staging_;
    bool applied_ = false;
    // limiter: nothing is allocated or launched until limiter_configure
    LmArgs limiter_args() const;
    std::unique_ptr<ProgramLimiter> limiter_;
    // PCM formats: nothing is allocated or launched until import_pcm / export_configure
    DeviceBuffer<PcStreamCall> import_calls_;
    std::vector<PcStreamCall> h_import_calls_;
    BlobStaging import_staging_;
    std::unique_ptr<ProgramExporter> exporter_;
    // sample-rate conversion: nothing is allocated or launched until resampler_configure
    RsArgs resampler_args() const;
    std::unique_ptr<ProgramResampler> resampler_;
    // channel remix: nothing is allocated or launched until remix_configure
    RmArgs remix_args() const;
    std::unique_ptr<ProgramRemix> remix_;
    // signal QC: nothing is allocated or launched until inspect_configure
    InArgs inspect_args() const;
    std::unique_ptr<ProgramInspector> inspector_;
    // edit: nothing is allocated or launched until edit_configure
    std::unique_ptr<ProgramEdit> edit_;
    // filter: nothing is allocated or launched until filter_configure
    FlArgs filter_args() const;
    std::unique_ptr<ProgramFilter> filter_;
    int filter_form_ = 0, filter_last_form_ = 0;
    // mix: nothing is allocated or launched until mix_configure
    std::unique_ptr<ProgramMix> mix_;
    // convolve: nothing is allocated or launched until convolve_configure
    CvArgs convolve_args() const;
    std::unique_ptr<ProgramConvolve> convolve_;
    // dynamics: nothing is allocated or launched until dynamics_configure
    DyArgs dynamics_args() const;
    std::unique_ptr<ProgramDynamics> dynamics_;
    // spectrum: nothing is allocated or launched until spectrum_configure
    SpArgs spectrum_args() const;
    std::unique_ptr<ProgramSpectrum> spectrum_;
};

}  // namespace omx

struct omx_program_loudness_bank {
    omx::ProgramLoudnessBank impl;
    omx_program_loudness_bank(const omx_loudness_config& c, uint32_t n, uint32_t cap, bool bounded = false) : impl(c, n, cap, bounded) {}
};
