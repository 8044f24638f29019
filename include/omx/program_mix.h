/* Programme loudness bank, mix: stem mix buses, many streams into one.  The edit pass puts at most two clips over an output frame and
 * adds them in f32; a third is refused, so an eight-stem mix is seven chained edit calls through scratch buffers, each rounding to
 * f32, and the result depends on the order of the chain.  This header adds the bus pass: a table of SENDS says which source frames of
 * which input stream land where on which bus, each with a gain; up to 64 sends may cover a bus frame, and the bytes of their sum are
 * defined exactly.  Dialogue, music and effects become the full mix, the stems without dialogue the M&E, a bed goes under a voice at
 * -18 dB, and the null test of a stem delivery (the stems minus the printmaster leave nothing) is one call.
 *
 * Additive: this header adds three structures, six functions and a few constants; nothing declared in the headers it includes changes
 * and OMX_ABI_VERSION stays as it is.  A bank that never calls mix_configure allocates and launches nothing more.  All work goes on the
 * caller's stream; only fetch_mixed synchronises (and mix_configure, see there).  No call of this header touches measurement state,
 * gain plans or the records of any earlier header: each has the same bytes before and after.
 *
 * DEFINITION ("Mix: stem mix buses"; tests/program_mix_ref.py restates it).
 *   Send    puts source frames [src_first, src_first + frames) of input stream src_stream at frames [dst_first, dst_first + frames) of
 *           bus dst_bus, times gain.  A negative gain inverts polarity.  The table is sorted by (dst_bus, dst_first); among equal keys
 *           the table's order stands.  At most OMX_MIX_MAX_LAYERS (64) sends cover any bus frame; a call holds at most 2^20 sends;
 *           dst_first + frames <= 2^40.  Two sends may read the same source frames.  A send of 0 frames does nothing.  The channel
 *           count is the same in and out: remix does the routing.
 *   Sample  let k_0 < k_1 < ... be the table indices of the sends that cover a bus frame, x_i the source sample of send k_i:
 *             acc = (double)gain[k_0] * (double)x_0
 *             acc = acc + (double)gain[k_i] * (double)x_i      for i = 1, 2, ..., in table order
 *             y   = (float)acc      (round to nearest even; f32 denormals are produced, nothing is flushed)
 *           A frame under no send is +0.0f.
 *           Every product is EXACT in f64: 24 x 24 significant bits fit in 53, and the smallest product (2^-298) and the largest
 *           (below 2^256) lie inside the f64 exponent range.  Because the products are exact, it does not matter whether a product
 *           and its sum are fused: fma(g, x, acc) and acc + g * x are the same f64 value, and the kernel may use either.  Each sum
 *           is rounded to f64 once, and the order is the table's: a tree over the layers is a different function.
 *           Two consequences:
 *             - a frame under ONE send of gain 1.0f keeps its bits (-0.0f, denormals and infinities included; NOT NaN payloads: the
 *               bits of a NaN that comes out are not defined);
 *             - a table without overlaps gives, byte for byte, what edit gives for the same clips without fades (one rounding of an
 *               exact product to f32 is the f32 product).
 *   The output frame depends only on its absolute position and the table: it has the same bits through whichever window
 *   (out_first, out_frames) it is rendered.
 *
 * REFUSALS.  A refused call returns OMX_ERR_INVALID and sets omx_last_error() to "program loudness <who>: <why>", where <who> names
 * the function: "mix" (omx_program_loudness_bank_mix), "mix_configure", "fetch_mixed", "mix plan", "mix extent", "mix null".
 *
 * RECORD.  Written fresh by every call, per bus.  It holds integer counts and a maximum only, so it does not depend on the schedule.
 * Over windows that tile a bus the counts silent_frames, mixed_frames, samples_over, samples_nonfinite and frames add up; the peak and
 * max_layers are maxima. */
#ifndef OMX_PROGRAM_MIX_H
#define OMX_PROGRAM_MIX_H

#include "program_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_MIX_MAX_LAYERS 64u                   /* sends over one bus frame */
#define OMX_MIX_MAX_SENDS 1048576u               /* 2^20 sends of one call */
#define OMX_MIX_MAX_BUSES 16777216u              /* 2^24 buses */
#define OMX_MIX_MAX_POSITION 1099511627776ull    /* 2^40: no bus frame lies at or beyond it */

typedef struct omx_program_mix_send {
    uint32_t src_stream;            /* input stream, below the bank's n_streams */
    uint32_t dst_bus;               /* bus, below the call's n_out */
    uint64_t src_first;             /* first source frame */
    uint64_t dst_first;             /* first bus frame */
    uint64_t frames;
    float gain;                     /* finite; negative inverts polarity */
    uint32_t flags;                 /* must be 0 */
} omx_program_mix_send;             /* 40 bytes */

typedef struct omx_program_mix_info {
    uint32_t tile_frames;           /* bus frames one workgroup of the main kernel takes at this channel count */
    uint32_t layers_per_batch;      /* sources whose loads the kernel keeps in flight together */
    uint32_t channels;
    uint32_t _pad;
} omx_program_mix_info;             /* 16 bytes */

typedef struct omx_program_mix_record {
    uint64_t out_first;             /* the window this call rendered */
    uint64_t frames;
    uint64_t silent_frames;         /* frames of the window under no send */
    uint64_t mixed_frames;          /* frames under two or more sends */
    uint64_t samples_over;          /* output samples with |out| > 1.0f (NaN is not counted, infinity is) */
    uint64_t samples_nonfinite;     /* output samples that are NaN or infinite */
    float out_sample_peak;          /* max |out|, fmaxf semantics (NaN ignored) */
    float out_sample_peak_db;       /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t sends;                 /* sends of the table that touch the window */
    uint32_t max_layers;            /* the deepest cover inside the window */
} omx_program_mix_record;           /* 64 bytes */

/* Host only, needs no device: the main kernel's tile and batch at a channel count.  OMX_ERR_INVALID, with nothing written: channels
 * outside 1 .. 8, a null info. */
int omx_program_mix_plan(uint32_t channels, omx_program_mix_info* info);
/* Host only, needs no device: validates a table and writes, per bus, one past its last covered frame (0 for a bus without a send
 * that has frames).  frames_in[i]: the frames input stream i holds.
 * OMX_ERR_INVALID, with nothing written: a null sends with n_sends > 0, a null frames_in with n_in > 0, a null out_frames with
 * n_out > 0; more than 2^20 sends; a src_stream at or above n_in, a dst_bus at or above n_out; a table that is not sorted by
 * (dst_bus, dst_first); a 65th send over a frame; src_first + frames beyond frames_in[src_stream]; dst_first + frames beyond 2^40; a
 * flag set; a gain that is not finite. */
int omx_program_mix_extent(const omx_program_mix_send* sends, uint64_t n_sends, uint32_t n_in, const uint32_t* frames_in, uint32_t n_out,
                           uint64_t* out_frames);
/* Host only, needs no device: the table of a null test, n_stems + 1 sends into sends_out: every stem (stems[i], frames [0, frames))
 * at gain +1.0f onto frames [0, frames) of `bus`, in the order given, then reference_stream at -1.0f.  What the bus holds is what the
 * stems do not explain of the reference.
 * OMX_ERR_INVALID, with nothing written: a null stems or sends_out, n_stems 0 or above 63, frames beyond 2^40. */
int omx_program_mix_null(const uint32_t* stems, uint32_t n_stems, uint32_t reference_stream, uint64_t frames, uint32_t bus,
                         omx_program_mix_send* sends_out);

/* Sets the channel count of the PCM and the largest n_out of a call and allocates the records ([max_buses], each the record of a call
 * that brought nothing).  Allowed at any time: the pass keeps no per-stream state.  Mix calls still enqueued on any stream are waited
 * for (the device is synchronised) before an earlier allocation is released; *d_mixed of an earlier call is invalid afterwards.
 * OMX_ERR_INVALID, with nothing changed: channels outside 1 .. 8, max_buses 0 or above 2^24. */
int omx_program_loudness_bank_mix_configure(omx_program_loudness_bank* b, uint32_t channels, uint32_t max_buses);

/* d_in: device f32 [n_streams][frames_capacity][channels]; frames_in: host array [n_streams] of the frames each input stream holds, or
 * NULL = frames_capacity for every stream.  sends: host array [n_sends], the table (DEFINITION).  d_out: device f32
 * [n_out][out_capacity][channels].  The call renders bus frames [out_first[o], out_first[o] + out_frames[o]) of bus o into
 * d_out[o][0 ..]; out_first: host array [n_out] or NULL = 0 for every bus; out_frames: host array [n_out], out_frames[o] <=
 * out_capacity.  No float of d_out[o] at or beyond out_frames[o] * channels is written; frames of the window under no send are written
 * as +0.0f.  Out of place only: any overlap of d_in and d_out is OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID: a call before configure; n_out 0 or above max_buses; whatever omx_program_mix_extent refuses (with the bank's
 * n_streams as n_in); frames_in[s] > frames_capacity; a capacity beyond 2^32 - 1; out_frames[o] > out_capacity;
 * out_first[o] + out_frames[o] beyond 2^40; a null out_frames or d_mixed; a null d_out when any window holds a frame; a null d_in when
 * the table holds a send with frames.
 * A refused call changes nothing: neither d_out nor the records.
 * *d_mixed: device array [max_buses] of the records, entries below n_out written fresh by this call, valid until mix_configure or
 * destroy; work on `stream` that reads it has to be ordered behind the call.  Returns OMX_PRODUCED when any bus frame was written,
 * else OMX_NONE. */
int omx_program_loudness_bank_mix(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in,
                                  const omx_program_mix_send* sends, uint64_t n_sends, float* d_out, uint64_t out_capacity, uint32_t n_out,
                                  const uint64_t* out_first, const uint32_t* out_frames, void* stream, const omx_program_mix_record** d_mixed);
/* Copy of one bus's record; synchronises.  OMX_ERR_INVALID: before configure, an index at or above max_buses, a null dst. */
int omx_program_loudness_bank_fetch_mixed(omx_program_loudness_bank* b, uint64_t bus, omx_program_mix_record* dst);

#ifdef __cplusplus
}
#endif
#endif
