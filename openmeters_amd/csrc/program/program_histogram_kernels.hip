// Bounded storage of the programme loudness bank (include/omx/program_histogram.h): the fold of a call's new segments into the
// histograms and the result pass over them.
//
// Fold, one workgroup per stream.  For every tile of new segments the lanes form the gating and short-term blocks from an LDS copy of
// the energies (the 29 before the tile, then the tile), find each block's bin by binary search in the boundaries (10 comparisons on
// f64, no logarithm) and leave (bin, energy) in LDS.  Then every lane walks the tile's bins in ascending j (all lanes read the same
// LDS word: a broadcast) and adds the blocks of the four bins it owns, in registers: no atomics, and the additions into one bin
// happen in ascending j within a call and across calls whatever the tile or the call length.  A bin is loaded from HBM the first time
// its owner meets it and stored once at the end, so a call that brings one segment touches two bins per stream and a call that
// brings tens of thousands still reads and writes each bin once.
// Result pass, one workgroup per stream: the 2 x 1000 bins go to LDS in parallel, lane 0 (gating) and lane 64 (short-term) add them in
// ascending bin order as the definition says, the bin means and gate decisions are made in parallel in between.
// Built with -ffp-contract=off like the rest of the bank.
#include "program_histogram_device.hpp"

namespace omx {
namespace {

constexpr uint32_t PT = kPhThreads;
constexpr uint32_t kNoBin = 0xFFFFu;

// the largest i <= 999 with bnd[i] < z (z > bnd[0])
__device__ __forceinline__ uint32_t find_bin(const double* bnd, double z) {
    uint32_t lo = 0, hi = kPhBins - 1;
#pragma unroll
    for (int step = 0; step < 10; ++step) {  // 2^10 >= 1000
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (bnd[mid] < z) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ double ph_block_max(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = PT / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + d]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(PT) void ph_fold_kernel(PhFoldArgs a) {
    __shared__ double bnd[kPhBins + 1];
    __shared__ double ext[kPhTile + kPhTail];  // ext[i]: the energy of new segment k0 - 29 + i (before the call's first: the tail)
    __shared__ double val[2][kPhTile];         // gating / short-term block that completes with new segment k0 + k
    __shared__ __align__(16) uint32_t bins[kPhTile];  // its bins: gating | short-term << 16, kNoBin = not binned
    __shared__ double red[PT];
    __shared__ double latest[2];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const PlStreamCall call = a.calls[s];
    if (call.n_new == 0 && call.reset == 0) return;  // (uniform)
    omx_program_histogram& h = a.hist[s];
    const uint32_t n_new = call.n_new;
    const double* fresh = a.fresh + (uint64_t)s * a.max_new;

    if (call.reset) {  // the lane that clears a bin is the lane that owns it: its later loads see the zeros
        for (uint32_t i = tid; i < kPhBins; i += PT) {
            h.gating_count[i] = 0;
            h.gating_sum[i] = 0.0;
            h.short_term_count[i] = 0;
            h.short_term_sum[i] = 0.0;
        }
    }
    const uint64_t base = call.reset ? 0ull : h.segments;
    const uint32_t tail_count = call.reset ? 0u : h.tail_count;
    PhRunning run = a.running[s];
    if (call.reset) run = PhRunning{0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = tid; i <= kPhBins; i += PT) bnd[i] = a.boundaries[i];
    if (tid == 0) {
        latest[0] = run.momentary;
        latest[1] = run.short_term;
    }

    unsigned long long cnt[2][4];
    double sum[2][4];
    uint32_t loaded = 0;  // bit 4 * which + q: registers hold bin tid + 256 q of histogram `which`
    double g_max = run.max_momentary, s_max = run.max_short_term;
    for (uint32_t k0 = 0; k0 < n_new; k0 += kPhTile) {
        const uint32_t n_here = min(kPhTile, n_new - k0);
        for (uint32_t i = tid; i < n_here + kPhTail; i += PT) {
            const int64_t idx = (int64_t)k0 + (int64_t)i - (int64_t)kPhTail;
            double v = 0.0;
            if (idx >= 0) {
                v = fresh[idx];
            } else if ((int64_t)tail_count + idx >= 0) {
                v = h.tail[(int64_t)tail_count + idx];
            }
            ext[i] = v;
        }
        __syncthreads();
        const uint32_t n_walk = (n_here + 3u) & ~3u;  // the walk reads four bin words at a time
        for (uint32_t k = tid; k < n_walk; k += PT) {
            if (k >= n_here) {
                bins[k] = kNoBin | (kNoBin << 16);
                continue;
            }
            const uint64_t j = base + k0 + k;
            const double* e = ext + k;  // e[29] = e[j], e[0] = e[j - 29]
            uint32_t gb = kNoBin, sb = kNoBin;
            double g = 0.0, st = 0.0;
            if (j >= 3) {
                g = (((e[26] + e[27]) + e[28]) + e[29]) * 0.25;
                g_max = fmax(g_max, g);
                if (g > bnd[0]) gb = find_bin(bnd, g);
            }
            if (j >= 29) {
                double acc = e[0];
#pragma unroll
                for (uint32_t m = 1; m < 30; ++m) acc += e[m];
                st = acc / 30.0;
                s_max = fmax(s_max, st);
                if (st > bnd[0]) sb = find_bin(bnd, st);
            }
            val[0][k] = g;
            val[1][k] = st;
            bins[k] = gb | (sb << 16);
            if (k0 + k + 1 == n_new) {  // the call's last segment leaves the latest blocks
                if (j >= 3) latest[0] = g;
                if (j >= 29) latest[1] = st;
            }
        }
        __syncthreads();
        for (uint32_t k4 = 0; k4 < n_walk; k4 += 4) {
            const uint4 four = *reinterpret_cast<const uint4*>(&bins[k4]);  // one address for every lane: a broadcast, one wait per four
            const uint32_t word[4] = {four.x, four.y, four.z, four.w};
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {  // ascending j
#pragma unroll
                for (uint32_t which = 0; which < 2; ++which) {
                    const uint32_t b = which ? word[i] >> 16 : word[i] & 0xFFFFu;
                    if ((b & (PT - 1)) != tid || b == kNoBin) continue;
                    const double z = val[which][k4 + i];
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) {
                        if (b != tid + PT * q) continue;
                        const uint32_t bit = 1u << (4 * which + q);
                        if (!(loaded & bit)) {
                            cnt[which][q] = which ? h.short_term_count[b] : h.gating_count[b];
                            sum[which][q] = which ? h.short_term_sum[b] : h.gating_sum[b];
                            loaded |= bit;
                        }
                        cnt[which][q] += 1ull;
                        sum[which][q] += z;
                    }
                }
            }
        }
        __syncthreads();  // the next tile overwrites ext / val / bins
    }
#pragma unroll
    for (uint32_t which = 0; which < 2; ++which) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (!(loaded & (1u << (4 * which + q)))) continue;
            const uint32_t b = tid + PT * q;  // (< 1000: only bins that exist were ever matched)
            if (which) {
                h.short_term_count[b] = cnt[which][q];
                h.short_term_sum[b] = sum[which][q];
            } else {
                h.gating_count[b] = cnt[which][q];
                h.gating_sum[b] = sum[which][q];
            }
        }
    }
    g_max = ph_block_max(g_max, red);
    s_max = ph_block_max(s_max, red);

    // the new tail: the newest min(29, tail_count + n_new) of (old tail, then the call's segments); read, barrier, write
    const uint64_t total = (uint64_t)tail_count + n_new;
    const uint32_t new_count = (uint32_t)min(total, (uint64_t)kPhTail);
    double t_val = 0.0;
    if (tid < new_count) {
        const uint64_t pos = total - new_count + tid;
        t_val = pos < tail_count ? h.tail[pos] : fresh[pos - tail_count];
    }
    __syncthreads();
    if (tid < kPhTail) h.tail[tid] = tid < new_count ? t_val : 0.0;
    if (tid == 0) {
        h.segments = base + n_new;
        h.tail_count = new_count;
        h._pad = 0;
        a.running[s] = PhRunning{latest[0], latest[1], g_max, s_max};
    }
}

// ---- result pass (the bins to the record: program_histogram_device.hpp, shared with the bounded group kernel)
__global__ __launch_bounds__(PT) void ph_result_kernel(PhResultArgs a) {
    __shared__ PhResultLds lds;
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const omx_program_histogram& h = a.hist[s];
    for (uint32_t i = tid; i < kPhBins; i += PT) {
        lds.cnt[0][i] = h.gating_count[i];
        lds.sum[0][i] = h.gating_sum[i];
        lds.cnt[1][i] = h.short_term_count[i];
        lds.sum[1][i] = h.short_term_sum[i];
    }
    __syncthreads();
    ph_result_from_bins(lds, a.floor_db, a.records + s, [&] {
        const PlStreamMeta meta = a.meta[s];
        PhRecordTail t;
        t.run = a.running[s];
        t.frames = meta.frames;
        t.segments = meta.segments;
        t.gating_blocks = meta.segments >= 4 ? meta.segments - 3 : 0;
        t.short_term_blocks = meta.segments >= 30 ? meta.segments - 29 : 0;
        t.max_true_peak_db = a.peaks ? fmaxf(a.tp_max[s], a.peaks[s].max_true_peak_db) : a.tp_max[s];
        return t;
    });
}

}  // namespace

void launch_ph_fold(const PhFoldArgs& a, uint32_t n_streams, hipStream_t stream) {
    hipLaunchKernelGGL(ph_fold_kernel, dim3(n_streams), dim3(PT), 0, stream, a);
}
void launch_ph_results(const PhResultArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(ph_result_kernel, dim3(a.n_streams), dim3(PT), 0, stream, a);
}

}  // namespace omx
