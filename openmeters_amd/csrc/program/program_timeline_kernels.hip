// Timeline of the programme loudness bank (include/omx/program_timeline.h): momentary, short-term and running integrated loudness on
// the 100 ms grid, from the stored segment energies.
//
// The running integrated loudness of row j is a dominance sum: the mean of the gating blocks g[k], k <= j, above the absolute gate
// and above a relative gate that itself depends on j.  Two kernels:
//   scan : one workgroup per stream.  g[k] once per k (gated: 0 where it does not exceed the absolute gate, so that the all-pairs pass
//          needs one comparison per visit), and the prefix sum / count of the gated blocks, hence the relative gate of every k.  The
//          prefix sum is blocked on a tile grid anchored at k = 0 (a lane adds 8 consecutive blocks, a Hillis-Steele scan over the 256
//          lane totals, a carry from tile to tile): the order of the additions behind entry k depends on k alone.
//   rows : one lane per output row, 256 rows per workgroup, the longest rows in the first workgroups.  The workgroup streams the gated
//          blocks through an LDS tile; every lane reads the same entry (a broadcast: no bank conflict) and adds it, in ascending k, when
//          it exceeds the lane's gate.  Tiles that lie wholly below the wavefront's smallest j need no k <= j test; tiles beyond the
//          workgroup's largest j are not visited.  Then the lane forms its momentary and short-term block from e[] and stores its row.
// Both orders depend on nothing but k and j: row j has the same bits through any (first, stride, count) and after later appends.
// f64 sums, no fused multiply-add (-ffp-contract=off), no atomics.
#include "program_result_device.hpp"  // ms_to_lufs and the block expressions of the result pass

namespace omx {
namespace {

constexpr uint32_t T = kTlThreads, E = kTlScanItems;

// blocks [0, limit) of a stream are needed: limit = min(segments, 1 + the last j asked for)
__device__ __forceinline__ uint32_t stream_limit(const TlArgs& a, uint32_t s) {
    const uint64_t n = min((uint64_t)a.meta[s].segments, a.capacity);
    const uint64_t last = a.first + (uint64_t)(a.count - 1) * a.stride;
    return (uint32_t)min(min(n, last + 1), (uint64_t)a.pitch);
}

__global__ __launch_bounds__(T) void tl_scan_kernel(TlArgs a) {
    __shared__ double tot[2][T];
    __shared__ uint32_t totc[2][T];
    const uint32_t local = blockIdx.x, s = a.stream_base + local, tid = threadIdx.x;
    const uint32_t limit = stream_limit(a, s);
    const double* e = a.segments + (uint64_t)s * a.capacity;
    double* gated = a.gated + (uint64_t)local * a.pitch;
    double* threshold = a.threshold + (uint64_t)local * a.pitch;
    uint32_t* above = a.above + (uint64_t)local * a.pitch;
    const double gate = a.absolute_gate;
    double carry = 0.0;
    uint32_t carry_n = 0;
    for (uint32_t k0 = 0; k0 < limit; k0 += T * E) {
        const uint32_t base = k0 + tid * E;
        double v[E], ps[E];
        uint32_t pc[E];
        double sum = 0.0;
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t q = 0; q < E; ++q) {
            const uint32_t k = base + q;
            const double g = (k >= 3 && k < limit) ? gating_block(e, k) : 0.0;
            v[q] = g > gate ? g : 0.0;
            sum += v[q];  // (adding 0.0 leaves the bits)
            cnt += g > gate ? 1u : 0u;
            ps[q] = sum;
            pc[q] = cnt;
        }
        // inclusive scan of the lane totals, the same tree for every tile
        uint32_t cur = 0;
        tot[0][tid] = sum;
        totc[0][tid] = cnt;
        __syncthreads();
        for (uint32_t d = 1; d < T; d <<= 1) {
            double x = tot[cur][tid];
            uint32_t c = totc[cur][tid];
            if (tid >= d) {
                x = tot[cur][tid - d] + x;
                c += totc[cur][tid - d];
            }
            tot[cur ^ 1][tid] = x;
            totc[cur ^ 1][tid] = c;
            cur ^= 1;
            __syncthreads();
        }
        const double before = tid ? carry + tot[cur][tid - 1] : carry;
        const uint32_t before_n = tid ? carry_n + totc[cur][tid - 1] : carry_n;
        carry += tot[cur][T - 1];
        carry_n += totc[cur][T - 1];
        __syncthreads();  // (the next tile writes tot[0])
#pragma unroll
        for (uint32_t q = 0; q < E; ++q) {
            const uint32_t k = base + q;
            if (k < limit) {
                const double p = before + ps[q];
                const uint32_t c = before_n + pc[q];
                gated[k] = v[q];
                threshold[k] = c ? 0.1 * (p / (double)c) : 0.0;
                above[k] = c;
            }
        }
    }
}

__global__ __launch_bounds__(T) void tl_rows_kernel(TlArgs a) {
    __shared__ double tile[kTlTile];
    const uint32_t local = blockIdx.y, s = a.stream_base + local, tid = threadIdx.x;
    const uint32_t limit = stream_limit(a, s);
    const uint32_t n_groups = gridDim.x, group = n_groups - 1 - blockIdx.x;  // the longest rows first
    const uint32_t i0 = group * T, i = i0 + tid;
    if (i0 >= a.count) return;
    // j of this lane, of the wavefront's first lane and of the workgroup's first lane (the smallest ones: j grows with the lane)
    const uint64_t j64 = a.first + (uint64_t)i * a.stride;
    const uint64_t wave_j64 = a.first + (uint64_t)(i - (tid & 63u)) * a.stride;
    const uint64_t group_j64 = a.first + (uint64_t)i0 * a.stride;
    const bool in_window = i < a.count;
    const bool valid = in_window && j64 < limit;
    const uint32_t j = valid ? (uint32_t)j64 : 0u;
    const double* gated = a.gated + (uint64_t)local * a.pitch;

    double sum = 0.0;
    uint32_t cnt = 0, n_abs = 0;
    double thr = 0.0;
    if (group_j64 < limit) {  // (uniform) some row of the workgroup exists
        // a lane without a row takes part in the tile loads and adds nothing: no block exceeds an infinite gate
        thr = valid ? a.threshold[(uint64_t)local * a.pitch + j] : __longlong_as_double(0x7FF0000000000000ll);
        n_abs = valid ? a.above[(uint64_t)local * a.pitch + j] : 0u;
        const uint32_t last_i = min(i0 + T, a.count) - 1;
        const uint64_t group_last = min(a.first + (uint64_t)last_i * a.stride, (uint64_t)limit - 1);  // the workgroup's largest j
        const uint32_t wave_j = (uint32_t)min(wave_j64, (uint64_t)limit);
        const uint64_t wave_last = a.first + (uint64_t)min(i - (tid & 63u) + 63u, last_i) * a.stride;  // the wavefront's largest j
        for (uint32_t k0 = 0; k0 <= (uint32_t)group_last; k0 += kTlTile) {
            __syncthreads();
            for (uint32_t t = tid; t < kTlTile; t += T) tile[t] = k0 + t < limit ? gated[k0 + t] : 0.0;
            __syncthreads();
            if (wave_j64 >= limit || k0 > wave_last) continue;  // (uniform in the wavefront) no row of the wavefront reaches the tile
            if (k0 + kTlTile - 1 <= wave_j) {  // (uniform) every entry is at or before every row of the wavefront
#pragma unroll 16
                for (uint32_t t = 0; t < kTlTile; ++t) {
                    const double g = tile[t];
                    const bool pass = g > thr;
                    sum += pass ? g : 0.0;
                    cnt += pass ? 1u : 0u;
                }
            } else {  // the tile holds the diagonal for some row of the wavefront
                const bool reaches = valid && j >= k0;
                const uint32_t rel = reaches ? j - k0 : 0u;  // entries t <= rel belong to the row
#pragma unroll 8
                for (uint32_t t = 0; t < kTlTile; ++t) {
                    const double g = tile[t];
                    const bool pass = reaches && t <= rel && g > thr;
                    sum += pass ? g : 0.0;
                    cnt += pass ? 1u : 0u;
                }
            }
        }
    }
    if (!in_window) return;
    omx_program_timeline_row r{};
    const float floor = a.floor_db;
    r.momentary_lufs = r.short_term_lufs = r.integrated_lufs = floor;
    if (valid) {
        const double* e = a.segments + (uint64_t)s * a.capacity;
        const double integrated = cnt ? sum / (double)cnt : 0.0;
        r.integrated_energy = integrated;
        r.relative_threshold_energy = thr;
        r.momentary_lufs = j >= 3 ? ms_to_lufs(gating_block(e, j), floor) : floor;
        r.short_term_lufs = j >= 29 ? ms_to_lufs(short_term_block(e, j), floor) : floor;
        r.integrated_lufs = ms_to_lufs(integrated, floor);
        r.gating_above_absolute = n_abs;
        r.gating_above_relative = cnt;
        r.valid = 1;
    }
    a.rows[(uint64_t)local * a.count + i] = r;
}

}  // namespace

void launch_tl_scan(const TlArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(tl_scan_kernel, dim3(a.n_streams), dim3(T), 0, stream, a);
}
void launch_tl_rows(const TlArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(tl_rows_kernel, dim3((a.count + T - 1) / T, a.n_streams), dim3(T), 0, stream, a);  // (the host refuses n_streams > kTlMaxStreams)
}

}  // namespace omx
