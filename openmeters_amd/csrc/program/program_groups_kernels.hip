// Groups of the programme loudness bank (include/omx/program_groups.h): one 256-lane workgroup per group.
//
// Stored mode.  The result pass of program_result_device.hpp (four reductions, eight-pass radix select, record writer) over a GROUP
// SOURCE: the lanes walk the group's members in order, and within member m lane t starts at block k = 3 + ((t - before_m) mod 256)
// (29 + ... for the short-term blocks) and takes every 256th.  before_m is the number of blocks of the members before it, so the
// block with flat index i over the concatenation lands on lane i mod 256 and every lane meets its blocks in ascending i, without a
// search per block.  A group of one member is the interval pass, instruction for instruction in what touches a block.
// Each of the twelve walks (4 reductions + 8 select passes) forms its blocks from e[] again, as the per-stream pass does, except that
// a long group (program_groups.hpp: kPgStageMin) stages its short-term blocks in the first of their ten walks and reads them back
// in the other nine.  A lane reads only what it wrote itself, in program order: no barrier, no fence, and the same bits.
// LDS atomics in the select as there; no global atomics.
//
// Bounded mode.  Lane t owns bins t, t + 256, t + 512, t + 768 of both histograms, adds the members' counts and sums in member order
// in registers, leaves them in LDS, and the bins-to-record code of the per-stream pass runs (program_histogram_device.hpp).
// Built with -ffp-contract=off like the rest of the bank.
#include "program_histogram_device.hpp"

namespace omx {
namespace {

constexpr uint32_t GT = kPlResultThreads;
static_assert(GT == kPhThreads && GT == 256, "one workgroup shape for both modes; the lane of a block is its flat index mod 256");

struct PlGroupSource {
    const double* energies;   // the bank's [n_streams][capacity]
    const PgMember* members;  // the whole table
    PgGroup g;
    double* stage;            // the group's staged short-term blocks, by flat index; null: not staged
    mutable bool staged;      // the first walk over the short-term blocks has filled `stage`
    template <class F>
    __device__ __forceinline__ void for_gating(F&& f) const {
        if (g.count == 0) return;
        const uint32_t base = members[g.first].gating_before;
        for (uint32_t m = 0; m < g.count; ++m) {  // (uniform: the member's fields are scalar loads)
            const PgMember mb = members[g.first + m];
            const double* e = energies + mb.offset;
            const uint32_t lane = (threadIdx.x - (mb.gating_before - base)) & (GT - 1);
            for (uint32_t j = 3 + lane; j < mb.n; j += GT) f(gating_block(e, j));
        }
    }
    template <class F>
    __device__ __forceinline__ void for_short_term(F&& f) const {
        if (g.count == 0) return;
        const uint32_t base = members[g.first].short_term_before;
        for (uint32_t m = 0; m < g.count; ++m) {
            const PgMember mb = members[g.first + m];
            const double* e = energies + mb.offset;
            const uint32_t at = mb.short_term_before - base;  // flat index of the member's first block
            const uint32_t lane = (threadIdx.x - at) & (GT - 1);
            if (!stage) {  // (uniform, as is `staged`)
                for (uint32_t j = 29 + lane; j < mb.n; j += GT) f(short_term_block(e, j));
            } else if (!staged) {
                for (uint32_t j = 29 + lane; j < mb.n; j += GT) {
                    const double v = short_term_block(e, j);
                    stage[at + (j - 29)] = v;
                    f(v);
                }
            } else {
                for (uint32_t j = 29 + lane; j < mb.n; j += GT) f(stage[at + (j - 29)]);
            }
        }
        staged = true;
    }
    __device__ __forceinline__ uint64_t segments() const { return g.segments; }
    __device__ __forceinline__ uint64_t gating_blocks() const { return g.gating_blocks; }
    __device__ __forceinline__ uint64_t short_term_blocks() const { return g.short_term_blocks; }
    // the latest blocks are the last member's
    __device__ __forceinline__ double momentary() const {
        if (g.count == 0) return 0.0;
        const PgMember mb = members[g.first + g.count - 1];
        return mb.n >= 4 ? gating_block(energies + mb.offset, mb.n - 1) : 0.0;
    }
    __device__ __forceinline__ double short_term() const {
        if (g.count == 0) return 0.0;
        const PgMember mb = members[g.first + g.count - 1];
        return mb.n >= 30 ? short_term_block(energies + mb.offset, mb.n - 1) : 0.0;
    }
};

__global__ __launch_bounds__(GT) void pg_stored_kernel(PlResultArgs a, const PgMember* members, const PgGroup* groups, double* stage) {
    const PgGroup g = groups[blockIdx.x];
    const PlGroupSource src{a.segments, members, g, g.stage_at != kPgNoStage ? stage + g.stage_at : nullptr, false};
    const PlRecordTail tail{src.g.frames, 0u, nullptr, nullptr};
    pl_result_pass(src, tail, a.absolute_gate, a.floor_db, a.records + blockIdx.x);
}

__global__ __launch_bounds__(GT) void pg_bounded_kernel(PgBoundedArgs a) {
    __shared__ PhResultLds lds;
    __shared__ double red[GT];
    const uint32_t tid = threadIdx.x;
    const PgGroup g = a.groups[blockIdx.x];
    unsigned long long cnt[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    double sum[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll 2
    for (uint32_t m = 0; m < g.count; ++m) {  // member order: the order of the additions into a bin's sum
        const omx_program_histogram& h = a.hist[a.members[g.first + m].stream];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t b = tid + GT * q;
            if (b >= kPhBins) continue;
            cnt[0][q] += h.gating_count[b];
            sum[0][q] += h.gating_sum[b];
            cnt[1][q] += h.short_term_count[b];
            sum[1][q] += h.short_term_sum[b];
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t b = tid + GT * q;
        if (b >= kPhBins) continue;
#pragma unroll
        for (uint32_t w = 0; w < 2; ++w) {
            lds.cnt[w][b] = cnt[w][q];
            lds.sum[w][b] = sum[w][q];
        }
    }
    // the maxima: the largest of the members' running maxima
    double g_max = 0.0, s_max = 0.0;
    for (uint32_t m = tid; m < g.count; m += GT) {
        const PhRunning run = a.running[a.members[g.first + m].stream];
        g_max = fmax(g_max, run.max_momentary);
        s_max = fmax(s_max, run.max_short_term);
    }
    g_max = block_max(g_max, red);
    s_max = block_max(s_max, red);  // (its barriers also publish lds.cnt / lds.sum)
    ph_result_from_bins(lds, a.floor_db, a.records + blockIdx.x, [&] {
        PhRecordTail t;
        t.run = PhRunning{0.0, 0.0, g_max, s_max};
        if (g.count != 0) {  // the latest blocks are the last member's
            const PhRunning last = a.running[a.members[g.first + g.count - 1].stream];
            t.run.momentary = last.momentary;
            t.run.short_term = last.short_term;
        }
        t.frames = g.frames;
        t.segments = g.segments;
        t.gating_blocks = g.gating_blocks;
        t.short_term_blocks = g.short_term_blocks;
        t.max_true_peak_db = a.floor_db;
        return t;
    });
}

}  // namespace

void launch_pg_stored(const PlResultArgs& a, const PgMember* members, const PgGroup* groups, double* stage, uint32_t n_groups, hipStream_t stream) {
    hipLaunchKernelGGL(pg_stored_kernel, dim3(n_groups), dim3(GT), 0, stream, a, members, groups, stage);
}
void launch_pg_bounded(const PgBoundedArgs& a, uint32_t n_groups, hipStream_t stream) {
    hipLaunchKernelGGL(pg_bounded_kernel, dim3(n_groups), dim3(GT), 0, stream, a);
}

}  // namespace omx
