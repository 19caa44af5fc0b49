// What the segment passes share (tmf_train.hip, tmf_feat.hip): the device view of a tmf_segments table, a segment's range and
// end, and the host side that checks a table and sends its segments out in launches.
#pragma once
#include "tmf_common.h"

namespace tmf {

constexpr int kWavesPerBlock = 2;   // independent waves, no barrier; 2 per workgroup measured best (C4 item pass 32.1 ms; 4: 32.5, 8: 36.6; MSE epoch 11.1 vs 11.45)
constexpr int64_t kMaxBlocks = ((int64_t)1 << 32) / (64 * kWavesPerBlock) - 1;   // workgroups of one launch: < 2^32 work-items

struct SegView {
    const int64_t* rowptr;
    const int32_t* seg_row;
    const int32_t* seg_chunk;
    const int32_t* seg_slab;
    int64_t nseg;
    int32_t chunk;
    int32_t row_mod;  // > 0: list rows are (block * row_mod + table row); 0: list row == table row
    int64_t seg0;     // first segment of this launch (a launch carries < 2^32 work-items: long segment lists go out in pieces)
    int xcd_run;      // k_wsum_pass_pg: consecutive workgroups per XCD run (0 = plain block order)
};

struct SegRange { int row; int64_t beg, end; };   // the table row a segment's list belongs to, and its entries
__device__ __forceinline__ SegRange seg_range(const SegView& sv, int64_t seg) {
    const int lrow = sv.seg_row[seg];
    const int row = sv.row_mod > 0 ? lrow % sv.row_mod : lrow;
    const int64_t rbeg = sv.rowptr[lrow], rend = sv.rowptr[lrow + 1];
    const int64_t beg = rbeg + (int64_t)sv.seg_chunk[seg] * sv.chunk;
    return SegRange{row, beg, (beg + sv.chunk < rend) ? beg + sv.chunk : rend};
}

// The end of a segment: its slab slot when the row is cut into several (k_combine_rows), else the epilogue at once.  adam by
// reference: a copy made here moves the kernels' loads of adam and epi, 2 - 5 instructions more in every instance.
template <int G, int NV, typename T>
__device__ __forceinline__ void finish_segment(const SegView& sv, int64_t seg, const Frag<NV>& acc, const T* __restrict__ X_old,
                                               void* __restrict__ X_out, float* __restrict__ slab, int row, int g, int epi,
                                               const tmf_adam& adam) {
    const int slot = sv.seg_slab[seg];
    if (slot < 0) row_epilogue<G, NV, T>(acc, X_old, X_out, row, g, epi, adam);
    else store_row_f32<G, NV, T>(acc, slab, slot, g);
}

static inline SegView view(const tmf_segments* s) {
    return SegView{s->rowptr, s->seg_row, s->seg_chunk, s->seg_slab, s->nseg, s->chunk, s->row_mod, 0, 0};
}

// A launch carries < 2^32 work-items (tmf::launch_fits): the segments go out in pieces of kMaxBlocks workgroups, sv.seg0 first
template <typename F>
static void for_segment_pieces(SegView& sv, int64_t segs_per_block, F&& launch) {
    for (sv.seg0 = 0; sv.seg0 < sv.nseg; sv.seg0 += kMaxBlocks * segs_per_block) {
        const int64_t want = (sv.nseg - sv.seg0 + segs_per_block - 1) / segs_per_block;
        launch((unsigned)(want < kMaxBlocks ? want : kMaxBlocks));
    }
}

static int check_segments(const tmf_segments* s) {
    TMF_REQUIRE(s != nullptr, "segments is null");
    TMF_REQUIRE(s->nseg >= 0 && s->chunk > 0, "segments: nseg=%lld chunk=%d", (long long)s->nseg, s->chunk);
    TMF_REQUIRE(s->nseg == 0 || (s->rowptr && s->seg_row && s->seg_chunk && s->seg_slab), "segments: null array");
    return TMF_OK;
}

}  // namespace tmf
