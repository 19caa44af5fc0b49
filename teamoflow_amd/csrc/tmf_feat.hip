// LinearEmbedding over a sparse feature matrix F: the effective table E = F W the passes of tmf_train.hip / tmf_wmrb.hip read, and
// the step of the weights W from the gradient G = dL/dE those passes emit under TMF_EPI_GRAD (dW = F^T G, then fresh Adam).  Both
// directions are ONE kernel over a list view of F: the CSR lists (row -> features) for E, the CSC lists (feature -> rows) for the
// step.  Contract in include/tmf.h.
#include "tmf_common.h"
#include "tmf_segments.h"

namespace tmf {

constexpr int kFeatUnroll = 4;   // list entries a lane group keeps in flight (k_mse_pass's kMseUnroll)

// ---------------------------------------------------------------------------------------------
// k_mse_pass without the dot product.  One wave per segment; the 64/G lane groups take every (64/G)-th entry, kFeatUnroll
// of them in flight per group; the value of an entry streams beside its id (no second index, nothing skipped: an explicit
// zero multiplies its row like any value).  Every group adds its entries in list order to one running fp32 sum, the groups
// are added in the fixed butterfly order, a row of several segments goes through the slab: the order of additions depends
// on the lists alone, so two calls give the same bits.  An empty list leaves acc = +0: the GRAD epilogue writes a zero
// row, the ADAM epilogue w - 0 / (0 + eps) = w.
// ---------------------------------------------------------------------------------------------
template <int G, int NV>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_feat_pass(
    SegView sv, const int32_t* __restrict__ id, const float* __restrict__ val, const float* __restrict__ Tab,
    const float* __restrict__ X_old, void* __restrict__ X_out, float* __restrict__ slab, int epi, tmf_adam adam) {
    constexpr int NG = 64 / G;
    const int lane = threadIdx.x & 63;
    const int64_t seg = sv.seg0 + (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (seg >= sv.nseg) return;
    const int g = lane & (G - 1), grp = lane / G;
    const auto [row, beg, end] = seg_range(sv, seg);

    Frag<NV> acc;
    zero<NV>(acc);
    for (int64_t k0 = beg + grp; k0 < end; k0 += (int64_t)NG * kFeatUnroll) {
        Raw<NV, float> raw[kFeatUnroll];
        float a[kFeatUnroll];
        int j[kFeatUnroll];
        // ids and values first, unconditionally (index clamped into the segment), so that the id loads are in flight together
#pragma unroll
        for (int t = 0; t < kFeatUnroll; ++t) {
            const int64_t k = k0 + (int64_t)t * NG;
            const bool ok = k < end;
            const int64_t kc = ok ? k : end - 1;
            j[t] = id[kc];
            const float v = val[kc];
            a[t] = ok ? v : 0.f;   // padded slots re-read the segment's last entry (a row the sum holds anyway) with weight 0
        }
#pragma unroll
        for (int t = 0; t < kFeatUnroll; ++t) load_raw<G, NV>(raw[t], Tab, j[t], g);
#pragma unroll
        for (int t = 0; t < kFeatUnroll; ++t) {
            Frag<NV> y;
            to_frag<NV>(y, raw[t]);
            axpy<NV>(acc, a[t], y);
        }
    }
    across_groups_sum<G, NV>(acc);
    if (grp == 0) finish_segment<G, NV, float>(sv, seg, acc, X_old, X_out, slab, row, g, epi, adam);
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_feat_pass_f32(const tmf_segments* seg, const int32_t* id, const float* val, const float* T,
                                 const float* X_old, float* X_out, float* slab, int n_components, int epi, tmf_adam adam,
                                 void* stream) {
    if (int rc = check_segments(seg)) return rc;
    if (seg->nseg == 0) return TMF_OK;
    TMF_REQUIRE(epi == TMF_EPI_ADAM || epi == TMF_EPI_GRAD, "feat_pass: bad epilogue %d", epi);
    TMF_REQUIRE(T && X_out && (epi == TMF_EPI_GRAD || X_old), "feat_pass: null table");
    TMF_REQUIRE(id && val, "feat_pass: null entry list");
    const RowGeom geom = row_geom(n_components);
    SegView sv = view(seg);
#define CALL(G_, NV_) \
    for_segment_pieces(sv, kWavesPerBlock, [&](unsigned blocks) { \
        hipLaunchKernelGGL((k_feat_pass<G_, NV_>), dim3(blocks), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, \
                           sv, id, val, T, X_old, (void*)X_out, slab, epi, adam); \
    })
    TMF_DISPATCH_GEOM(geom, CALL);
#undef CALL
    return check_launch("tmf_feat_pass_f32");
}
