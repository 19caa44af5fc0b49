// Row pass of LogisticLoss (the pointwise logistic loss over signed feedback): k_mse_pass's walk - gather -> dot -> loss ->
// gradient -> epilogue - with the logistic coefficient in place of -2 (a_k - p_k).  It moves exactly the MSE pass's bytes.
// Contract in include/tmf.h.
#include "tmf_common.h"
#include "tmf_segments.h"

namespace tmf {

constexpr int kLogisticUnroll = 4;   // list entries a lane group keeps in flight (k_mse_pass's kMseUnroll)

// log1p(t) for t in [0, 1] as 2 atanh(s), s = t / (2 + t) <= 1/3: the odd series through s^15 (the next term is below 1.4e-9
// of the sum) keeps the RELATIVE accuracy for small t that log(1 + t) loses, in a dozen instructions and two registers - the
// library's log1pf costs the user pass 23 more VGPRs (98 against 75 for rows of 64 lanes: 4 waves per SIMD against 6).
__device__ __forceinline__ float log1p_unit(float t) {
    const float s = t * __builtin_amdgcn_rcpf(2.f + t), z = s * s;
    float q = 1.f / 15.f;
    q = fmaf(q, z, 1.f / 13.f);
    q = fmaf(q, z, 1.f / 11.f);
    q = fmaf(q, z, 1.f / 9.f);
    q = fmaf(q, z, 1.f / 7.f);
    q = fmaf(q, z, 1.f / 5.f);
    q = fmaf(q, z, 1.f / 3.f);
    q = fmaf(q, z, 1.f);
    return 2.f * s * q;
}

// ---------------------------------------------------------------------------------------------
// One wave per segment; 64/G groups of G lanes each take every (64/G)-th entry of the segment, kLogisticUnroll entries in
// flight per group.  For an entry with value a and score p:  y = a > 0 ? +1 : -1 (a stored 0 and a NaN are negatives, the
// class split of k_kl_pass), w = |a| if `weighted` else 1, x = -y p, and with t = exp(-|x|) in (0, 1]
//   sigma(x) = (x >= 0 ? 1 : t) / (1 + t),   softplus(x) = max(x, 0) + log1p(t):
// nothing overflows for any finite p (t underflows to 0 beyond |p| = 104: sigma is 0 or 1, softplus 0 or x), the quotient is
// the correctly rounded one, so p = 0 gives t = 1 and the coefficient -+w / 2 exactly.  exp is the hardware's (its error in t,
// ~|x| 6e-8 relative, sits where sigma is ~t itself); log1p_unit keeps its relative accuracy for small t - a fit that has
// separated the classes sums terms of 1e-4 and less.  LOSS = false (the item pass) holds no log at all.
// Every lane of a group computes the coefficient of the group's entry; a group adds its entries in list order to one running
// fp32 sum, the groups are added in the fixed butterfly order, a row of several segments goes through the slab: no atomics,
// the order of additions depends on the lists alone, two calls give the same bits.
// ---------------------------------------------------------------------------------------------
template <int G, int NV, typename T, bool LOSS>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_logistic_pass(
    SegView sv, const int32_t* __restrict__ other, const float* __restrict__ val, const T* __restrict__ X_old,
    const T* __restrict__ Y_old, void* __restrict__ X_out, float* __restrict__ slab, float* __restrict__ loss_part, int weighted,
    int epi, tmf_adam adam) {
    constexpr int NG = 64 / G;
    const int lane = threadIdx.x & 63;
    const int64_t seg = sv.seg0 + (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (seg >= sv.nseg) return;
    const int g = lane & (G - 1), grp = lane / G;
    const auto [row, beg, end] = seg_range(sv, seg);

    Frag<NV> x, acc;
    load_row<G, NV>(x, X_old, row, g);
    zero<NV>(acc);
    float lsum = 0.f;

    for (int64_t k0 = beg + grp; k0 < end; k0 += (int64_t)NG * kLogisticUnroll) {
        Raw<NV, T> raw[kLogisticUnroll];
        float a[kLogisticUnroll];
        int j[kLogisticUnroll];
        bool ok[kLogisticUnroll];
        // ids and values first, unconditionally (index clamped into the segment), so that the four id loads - and then the
        // four row loads - are in flight together (k_mse_pass)
#pragma unroll
        for (int t = 0; t < kLogisticUnroll; ++t) {
            const int64_t k = k0 + (int64_t)t * NG;
            ok[t] = k < end;
            const int64_t kc = ok[t] ? k : end - 1;
            j[t] = other[kc];
            a[t] = val[kc];
        }
#pragma unroll
        for (int t = 0; t < kLogisticUnroll; ++t) {
            load_raw<G, NV>(raw[t], Y_old, j[t], g);   // padded slots re-read the segment's last entry; masked below
        }
#pragma unroll
        for (int t = 0; t < kLogisticUnroll; ++t) {
            Frag<NV> y;
            to_frag<NV>(y, raw[t]);
            const float p = group_allsum<G>(dot_partial<NV>(x, y));
            const bool pos = a[t] > 0.f;
            const float w = ok[t] ? (weighted ? fabsf(a[t]) : 1.f) : 0.f;   // padded slots contribute nothing
            const float xx = pos ? -p : p;                                  // x = -y p
            const float e = __expf(-fabsf(xx));
            const float sig = __fdiv_rn(xx >= 0.f ? 1.f : e, 1.f + e);
            if constexpr (LOSS) {
                const float sp = fmaxf(xx, 0.f) + log1p_unit(e);
                lsum += ok[t] ? w * sp : 0.f;   // not w * sp alone: a padded slot of an infinite score would add 0 * inf
            }
            axpy<NV>(acc, (pos ? -w : w) * sig, y);   // d loss / d p = -y w sigma(-y p)
        }
    }
    across_groups_sum<G, NV>(acc);
    if constexpr (LOSS) {
        // every lane of a group carries the same sum: take lane 0 of each group
        float l = (g == 0) ? lsum : 0.f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off, 64);
        if (lane == 0) loss_part[seg] = l;
    }
    if (grp == 0) finish_segment<G, NV, T>(sv, seg, acc, X_old, X_out, slab, row, g, epi, adam);
}

}  // namespace tmf

using namespace tmf;

template <typename T>
static int logistic_pass_impl(const tmf_segments* seg, const int32_t* other, const float* val, const void* X_old,
                              const void* Y_old, void* X_out, float* slab, float* loss_part, int n_components, int epi,
                              tmf_adam adam, int weighted, void* stream) {
    if (int rc = check_segments(seg)) return rc;
    if (seg->nseg == 0) return TMF_OK;
    TMF_REQUIRE(X_old && Y_old && X_out, "logistic_pass: null table");
    TMF_REQUIRE(other && val, "logistic_pass: null entry list");
    TMF_REQUIRE(epi == TMF_EPI_ADAM || epi == TMF_EPI_GRAD, "logistic_pass: bad epilogue %d", epi);
    const RowGeom geom = row_geom_of<T>(n_components);
    TMF_REQUIRE(geom.ld > 0, "logistic_pass: unsupported n_components %d", n_components);
    SegView sv = view(seg);
    const int wt = weighted != 0;
#define CALL_L(G_, NV_, LOSS_) \
    for_segment_pieces(sv, kWavesPerBlock, [&](unsigned blocks) { \
        hipLaunchKernelGGL((k_logistic_pass<G_, NV_, T, LOSS_>), dim3(blocks), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, \
                           sv, other, val, (const T*)X_old, (const T*)Y_old, X_out, slab, loss_part, wt, epi, adam); \
    })
#define CALL(G_, NV_) \
    if (loss_part != nullptr) { CALL_L(G_, NV_, true); } else { CALL_L(G_, NV_, false); }
    TMF_DISPATCH(T, geom, CALL);
#undef CALL
#undef CALL_L
    return check_launch("tmf_logistic_pass");
}

extern "C" int tmf_logistic_pass_f32(const tmf_segments* seg, const int32_t* other, const float* val, const float* X_old,
                                     const float* Y_old, float* X_out, float* slab, float* loss_part, int n_components, int epi,
                                     tmf_adam adam, int weighted, void* stream) {
    return logistic_pass_impl<float>(seg, other, val, X_old, Y_old, X_out, slab, loss_part, n_components, epi, adam, weighted, stream);
}
extern "C" int tmf_logistic_pass_bf16(const tmf_segments* seg, const int32_t* other, const float* val, const void* X_old,
                                      const void* Y_old, void* X_out, float* slab, float* loss_part, int n_components, int epi,
                                      tmf_adam adam, int weighted, void* stream) {
    return logistic_pass_impl<__bf16>(seg, other, val, X_old, Y_old, X_out, slab, loss_part, n_components, epi, adam, weighted, stream);
}
