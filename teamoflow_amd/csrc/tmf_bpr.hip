// BPR pair step of the sliced user pass: the pairwise logistic loss -log sigmoid(p_k - sp[u, s]) over the static negative table, in
// the slot tmf_hinge.hip fills for WMRB (an extension: the reference has no such loss; mf/loss_graphs.py BPRLoss is the definition).
//
// Inputs per user u: the sampled scores sp[u, 0..S) and, for its interactions k, the scores p_k and values a_k.  For a_k > 0
//     x_ks    = sp[u, s] - p_k                       e = exp(-|x|), t = 1 + e
//     sigma   = x >= 0 ? 1 / t : e / t               softplus = max(x, 0) + log1p(e)
//     delta_k = -(1 / S) sum_s sigma(x_ks)           D[u, s] = (1 / S) sum_k sigma(x_ks)       loss_part[u] = (1 / S) sum_k sum_s softplus(x_ks)
// and delta_k = 0 for a_k <= 0.  Every pair costs its own exponential, so the step is O(P S) per user - 1e11 pairs at C4 - and bound
// by the transcendental unit (v_exp_f32, v_rcp_f32, v_log_f32 at a quarter of the plain rate), not by memory.
// One wave per user (tmf_hinge.hip: one user per workgroup was the fastest form there too).  Lanes own samples, tiles of 64 x BSPL
// in registers, tiles outermost; inside a tile the user's stored interactions are staged 64 at a time, the positive ones compacted
// into LDS in their CSR order, and every positive is broadcast from there to all lanes:
//   D       every lane adds sigma to the accumulators of its own samples, in ascending k: no reduction at all;
//   delta   the sum over s crosses the lanes: every lane leaves its partial of positive kk at red[kk][lane], and after a round of 32
//           positives lane (kk, half) adds half a row in index order, the two halves meet in one shuffle - two LDS operations per
//           (positive, tile) instead of a six-step butterfly.  A later tile adds its share to what the earlier ones stored;
//   loss    eight terms in fp32, then into the lane's fp64 accumulator; one fixed butterfly per user at the end.
// Sums of sigma are fp32 with all-positive terms; 1 / S is applied once to each finished sum.  No atomics: every sum has one order,
// a function of (S, the user's row) alone, so runs are bit-reproducible whatever the user order, the occupancy or the timing.
// log1p(e) = log(t) + (e - (t - 1)) / t: the second term gives back what the rounding of 1 + e took (t - 1 is exact), so a pair
// ranked far apart costs e, not 0 or 1.2e-7.  x = +inf: e = 0, sigma = 1, softplus = inf; x = -inf: sigma = 0, softplus = 0; a NaN
// score makes NaN of what it enters - the D of its sample, or every output of the user if it is a p_k - and of nothing else.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int BSPL = 8;                 // samples per lane and tile (a tile = 512 samples)
constexpr int BTILE = 64 * BSPL;
constexpr int BCHUNK = 64;              // stored interactions staged per pass: one per lane
constexpr int BROUND = 32;              // positives per reduction round
constexpr int BROW = 65;                // floats between the rows of red: row kk, element i lives in bank (kk + i) % 32

struct BprLds {                         // per wave, 8640 bytes
    float red[BROUND * BROW];           // red[kk * BROW + lane]: the lane's sum of sigma over its samples for positive kk of the round
    float pk[BCHUNK];                   // scores of the chunk's positives, CSR order
    unsigned char src[BCHUNK];          // chunk-local index of the entry a compacted positive came from
};

// One positive against the lane's BSPL samples.  TAIL: the tile holds the end of the row, samples at or beyond S take no part.
template <bool TAIL>
__device__ __forceinline__ void bpr_pairs_of(const float (&x)[BSPL], const bool (&live)[BSPL], float pk, float (&dacc)[BSPL],
                                             float& dsum, float& lsum) {
    constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
    float ds = 0.f, ls = 0.f;
#pragma unroll
    for (int j = 0; j < BSPL; ++j) {
        const float d = x[j] - pk;
        const float e = __builtin_amdgcn_exp2f(fabsf(d) * -kLog2e);
        const float t = 1.0f + e;
        const float r = __builtin_amdgcn_rcpf(t);
        float sg = (d >= 0.f) ? r : e * r;
        float sf = fmaxf(d, 0.f) + fmaf(__builtin_amdgcn_logf(t), kLn2, (e - (t - 1.0f)) * r);
        if (TAIL) {
            sg = live[j] ? sg : 0.f;
            sf = live[j] ? sf : 0.f;
        }
        dacc[j] += sg;
        ds += sg;
        ls += sf;
    }
    dsum = ds;
    lsum = ls;
}

// A round: positives r0 .. r0 + nk of the staged chunk against the lane's samples; the lane's partials of delta go to red.
template <bool TAIL>
__device__ __forceinline__ void bpr_round(BprLds& L, int r0, int nk, int lane, const float (&x)[BSPL], const bool (&live)[BSPL],
                                          float (&dacc)[BSPL], double& lacc) {
    for (int kk = 0; kk < nk; ++kk) {
        const float pk = L.pk[r0 + kk];  // same address in every lane: broadcast
        float dsum, lsum;
        bpr_pairs_of<TAIL>(x, live, pk, dacc, dsum, lsum);
        L.red[kk * BROW + lane] = dsum;
        lacc += (double)lsum;
    }
}

__global__ __launch_bounds__(64) void k_bpr_pairs(const int64_t* __restrict__ rowptr, const float* __restrict__ val,
                                                  const float* __restrict__ p, const float* __restrict__ sp, int S, float inv_s,
                                                  int64_t n_users, float* __restrict__ delta, float* __restrict__ D,
                                                  float* __restrict__ loss_part, const int32_t* __restrict__ order) {
    __shared__ BprLds L;
    const int lane = threadIdx.x;
    const int64_t slot = blockIdx.x;
    if (slot >= n_users) return;
    // `order` (optional): the users in the order the waves should take them, the heavy ones first (tmf_hinge.hip).  Every user is
    // computed by itself; the order changes no result.
    const int64_t u = order ? (int64_t)order[slot] : slot;
    const int64_t rb = rowptr[u], re = rowptr[u + 1];
    const float* spu = sp + u * (int64_t)S;
    float* Du = D + u * (int64_t)S;
    const int kk_own = lane & (BROUND - 1), half = lane >> 5;  // the row of red this lane adds up, and which half of it

    double lacc = 0.0;
    for (int s0 = 0; s0 < S; s0 += BTILE) {
        const bool tail = s0 + BTILE > S;  // wave-uniform
        float x[BSPL], dacc[BSPL];
        bool live[BSPL];
#pragma unroll
        for (int j = 0; j < BSPL; ++j) {
            const int s = s0 + lane + 64 * j;
            live[j] = s < S;
            x[j] = live[j] ? spu[s] : 0.f;
            dacc[j] = 0.f;
        }
        for (int64_t cb = rb; cb < re; cb += BCHUNK) {
            // ---- the chunk's positives, compacted in CSR order ----
            const int len = (int)((re - cb < BCHUNK) ? (re - cb) : BCHUNK);
            const bool have = lane < len;
            const bool pos = have && val[cb + lane] > 0.f;
            const uint64_t votes = __builtin_amdgcn_ballot_w64(pos);
            const int npos = __popcll(votes);
            if (pos) {
                const int at = __popcll(votes & ((1ull << lane) - 1ull));
                L.pk[at] = p[cb + lane];
                L.src[at] = (unsigned char)lane;
            }
            if (s0 == 0 && have && !pos) delta[cb + lane] = 0.f;  // stored values <= 0 take no part
            wave_lds_sync();
            for (int r0 = 0; r0 < npos; r0 += BROUND) {
                const int nk = (npos - r0 < BROUND) ? (npos - r0) : BROUND;
                if (tail) bpr_round<true>(L, r0, nk, lane, x, live, dacc, lacc);
                else bpr_round<false>(L, r0, nk, lane, x, live, dacc, lacc);
                wave_lds_sync();
                // ---- delta of the round's positives: lane (kk_own, half) adds 32 partials in lane order, half 0 + half 1 ----
                float v = 0.f;
                if (kk_own < nk) {
                    const float* row = L.red + kk_own * BROW + 32 * half;
#pragma unroll 8
                    for (int i = 0; i < 32; ++i) v += row[i];
                }
                v += __shfl_xor(v, 32, 64);
                if (half == 0 && kk_own < nk) {
                    const int64_t k = cb + L.src[r0 + kk_own];
                    const float dk = -(v * inv_s);
                    if (s0 == 0) delta[k] = dk;
                    else delta[k] += dk;  // the tiles in ascending order: one order of additions
                }
                wave_lds_sync();  // the next round rewrites red, the next chunk pk and src
            }
        }
#pragma unroll
        for (int j = 0; j < BSPL; ++j) {
            const int s = s0 + lane + 64 * j;
            if (live[j]) Du[s] = dacc[j] * inv_s;  // zeros for a user without positives
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lacc += __shfl_xor(lacc, off, 64);  // fixed butterfly: every lane ends with the same bits
    if (lane == 0 && loss_part) loss_part[u] = (float)(lacc * (double)inv_s);
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_bpr_pairs(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users,
                             int32_t n_samples, float* delta, float* D, float* loss_part, const int32_t* user_order, void* stream) {
    if (n_users == 0) return TMF_OK;
    // val, p and delta are read only where a row has entries: a table without interactions may pass NULL for them
    TMF_REQUIRE(rowptr && sp && D && n_users > 0 && n_samples > 0, "bpr_pairs: bad arguments");
    TMF_REQUIRE_LAUNCH(n_users, 64, "tmf_bpr_pairs");
    hipLaunchKernelGGL(k_bpr_pairs, dim3((unsigned)n_users), dim3(64), 0, (hipStream_t)stream, rowptr, val, p, sp, (int)n_samples,
                       1.0f / (float)n_samples, (int64_t)n_users, delta, D, loss_part, user_order);
    return check_launch("tmf_bpr_pairs");
}
