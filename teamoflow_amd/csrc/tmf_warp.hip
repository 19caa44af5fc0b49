// WARP pair step of the sliced user pass: the first-violator ranking loss (Weston et al.; LightFM's 'warp') over the static negative
// table, in the slot tmf_hinge.hip fills for WMRB and tmf_bpr.hip for BPR (an extension: the reference has no such loss;
// mf/loss_graphs.py WARPLoss is the definition).
//
// Inputs per user u: the sampled scores sp[u, 0..S) in table order and, for its interactions k, the scores p_k and values a_k.  For
// a_k > 0, with t_k = fl(p_k - 1) (one fp32 rounding):
//     s*_k    = the smallest s with sp[u, s] > t_k (strict; a NaN on either side never violates)        N_k = s*_k + 1
//     w_k     = log(max(1, floor((n_items - 1) / N_k)))   (0 when nothing violates or N_k > n_items - 1)
//     delta_k = -w_k          D[u, s*_k] += w_k          loss_part[u] = sum_k w_k (1 - p_k + sp[u, s*_k])
// and delta_k = 0 for a_k <= 0.  No transcendental per pair: one logarithm per positive.
//
// One wave per user.  The row is taken in SEGMENTS of at most WCAP samples, and a segment is what the LDS holds:
//   prefix maximum  the wave reads the segment in tiles of 64 consecutive samples (lane = s - s0: coalesced), NaN samples as -inf,
//           and forms M[s] = max(sp[u, 0..s]) by a DPP scan (row_shr 1, 2, 4, 8, row_bcast 15 and 31) carried from tile to tile
//           and from segment to segment; M goes to LDS beside a zeroed copy of the segment's part of the D row.
//   search  M never decreases, so s*_k is the first s with M[s] > t_k: lanes own stored interactions, 64 at a time in CSR order, and
//           every lane makes the same ~log2(segment) branch-free halving steps in LDS.  max and > are exact: the index is the one a
//           linear scan of sp finds, bit for bit.  At s* the maximum has just risen, so M[s*] == sp[u, s*]: the row itself is not kept.
//   D       several positives of a chunk often share s* (early in training nearly all have s* = 0).  Distinct values are peeled
//           off: the lowest pending lane leads, a ballot finds the lanes with its s*, their w (zeros from everybody else) are added
//           by one fixed xor butterfly, and the leader adds the sum to the LDS copy of D[u, s*].  Leaders in ascending lane order,
//           chunks in ascending order: one order of additions, a function of the row alone.  A group of one skips the butterfly
//           (w + 0 + ... + 0 = w exactly).  No atomics.
//   loss    w_k ((double)sp[s*] - ((double)p_k - 1)) into the lane's fp64 accumulator; one fixed butterfly per user at the end.
//   out     delta[k] in the lane's own slot; the D segment from LDS, zeros included, coalesced; plain vector stores only.
// Rows longer than WCAP take the same code segment by segment.  A positive resolves in the segment g whose incoming maximum is
// not above t_k and whose last maximum is: the two comparisons need no state per positive, so every segment walks the user's
// chunks again, and only while some positive is still unresolved - after that the remaining segments just write their zeros (the
// early exit).  delta[k] is written for every entry in segment 0 (0 where nothing resolved yet) and rewritten by the same lane in
// the segment that resolves it.  Every element of delta, D and loss_part is written once the kernel has run; outputs depend on the
// row alone, never on user_order, occupancy or timing.
// +inf in sp is a violator like any other (its loss is inf); -inf never violates; a NaN p_k takes no part (delta 0).
//
// The sliced user pass keeps every user's negatives sorted by item, and unlike the hinge and BPR this loss depends on the order of
// the samples.  tmf_warp_pairs_ranked is the form the engine calls: sp and D are in the engine's order, rank[u, pos] (16 bits) is
// the place in the model's table of the sample at sorted place pos.  A segment is then staged first - the wave reads sp and rank
// in sorted order, coalesced, and every lane whose rank falls into the segment leaves its score at M[rank] in LDS - and scanned
// from there.  A row that is one segment (S <= WCAP) also notes the place of every table index (16 bits in LDS), a leader adds
// its sum at the place of s*, and D leaves as it lies; a longer row keeps D by table index and sends the segment out through the
// map, Du[pos] = D[rank[pos]] - coalesced in global memory either way, and a long row is read once per segment.  Everything else is
// the same code, and the same bits: rank = identity gives tmf_warp_pairs.
//
// tmf_warp_pairs_kos is the weighted form (KOSWARPLoss; tmf_kos.hip makes the weights): with omega[k] beside the entries, the weight
// of an entry is w' = fl(omega_k w_k), one fp32 rounding, and w' stands wherever w stands above - the test w' > 0, delta, the sum
// into D and the loss.  It is a second instance of the kernel template: the instance without omega is the code it was before.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int WCAP = 4096;              // samples of a segment: 8 bytes of LDS each (M and D) + 2 in the ranked form, 40 KB per wave at most
constexpr int WCHUNK = 64;              // stored interactions per pass: one per lane
constexpr int WTILES = 4;               // tiles of 64 samples loaded before the first of them is scanned

#define TMF_DPP_MAX(v, ctrl, rows) \
    fmaxf((v), __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(v), (ctrl), (rows), 0xf, false)))

// Inclusive prefix maximum over the 64 lanes (no NaN among the inputs).  A lane without a source keeps -inf.
__device__ __forceinline__ float wave_prefix_max(float v) {
    v = TMF_DPP_MAX(v, 0x111, 0xf);     // row_shr:1
    v = TMF_DPP_MAX(v, 0x112, 0xf);     // row_shr:2
    v = TMF_DPP_MAX(v, 0x114, 0xf);     // row_shr:4
    v = TMF_DPP_MAX(v, 0x118, 0xf);     // row_shr:8: every row of 16 lanes is scanned
    v = TMF_DPP_MAX(v, 0x142, 0xa);     // row_bcast:15 into rows 1 and 3
    v = TMF_DPP_MAX(v, 0x143, 0xc);     // row_bcast:31 into rows 2 and 3
    return v;
}

template <bool KOS>
__global__ __launch_bounds__(64) void k_warp_pairs(const int64_t* __restrict__ rowptr, const float* __restrict__ val,
                                                   const float* __restrict__ p, const float* __restrict__ sp, int S, int cap,
                                                   int nm1, int64_t n_users, float* __restrict__ delta, float* __restrict__ D,
                                                   float* __restrict__ loss_part, const int32_t* __restrict__ order,
                                                   const uint16_t* __restrict__ rank, const float* __restrict__ omega) {
    extern __shared__ float wlds[];     // M[cap] | D[cap] | place[cap] (16 bits each; the ranked form only)
    float* Ml = wlds;
    float* Dl = wlds + cap;
    uint16_t* Pl = reinterpret_cast<uint16_t*>(wlds + 2 * cap);
    const int lane = threadIdx.x;
    const int64_t slot = blockIdx.x;
    if (slot >= n_users) return;
    // `order` (optional): the users in the order the waves should take them, the heavy ones first (tmf_hinge.hip).  Every user is
    // computed by itself; the order changes no result.
    const int64_t u = order ? (int64_t)order[slot] : slot;
    const int64_t rb = rowptr[u], re = rowptr[u + 1];
    const float* spu = sp + u * (int64_t)S;
    float* Du = D + u * (int64_t)S;
    const uint16_t* ranku = rank ? rank + u * (int64_t)S : nullptr;   // wave-uniform: sp and D are in another order than the table
    // a ranked row that is one segment keeps its D in the order it leaves in: staging notes the place of every table index
    const bool by_place = ranku && S <= cap;

    double lacc = 0.0;
    float carry = -INFINITY;            // max of the row before this segment (wave-uniform)
    bool unresolved = re > rb;          // some positive may still find its violator (wave-uniform)
    for (int g0 = 0; g0 < S; g0 += cap) {
        const int len = (S - g0 < cap) ? (S - g0) : cap;
        const float carry_in = carry;
        if (unresolved) {
            if (ranku) {
                // ---- stage: the scores of the segment into table order (every place of it is some sample's rank) ----
                for (int q0 = 0; q0 < S; q0 += 64 * WTILES) {
                    float x[WTILES];
                    int at[WTILES];
#pragma unroll
                    for (int j = 0; j < WTILES; ++j) {
                        const int q = q0 + 64 * j + lane;
                        x[j] = (q < S) ? spu[q] : 0.f;
                        at[j] = (q < S) ? (int)ranku[q] - g0 : -1;
                    }
#pragma unroll
                    for (int j = 0; j < WTILES; ++j) {
                        if (at[j] >= 0 && at[j] < len) {
                            Ml[at[j]] = x[j];
                            if (by_place) Pl[at[j]] = (uint16_t)(q0 + 64 * j + lane);
                        }
                    }
                }
                wave_lds_sync();
            }
            for (int s0 = 0; s0 < len; s0 += 64 * WTILES) {
                float x[WTILES];
#pragma unroll
                for (int j = 0; j < WTILES; ++j) {                     // the loads of WTILES tiles are in flight together
                    const int s = s0 + 64 * j + lane;
                    x[j] = (s < len) ? (ranku ? Ml[s] : spu[g0 + s]) : -INFINITY;
                }
#pragma unroll
                for (int j = 0; j < WTILES; ++j) {
                    const int s = s0 + 64 * j + lane;
                    float m = (x[j] == x[j]) ? x[j] : -INFINITY;       // a NaN sample is skipped
                    m = fmaxf(wave_prefix_max(m), carry);
                    carry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 63));
                    if (s < len) {
                        Ml[s] = m;
                        Dl[s] = 0.f;
                    }
                }
            }
        } else {
            for (int s = lane; s < len; s += 64) Dl[s] = 0.f;
        }
        wave_lds_sync();
        if (unresolved) {
            int top = 1;                // the largest power of two <= len
            while (2 * top <= len) top *= 2;
            bool left = false;
            for (int64_t cb = rb; cb < re; cb += WCHUNK) {
                const int n_here = (int)((re - cb < WCHUNK) ? (re - cb) : WCHUNK);
                const bool have = lane < n_here;
                const bool pos = have && val[cb + lane] > 0.f;
                const float pk = pos ? p[cb + lane] : 0.f;
                const float t = pk - 1.0f;
                // resolves here: nothing before the segment is above t, something inside it is
                const bool hit = pos && !(carry_in > t) && (carry > t);
                left = left || (pos && t >= carry);
                // ---- the first s with M[s] > t: lo counts the samples in front of it ----
                int lo = 0;
                for (int b = top; b > 0; b >>= 1) {
                    const int at = lo + b;
                    const float m = Ml[(at <= len ? at : len) - 1];
                    lo = (at <= len && !(m > t)) ? at : lo;
                }
                const int sstar = hit ? lo : 0;                        // hit: lo < len
                float w = 0.f;
                if (hit) {
                    const int N = g0 + sstar + 1;
                    const int q = (N <= nm1) ? nm1 / N : 1;
                    w = (q > 1) ? logf((float)q) : 0.f;
                    if (KOS) w = omega[cb + lane] * w;                 // w' = fl(omega w)
                }
                const bool act = hit && w > 0.f;
                if (act) lacc += (double)w * ((double)Ml[sstar] - ((double)pk - 1.0));
                if (have && (g0 == 0 || act)) delta[cb + lane] = act ? -w : 0.f;
                // ---- D[u, s*] += w: one leader per distinct s*, lowest lane first ----
                uint64_t pending = __builtin_amdgcn_ballot_w64(act);
                while (pending) {
                    const int leader = __builtin_ctzll(pending);
                    const int s_lead = __builtin_amdgcn_readlane(sstar, leader);
                    const bool member = act && sstar == s_lead;
                    const uint64_t members = __builtin_amdgcn_ballot_w64(member);
                    float v = member ? w : 0.f;
                    if (members & (members - 1)) {
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
                    }
                    if (lane == leader) Dl[by_place ? (int)Pl[s_lead] : s_lead] += v;
                    pending &= ~members;
                }
            }
            unresolved = __builtin_amdgcn_ballot_w64(left) != 0;
            wave_lds_sync();
        }
        if (ranku && !by_place) {
            for (int q = lane; q < S; q += 64) {
                const int at = (int)ranku[q] - g0;
                if (at >= 0 && at < len) Du[q] = Dl[at];
            }
        } else {
            for (int s = lane; s < len; s += 64) Du[g0 + s] = Dl[s];
        }
        wave_lds_sync();                // the next segment rewrites M and D
    }
    // entries of a row without samples to compare with cannot occur (S >= 1): segment 0 wrote every delta
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lacc += __shfl_xor(lacc, off, 64);  // fixed butterfly: every lane ends with the same bits
    if (lane == 0 && loss_part) loss_part[u] = (float)lacc;
}

}  // namespace tmf

using namespace tmf;

static int warp_pairs(const int64_t* rowptr, const float* val, const float* p, const float* sp, const uint16_t* rank, const float* omega,
                      int32_t n_users, int32_t n_samples, int32_t n_items, float* delta, float* D, float* loss_part,
                      const int32_t* user_order, void* stream, const char* what) {
    if (n_users == 0) return TMF_OK;
    // val, p and delta are read only where a row has entries: a table without interactions may pass NULL for them
    TMF_REQUIRE(rowptr && sp && D && n_users > 0 && n_samples > 0 && n_items > 0, "%s: bad arguments", what);
    TMF_REQUIRE_LAUNCH(n_users, 64, what);
    const int cap = n_samples < WCAP ? (int)n_samples : WCAP;
    const size_t lds = (size_t)cap * (2 * sizeof(float) + (rank ? sizeof(uint16_t) : 0));
    if (omega)
        hipLaunchKernelGGL(k_warp_pairs<true>, dim3((unsigned)n_users), dim3(64), lds, (hipStream_t)stream, rowptr, val, p, sp,
                           (int)n_samples, cap, (int)n_items - 1, (int64_t)n_users, delta, D, loss_part, user_order, rank, omega);
    else
        hipLaunchKernelGGL(k_warp_pairs<false>, dim3((unsigned)n_users), dim3(64), lds, (hipStream_t)stream, rowptr, val, p, sp,
                           (int)n_samples, cap, (int)n_items - 1, (int64_t)n_users, delta, D, loss_part, user_order, rank, nullptr);
    return check_launch(what);
}

extern "C" int tmf_warp_pairs(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users,
                              int32_t n_samples, int32_t n_items, float* delta, float* D, float* loss_part,
                              const int32_t* user_order, void* stream) {
    return warp_pairs(rowptr, val, p, sp, nullptr, nullptr, n_users, n_samples, n_items, delta, D, loss_part, user_order, stream,
                      "tmf_warp_pairs");
}

extern "C" int tmf_warp_pairs_ranked(const int64_t* rowptr, const float* val, const float* p, const float* sp, const uint16_t* rank,
                                     int32_t n_users, int32_t n_samples, int32_t n_items, float* delta, float* D, float* loss_part,
                                     const int32_t* user_order, void* stream) {
    TMF_REQUIRE(n_users == 0 || (rank && n_samples <= 65536), "tmf_warp_pairs_ranked: bad arguments (ranks are 16 bits: n_samples <= 65536)");
    return warp_pairs(rowptr, val, p, sp, rank, nullptr, n_users, n_samples, n_items, delta, D, loss_part, user_order, stream,
                      "tmf_warp_pairs_ranked");
}

extern "C" int tmf_warp_pairs_kos(const int64_t* rowptr, const float* val, const float* p, const float* sp, const uint16_t* rank,
                                  const float* omega, int32_t n_users, int32_t n_samples, int32_t n_items, float* delta, float* D,
                                  float* loss_part, const int32_t* user_order, void* stream) {
    TMF_REQUIRE(n_users == 0 || (omega && (!rank || n_samples <= 65536)),
                "tmf_warp_pairs_kos: bad arguments (omega is required; ranks are 16 bits: n_samples <= 65536)");
    return warp_pairs(rowptr, val, p, sp, rank, omega, n_users, n_samples, n_items, delta, D, loss_part, user_order, stream,
                      "tmf_warp_pairs_kos");
}
