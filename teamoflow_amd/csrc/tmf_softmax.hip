// Sampled-softmax pair step of the sliced user pass: the softmax of a positive against the user's row of the static negative table,
// in the slot tmf_hinge.hip fills for WMRB, tmf_bpr.hip for BPR and tmf_warp.hip for WARP (an extension: the reference has no such
// loss; mf/loss_graphs.py SampledSoftmaxLoss is the definition).
//
// Inputs per user u: the sampled scores sp[u, 0..S) and, for its interactions k, the scores p_k and values a_k.  For a_k > 0
//     loss_k = -log( exp(p_k) / (exp(p_k) + c sum_s exp(sp[u, s])) )
// The log-sum-exp factorises per user: with M = max_s sp[u, s], e_s = exp(sp[u, s] - M), Z = sum_s e_s and per positive
//     m_k = max(p_k, M)     t_k = exp(M - m_k)     a_k = exp(p_k - m_k)     b_k = c Z t_k     den_k = a_k + b_k
//     loss_k  = log(den_k) + (m_k - p_k)
//     delta_k = -b_k / den_k                        D[u, s] = e_s C_u,   C_u = sum_k c t_k / den_k
// and delta_k = 0 for a_k <= 0.  No argument of an exponential is positive, and one of a_k, t_k is 1: den_k >= 1 when c Z >= 1.
// One exponential per (user, sample) and two per positive - 1e9 + 2e8 at C4 where the BPR step pays 1e11 - so the step is bound by
// the row it reads and the row it writes, not by the transcendental unit.
// Counted per user with P stored interactions: read 4 S bytes of sp (once while S <= XCAP; three times beyond, twice of them from the
// caches) + 8 P of val / p, write 4 S of D + 4 P of delta + 4; S + 2 P v_exp_f32, P logarithms, 3 P divisions and a handful of
// other vector operations per sample.  Measured at 1M users x 1024 samples: 1.72 ms = 4.8 TB/s of its 8.2 GB.
//
// One wave per user (tmf_hinge.hip: one user per workgroup was the fastest form there too).
//   row     lanes own samples, s = s0 + lane + 64 j: the first XCAP = 1024 samples stay in registers, 16 per lane, from the one read
//           to the D write; a longer row reads its other tiles again for Z and for D.  M by max (exact: any order), Z by
//           lane = its samples in ascending j, tile after tile, then one fixed xor butterfly over the lanes.
//   pairs   lanes own stored interactions, 64 per pass in CSR order: loss_k, delta_k (stored coalesced) and w_k = c t_k / den_k;
//           the pass's w by the same butterfly (zeros from the lanes without a positive), the passes added in ascending order: C_u.
//           loss_k into the lane's fp64 accumulator, one fixed butterfly per user at the end.
//   out     D[u, s] = e_s C_u from the registers (and the recomputed e_s of a longer row's other tiles), coalesced.
// No atomics: every sum has one order, a function of (S, the user's row) alone, so runs are bit-reproducible whatever the user order,
// the occupancy or the timing.  A user without a value > 0 gets zeros in its D row and loss_part whatever its scores are.
// log(den) = log(fl(hi + lo)) + (lo - (fl(hi + lo) - hi)) / fl(hi + lo) with hi, lo the larger and the smaller of a_k, b_k: the second
// term gives back what the rounding of the sum took (tmf_bpr.hip's log1p), so a positive ranked far above every sample costs b_k,
// not 0.  exp(x) = exp2(h) (1 + l ln 2) with h + l = x log2(e) to 48 bits: an argument of -100 costs no more than one near 0.
// A NaN or an infinity among a user's scores may make that user's outputs non-finite (a sample of -inf alone does not: e_s = 0);
// no other user reads them.
//
// The logQ correction (tmf_softmax_pairs_offset): the same body on x_s = sp[u, s] - off[u, s], off[u, s] = the log of how often the
// sampler proposes the item in slot s - a table built once per negative table by tmf_slot_offsets (off[j] = ell[R[j]]), because the
// gather it replaces would move a 128-byte line per 4-byte offset in every epoch.  The pair step reads it as a third
// coalesced stream beside sp and D: 12 S bytes per user where the plain step moves 8 S.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int XSPL = 16;                // samples per lane and tile
constexpr int XCAP = 64 * XSPL;         // samples of a tile; tile 0 is the register-resident part of a row
constexpr int XCHUNK = 64;              // stored interactions per pass: one per lane

// exp(x) for x <= 0 (NaN stays NaN; -inf and everything below the normal range give 0)
__device__ __forceinline__ float exp_nonpos(float x) {
    constexpr float kLog2eHi = 1.4426950216293335f, kLog2eLo = 1.9259629911266175e-8f, kLn2 = 0.6931471805599453f;
    const float h = __fmul_rn(x, kLog2eHi);
    float l = fmaf(x, kLog2eLo, fmaf(x, kLog2eHi, -h));    // what the rounding of h took, and the rest of log2(e)
    l = (h == -INFINITY) ? 0.f : l;                        // -inf - (-inf)
    return __builtin_amdgcn_exp2f(h) * fmaf(l, kLn2, 1.0f);
}

__device__ __forceinline__ float wave_sum_f32(float v) {   // fixed butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The scores of tile s0 (-inf beyond the row) and the largest of the lane's.  OFF: the corrected scores sp[u, s] - off[u, s], one
// fp32 subtraction each; both streams' loads of the tile are in flight together (offu is not read otherwise)
template <bool OFF>
__device__ __forceinline__ float softmax_load_tile(const float* __restrict__ spu, const float* __restrict__ offu, int64_t s0, int S,
                                                   int lane, float (&x)[XSPL]) {
#pragma unroll
    for (int j = 0; j < XSPL; ++j) {                       // the loads of a tile are in flight together
        const int64_t s = s0 + lane + 64 * j;
        x[j] = (s < S) ? spu[s] : -INFINITY;
    }
    if constexpr (OFF) {
        float o[XSPL];
#pragma unroll
        for (int j = 0; j < XSPL; ++j) {
            const int64_t s = s0 + lane + 64 * j;
            o[j] = (s < S) ? offu[s] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < XSPL; ++j) x[j] = __fsub_rn(x[j], o[j]);
    }
    float mx = x[0];
#pragma unroll
    for (int j = 1; j < XSPL; ++j) mx = fmaxf(mx, x[j]);
    return mx;
}

// x[j] -> e = exp(x[j] - M) in place; returns the lane's sum of them in ascending j
__device__ __forceinline__ float softmax_exps(float (&x)[XSPL], float M) {
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < XSPL; ++j) {
        x[j] = exp_nonpos(x[j] - M);
        z += x[j];
    }
    return z;
}

__device__ __forceinline__ void softmax_store_tile(float* __restrict__ Du, int64_t s0, int S, int lane, const float (&e)[XSPL], float C) {
#pragma unroll
    for (int j = 0; j < XSPL; ++j) {
        const int64_t s = s0 + lane + 64 * j;
        if (s < S) Du[s] = e[j] * C;
    }
}

// OFF = false: the plain step (off is not read).  OFF = true: the same step on x_s = sp[u, s] - off[u, s] - M, e_s, Z and D are those
// of the corrected scores; p_k stays raw.
template <bool OFF>
__global__ __launch_bounds__(64) void k_softmax_pairs(const int64_t* __restrict__ rowptr, const float* __restrict__ val,
                                                      const float* __restrict__ p, const float* __restrict__ sp,
                                                      const float* __restrict__ off, int S, float c, int64_t n_users,
                                                      float* __restrict__ delta, float* __restrict__ D,
                                                      float* __restrict__ loss_part, const int32_t* __restrict__ order) {
    const int lane = threadIdx.x;
    const int64_t slot = blockIdx.x;
    if (slot >= n_users) return;
    // `order` (optional): the users in the order the waves should take them, the heavy ones first (tmf_hinge.hip).  Every user is
    // computed by itself; the order changes no result.
    const int64_t u = order ? (int64_t)order[slot] : slot;
    const int64_t rb = rowptr[u], re = rowptr[u + 1];
    const float* spu = sp + u * (int64_t)S;
    const float* offu = OFF ? off + u * (int64_t)S : nullptr;
    float* Du = D + u * (int64_t)S;

    if (rb == re) {                                        // nothing stored: the row is not read
        for (int64_t s = lane; s < S; s += 64) Du[s] = 0.f;
        if (lane == 0 && loss_part) loss_part[u] = 0.f;
        return;
    }

    // ---- the row: M, e_s, Z ----
    float e[XSPL];                                         // tile 0: scores, then e_s, until the D write
    float mx = softmax_load_tile<OFF>(spu, offu, 0, S, lane, e);
    for (int64_t s0 = XCAP; s0 < S; s0 += XCAP) {
        float y[XSPL];
        mx = fmaxf(mx, softmax_load_tile<OFF>(spu, offu, s0, S, lane, y));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const float M = mx;
    float z = softmax_exps(e, M);
    for (int64_t s0 = XCAP; s0 < S; s0 += XCAP) {
        float y[XSPL];
        (void)softmax_load_tile<OFF>(spu, offu, s0, S, lane, y);
        z += softmax_exps(y, M);                           // tile after tile
    }
    const float cZ = c * wave_sum_f32(z);

    // ---- the pairs: lanes own stored interactions ----
    float C = 0.f;
    double lacc = 0.0;
    bool any_pos = false;                                  // wave-uniform
    for (int64_t cb = rb; cb < re; cb += XCHUNK) {
        const bool have = cb + lane < re;
        const bool pos = have && val[cb + lane] > 0.f;
        any_pos = any_pos || __builtin_amdgcn_ballot_w64(pos) != 0;
        float dk = 0.f, w = 0.f;
        if (pos) {
            const float pk = p[cb + lane];
            const float m = fmaxf(pk, M);
            const float t = exp_nonpos(M - m), a = exp_nonpos(pk - m);
            const float b = cZ * t;
            const float hi = (b > a) ? b : a, lo = (b > a) ? a : b;   // not fmaxf / fminf: they would drop a NaN
            const float den = hi + lo;
            dk = -(b / den);
            w = (c * t) / den;
            lacc += (double)((logf(den) + (lo - (den - hi)) / den) + (m - pk));
        }
        if (have) delta[cb + lane] = dk;
        C += wave_sum_f32(w);                              // the passes in ascending order
    }

    // ---- D[u, s] = e_s C_u ----
    if (!any_pos) {                                        // only values <= 0: zeros whatever the scores are (lacc is 0)
        for (int64_t s = lane; s < S; s += 64) Du[s] = 0.f;
        if (lane == 0 && loss_part) loss_part[u] = 0.f;
        return;
    }
    softmax_store_tile(Du, 0, S, lane, e, C);
    for (int64_t s0 = XCAP; s0 < S; s0 += XCAP) {
        float y[XSPL];
        (void)softmax_load_tile<OFF>(spu, offu, s0, S, lane, y);
        (void)softmax_exps(y, M);
        softmax_store_tile(Du, s0, S, lane, y, C);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lacc += __shfl_xor(lacc, off, 64);  // fixed butterfly: every lane ends with the same bits
    if (lane == 0 && loss_part) loss_part[u] = (float)lacc;
}

constexpr int kSoThreads = 256;
constexpr unsigned kSoBlocks = 16384;          // grid-stride workgroups (64 per CU), as tmf_item_bias_add

static inline bool so_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// off[j] = ell[R[j]] over the flat table - n4 int4 / float4 pieces when both are 16-byte aligned (VEC), the elements behind the last
// whole piece (or all of them) one by one: k_item_bias_add's walk with a store where it adds.
template <bool VEC>
__global__ __launch_bounds__(kSoThreads) void k_slot_offsets(const float* __restrict__ ell, const int32_t* __restrict__ R,
                                                             float* __restrict__ off, int64_t total) {
    const int64_t gid = (int64_t)blockIdx.x * kSoThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kSoThreads;
    int64_t done = 0;
    if constexpr (VEC) {
        const int64_t n4 = total / 4;
        const int4* R4 = reinterpret_cast<const int4*>(R);
        float4* off4 = reinterpret_cast<float4*>(off);
        for (int64_t i = gid; i < n4; i += stride) {
            const int4 id = R4[i];
            float4 v;
            v.x = ell[id.x];
            v.y = ell[id.y];
            v.z = ell[id.z];
            v.w = ell[id.w];
            off4[i] = v;
        }
        done = 4 * n4;
    }
    for (int64_t j = done + gid; j < total; j += stride) off[j] = ell[R[j]];
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_softmax_pairs(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users,
                                 int32_t n_samples, float c, float* delta, float* D, float* loss_part, const int32_t* user_order,
                                 void* stream) {
    if (n_users == 0) return TMF_OK;
    // val, p and delta are read only where a row has entries: a table without interactions may pass NULL for them
    TMF_REQUIRE(rowptr && sp && D && n_users > 0 && n_samples > 0, "softmax_pairs: bad arguments");
    TMF_REQUIRE_LAUNCH(n_users, 64, "tmf_softmax_pairs");
    hipLaunchKernelGGL(k_softmax_pairs<false>, dim3((unsigned)n_users), dim3(64), 0, (hipStream_t)stream, rowptr, val, p, sp,
                       (const float*)nullptr, (int)n_samples, c, (int64_t)n_users, delta, D, loss_part, user_order);
    return check_launch("tmf_softmax_pairs");
}

extern "C" int tmf_softmax_pairs_offset(const int64_t* rowptr, const float* val, const float* p, const float* sp, const float* off,
                                        int32_t n_users, int32_t n_samples, float c, float* delta, float* D, float* loss_part,
                                        const int32_t* user_order, void* stream) {
    TMF_REQUIRE(n_users >= 0 && n_samples >= 0, "softmax_pairs_offset: n_users=%d n_samples=%d", n_users, n_samples);
    if (n_users == 0) return TMF_OK;
    TMF_REQUIRE(rowptr && sp && off && D && n_samples > 0, "softmax_pairs_offset: bad arguments");
    TMF_REQUIRE_LAUNCH(n_users, 64, "tmf_softmax_pairs_offset");
    hipLaunchKernelGGL(k_softmax_pairs<true>, dim3((unsigned)n_users), dim3(64), 0, (hipStream_t)stream, rowptr, val, p, sp, off,
                       (int)n_samples, c, (int64_t)n_users, delta, D, loss_part, user_order);
    return check_launch("tmf_softmax_pairs_offset");
}

// off[j] = ell[R[j]] over the flat [n_users * n_samples] table: the slot offsets of a logQ-corrected fit, once per table
extern "C" int tmf_slot_offsets(const float* ell, int32_t n_items, const int32_t* R, int64_t n_users, int32_t n_samples, float* off,
                                void* stream) {
    TMF_REQUIRE(n_items >= 0 && n_users >= 0 && n_samples >= 0, "slot_offsets: n_items=%d n_users=%lld n_samples=%d", n_items,
                (long long)n_users, n_samples);
    const int64_t total = n_users * (int64_t)n_samples;
    if (total == 0) return TMF_OK;
    TMF_REQUIRE(ell != nullptr && n_items > 0, "slot_offsets: samples without a table of offsets (n_items=%d)", n_items);
    TMF_REQUIRE(R && off, "slot_offsets: null R / off for %lld samples", (long long)total);
    TMF_REQUIRE(so_aligned(ell, 4) && so_aligned(R, 4) && so_aligned(off, 4), "slot_offsets: a pointer is not 4-byte aligned");
    const bool vec = total >= 4 && so_aligned(R, 16) && so_aligned(off, 16);
    const int64_t work = vec ? total / 4 : total;
    const int64_t want = (work + kSoThreads - 1) / kSoThreads;
    const unsigned blocks = (unsigned)(want < (int64_t)kSoBlocks ? want : kSoBlocks);
    if (vec) {
        hipLaunchKernelGGL(k_slot_offsets<true>, dim3(blocks), dim3(kSoThreads), 0, (hipStream_t)stream, ell, R, off, total);
    } else {
        hipLaunchKernelGGL(k_slot_offsets<false>, dim3(blocks), dim3(kSoThreads), 0, (hipStream_t)stream, ell, R, off, total);
    }
    return check_launch("tmf_slot_offsets");
}
