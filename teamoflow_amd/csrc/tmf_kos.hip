// The weights of KOSWARPLoss (mf/loss_graphs.py is the definition; an extension modelled on LightFM's 'warp-kos', the k-th order
// statistic loss of Weston, Yee and Weiss): omega[j] = the probability that the k'-th best of n' uniform draws with replacement
// from the user's P stored positives is entry j.  tmf_warp_pairs_kos (tmf_warp.hip) multiplies WARP's weight by it.
//
// Per user u, over its stored entries with a value > 0 (P of them, duplicates as often as they are stored), with scores p_j:
//     a_j = #{i : p_i > p_j}      b_j = #{i : p_i >= p_j}      (a NaN orders below -inf and ties with the other NaNs; -0 == +0)
//     n' = min(n, P)   k' = min(k, n')   B(q) = sum_{i < k'} C(n', i) q^i (1 - q)^(n' - i)      B(0) = 1 and B(1) = 0 exactly
//     omega_j = (B(a_j / P) - B(b_j / P)) / (b_j - a_j)          and omega_j = 0 for a stored value <= 0
// B in fp64, omega rounded to fp32 once (never below zero).  The scores are compared as 32-bit keys whose unsigned order is the
// order above: the counts are exactly the definition's.
//
// One wave per user.  The keys of the positives go into LDS, KCAP at a time, and are sorted descending by a bitonic network over
// the next power of two (pads are the lowest key and stay behind the real ones).  Lanes own stored entries, 64 at a time in CSR
// order, and find their counts by branch-free bisections in the sorted keys.
//   P <= KCAP   one segment: a_j and b_j by two bisections, omega_j straight into the entry's slot.
//   P > KCAP    the row is taken segment by segment of KCAP positives.  Every entry adds the number of keys above its own in each
//               sorted segment; the running count lives in the entry's own omega slot (as ~a: the sign bit says "not yet a
//               weight"), read and written by the lane that owns it.  Then b_j: the entries of a tie block share a_j and the next
//               block's a is a_j + its size, so b_j = the smallest a present above a_j, or P.  The rank range [0, P) is walked in
//               windows of KCAP ranks from the top down: the entries whose a falls into the window mark it in LDS (equal values
//               write the same word), a suffix minimum over the marks (carried from window to window) gives every rank its
//               successor, and those entries get their weight.  Cost: P / KCAP segments and as many windows, each a walk of the
//               row - (P / KCAP) (L / 64) steps for a row of L entries, KU chunks in flight together (DESIGN.md has the figures).
// Every slot of omega is written once the kernel has run; the outputs depend on the row alone, never on user_order, occupancy or
// timing.  No atomics; plain vector stores only.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int KCAP = 2048;              // keys of a segment: 4 bytes of LDS each, 8 KB per wave
constexpr int KCHUNK = 64;              // stored interactions per pass: one per lane
constexpr int KOS_MAX_N = 64;           // n <= 64 draws
constexpr int KU = 4;                   // chunks of a long row in flight together: its walks are chains of dependent reads

// The key of a score: unsigned order = the definition's order.  NaN -> 0, below -inf; -0 and +0 share a key.
__device__ __forceinline__ uint32_t kos_key(float x) {
    if (!(x == x)) return 0u;
    if (x == 0.f) x = 0.f;
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Sorts K[0, npad) descending: npad a power of two >= 64, the whole wave calls it.
__device__ __forceinline__ void kos_sort_desc(uint32_t* K, int npad, int lane) {
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (npad >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));       // bit j of i is clear
                const uint32_t x = K[i], y = K[i + j];
                const bool desc = (i & k) == 0;
                if (desc ? (x < y) : (x > y)) {
                    K[i] = y;
                    K[i + j] = x;
                }
            }
            wave_lds_sync();
        }
    }
}

// The number of keys of the sorted segment K[0, len) above x (STRICT) or not below it: the first place whose key is not.
template <bool STRICT>
__device__ __forceinline__ int kos_count(const uint32_t* K, int len, int top, uint32_t x) {
    int lo = 0;
    for (int b = top; b > 0; b >>= 1) {
        const int at = lo + b;
        const uint32_t m = K[(at <= len ? at : len) - 1];
        lo = (at <= len && (STRICT ? (m > x) : (m >= x))) ? at : lo;
    }
    return lo;
}

// kos_count<STRICT> for KU keys at once: the KU chains of LDS reads overlap.
template <bool STRICT>
__device__ __forceinline__ void kos_count_ku(const uint32_t* K, int len, int top, const uint32_t (&x)[KU], int (&lo)[KU]) {
#pragma unroll
    for (int j = 0; j < KU; ++j) lo[j] = 0;
    for (int b = top; b > 0; b >>= 1) {
#pragma unroll
        for (int j = 0; j < KU; ++j) {
            const int at = lo[j] + b;
            const uint32_t m = K[(at <= len ? at : len) - 1];
            lo[j] = (at <= len && (STRICT ? (m > x[j]) : (m >= x[j]))) ? at : lo[j];
        }
    }
}

// B(c / P) in fp64: c of the P positives stand above.  ctop = C(n', k' - 1).  The end points are exact by definition; between
// them every term is positive: sum_{i < k'} C(n', i) q^i r^(k' - 1 - i), Horner from the top, times r^(n' - k' + 1).
__device__ __forceinline__ double kos_B(int c, int P, int np, int kp, double ctop) {
    if (c <= 0) return 1.0;
    if (c >= P) return 0.0;
    const double q = (double)c / (double)P, r = (double)(P - c) / (double)P;
    double h = ctop, cb = ctop, rp = 1.0;
    for (int i = kp - 2; i >= 0; --i) {
        cb = cb * (double)(i + 1) / (double)(np - i);                      // C(n', i) from C(n', i + 1)
        rp *= r;
        h = h * q + cb * rp;
    }
    for (int e = np - kp + 1; e > 0; --e) h *= r;
    return h;
}

__device__ __forceinline__ float kos_omega(int a, int b, int P, int np, int kp, double ctop) {
    const double w = (kos_B(a, P, np, kp, ctop) - kos_B(b, P, np, kp, ctop)) / (double)(b - a);
    return w > 0.0 ? (float)w : 0.f;
}

// Segment `seg` of the row's positives (those with ordinal in [seg KCAP, (seg + 1) KCAP)) into K, in CSR order; -> P, the number of
// positives of the whole row.
__device__ __forceinline__ int64_t kos_load_segment(const float* __restrict__ val, const float* __restrict__ p, int64_t rb, int64_t re,
                                                    int64_t seg, uint32_t* K, int lane) {
    int64_t seen = 0;
    const int64_t first = seg * KCAP;
    for (int64_t cb = rb; cb < re; cb += KCHUNK) {
        const bool have = cb + lane < re;
        const bool pos = have && val[cb + lane] > 0.f;
        const uint64_t mask = __builtin_amdgcn_ballot_w64(pos);
        const int64_t ord = seen + __builtin_popcountll(mask & ((1ull << lane) - 1ull)) - first;
        if (pos && ord >= 0 && ord < KCAP) K[ord] = kos_key(p[cb + lane]);
        seen += __builtin_popcountll(mask);
    }
    return seen;
}

// The same for a later segment of a long row: by then every positive's slot holds a count (sign bit set), every other slot +0.
// KU chunks are read together, and the walk ends with the segment.
__device__ __forceinline__ void kos_load_later_segment(const int32_t* slots, const float* __restrict__ p, int64_t rb, int64_t re,
                                                       int64_t seg, uint32_t* K, int lane) {
    int64_t seen = 0;
    const int64_t first = seg * KCAP;
    for (int64_t cb = rb; cb < re && seen < first + KCAP; cb += KCHUNK * KU) {
        int32_t v[KU];
#pragma unroll
        for (int j = 0; j < KU; ++j) {
            const int64_t e = cb + KCHUNK * j + lane;
            v[j] = (e < re) ? slots[e] : 0;
        }
#pragma unroll
        for (int j = 0; j < KU; ++j) {
            const bool pos = v[j] < 0;
            const uint64_t mask = __builtin_amdgcn_ballot_w64(pos);
            const int64_t ord = seen + __builtin_popcountll(mask & ((1ull << lane) - 1ull)) - first;
            if (pos && ord >= 0 && ord < KCAP) K[ord] = kos_key(p[cb + KCHUNK * j + lane]);
            seen += __builtin_popcountll(mask);
        }
    }
}

__global__ __launch_bounds__(64) void k_kos_weights(const int64_t* __restrict__ rowptr, const float* __restrict__ val,
                                                    const float* __restrict__ p, int64_t n_users, int k, int n,
                                                    float* __restrict__ omega, const int32_t* __restrict__ order) {
    __shared__ uint32_t K[KCAP];
    const int lane = threadIdx.x;
    const int64_t slot = blockIdx.x;
    if (slot >= n_users) return;
    // `order` (optional): the users in the order the waves should take them, the heavy ones first (tmf_hinge.hip).  Every user is
    // computed by itself; the order changes no result.
    const int64_t u = order ? (int64_t)order[slot] : slot;
    const int64_t rb = rowptr[u], re = rowptr[u + 1];
    if (re <= rb) return;

    const int64_t P64 = kos_load_segment(val, p, rb, re, 0, K, lane);
    if (P64 == 0) {
        for (int64_t e = rb + lane; e < re; e += 64) omega[e] = 0.f;
        return;
    }
    const int P = (int)P64;             // entries of one table: < 2^31
    const int np = n < P ? n : P, kp = k < np ? k : np;
    double ctop = 1.0;                  // C(n', k' - 1)
    for (int i = 0; i < kp - 1; ++i) ctop = ctop * (double)(np - i) / (double)(i + 1);

    if (P <= KCAP) {
        int npad = 64;
        while (npad < P) npad <<= 1;
        for (int i = P + lane; i < npad; i += 64) K[i] = 0u;
        wave_lds_sync();
        kos_sort_desc(K, npad, lane);
        int top = 1;                    // the largest power of two <= P
        while (2 * top <= P) top *= 2;
        for (int64_t cb = rb; cb < re; cb += KCHUNK) {
            const bool have = cb + lane < re;
            const bool pos = have && val[cb + lane] > 0.f;
            const uint32_t x = pos ? kos_key(p[cb + lane]) : 0u;
            const int a = kos_count<true>(K, P, top, x), b = kos_count<false>(K, P, top, x);
            if (have) omega[cb + lane] = pos ? kos_omega(a, b, P, np, kp, ctop) : 0.f;
        }
        return;
    }

    // ---- a long row, part 1: a_j summed over the sorted segments, kept as ~a_j in the entry's slot ----
    // (every access of this path goes through one integer view of omega: counts and weights change places in the same words)
    int32_t* slots = reinterpret_cast<int32_t*>(omega);
    const int64_t n_seg = (P64 + KCAP - 1) / KCAP;
    for (int64_t seg = 0; seg < n_seg; ++seg) {
        if (seg > 0) {
            wave_lds_sync();            // the walk over the last segment has read K
            kos_load_later_segment(slots, p, rb, re, seg, K, lane);
        }
        const int len = (int)((P64 - seg * KCAP < KCAP) ? (P64 - seg * KCAP) : KCAP);
        for (int i = len + lane; i < KCAP; i += 64) K[i] = 0u;
        wave_lds_sync();
        kos_sort_desc(K, KCAP, lane);
        int top = 1;
        while (2 * top <= len) top *= 2;
        for (int64_t cb = rb; cb < re; cb += KCHUNK * KU) {
            int32_t v[KU];              // < 0: a positive, ~v the keys above it so far
            uint32_t x[KU];
            int above[KU];
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                const int64_t e = cb + KCHUNK * j + lane;
                const bool have = e < re;
                v[j] = !have ? 0 : seg ? slots[e] : (val[e] > 0.f ? ~0 : 0);
                x[j] = have ? kos_key(p[e]) : 0u;
            }
            kos_count_ku<true>(K, len, top, x, above);
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                const int64_t e = cb + KCHUNK * j + lane;
                if (v[j] < 0) slots[e] = ~(~v[j] + above[j]);
                else if (e < re && seg == 0) slots[e] = 0;               // +0.f
            }
        }
    }
    // ---- part 2: b_j = the smallest a present above a_j (or P), by windows of KCAP ranks from the top down ----
    int32_t* N = reinterpret_cast<int32_t*>(K);
    int32_t carry = P;                  // the smallest a present above the window (wave-uniform)
    for (int64_t wb = (n_seg - 1) * KCAP; wb >= 0; wb -= KCAP) {
        const int wlen = (int)((P64 - wb < KCAP) ? (P64 - wb) : KCAP);
        wave_lds_sync();                // the last window's entries have read N
        for (int i = lane; i < wlen; i += 64) N[i] = 0x7fffffff;
        wave_lds_sync();
        for (int64_t cb = rb; cb < re; cb += KCHUNK * KU) {
            int32_t v[KU];
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                const int64_t e = cb + KCHUNK * j + lane;
                v[j] = (e < re) ? slots[e] : 0;
            }
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                const int64_t at = (int64_t)(~v[j]) - wb;                // v < 0: still a count
                if (v[j] < 0 && at >= 0 && at < wlen) N[at] = ~v[j];     // the entries of a tie block write the same value
            }
        }
        wave_lds_sync();
        const int32_t carry_in = carry;
        for (int t0 = ((wlen - 1) / 64) * 64; t0 >= 0; t0 -= 64) {       // suffix minimum, tiles from the top down
            const int i = t0 + lane;
            int32_t m = (i < wlen) ? N[i] : 0x7fffffff;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int32_t o = __shfl_down(m, off, 64);
                if (lane + off < 64) m = o < m ? o : m;
            }
            m = m < carry ? m : carry;
            if (i < wlen) N[i] = m;
            carry = __builtin_amdgcn_readlane(m, 0);
        }
        wave_lds_sync();
        for (int64_t cb = rb; cb < re; cb += KCHUNK * KU) {
            int32_t v[KU];
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                const int64_t e = cb + KCHUNK * j + lane;
                v[j] = (e < re) ? slots[e] : 0;
            }
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                const int64_t at = (int64_t)(~v[j]) - wb;
                if (v[j] < 0 && at >= 0 && at < wlen) {
                    const int a = ~v[j];
                    const int b = (at + 1 < wlen) ? N[at + 1] : carry_in;
                    slots[cb + KCHUNK * j + lane] = __float_as_int(kos_omega(a, b, P, np, kp, ctop));
                }
            }
        }
    }
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_kos_weights(const int64_t* rowptr, const float* val, const float* p, int32_t n_users, int32_t k, int32_t n,
                               float* omega, const int32_t* user_order, void* stream) {
    TMF_REQUIRE(n_users >= 0 && k >= 1 && k <= n && n <= KOS_MAX_N, "tmf_kos_weights: bad arguments (1 <= k <= n <= %d)", KOS_MAX_N);
    if (n_users == 0) return TMF_OK;
    // val, p and omega are read and written only where a row has entries: a table without interactions may pass NULL for them
    TMF_REQUIRE(rowptr, "tmf_kos_weights: bad arguments");
    TMF_REQUIRE_LAUNCH(n_users, 64, "tmf_kos_weights");
    hipLaunchKernelGGL(k_kos_weights, dim3((unsigned)n_users), dim3(64), 0, (hipStream_t)stream, rowptr, val, p, (int64_t)n_users,
                       (int)k, (int)n, omega, user_order);
    return check_launch("tmf_kos_weights");
}
