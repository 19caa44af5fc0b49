// DCG@k and IDCG@k of a graded test table without the [m, n] scores (matrix_factorization.py:320-413 on a sparse table).
//
// Row u of the test table is a CSR row: distinct item ids ascending, their gains 2^a - 1 (stored entries only; every other eligible
// item has gain 0).  DCG@k(u) = sum_j gain(u, top[u, j]) / den[j] over the user's top-k list (-1 slots count nothing); IDCG@k(u) =
// sum_j g_(j) / den[j] over the k largest values of the multiset {stored gains} + n_zero[u] zeros.  Every sum runs over the slots in
// order, slot 0 first, so a call is deterministic and each per-slot term is the IEEE quotient the dense path forms.
//
// A wave owns a user.  Rows of at most 64 stored gains sit one per lane: the list ids are matched against the lanes' item ids with
// shuffles, and the ideal order is each lane's rank in the row (one compare per stored entry), the implicit zeros put in front of
// the negative gains.  Longer rows take the whole workgroup for their IDCG: a radix select (four 8-bit passes over the row, LDS
// histograms) finds the key at the last slot of a round of at most ND_ROUND slots; only the gains strictly between it and the
// previous round's last value need sorting (bitonic, in LDS) - the copies of the two boundary values are counted.  The DCG of a long
// row binary-searches the list ids in the row.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int ND_THREADS = 256;        // four waves
constexpr int ND_WAVES = ND_THREADS / 64;
constexpr int ND_LIGHT = 64;           // rows up to this many stored gains: one per lane
constexpr int ND_ROUND = 1024;         // slots placed per round of the long-row IDCG
constexpr int ND_MAX_BLOCKS = 4096;    // workgroups of a launch (each loops over groups of ND_WAVES users)

// Gain as an order-preserving key: a > b  <=>  key(a) > key(b); -0 is keyed as +0.
__device__ __forceinline__ unsigned gain_key_nd(float g) {
    unsigned u = __float_as_uint(g);
    if (u == 0x80000000u) u = 0u;
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_gain_nd(unsigned o) { return __uint_as_float((o >> 31) ? (o ^ 0x80000000u) : ~o); }
constexpr unsigned kZeroKeyNd = 0x80000000u;   // gain_key_nd(0.0f)
constexpr uint64_t kNoKeyNd = 1ull << 32;      // above every key

struct NdcgArgs {
    const int64_t* rowptr;
    const int32_t* cols;
    const float* gain;
    int64_t m, n_items;
    const int32_t* top;      // [m, ldt] or NULL
    int64_t ldt;
    int k;
    const float* den;        // [k]
    const int64_t* n_zero;   // [m] or NULL = n_items - stored
    float* dcg;              // [m] or NULL
    float* idcg;             // [m] or NULL
};

__device__ __forceinline__ int64_t zeros_of(const NdcgArgs& a, int64_t u, int64_t s) {
    const int64_t z = a.n_zero ? a.n_zero[u] : a.n_items - s;
    return z > 0 ? z : 0;
}

// DCG of user u by its wave.  Short rows: lane i < s holds stored entry i (col_l, g_l).
__device__ float wave_dcg(const NdcgArgs& a, int64_t u, int64_t lo, int64_t s, int lane, int col_l, float g_l) {
    float sum = 0.0f;
    for (int base = 0; base < a.k; base += 64) {
        const int j = base + lane;
        const int id = j < a.k ? a.top[u * a.ldt + j] : -1;
        float g = 0.0f;
        bool hit = false;
        if (s <= ND_LIGHT) {   // wave-uniform: every lane takes part in the shuffles
            for (int i = 0; i < (int)s; ++i) {
                const int c = __shfl(col_l, i);
                const float gi = __shfl(g_l, i);
                if (id >= 0 && c == id) { g = gi; hit = true; }
            }
        } else if (id >= 0) {
            int64_t l = 0, h = s;   // first stored id >= id
            while (l < h) {
                const int64_t mid = (l + h) >> 1;
                if (a.cols[lo + mid] < id) l = mid + 1; else h = mid;
            }
            if (l < s && a.cols[lo + l] == id) { g = a.gain[lo + l]; hit = true; }
        }
        const float t = hit ? g / a.den[j] : 0.0f;   // hit implies j < k
        const int cnt = a.k - base < 64 ? a.k - base : 64;
        for (int q = 0; q < cnt; ++q) sum += __shfl(t, q);
    }
    return sum;
}

// IDCG of a row of s <= 64 stored gains by its wave: lane i < s holds gain i, lane l < k holds den[l].
__device__ float wave_idcg(const NdcgArgs& a, int64_t s, int64_t z, int lane, float g_l, float den_l) {
    const int64_t total = s + z;
    const int64_t kk = total < a.k ? total : a.k;
    const bool mine = lane < s;
    const unsigned key = mine ? gain_key_nd(g_l) : 0u;
    int rank = 0;   // among the stored gains: the larger ones, then the equal ones of lower lanes
    for (int i = 0; i < (int)s; ++i) {
        const unsigned ki = __shfl(key, i);
        rank += (ki > key || (ki == key && i < lane)) ? 1 : 0;
    }
    const int64_t slot = rank + (key < kZeroKeyNd ? z : 0);   // negative gains go behind the implicit zeros
    const float d = __shfl(den_l, slot < 64 ? (int)slot : 0);
    float t = 0.0f;
    if (mine && slot < kk) t = g_l / (slot < 64 ? d : a.den[slot]);
    float sum = 0.0f;
    for (int r = 0; r < (int)s; ++r) {   // slot order = stored-rank order (ranks are a permutation of 0 .. s - 1)
        const uint64_t b = __ballot(mine && rank == r);
        sum += __shfl(t, (int)__builtin_ctzll(b));
    }
    return sum;
}

struct NdLds {
    unsigned keys[2 * ND_ROUND];   // a round's keys (the sorted middle padded to a power of two), then its terms as float bits
    unsigned hist[256];
    int sel[4];                    // [0] selected bin, [1] candidates above it, [2] unused, [3] collect cursor
};

// Radix select over the candidates {stored keys < ub} + (z zeros when kZeroKeyNd < ub): the key at rank `target` (0 = the
// largest; target < the number of candidates).  *above = candidates greater than it, *equal = candidates equal to it.
__device__ unsigned wg_select(const NdcgArgs& a, NdLds& sh, int64_t lo, int64_t s, int64_t z, uint64_t ub, int64_t target,
                              int64_t* above, int64_t* equal) {
    const int tid = threadIdx.x;
    unsigned prefix = 0;
    int64_t gt = 0, eq = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        __syncthreads();
        for (int b = tid; b < 256; b += ND_THREADS) sh.hist[b] = 0;
        if (tid == 0) sh.sel[0] = sh.sel[1] = 0;
        __syncthreads();
        int64_t i = tid;
        for (; i + 7 * ND_THREADS < s; i += 8 * ND_THREADS) {   // eight loads in flight per lane
            float g[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) g[t] = a.gain[lo + i + t * ND_THREADS];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const unsigned key = gain_key_nd(g[t]);
                if ((uint64_t)key < ub && (key & hi_mask) == (prefix & hi_mask)) atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
            }
        }
        for (; i < s; i += ND_THREADS) {
            const unsigned key = gain_key_nd(a.gain[lo + i]);
            if ((uint64_t)key < ub && (key & hi_mask) == (prefix & hi_mask)) atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0 && z > 0 && (uint64_t)kZeroKeyNd < ub && (kZeroKeyNd & hi_mask) == (prefix & hi_mask))
            sh.hist[(kZeroKeyNd >> shift) & 255u] += (unsigned)z;
        __syncthreads();
        if (tid < 64) {   // bins from the top: lane l scans 255 - 4l .. 252 - 4l after the counts of the lanes before it
            unsigned c[4];
            int64_t run = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) { c[t] = sh.hist[255 - 4 * tid - t]; run += c[t]; }
            int64_t incl = run;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int64_t o = __shfl_up(incl, off);
                if (tid >= off) incl += o;
            }
            int64_t acc = incl - run;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (acc <= target && target < acc + (int64_t)c[t]) {
                    sh.sel[0] = 255 - 4 * tid - t;
                    sh.sel[1] = (int)acc;   // acc <= target < ND_ROUND
                }
                acc += c[t];
            }
        }
        __syncthreads();
        const int bin = sh.sel[0];
        prefix |= (unsigned)bin << shift;
        target -= sh.sel[1];
        gt += sh.sel[1];
        eq = sh.hist[bin];
    }
    *above = gt;
    *equal = eq;
    return prefix;
}

// IDCG of a long row by the whole workgroup; the result is valid in thread 0.
__device__ float wg_idcg(const NdcgArgs& a, NdLds& sh, int64_t lo, int64_t s, int64_t z) {
    const int tid = threadIdx.x;
    const int64_t total = s + z;
    const int64_t kk = total < a.k ? total : a.k;
    float sum = 0.0f;
    uint64_t prev = kNoKeyNd;   // the previous round's last key
    int64_t prev_left = 0;      // its copies not placed yet
    for (int64_t base = 0; base < kk; base += ND_ROUND) {
        const int width = (int)(kk - base < ND_ROUND ? kk - base : ND_ROUND);
        const int64_t q = width - 1;   // rank of the round's last slot among the candidates, the previous key's copies first
        int lead, mid = 0;             // [lead copies of prev][mid keys in (T, prev), sorted descending][copies of T]
        unsigned T;
        int64_t t_eq = 0;
        if (q < prev_left) {
            T = (unsigned)prev;
            lead = width;
        } else {
            lead = (int)prev_left;
            int64_t gt;
            T = wg_select(a, sh, lo, s, z, prev, q - prev_left, &gt, &t_eq);
            mid = (int)gt;   // gt <= q - prev_left
        }
        __syncthreads();
        if (tid == 0) sh.sel[3] = 0;
        __syncthreads();
        if (mid > 0) {
            unsigned* x = sh.keys + lead;   // lead + (mid rounded up to a power of two) < 2 * width
            for (int64_t i = tid; i < s; i += ND_THREADS) {
                const unsigned key = gain_key_nd(a.gain[lo + i]);
                if (key > T && (uint64_t)key < prev) {
                    const int p = atomicAdd(&sh.sel[3], 1);
                    if (p < mid) x[p] = key;
                }
            }
            __syncthreads();
            const int got = sh.sel[3] < mid ? sh.sel[3] : mid;
            if (kZeroKeyNd > T && (uint64_t)kZeroKeyNd < prev)   // the implicit zeros fall in this round: mid - got of them
                for (int i = got + tid; i < mid; i += ND_THREADS) x[i] = kZeroKeyNd;
            int p2 = 1;
            while (p2 < mid) p2 <<= 1;
            for (int i = mid + tid; i < p2; i += ND_THREADS) x[i] = 0u;   // padding sorts behind every key
            __syncthreads();
            for (int size = 2; size <= p2; size <<= 1) {
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int i = tid; i < p2; i += ND_THREADS) {
                        const int j = i ^ stride;
                        if (j > i) {
                            const bool desc = (i & size) == 0;
                            const unsigned xi = x[i], xj = x[j];
                            if (desc ? xi < xj : xi > xj) { x[i] = xj; x[j] = xi; }
                        }
                    }
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < width; i += ND_THREADS) {   // slot base + i
            const unsigned key = i < lead ? (unsigned)prev : (i < lead + mid ? sh.keys[i] : T);
            sh.keys[i] = __float_as_uint(key_gain_nd(key) / a.den[base + i]);
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < width; ++i) sum += __uint_as_float(sh.keys[i]);
        if (lead == width) {
            prev_left -= width;
        } else {
            prev_left = t_eq - (width - lead - mid);
            prev = T;
        }
    }
    return sum;
}

__global__ __launch_bounds__(ND_THREADS) void k_dcg_idcg(NdcgArgs a) {
    __shared__ NdLds sh;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float den_l = lane < a.k ? a.den[lane] : 1.0f;
    for (int64_t u0 = (int64_t)blockIdx.x * ND_WAVES; u0 < a.m; u0 += (int64_t)gridDim.x * ND_WAVES) {
        const int64_t u = u0 + w;
        if (u < a.m) {   // wave-uniform
            const int64_t lo = a.rowptr[u], s = a.rowptr[u + 1] - lo;
            int col_l = -1;
            float g_l = 0.0f;
            if (s <= ND_LIGHT && lane < s) { col_l = a.cols[lo + lane]; g_l = a.gain[lo + lane]; }
            if (a.dcg) {
                const float d = a.top ? wave_dcg(a, u, lo, s, lane, col_l, g_l) : 0.0f;
                if (lane == 0) a.dcg[u] = d;
            }
            if (a.idcg && s <= ND_LIGHT) {
                const float d = wave_idcg(a, s, zeros_of(a, u, s), lane, g_l, den_l);
                if (lane == 0) a.idcg[u] = d;
            }
        }
        if (!a.idcg) continue;
        for (int t = 0; t < ND_WAVES && u0 + t < a.m; ++t) {   // the group's long rows, one after the other (workgroup-uniform)
            const int64_t v = u0 + t;
            const int64_t lo = a.rowptr[v], s = a.rowptr[v + 1] - lo;
            if (s <= ND_LIGHT) continue;
            const float d = wg_idcg(a, sh, lo, s, zeros_of(a, v, s));
            if (threadIdx.x == 0) a.idcg[v] = d;
        }
    }
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_dcg_idcg_f32(const int64_t* rowptr, const int32_t* cols, const float* gain, int64_t m, int64_t n_items,
                                const int32_t* top, int64_t ldt, int k, const float* den, const int64_t* n_zero, float* dcg,
                                float* idcg, void* stream) {
    TMF_REQUIRE(m >= 0 && n_items >= 0 && n_items < ((int64_t)1 << 31) && k >= 1, "dcg_idcg_f32: bad arguments");
    if (m == 0 || (!dcg && !idcg)) return TMF_OK;
    TMF_REQUIRE(rowptr && cols && gain && den && (!dcg || top), "dcg_idcg_f32: rowptr, cols, gain, den (and top with dcg) are required");
    TMF_REQUIRE(!dcg || ldt >= k, "dcg_idcg_f32: ldt %lld < k %d", (long long)ldt, k);
    NdcgArgs a{rowptr, cols, gain, m, n_items, dcg ? top : nullptr, ldt, k, den, n_zero, dcg, idcg};
    const int64_t groups = (m + ND_WAVES - 1) / ND_WAVES;
    const int64_t blocks = groups < ND_MAX_BLOCKS ? groups : ND_MAX_BLOCKS;
    hipLaunchKernelGGL(k_dcg_idcg, dim3((unsigned)blocks), dim3(ND_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("tmf_dcg_idcg_f32");
}
