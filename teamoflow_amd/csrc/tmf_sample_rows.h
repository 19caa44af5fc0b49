// What the negative-table samplers share (tmf_sample.hip: uniform; tmf_sample_weighted.hip: weighted): counter_hash of mf/utils.py,
// the bitonic network and the row loop - draw, sort, redraw the repeats, shuffle, store.  The two kernels differ in one function,
// word -> item, and in the round at which a row that still holds a repeat fails.
//
// Shape: the row lives in LDS, padded to NPAD = the power of two >= max(S, 64) with a sentinel that sorts last - ids as 32-bit
// words, the 64-bit shuffle keys and their 16-bit positions beside them (14 bytes per element) - and is sorted by a bitonic network,
// one compare-exchange per thread and stage, a barrier between stages.  A workgroup holds T = max(NPAD, 256) elements: four rows
// at NPAD = 64 (one wave per user), two at 128, one from 256 on, with NPAD / 4 threads beyond 1024.  Every barrier is uniform over
// the workgroup: the redraw loop runs until NO row of the workgroup holds a repeat (__syncthreads_or), which costs a finished row
// nothing but a sort of a sorted row.  Each thread keeps the (user, pos) half of counter_hash for its EPT <= 4 places in registers,
// so a draw is one mix and the kernel's word -> item function.  No atomics; plain vector stores; the flag is written, never incremented.
#pragma once
#include "tmf_common.h"

namespace tmf {

constexpr int SR_MAX_SAMPLES = 4096;     // 14 bytes of LDS per element: 56 KB of the 64 KB a static allocation may take
constexpr int64_t SR_MAX_BLOCKS = 1 << 20;   // the workgroups stride the rest

__device__ __forceinline__ uint64_t sr_mix64(uint64_t x) {   // splitmix64's finaliser (utils._mix64)
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// counter_hash(seed, a, b, c) in its three steps: the caller keeps the first two
__device__ __forceinline__ uint64_t sr_hash_a(uint64_t seed_add, uint64_t a) { return sr_mix64(a + seed_add); }
__device__ __forceinline__ uint64_t sr_hash_b(uint64_t h, uint64_t b) { return sr_mix64(h ^ (b * 0xD6E8FEB86659FD93ull + 0xA0761D6478BD642Full)); }
__device__ __forceinline__ uint64_t sr_hash_c(uint64_t h, uint64_t c) { return sr_mix64(h ^ (c * 0xE7037ED1A0B428DBull + 0x8EBC6AF09C88C6E3ull)); }
// counter_hash's a + (2 seed + 1) * golden ratio: the part of the first step that every user shares
inline uint64_t sr_seed_add(int64_t seed) { return (2 * (uint64_t)seed + 1) * 0x9E3779B97F4A7C15ull; }

// One stage of the bitonic network over rows of NPAD elements laid end to end: pair p of T / 2, partner distance j, run length k.
// less(a, b): whether the element at a must stand before the one at b; swap(a, b) exchanges them.
template <int NPAD, int T, int THREADS, typename Less, typename Swap>
__device__ __forceinline__ void sr_sort(Less less, Swap swap) {
    for (int k = 2; k <= NPAD; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int p = threadIdx.x; p < T / 2; p += THREADS) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));   // bit j clear; rows are NPAD apart and j, k <= NPAD
                const int hi = lo | j;
                const bool up = (lo & k) == 0 || k == NPAD;              // the last merge sorts every row ascending
                if (up ? less(hi, lo) : less(lo, hi)) swap(lo, hi);
            }
            __syncthreads();
        }
    }
}

// The rows of one workgroup, for every stride of the grid.  item(w): the item of the random word w = counter_hash(seed, u, pos, c),
// c = 2 for the draw and c = rnd for the redraws of round rnd = 3 .. FAIL_ROUND; a row that still holds a repeat when round
// FAIL_ROUND begins sets *failed.
template <int NPAD, int THREADS, int FAIL_ROUND, typename Item>
__device__ __forceinline__ void sr_rows(Item item, int64_t n_users, int32_t S, uint64_t seed_add, int64_t user_offset,
                                        int32_t* __restrict__ R, int32_t* __restrict__ failed) {
    constexpr int T = NPAD < THREADS ? THREADS : NPAD;   // elements per workgroup
    constexpr int RPW = T / NPAD;                        // rows per workgroup
    constexpr int EPT = T / THREADS;                     // places per thread
    static_assert(T % NPAD == 0 && T % THREADS == 0 && EPT <= 4, "workgroup geometry");
    __shared__ uint64_t key[T];
    __shared__ uint32_t ids[T];
    __shared__ uint16_t ord[T];
    auto ids_less = [&](int a, int b) { return ids[a] < ids[b]; };
    auto ids_swap = [&](int a, int b) { const uint32_t t = ids[a]; ids[a] = ids[b]; ids[b] = t; };
    auto key_less = [&](int a, int b) { return key[a] < key[b] || (key[a] == key[b] && ord[a] < ord[b]); };
    auto key_swap = [&](int a, int b) {
        const uint64_t t = key[a]; key[a] = key[b]; key[b] = t;
        const uint16_t o = ord[a]; ord[a] = ord[b]; ord[b] = o;
    };
    for (int64_t base = (int64_t)blockIdx.x * RPW; base < n_users; base += (int64_t)gridDim.x * RPW) {   // uniform over the workgroup
        uint64_t h[EPT];   // counter_hash's state after (seed, user, pos) for this thread's places
#pragma unroll
        for (int v = 0; v < EPT; ++v) {
            const int e = threadIdx.x + v * THREADS, pos = e & (NPAD - 1);
            const uint64_t u = (uint64_t)(user_offset + base + e / NPAD);   // a row beyond n_users is computed and not stored
            h[v] = sr_hash_b(sr_hash_a(seed_add, u), (uint64_t)pos);
            ids[e] = pos < S ? item(sr_hash_c(h[v], 2)) : 0xFFFFFFFFu;
            key[e] = pos < S ? sr_hash_c(h[v], 0) >> 1 : ~0ull;   // real keys have 63 bits
            ord[e] = (uint16_t)pos;
        }
        __syncthreads();
        sr_sort<NPAD, T, THREADS>(ids_less, ids_swap);
        for (uint64_t rnd = 3; rnd <= FAIL_ROUND; ++rnd) {
            bool dup[EPT], any = false;
#pragma unroll
            for (int v = 0; v < EPT; ++v) {
                const int e = threadIdx.x + v * THREADS, pos = e & (NPAD - 1);
                dup[v] = pos > 0 && pos < S && ids[e] == ids[e - 1];
                any = any || dup[v];
            }
            if (rnd == FAIL_ROUND && any) *failed = 1;
            if (!__syncthreads_or(any)) break;   // also the barrier between the reads above and the writes below
#pragma unroll
            for (int v = 0; v < EPT; ++v)
                if (dup[v]) ids[threadIdx.x + v * THREADS] = item(sr_hash_c(h[v], rnd));
            __syncthreads();
            sr_sort<NPAD, T, THREADS>(ids_less, ids_swap);
        }
        sr_sort<NPAD, T, THREADS>(key_less, key_swap);
#pragma unroll
        for (int v = 0; v < EPT; ++v) {
            const int e = threadIdx.x + v * THREADS, pos = e & (NPAD - 1), row = e / NPAD;
            if (pos < S && base + row < n_users) R[(base + row) * (int64_t)S + pos] = (int32_t)ids[row * NPAD + ord[e]];
        }
        __syncthreads();   // the next rows overwrite what the stores above read
    }
}

// workgroups of a launch of K<NPAD, THREADS> over n_users rows
template <int NPAD, int THREADS>
inline int64_t sr_blocks(int64_t n_users) {
    constexpr int RPW = (NPAD < THREADS ? THREADS : NPAD) / NPAD;
    const int64_t blocks = (n_users + RPW - 1) / RPW;
    return blocks > SR_MAX_BLOCKS ? SR_MAX_BLOCKS : blocks;
}

// the template ladder: CALL(NPAD, THREADS) for the row length n_samples <= SR_MAX_SAMPLES
#define TMF_SR_DISPATCH(n_samples, CALL)     \
    if ((n_samples) <= 64) CALL(64, 256);    \
    if ((n_samples) <= 128) CALL(128, 256);  \
    if ((n_samples) <= 256) CALL(256, 256);  \
    if ((n_samples) <= 512) CALL(512, 256);  \
    if ((n_samples) <= 1024) CALL(1024, 256); \
    if ((n_samples) <= 2048) CALL(2048, 512); \
    CALL(4096, 1024)

}  // namespace tmf
