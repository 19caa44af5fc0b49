// Full-catalog ranks of held-out (user, item) pairs - LightFM's predict_rank, the input of auc_score and reciprocal_rank - without
// materialising the [m, n] scores.  rank(u, i) = the number of ELIGIBLE items j != i (not excluded; other positives count) that the
// fused top-k's order (value desc, index asc) puts before i; an item whose score is NaN is never counted above anyone.
//
// The work is the GEMM of the fused top-k (tmf_predict.hip / tmf_predict_split.hip) with another epilogue.  A workgroup owns 128
// VIRTUAL rows: a user with P positives becomes ceil(P / RPC) rows that load the same user vector and hold at most RPC positives
// each (their pair scores come from tmf_pair_scores_*, bit for bit what the tile produces, so a positive meets itself as a tie and
// is not counted).  Per row the positives are orderable 64-bit keys in LDS, and the lowest positive VALUE sits in a register like
// the top-k thresholds: a 32-lane half-wave whose four scores of a row are all below it skips the row at the cost of a max and a
// compare.  Otherwise every score becomes a key once and, for each positive s of the row, the lanes vote "my score beats s" - one
// 64-bit compare and one ballot per 32-column block; the two popcounts of the ballot are the tile's contribution to positive s of
// the half-wave's row, and lane s of that half adds it to its running count (a register).  No LDS atomic (the plane kernel's LDS-DMA
// queue would be drained in front of each) and no histogram: a row's counts are the ranks themselves.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

typedef float f32x16_r __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8_r __attribute__((ext_vector_type(8)));
typedef unsigned int raw16_r __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_r __attribute__((ext_vector_type(4)));
typedef float f32x4_r __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_r;
typedef __attribute__((address_space(1))) const void gbl_void_r;

constexpr int RPC = TMF_RANK_ROW_PAIRS;   // positives per virtual row (lane s of a half-wave counts positive s)
static_assert(RPC <= 32, "one counting lane per positive of a half-wave");

// (value, index) as an orderable key: a before b (value desc, index asc)  <=>  key(a) > key(b).  -0 is keyed as +0 (they compare
// equal in the top-k's comparator).
__device__ __forceinline__ uint64_t rank_key_r(float v, int ix) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    const unsigned o = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    return ((uint64_t)o << 32) | (unsigned)(0x7fffffff - ix);
}
// A score: NaN (also an excluded pair, knocked out by excl_apply) beats nothing.
__device__ __forceinline__ uint64_t score_key_r(float v, int ix) { return v != v ? 0ull : rank_key_r(v, ix); }
// A positive: a NaN score sits below every non-NaN one, (-inf, INT_MAX); item ids stay below INT_MAX.
__device__ __forceinline__ uint64_t pos_key_r(float v, int ix) { return rank_key_r(v != v ? -INFINITY : v, v != v ? 0x7fffffff : ix); }
constexpr uint64_t kNoPositive = ~0ull;   // an empty slot: never beaten

__device__ __forceinline__ int qoff_r(int q) { return (q & 3) + 8 * (q >> 2); }

// Keys [rows][RPC] and lowest positive value [rows] of virtual rows [row0, row0 + rows).  Rows past the end: no positive, +inf.
__device__ __forceinline__ void rank_rows_init(const tmf_rank_rows& vr, int64_t row0, int rows, int tid, int threads,
                                               const int32_t* __restrict__ pos_item, const float* __restrict__ pos_score,
                                               uint64_t* keys, float* low) {
    for (int t = tid; t < rows * RPC; t += threads) {
        const int64_t v = row0 + t / RPC;
        const int s = t % RPC;
        uint64_t key = kNoPositive;
        if (v < vr.n_rows && s < vr.count[v]) {
            const int64_t p = vr.begin[v] + s;
            key = pos_key_r(pos_score[p], pos_item[p]);
        }
        keys[t] = key;
    }
    for (int t = tid; t < rows; t += threads) {
        const int64_t v = row0 + t;
        float lo = INFINITY;
        if (v < vr.n_rows) {
            const int c = min(vr.count[v], RPC);
            for (int s = 0; s < c; ++s) {
                const float x = pos_score[vr.begin[v] + s];
                lo = fminf(lo, x != x ? -INFINITY : x);
            }
        }
        low[t] = lo;
    }
}

// The largest positive count over the wave's 32 rows (wave-uniform): the length of the vote loop.
__device__ __forceinline__ int rank_wave_pmax(const tmf_rank_rows& vr, int64_t my_row, int h) {
    int c = (h == 0 && my_row < vr.n_rows) ? min(vr.count[my_row], RPC) : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c = max(c, __shfl_xor(c, off));
    return __builtin_amdgcn_readfirstlane(c);
}

// One tile's votes.  acc[j][q] of lane (h, l31) = row rbase + qoff(q) of the workgroup (rbase = 32 wave + 4 h), column
// col0 + 32 j + l31; keys_l = keys + rbase * RPC; low[q] = that row's lowest positive value; cq[q] of lane (h, s) counts the
// eligible items above positive s of row (q, h).
template <int NJ>
__device__ __forceinline__ void rank_tile(const f32x16_r (&acc)[NJ], int64_t col0, int64_t n, const uint64_t* keys_l,
                                          const float (&low)[16], int (&cq)[16], int pmax, int h, int l31) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        float mx = acc[0][q];
#pragma unroll
        for (int j = 1; j < NJ; ++j) mx = fmaxf(mx, acc[j][q]);
        if (__builtin_amdgcn_ballot_w64(mx >= low[q]) == 0) continue;   // wave-uniform: no score of these two rows reaches a positive
        uint64_t kx[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t c = col0 + 32 * j + l31;
            kx[j] = c < n ? score_key_r(acc[j][q], (int)c) : 0ull;
        }
        const uint64_t* kr = keys_l + qoff_r(q) * RPC;
        int add = 0;
        for (int s = 0; s < pmax; ++s) {
            const uint64_t ks = kr[s];
            int c0 = 0, c1 = 0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const uint64_t b = __builtin_amdgcn_ballot_w64(kx[j] > ks);
                c0 += __builtin_popcount((unsigned)b);
                c1 += __builtin_popcount((unsigned)(b >> 32));
            }
            add = (l31 == s) ? (h ? c1 : c0) : add;
        }
        cq[q] += add;
    }
}

// Lane (h, s) writes the rank of positive s of each of its 16 rows.
__device__ __forceinline__ void rank_rows_write(const tmf_rank_rows& vr, int64_t rbase_g, const int (&cq)[16], int l31,
                                                int32_t* __restrict__ out_rank) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t v = rbase_g + qoff_r(q);
        if (v < vr.n_rows && l31 < min(vr.count[v], RPC)) out_rank[vr.begin[v] + l31] = cq[q];
    }
}

// ---------------------------------------------------------------------------------------------
// Pair scores.  32 pairs per wave on the DIAGONAL of one 32 x 32 MFMA block: A row t = the user of pair t, B column t = its item,
// the k-steps and (for the planes) the plane order of the fused kernels - so that a pair's score is bit for bit what the tile of
// the rank kernel produces (the position in the block does not change an MFMA's arithmetic).  31/32 of the block is thrown away;
// positives are ~1e-4 of the scores.
// Diagonal element t sits in accumulator register (t & 3) + 4 (t >> 3) of lane t of half (t >> 2) & 1.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float diag_of(const f32x16_r& acc, int l31) {
    const int qt = (l31 & 3) + 4 * (l31 >> 3);
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) d = (q == qt) ? acc[q] : d;
    return d;
}

// fp32: v_mfma_f32_32x32x2_f32 over k-steps of 2 up to K_PAD = 32 nch (the A / B fragments of k_predict_topk and k_item_ranks)
__global__ __launch_bounds__(256) void k_pair_scores_f32(const float* __restrict__ A, const float* __restrict__ B, int K, int64_t lda,
                                                         int64_t ldb, int nch, const int32_t* __restrict__ pu,
                                                         const int32_t* __restrict__ pi, int64_t np, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, h = lane >> 5, l31 = lane & 31;
    const int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + l31;
    const bool valid = p < np;
    const float* a = A + (valid ? (int64_t)pu[p] : 0) * lda;
    const float* b = B + (valid ? (int64_t)pi[p] : 0) * ldb;
    f32x16_r acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int qq = 0; qq < 8 * nch; ++qq) {   // float4 qq of the row: k-steps 2 qq (elements 4 qq + h) and 2 qq + 1 (4 qq + 2 + h)
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
        if (valid) {
            if (4 * qq + 3 < K) { x = *reinterpret_cast<const float4*>(a + 4 * qq); y = *reinterpret_cast<const float4*>(b + 4 * qq); }
            else {
                if (4 * qq < K) { x.x = a[4 * qq]; y.x = b[4 * qq]; }
                if (4 * qq + 1 < K) { x.y = a[4 * qq + 1]; y.y = b[4 * qq + 1]; }
                if (4 * qq + 2 < K) { x.z = a[4 * qq + 2]; y.z = b[4 * qq + 2]; }
            }
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? x.y : x.x, h ? y.y : y.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? x.w : x.z, h ? y.w : y.z, acc, 0, 0, 0);
    }
    const float d = diag_of(acc, l31);
    if (valid && h == ((l31 >> 2) & 1)) out[p] = d;
}

// This lane's eight factors of k-step kk of row `p` (zeros past K and for an invalid row), as three bf16 planes
__device__ __forceinline__ void planes8(const float* p, bool valid, int K, int kk, int h, raw16_r& o1, raw16_r& o2, raw16_r& o3) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.f;
    const int k0 = 16 * kk + 8 * h;
    if (valid && k0 < K) {
        if (k0 + 7 < K) {
            const f32x4_r lo = *reinterpret_cast<const f32x4_r*>(p + k0), hi = *reinterpret_cast<const f32x4_r*>(p + k0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] = lo[e]; x[4 + e] = hi[e]; }
        } else {
            for (int e = 0; e < 8; ++e) if (k0 + e < K) x[e] = p[k0 + e];
        }
    }
    bf16x8_r p1, p2, p3;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 u, v, w;
        split3(x[e], u, v, w);
        p1[e] = u; p2[e] = v; p3[e] = w;
    }
    o1 = __builtin_bit_cast(raw16_r, p1);
    o2 = __builtin_bit_cast(raw16_r, p2);
    o3 = __builtin_bit_cast(raw16_r, p3);
}

__device__ __forceinline__ f32x16_r mfma_bf16_r(const raw16_r a, const raw16_r b, const f32x16_r c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_r, a), __builtin_bit_cast(bf16x8_r, b), c, 0, 0, 0);
}

// Three bf16 planes: the six products in the order of k_predict_topk_split, u3 v1 + u1 v3 + u2 v2 + u2 v1 + u1 v2 + u1 v1 per
// k-step, over nk = ldp / 16 k-steps (split_ldp(r) - the padded width of the item planes)
__global__ __launch_bounds__(256) void k_pair_scores_split(const float* __restrict__ A, const float* __restrict__ B, int K, int64_t lda,
                                                           int64_t ldb, int nk, const int32_t* __restrict__ pu,
                                                           const int32_t* __restrict__ pi, int64_t np, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, h = lane >> 5, l31 = lane & 31;
    const int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + l31;
    const bool valid = p < np;
    const float* a = A + (valid ? (int64_t)pu[p] : 0) * lda;
    const float* b = B + (valid ? (int64_t)pi[p] : 0) * ldb;
    f32x16_r acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int kk = 0; kk < nk; ++kk) {
        raw16_r u1, u2, u3, v1, v2, v3;
        planes8(a, valid, K, kk, h, u1, u2, u3);
        planes8(b, valid, K, kk, h, v1, v2, v3);
        acc = mfma_bf16_r(u3, v1, acc);
        acc = mfma_bf16_r(u1, v3, acc);
        acc = mfma_bf16_r(u2, v2, acc);
        acc = mfma_bf16_r(u2, v1, acc);
        acc = mfma_bf16_r(u1, v2, acc);
        acc = mfma_bf16_r(u1, v1, acc);
    }
    const float d = diag_of(acc, l31);
    if (valid && h == ((l31 >> 2) & 1)) out[p] = d;
}

// ---------------------------------------------------------------------------------------------
// Fused rank count, fp32 MFMA: the GEMM of k_predict_topk (tmf_predict.hip) - 128 rows per 256-thread workgroup as A fragments in
// registers, 128-item tiles through a 3-slot LDS ring in k-chunks of 32, loads three chunks ahead - and rank_tile as the epilogue.
// ---------------------------------------------------------------------------------------------
constexpr int RBM = 128, RBN = 128, RBK = 32, RLD = RBN + 1;
typedef unsigned int u32x4_t_r __attribute__((ext_vector_type(4)));

// MODE 2: K % 4 == 0 and V < 4 GB (buffer loads), 1: K % 4 == 0 (branch-free), 0: any K - as k_predict_topk
template <int NCH, int MODE, bool EXCL>
__global__ __launch_bounds__(256, NCH >= 8 ? 1 : 2) void k_item_ranks(const float* __restrict__ A, const float* __restrict__ B,
                                                                      int64_t n, int K, int64_t lda, int64_t ldb, tmf_rank_rows vr,
                                                                      const int32_t* __restrict__ pos_item,
                                                                      const float* __restrict__ pos_score, tmf_exclusion ex,
                                                                      int32_t* __restrict__ out_rank) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* Bs = reinterpret_cast<float*>(smem_raw);                           // [3][RBK][RLD]
    uint64_t* keys = reinterpret_cast<uint64_t*>(Bs + 3 * RBK * RLD);        // [RBM][RPC]
    float* low = reinterpret_cast<float*>(keys + RBM * RPC);                  // [RBM]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * RBM;
    const int64_t my_row = row0 + 32 * wave + l31;
    const int64_t user = my_row < vr.n_rows ? (int64_t)vr.user[my_row] : -1;
    ExclCursor xc;
    if constexpr (EXCL) xc.init(ex, h == 0 ? user : -1);
    rank_rows_init(vr, row0, RBM, tid, 256, pos_item, pos_score, keys, low);
    const int pmax = rank_wave_pmax(vr, my_row, h);

    float a[16 * NCH];   // a[kk] = U[user][2 kk + h]
    {
        const float* p = A + (user >= 0 ? user : 0) * lda;
#pragma unroll
        for (int q = 0; q < 8 * NCH; ++q) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (user >= 0) {
                if (4 * q + 3 < K) v = *reinterpret_cast<const float4*>(p + 4 * q);
                else { if (4 * q < K) v.x = p[4 * q]; if (4 * q + 1 < K) v.y = p[4 * q + 1]; if (4 * q + 2 < K) v.z = p[4 * q + 2]; }
            }
            a[2 * q] = h ? v.y : v.x;
            a[2 * q + 1] = h ? v.w : v.z;
        }
    }

    const int s_item = tid >> 3, s_k4 = tid & 7;
    const int64_t ntiles = (n + RBN - 1) / RBN;
    const int64_t nchunks = ntiles * NCH;
    constexpr bool ALIGNED = MODE >= 1;
    uint32_t voff[4];
    const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(B), 0, MODE == 2 ? (int)(uint32_t)(n * ldb * 4) : 0, 0x00020000);
#pragma unroll
    for (int q = 0; q < 4; ++q) voff[q] = (uint32_t)(((int64_t)(s_item + 32 * q) * ldb + 4 * s_k4) * 4);
    float4 stg[2][4];
    auto g_load = [&](int64_t g, float4* stage) {
        if constexpr (MODE == 2) {   // rows >= n read as zeros (the range check of the descriptor)
            const uint32_t block_off = (uint32_t)(((g / NCH) * RBN * ldb + 32 * (g % NCH)) * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4_t_r raw = __builtin_amdgcn_raw_buffer_load_b128(vrsrc, (int)(voff[q] + block_off), 0, 0);
                stage[q] = make_float4(__uint_as_float(raw[0]), __uint_as_float(raw[1]), __uint_as_float(raw[2]), __uint_as_float(raw[3]));
            }
        } else if constexpr (MODE == 1) {   // indices clamped into range, k-slots past K zeroed at the LDS write
            const int64_t gg = g < nchunks ? g : nchunks - 1;
            const int64_t tile = gg / NCH;
            const int c = (int)(gg % NCH);
            const int kk = 32 * c + 4 * s_k4;
            const int kc = kk + 4 <= K ? kk : K - 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int64_t item = tile * RBN + s_item + 32 * q;
                item = item < n ? item : n - 1;
                stage[q] = *reinterpret_cast<const float4*>(B + item * ldb + kc);
            }
        } else {
            const int64_t tile = g / NCH;
            const int c = (int)(g % NCH);
            const int kk = 32 * c + 4 * s_k4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t item = tile * RBN + s_item + 32 * q;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g < nchunks && item < n) {
                    const float* p = B + item * ldb + kk;
                    if (kk + 3 < K) v = *reinterpret_cast<const float4*>(p);
                    else { if (kk < K) v.x = p[0]; if (kk + 1 < K) v.y = p[1]; if (kk + 2 < K) v.z = p[2]; }
                }
                stage[q] = v;
            }
        }
    };
    auto s_write_from = [&](int slot, const float4* src, int c) {
        float* dst = Bs + slot * RBK * RLD;
        const bool live = !ALIGNED || (32 * c + 4 * s_k4 < K);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int item = s_item + 32 * q;
            dst[(4 * s_k4 + 0) * RLD + item] = live ? src[q].x : 0.f;
            dst[(4 * s_k4 + 1) * RLD + item] = live ? src[q].y : 0.f;
            dst[(4 * s_k4 + 2) * RLD + item] = live ? src[q].z : 0.f;
            dst[(4 * s_k4 + 3) * RLD + item] = live ? src[q].w : 0.f;
        }
    };
    g_load(0, stg[0]); s_write_from(0, stg[0], 0);
    g_load(1, stg[0]); s_write_from(1, stg[0], 1 % NCH);
    g_load(2, stg[1]);
    __syncthreads();   // also publishes keys / low

    float lowq[16];
    int cq[16];
    const uint64_t* keys_l = keys + (32 * wave + 4 * h) * RPC;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        lowq[q] = low[32 * wave + 4 * h + qoff_r(q)];
        cq[q] = 0;
    }

    f32x16_r acc[4];
    int64_t g = 0;
    for (int64_t tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c, ++g) {
            g_load(g + 3, stg[c & 1]);
            const float* bs = Bs + (int)(g % 3) * RBK * RLD + h * RLD + l31;
            float bq[2][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bq[0][j] = bs[32 * j];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                if (ks + 1 < 16) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) bq[(ks + 1) & 1][j] = bs[2 * (ks + 1) * RLD + 32 * j];
                }
                __builtin_amdgcn_sched_barrier(0);
                const float av = a[16 * c + ks];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bq[ks & 1][j], acc[j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            s_write_from((int)((g + 2) % 3), stg[(c & 1) ^ 1], (c + 2) % NCH);
            if constexpr (NCH == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) stg[1][q] = stg[0][q];
            }
            __syncthreads();
        }
        if constexpr (EXCL) {
            unsigned xw[4];
            const unsigned xrows = excl_collect<4>(xc, tile * RBN, xw);
            excl_apply<4>(acc, xw, xrows, 0, h, l31);
        }
        rank_tile<4>(acc, tile * RBN, n, keys_l, lowq, cq, pmax, h, l31);
    }
    rank_rows_write(vr, row0 + 32 * wave + 4 * h, cq, l31, out_rank);
}

// ---------------------------------------------------------------------------------------------
// Fused rank count, three bf16 planes: the structure of k_predict_topk_split (tmf_predict_split.hip) on 4-wave workgroups - user
// rows split in registers, the item planes of the workspace (k_split3_rows) streamed through a 2-slot LDS ring by LDS-DMA with the
// source-side swizzle - and rank_tile as the epilogue.  No warm-up pass: ranks need no thresholds.
// ---------------------------------------------------------------------------------------------
void launch_split3_rows(const float* B, int64_t n, int r, int64_t ldb, __bf16* Bp, int64_t n_pad, int ldp, hipStream_t s);   // tmf_predict_split.hip

template <int NJ, int KS, int NCH, bool EXCL>
__global__ __launch_bounds__(256, 2) void k_item_ranks_split(const float* __restrict__ A, const uint16_t* __restrict__ Bp, int64_t n,
                                                             int64_t n_pad, int K, int64_t lda, tmf_rank_rows vr,
                                                             const int32_t* __restrict__ pos_item, const float* __restrict__ pos_score,
                                                             tmf_exclusion ex, int32_t* __restrict__ out_rank) {
    constexpr int NP = 3, WAVES = 4, SRING = 2;
    constexpr int LDP = 16 * KS * NCH, SBN = 32 * NJ, SROW = 32 * KS, SPLANE = SBN * SROW, SSLOT = NP * SPLANE;
    constexpr int NK = KS * NCH, SBM = 32 * WAVES;
    constexpr int LPW = NJ * KS / WAVES;
    static_assert(LPW * WAVES == NJ * KS, "the waves share the pieces of a plane evenly");
    static_assert(NJ == 2 || NJ == 4, "two or four column blocks");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* Bs = smem_raw;                                                  // [SRING][3][SBN][SROW] bytes
    uint64_t* keys = reinterpret_cast<uint64_t*>(Bs + SRING * SSLOT);    // [SBM][RPC]
    float* low = reinterpret_cast<float*>(keys + SBM * RPC);              // [SBM]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * SBM;
    const int64_t my_row = row0 + 32 * wave + l31;
    const int64_t user = my_row < vr.n_rows ? (int64_t)vr.user[my_row] : -1;
    ExclCursor xc;
    if constexpr (EXCL) xc.init(ex, h == 0 ? user : -1);
    rank_rows_init(vr, row0, SBM, tid, 64 * WAVES, pos_item, pos_score, keys, low);
    const int pmax = rank_wave_pmax(vr, my_row, h);

    raw16_r a[NP][NK];   // a[p][kk] = plane p of U[user][16 kk + 8 h .. + 8)
    {
        const float* p = A + (user >= 0 ? user : 0) * lda;
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) planes8(p, user >= 0, K, kk, h, a[0][kk], a[1][kk], a[2][kk]);
    }

    constexpr int SR = 2 * KS, RW = 64 / SR;
    static_assert(RW * NJ * KS == SBN, "NJ KS wave-instructions fill one plane of a tile");
    int s_off[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        const int row = RW * (LPW * wave + i) + lane / SR;
        s_off[i] = row * LDP + 8 * ((lane % SR) ^ ((row / (16 / SR)) % SR));
    }
    const int ntiles = (int)((n + SBN - 1) / SBN);
    const int nchunks = ntiles * NCH;
    const int64_t plane = n_pad * LDP;
    auto g_issue = [&](int g, int slot) {
        const int gg = g < nchunks ? g : nchunks - 1;   // the read-ahead past the last chunk re-reads it
        const uint16_t* s = Bp + (int64_t)(gg / NCH) * (SBN * LDP) + 16 * KS * (gg % NCH);
        char* dst = Bs + slot * SSLOT + wave * (1024 * LPW);
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < LPW; ++i)
                __builtin_amdgcn_global_load_lds((gbl_void_r*)(s + p * plane + s_off[i]), (lds_void_r*)(dst + p * SPLANE + i * 1024), 16, 0, 0);
    };
    auto ring_step = [&]() {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((SRING - 2) * NP * LPW) : "memory");
        __builtin_amdgcn_s_barrier();
    };
    __syncthreads();   // keys / low written; no DMA in flight yet
    g_issue(0, 0);
    ring_step();
    const int rd_swz = (l31 / (16 / SR)) % SR;

    float lowq[16];
    int cq[16];
    const uint64_t* keys_l = keys + (32 * wave + 4 * h) * RPC;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        lowq[q] = low[32 * wave + 4 * h + qoff_r(q)];
        cq[q] = 0;
    }

    f32x16_r acc[NJ];
    int g = 0, slot = 0;
    for (int tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c, ++g) {
            g_issue(g + SRING - 1, slot == 0 ? SRING - 1 : slot - 1);
            const char* bs = Bs + slot * SSLOT + l31 * SROW;
            int po[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) po[ks] = 16 * ((2 * ks + h) ^ rd_swz);
            raw16_r bq[2][NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) bq[0][p] = *reinterpret_cast<const raw16_r*>(bs + p * SPLANE + po[0]);
#pragma unroll
            for (int st = 0; st < KS * NJ; ++st) {   // st = NJ ks + j
                const int ks = st / NJ, j = st % NJ;
                const raw16_r* b = bq[st & 1];
                const int kk = KS * c + ks;
                acc[j] = mfma_bf16_r(a[2][kk], b[0], acc[j]);   // the smallest product first
                __builtin_amdgcn_sched_barrier(0);
                if (st + 1 < KS * NJ) {
                    const int ks1 = (st + 1) / NJ, j1 = (st + 1) % NJ;
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        bq[(st + 1) & 1][p] = *reinterpret_cast<const raw16_r*>(bs + p * SPLANE + 32 * j1 * SROW + po[ks1]);
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[j] = mfma_bf16_r(a[0][kk], b[2], acc[j]);
                acc[j] = mfma_bf16_r(a[1][kk], b[1], acc[j]);
                acc[j] = mfma_bf16_r(a[1][kk], b[0], acc[j]);
                acc[j] = mfma_bf16_r(a[0][kk], b[1], acc[j]);
                acc[j] = mfma_bf16_r(a[0][kk], b[0], acc[j]);
                __builtin_amdgcn_sched_barrier(0);
            }
            ring_step();
            slot = (slot == SRING - 1) ? 0 : slot + 1;
        }
        if constexpr (EXCL) {
            unsigned xw[NJ];
            const unsigned xrows = excl_collect<NJ>(xc, (int64_t)tile * SBN, xw);
            excl_apply<NJ>(acc, xw, xrows, 0, h, l31);
        }
        rank_tile<NJ>(acc, (int64_t)tile * SBN, n, keys_l, lowq, cq, pmax, h, l31);
    }
    rank_rows_write(vr, row0 + 32 * wave + 4 * h, cq, l31, out_rank);
}

// ---------------------------------------------------------------------------------------------
// Non-fused count over a dense score block X [rows, cols] of users [user_base, user_base + rows) (tmf_predict_gemm_f32): the
// excluded entries become NaN, then one workgroup per virtual row counts, for each of its positives, the entries whose key is above.
// A positive's own score is read from the block.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rank_mask_rows(float* __restrict__ X, int64_t cols, int64_t ldx, int64_t user_base,
                                                        tmf_exclusion ex) {
    const int64_t row = blockIdx.x, u = user_base + row;
    const int64_t b = ex.rowptr[u], e = ex.rowptr[u + 1];
    float* x = X + row * ldx;
    for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const int64_t c = (int64_t)ex.cols[p] - ex.item_base;
        if (c >= 0 && c < cols) x[c] = __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void k_rank_count_rows(const float* __restrict__ X, int64_t cols, int64_t ldx, int64_t user_base,
                                                         tmf_rank_rows vr, const int32_t* __restrict__ pos_item,
                                                         int32_t* __restrict__ out_rank) {
    __shared__ uint64_t keys[RPC];
    __shared__ int total[RPC];
    const int64_t v = blockIdx.x;
    const float* x = X + ((int64_t)vr.user[v] - user_base) * ldx;
    const int64_t beg = vr.begin[v];
    const int cnt = min(vr.count[v], RPC);
    if (threadIdx.x < RPC) {
        const int s = threadIdx.x;
        keys[s] = s < cnt ? pos_key_r(x[pos_item[beg + s]], pos_item[beg + s]) : kNoPositive;
        total[s] = 0;
    }
    __syncthreads();
    uint64_t ks[RPC];
#pragma unroll
    for (int s = 0; s < RPC; ++s) ks[s] = keys[s];
    int c[RPC];
#pragma unroll
    for (int s = 0; s < RPC; ++s) c[s] = 0;
    for (int64_t j = threadIdx.x; j < cols; j += 256) {
        const uint64_t kj = score_key_r(x[j], (int)j);
#pragma unroll
        for (int s = 0; s < RPC; ++s) c[s] += kj > ks[s] ? 1 : 0;
    }
#pragma unroll
    for (int s = 0; s < RPC; ++s) {
        int t = c[s];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&total[s], t);
    }
    __syncthreads();
    if (threadIdx.x < cnt) out_rank[beg + threadIdx.x] = total[threadIdx.x];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int rank_nch(int r) { return r <= 32 ? 1 : r <= 64 ? 2 : r <= 128 ? 4 : 8; }
static int rank_split_ldp(int r) { return r <= 32 ? 32 : r <= 64 ? 64 : r <= 128 ? 128 : 256; }   // split_ldp (tmf_predict_split.hip)
static int64_t rank_split_rows_pad(int64_t n) { return (n + 127) / 128 * 128; }

static int check_rank_rows(const char* what, const tmf_rank_rows* rows, const int32_t* pos_item, int32_t* out_rank) {
    TMF_REQUIRE(rows && rows->n_rows >= 0, "%s: bad virtual rows", what);
    TMF_REQUIRE(rows->n_rows == 0 || (rows->user && rows->begin && rows->count && pos_item && out_rank), "%s: bad arguments", what);
    return TMF_OK;
}

static int check_pair_args(const char* what, const float* A, const float* B, int r, int64_t lda, int64_t ldb, const int32_t* pu,
                           const int32_t* pi, int64_t np, float* out) {
    TMF_REQUIRE(np >= 0 && r > 0 && A && B && lda >= r && ldb >= r, "%s: bad arguments", what);
    TMF_REQUIRE(np == 0 || (pu && pi && out), "%s: bad pair arrays", what);
    TMF_REQUIRE((lda % 4 == 0) && (ldb % 4 == 0) && ((uintptr_t)A % 16 == 0) && ((uintptr_t)B % 16 == 0),
                "%s: operands must be 16-byte aligned with ld %% 4 == 0", what);
    return TMF_OK;
}

template <int NCH, int MODE, bool EXCL>
static int launch_item_ranks_mode(const float* A, const float* B, int64_t n, int K, int64_t lda, int64_t ldb, const tmf_rank_rows& vr,
                                  const int32_t* pos_item, const float* pos_score, const tmf_exclusion& ex, int32_t* out_rank,
                                  hipStream_t s) {
    const size_t lds = sizeof(float) * 3 * RBK * RLD + sizeof(uint64_t) * RBM * RPC + sizeof(float) * RBM;
    static LdsGrant grant;
    if (int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&k_item_ranks<NCH, MODE, EXCL>), lds, grant)) return rc;
    const int64_t blocks = (vr.n_rows + RBM - 1) / RBM;
    TMF_REQUIRE_LAUNCH(blocks, 256, "item_ranks_f32");
    hipLaunchKernelGGL((k_item_ranks<NCH, MODE, EXCL>), dim3((unsigned)blocks), dim3(256), lds, s, A, B, n, K, lda, ldb, vr, pos_item,
                       pos_score, ex, out_rank);
    return check_launch("tmf_item_ranks_f32");
}

template <int NCH, bool EXCL>
static int launch_item_ranks(const float* A, const float* B, int64_t n, int K, int64_t lda, int64_t ldb, const tmf_rank_rows& vr,
                             const int32_t* pos_item, const float* pos_score, const tmf_exclusion& ex, int32_t* out_rank, hipStream_t s) {
    if (K % 4 == 0 && (n + 4 * RBN) * ldb * 4 < ((int64_t)1 << 32))
        return launch_item_ranks_mode<NCH, 2, EXCL>(A, B, n, K, lda, ldb, vr, pos_item, pos_score, ex, out_rank, s);
    if (K % 4 == 0) return launch_item_ranks_mode<NCH, 1, EXCL>(A, B, n, K, lda, ldb, vr, pos_item, pos_score, ex, out_rank, s);
    return launch_item_ranks_mode<NCH, 0, EXCL>(A, B, n, K, lda, ldb, vr, pos_item, pos_score, ex, out_rank, s);
}

template <bool EXCL>
static int item_ranks_f32(const float* A, const float* B, int64_t n, int r, int64_t lda, int64_t ldb, const tmf_rank_rows& vr,
                          const int32_t* pos_item, const float* pos_score, const tmf_exclusion& ex, int32_t* out_rank, hipStream_t s) {
    switch (rank_nch(r)) {
        case 1: return launch_item_ranks<1, EXCL>(A, B, n, r, lda, ldb, vr, pos_item, pos_score, ex, out_rank, s);
        case 2: return launch_item_ranks<2, EXCL>(A, B, n, r, lda, ldb, vr, pos_item, pos_score, ex, out_rank, s);
        case 4: return launch_item_ranks<4, EXCL>(A, B, n, r, lda, ldb, vr, pos_item, pos_score, ex, out_rank, s);
        default: return launch_item_ranks<8, EXCL>(A, B, n, r, lda, ldb, vr, pos_item, pos_score, ex, out_rank, s);
    }
}

template <int NJ, int KS, int NCH, bool EXCL>
static int launch_item_ranks_split_w(const float* A, const uint16_t* Bp, int64_t n, int64_t n_pad, int K, int64_t lda,
                                     const tmf_rank_rows& vr, const int32_t* pos_item, const float* pos_score, const tmf_exclusion& ex,
                                     int32_t* out_rank, hipStream_t s) {
    const size_t lds = (size_t)2 * 3 * (32 * NJ) * (32 * KS) + sizeof(uint64_t) * 128 * RPC + sizeof(float) * 128;
    static LdsGrant grant;
    if (int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&k_item_ranks_split<NJ, KS, NCH, EXCL>), lds, grant)) return rc;
    const int64_t blocks = (vr.n_rows + 127) / 128;
    TMF_REQUIRE_LAUNCH(blocks, 256, "item_ranks_split");
    hipLaunchKernelGGL((k_item_ranks_split<NJ, KS, NCH, EXCL>), dim3((unsigned)blocks), dim3(256), lds, s, A, Bp, n, n_pad, K, lda, vr,
                       pos_item, pos_score, ex, out_rank);
    return check_launch("tmf_item_ranks_split");
}

// the tile shapes of the 4-wave plane kernels of the top-k (k <= 22): 128-item tiles up to r = 64, 64-item tiles above
template <bool EXCL>
static int item_ranks_split(int ldp, const float* A, const uint16_t* Bp, int64_t n, int64_t n_pad, int K, int64_t lda,
                            const tmf_rank_rows& vr, const int32_t* pos_item, const float* pos_score, const tmf_exclusion& ex,
                            int32_t* out_rank, hipStream_t s) {
    if (ldp == 32) return launch_item_ranks_split_w<4, 2, 1, EXCL>(A, Bp, n, n_pad, K, lda, vr, pos_item, pos_score, ex, out_rank, s);
    if (ldp == 64) return launch_item_ranks_split_w<4, 2, 2, EXCL>(A, Bp, n, n_pad, K, lda, vr, pos_item, pos_score, ex, out_rank, s);
    if (ldp == 128) return launch_item_ranks_split_w<2, 4, 2, EXCL>(A, Bp, n, n_pad, K, lda, vr, pos_item, pos_score, ex, out_rank, s);
    return launch_item_ranks_split_w<2, 4, 4, EXCL>(A, Bp, n, n_pad, K, lda, vr, pos_item, pos_score, ex, out_rank, s);
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_pair_scores_f32(const float* A, const float* B, int r, int64_t lda, int64_t ldb, const int32_t* pair_user,
                                   const int32_t* pair_item, int64_t n_pairs, float* out, void* stream) {
    if (int rc = check_pair_args("pair_scores_f32", A, B, r, lda, ldb, pair_user, pair_item, n_pairs, out)) return rc;
    if (n_pairs == 0) return TMF_OK;
    TMF_REQUIRE(r <= 256, "pair_scores_f32: n_components <= 256 (the fused kernel's widths), got %d", r);
    const int64_t blocks = (n_pairs + 127) / 128;
    TMF_REQUIRE_LAUNCH(blocks, 256, "pair_scores_f32");
    hipLaunchKernelGGL(k_pair_scores_f32, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A, B, r, lda, ldb, rank_nch(r),
                       pair_user, pair_item, n_pairs, out);
    return check_launch("tmf_pair_scores_f32");
}

extern "C" int tmf_pair_scores_split(const float* A, const float* B, int r, int64_t lda, int64_t ldb, const int32_t* pair_user,
                                     const int32_t* pair_item, int64_t n_pairs, float* out, void* stream) {
    if (int rc = check_pair_args("pair_scores_split", A, B, r, lda, ldb, pair_user, pair_item, n_pairs, out)) return rc;
    if (n_pairs == 0) return TMF_OK;
    if (r > 256) { set_error("pair_scores_split: n_components <= 256, got %d", r); return TMF_E_UNSUPPORTED; }
    const int64_t blocks = (n_pairs + 127) / 128;
    TMF_REQUIRE_LAUNCH(blocks, 256, "pair_scores_split");
    hipLaunchKernelGGL(k_pair_scores_split, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A, B, r, lda, ldb,
                       rank_split_ldp(r) / 16, pair_user, pair_item, n_pairs, out);
    return check_launch("tmf_pair_scores_split");
}

extern "C" int tmf_item_ranks_f32_supported(int r) { return r >= 1 && r <= 256; }
extern "C" int tmf_item_ranks_split_supported(int r) { return r >= 1 && r <= 256; }

extern "C" size_t tmf_item_ranks_split_workspace_bytes(int64_t n, int r) {
    if (n <= 0 || r < 1 || r > 256) return 0;
    return (size_t)3 * (size_t)rank_split_rows_pad(n) * (size_t)rank_split_ldp(r) * sizeof(uint16_t);
}

extern "C" int tmf_item_ranks_f32(const float* A, const float* B, int64_t n, int r, int64_t lda, int64_t ldb,
                                  const tmf_rank_rows* rows, const int32_t* pos_item, const float* pos_score,
                                  const tmf_exclusion* exclude, int32_t* out_rank, void* stream) {
    if (int rc = check_rank_rows("item_ranks_f32", rows, pos_item, out_rank)) return rc;
    if (rows->n_rows == 0) return TMF_OK;
    TMF_REQUIRE(A && B && pos_score && n > 0 && r > 0 && lda >= r && ldb >= r, "item_ranks_f32: bad arguments");
    TMF_REQUIRE((lda % 4 == 0) && (ldb % 4 == 0) && ((uintptr_t)A % 16 == 0) && ((uintptr_t)B % 16 == 0),
                "item_ranks_f32: operands must be 16-byte aligned with ld %% 4 == 0");
    TMF_REQUIRE(n < ((int64_t)1 << 31), "item_ranks_f32: too many items");
    if (!tmf_item_ranks_f32_supported(r)) {
        set_error("item_ranks_f32: the fused kernel supports n_components <= 256 (got %d)", r);
        return TMF_E_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    if (exclude) {
        TMF_REQUIRE(exclude->rowptr && exclude->cols && exclude->item_base >= 0, "item_ranks_f32: bad exclusion");
        return item_ranks_f32<true>(A, B, n, r, lda, ldb, *rows, pos_item, pos_score, *exclude, out_rank, s);
    }
    return item_ranks_f32<false>(A, B, n, r, lda, ldb, *rows, pos_item, pos_score, tmf_exclusion{}, out_rank, s);
}

extern "C" int tmf_item_ranks_split(const float* A, const float* B, int64_t n, int r, int64_t lda, int64_t ldb,
                                    const tmf_rank_rows* rows, const int32_t* pos_item, const float* pos_score,
                                    const tmf_exclusion* exclude, int32_t* out_rank, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    if (int rc = check_rank_rows("item_ranks_split", rows, pos_item, out_rank)) return rc;
    if (rows->n_rows == 0) return TMF_OK;
    TMF_REQUIRE(A && B && pos_score && n > 0 && r > 0 && lda >= r && ldb >= r, "item_ranks_split: bad arguments");
    TMF_REQUIRE((lda % 4 == 0) && ((uintptr_t)A % 16 == 0), "item_ranks_split: the user table must be 16-byte aligned with ld %% 4 == 0");
    TMF_REQUIRE(n < ((int64_t)1 << 31), "item_ranks_split: too many items");
    if (!tmf_item_ranks_split_supported(r)) {
        set_error("item_ranks_split: supports n_components <= 256 (got %d)", r);
        return TMF_E_UNSUPPORTED;
    }
    const size_t need = tmf_item_ranks_split_workspace_bytes(n, r);
    TMF_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace % 16 == 0),
                "item_ranks_split: workspace of %zu bytes (16-byte aligned) needed, got %zu", need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int ldp = rank_split_ldp(r);
    const int64_t n_pad = rank_split_rows_pad(n);
    __bf16* Bp = reinterpret_cast<__bf16*>(workspace);
    {
        const int64_t threads = n_pad * (ldp / 8), blocks = (threads + 255) / 256;
        TMF_REQUIRE_LAUNCH(blocks, 256, "item_ranks_split (item planes)");
        launch_split3_rows(B, n, r, ldb, Bp, n_pad, ldp, s);
        if (int rc = check_launch("tmf_item_ranks_split (item planes)")) return rc;
    }
    const uint16_t* P = reinterpret_cast<const uint16_t*>(Bp);
    if (exclude) {
        TMF_REQUIRE(exclude->rowptr && exclude->cols && exclude->item_base >= 0, "item_ranks_split: bad exclusion");
        return item_ranks_split<true>(ldp, A, P, n, n_pad, r, lda, *rows, pos_item, pos_score, *exclude, out_rank, s);
    }
    return item_ranks_split<false>(ldp, A, P, n, n_pad, r, lda, *rows, pos_item, pos_score, tmf_exclusion{}, out_rank, s);
}

extern "C" int tmf_rank_count_rows_f32(float* X, int64_t rows, int64_t cols, int64_t ldx, int64_t user_base,
                                       const tmf_rank_rows* vrows, const int32_t* pos_item, const tmf_exclusion* exclude,
                                       int32_t* out_rank, void* stream) {
    if (int rc = check_rank_rows("rank_count_rows_f32", vrows, pos_item, out_rank)) return rc;
    TMF_REQUIRE(X && rows > 0 && cols > 0 && ldx >= cols && user_base >= 0 && rows < ((int64_t)1 << 31) && cols < ((int64_t)1 << 31),
                "rank_count_rows_f32: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (exclude) {
        TMF_REQUIRE(exclude->rowptr && exclude->cols && exclude->item_base >= 0, "rank_count_rows_f32: bad exclusion");
        hipLaunchKernelGGL(k_rank_mask_rows, dim3((unsigned)rows), dim3(256), 0, s, X, cols, ldx, user_base, *exclude);
        if (int rc = check_launch("tmf_rank_count_rows_f32 (mask)")) return rc;
    }
    if (vrows->n_rows == 0) return TMF_OK;
    TMF_REQUIRE_LAUNCH(vrows->n_rows, 256, "rank_count_rows_f32");
    hipLaunchKernelGGL(k_rank_count_rows, dim3((unsigned)vrows->n_rows), dim3(256), 0, s, (const float*)X, cols, ldx, user_base, *vrows,
                       pos_item, out_rank);
    return check_launch("tmf_rank_count_rows_f32");
}
