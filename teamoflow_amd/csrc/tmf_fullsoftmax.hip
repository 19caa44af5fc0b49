// Full-catalog softmax (FullSoftmaxLoss, an extension: the reference has no softmax): the softmax of a positive against EVERY item,
// trained without materialising the [m, n] score matrix.  mf/loss_graphs.py FullSoftmaxLoss is the definition:
//     loss_k = lse_u - p_k,   lse_u = log sum_i exp(U[u].V[i]),   pi_ui = exp(U[u].V[i] - lse_u),   n_u = positives of u
//     G_U[u] = n_u sum_i pi_ui V[i] - sum_{k of u, val > 0} V[i_k]        G_V[i] = sum_u n_u pi_ui U[u] - sum_{k at i, val > 0} U[u_k]
// Three kernels, all fp32 tables on v_mfma_f32_32x32x2_f32, any n_components from 1 to FSM_MAX_COMPONENTS = 128:
//   k_fsm_lse        the GEMM loop of k_predict_topk (tmf_predict.hip; a COPY on purpose, as tmf_rank.hip's is): 128 rows per workgroup
//                    as A fragments in registers, 128-item tiles through a 3-slot LDS ring in k-chunks of 32, global loads three
//                    chunks ahead.  The epilogue of a tile is an online log-sum-exp in the base-2 domain: every lane keeps a running
//                    maximum and a scaled sum for each of its 16 rows over the columns it holds (column = lane mod 32), one
//                    v_exp_f32 and three other vector operations per score; the 32 lanes of a row are merged once, at the end, by a
//                    fixed xor butterfly.  Columns >= n of the ragged last tile are -inf; rows >= m are never written.  No atomics,
//                    one order of every sum: the output is bit-reproducible.
//   k_fsm_wsum       G[a] += sum_b w_u exp(A[a].B[b] - lse_u) B[b]: the 128 stationary rows a as A fragments in registers, b swept in
//                    tiles of 128 rows that are WHOLE in LDS ([128][K_PAD + 1], two buffers: the next tile is fetched a quarter at a
//                    time behind the MFMAs of the current one).  Per 32-column block of a tile: the score block by MFMA (B operand
//                    read down the columns of the LDS tile), P = w exp2(..) in the 16 accumulator registers, P through a wave-private
//                    [32][33] LDS block from accumulator layout (row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5), column = lane & 31)
//                    into A-operand layout (row = lane & 31, k = lane >> 5), then P . B_block by a second MFMA (B operand read along
//                    the rows of the same LDS tile) into the [32 x K_PAD] output accumulators the wave keeps for the whole kernel.
//                    The user - whose lse and w count - is the stationary row (USER_A: G_U) or the swept one (G_V).  A stationary row
//                    belongs to one workgroup and the tiles come in one order: no atomics, bit-reproducible.  `+=`: the kernel adds
//                    onto what G holds; a stationary user row with w = 0 is not touched at all, a swept user with w = 0 adds nothing.
//                    LDS at K_PAD = 128: 2 x 128 x 129 x 4 + 4 x 32 x 33 x 4 = 148992 bytes, one workgroup per CU; registers per lane:
//                    64 of A fragments, 64 output accumulators, 16 score accumulators, 16 of staging.  Every ds_read_b32 / ds_write_b32
//                    here is conflict-free over its 32-lane half (odd leading dimensions).
//   k_fsm_pos_pass   the positives' term and the loss: k_mse_pass's walk (tmf_train.hip; a copy of its loop, as k_kl_pass is) with the
//                    weight -1 on entries with a value > 0 and 0 on the others, the raw gradient always (TMF_EPI_GRAD), and
//                    sum_k (lse_u - p_k) of the segment into loss_part on the user side.
#include <math.h>

#include "tmf_common.h"
#include "tmf_segments.h"

namespace tmf {

constexpr int SBM = 128, SBN = 128, SBK = 32, SLD = SBN + 1;
constexpr int FSM_MAX_COMPONENTS = 128;
constexpr int SLDP = 33;   // k_fsm_wsum: leading dimension of a wave's [32][32] P block
constexpr float kFsmLog2eHi = 1.4426950216293335f, kFsmLog2eLo = 1.9259629911266175e-8f, kFsmLn2 = 0.6931471805599453f;
typedef unsigned int fsm_u32x4 __attribute__((ext_vector_type(4)));
typedef float fsm_f32x16 __attribute__((ext_vector_type(16)));

// MODE 2: K % 4 == 0 and B < 4 GB (buffer loads, constant per-thread offsets), 1: K % 4 == 0 (branch-free), 0: any K
template <int NCH, int MODE>  // K_PAD = 32 * NCH
__global__ __launch_bounds__(256, 2) void k_fsm_lse(const float* __restrict__ A, const float* __restrict__ B, int64_t m, int64_t n,
                                                    int K, int64_t lda, int64_t ldb, float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* Bs = reinterpret_cast<float*>(smem_raw);          // [3][SBK][SLD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * SBM;

    // ---- A fragments of this wave's 32 rows: a[kk] = A[row0 + 32 wave + l31][2 kk + h] ----
    float a[16 * NCH];
    {
        const int64_t r = row0 + 32 * wave + l31;
        const float* p = A + (r < m ? r : 0) * lda;
#pragma unroll
        for (int q = 0; q < 8 * NCH; ++q) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < m) {
                if (4 * q + 3 < K) v = *reinterpret_cast<const float4*>(p + 4 * q);
                else { if (4 * q < K) v.x = p[4 * q]; if (4 * q + 1 < K) v.y = p[4 * q + 1]; if (4 * q + 2 < K) v.z = p[4 * q + 2]; }
            }
            a[2 * q] = h ? v.y : v.x;
            a[2 * q + 1] = h ? v.w : v.z;
        }
    }

    // ---- staging: thread -> (item = tid/8 + 32 q, float4 #tid%8 of the 32-wide k-chunk) ----
    const int s_item = tid >> 3, s_k4 = tid & 7;
    const int64_t ntiles = (n + SBN - 1) / SBN;
    const int64_t nchunks = ntiles * NCH;
    constexpr bool ALIGNED = MODE >= 1;
    uint32_t voff[4];  // MODE 2: byte offset of this thread's four 16-byte pieces inside a (tile, k-chunk) block of B
    const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(B), 0, MODE == 2 ? (int)(uint32_t)(n * ldb * 4) : 0, 0x00020000);
#pragma unroll
    for (int q = 0; q < 4; ++q) voff[q] = (uint32_t)(((int64_t)(s_item + 32 * q) * ldb + 4 * s_k4) * 4);
    float4 stg[2][4];  // two staging register sets, alternating by chunk parity
    auto g_load = [&](int64_t g, float4* stage) {
        if constexpr (MODE == 2) {
            // the hardware range check returns zeros for rows >= n (the ragged last tile and the prefetches past the end); k-slots >= K
            // are zeroed at the LDS write
            const uint32_t block_off = (uint32_t)(((g / NCH) * SBN * ldb + 32 * (g % NCH)) * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const fsm_u32x4 raw = __builtin_amdgcn_raw_buffer_load_b128(vrsrc, (int)(voff[q] + block_off), 0, 0);
                stage[q] = make_float4(__uint_as_float(raw[0]), __uint_as_float(raw[1]), __uint_as_float(raw[2]),
                                       __uint_as_float(raw[3]));
            }
        } else if constexpr (MODE == 1) {
            // branch-free: chunk and item indices are clamped into range (columns >= n are masked in the epilogue, the prefetches past
            // the last chunk re-read it) and a k-slot past K is zeroed by a select at the LDS write
            const int64_t gg = g < nchunks ? g : nchunks - 1;
            const int64_t tile = gg / NCH;
            const int c = (int)(gg % NCH);
            const int kk = 32 * c + 4 * s_k4;
            const int kc = kk + 4 <= K ? kk : K - 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int64_t item = tile * SBN + s_item + 32 * q;
                item = item < n ? item : n - 1;
                stage[q] = *reinterpret_cast<const float4*>(B + item * ldb + kc);
            }
        } else {
            const int64_t tile = g / NCH;
            const int c = (int)(g % NCH);
            const int kk = 32 * c + 4 * s_k4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t item = tile * SBN + s_item + 32 * q;
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
    auto s_write_from = [&](int slot, const float4* src, int c) {  // c = k-chunk of the data in `src`
        float* dst = Bs + slot * SBK * SLD;
        const bool live = !ALIGNED || (32 * c + 4 * s_k4 < K);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int item = s_item + 32 * q;
            dst[(4 * s_k4 + 0) * SLD + item] = live ? src[q].x : 0.f;
            dst[(4 * s_k4 + 1) * SLD + item] = live ? src[q].y : 0.f;
            dst[(4 * s_k4 + 2) * SLD + item] = live ? src[q].z : 0.f;
            dst[(4 * s_k4 + 3) * SLD + item] = live ? src[q].w : 0.f;
        }
    };
    // global loads run three chunks ahead of the MFMAs that consume them (k_predict_topk)
    g_load(0, stg[0]); s_write_from(0, stg[0], 0);
    g_load(1, stg[0]); s_write_from(1, stg[0], 1 % NCH);
    g_load(2, stg[1]);
    __syncthreads();

    fsm_f32x16 acc[4];  // the wave's 32 rows x the tile's 4 x 32 items
    // online log-sum-exp in the base-2 domain, per (row of this lane, columns of this lane): mx = the largest t = s log2(e) so far
    // (a finite start, so that a lane that has seen only masked columns forms no inf - inf), sm = sum of exp2(t - mx)
    float mx[16], sm[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { mx[q] = -3.0e38f; sm[q] = 0.f; }

    int64_t g = 0;
    for (int64_t tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c, ++g) {
            g_load(g + 3, stg[c & 1]);
            const float* bs = Bs + (int)(g % 3) * SBK * SLD + h * SLD + l31;
            float bq[2][4];  // B operands one k-step ahead of the MFMAs that consume them
#pragma unroll
            for (int j = 0; j < 4; ++j) bq[0][j] = bs[32 * j];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                if (ks + 1 < 16) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) bq[(ks + 1) & 1][j] = bs[2 * (ks + 1) * SLD + 32 * j];
                }
                __builtin_amdgcn_sched_barrier(0);  // keep the reads of step ks + 1 ahead of the MFMAs of step ks
                const float av = a[16 * c + ks];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bq[ks & 1][j], acc[j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            s_write_from((int)((g + 2) % 3), stg[(c & 1) ^ 1], (c + 2) % NCH);
            if constexpr (NCH == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) stg[1][q] = stg[0][q];
            }
            __syncthreads();
        }
        // the tile's scores into the running sums; only the ragged last tile has columns to mask (wave-uniform branch)
        const int64_t col0 = tile * SBN;
        const bool ragged = col0 + SBN > n;
        bool ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = !ragged || (col0 + 32 * j + l31 < n);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = ok[j] ? acc[j][q] * kFsmLog2eHi : -INFINITY;
            const float nm = fmaxf(fmaxf(mx[q], fmaxf(t[0], t[1])), fmaxf(t[2], t[3]));   // finite or +inf; a NaN score is not a maximum
            float s = sm[q] * __builtin_amdgcn_exp2f(mx[q] - nm);
#pragma unroll
            for (int j = 0; j < 4; ++j) s += __builtin_amdgcn_exp2f(t[j] - nm);            // ... but makes the sum NaN: it stays in its row
            sm[q] = s;
            mx[q] = nm;
        }
    }
    // the 32 lanes of a row, by a fixed butterfly: both partners form the same two products and add them (commutative: same bits)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const float om = __shfl_xor(mx[q], off, 64), os = __shfl_xor(sm[q], off, 64);
            const float nm = fmaxf(mx[q], om);
            const float mine = sm[q] * __builtin_amdgcn_exp2f(mx[q] - nm), theirs = os * __builtin_amdgcn_exp2f(om - nm);
            sm[q] = mine + theirs;
            mx[q] = nm;
        }
        const int64_t row = row0 + 32 * wave + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (l31 == 0 && row < m) lse[row] = (mx[q] + log2f(sm[q])) * kFsmLn2;
    }
}

// One quarter (32 rows) of a B tile: thread -> (row = tid / 8, float4 #(tid % 8 + 8 c) of the row, c < NCH)
template <int NCH, int MODE>
__device__ __forceinline__ void fsm_quarter_load(const float* __restrict__ B, __amdgpu_buffer_rsrc_t rsrc, int64_t nb, int K, int64_t ldb,
                                                 int64_t tile, int64_t ntiles, int qd, int tid, float4 (&stg)[NCH]) {
    const int64_t item = tile * SBN + 32 * qd + (tid >> 3);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int kk = 4 * ((tid & 7) + 8 * c);
        if constexpr (MODE == 2) {
            // rows >= nb (the ragged last tile, the tile past the end) come back as zeros from the range check; k-slots >= K are
            // zeroed at the LDS write.  The byte offset fits 32 bits: the launcher takes MODE 2 only while (nb + 2 SBN) ldb 4 < 2^32
            const uint32_t off = (uint32_t)((item * ldb + kk) * 4);
            const fsm_u32x4 raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, 0, 0);
            stg[c] = make_float4(__uint_as_float(raw[0]), __uint_as_float(raw[1]), __uint_as_float(raw[2]), __uint_as_float(raw[3]));
        } else {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tile < ntiles && item < nb) {
                const float* p = B + item * ldb + kk;
                if (kk + 3 < K) v = *reinterpret_cast<const float4*>(p);
                else { if (kk < K) v.x = p[0]; if (kk + 1 < K) v.y = p[1]; if (kk + 2 < K) v.z = p[2]; }
            }
            stg[c] = v;
        }
    }
}

template <int NCH, int MODE>
__device__ __forceinline__ void fsm_quarter_write(float* __restrict__ Bt, int K, int qd, int tid, const float4 (&stg)[NCH]) {
    constexpr int LDB = 32 * NCH + 1;
    float* dst = Bt + (32 * qd + (tid >> 3)) * LDB;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int kk = 4 * ((tid & 7) + 8 * c);
        const bool live = MODE != 2 || kk < K;   // MODE 2 has K % 4 == 0: a piece is whole or not there
        dst[kk + 0] = live ? stg[c].x : 0.f;
        dst[kk + 1] = live ? stg[c].y : 0.f;
        dst[kk + 2] = live ? stg[c].z : 0.f;
        dst[kk + 3] = live ? stg[c].w : 0.f;
    }
}

// MODE 2: K % 4 == 0 and B < 4 GB (buffer loads); 0: any K, any size (guarded scalar loads)
template <int NCH, int MODE, bool USER_A>  // K_PAD = 32 * NCH; USER_A: lse / w belong to the stationary rows, else to the swept ones
__global__ __launch_bounds__(256, 1) void k_fsm_wsum(const float* __restrict__ A, const float* __restrict__ B, int64_t ma, int64_t nb,
                                                     int K, int64_t lda, int64_t ldb, const float* __restrict__ lse,
                                                     const float* __restrict__ w, float* __restrict__ G, int64_t ldg) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int KP = 32 * NCH, LDB = KP + 1;
    float* Bt = reinterpret_cast<float*>(smem_raw);          // [2][SBN][LDB]
    float* Pw = Bt + 2 * SBN * LDB;                          // [4 waves][32][SLDP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * SBM;
    float* pw = Pw + wave * 32 * SLDP;

    // ---- A fragments of this wave's 32 stationary rows: a[kk] = A[row0 + 32 wave + l31][2 kk + h] ----
    float a[16 * NCH];
    {
        const int64_t r = row0 + 32 * wave + l31;
        const float* p = A + (r < ma ? r : 0) * lda;
#pragma unroll
        for (int q = 0; q < 8 * NCH; ++q) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < ma) {
                if (4 * q + 3 < K) v = *reinterpret_cast<const float4*>(p + 4 * q);
                else { if (4 * q < K) v.x = p[4 * q]; if (4 * q + 1 < K) v.y = p[4 * q + 1]; if (4 * q + 2 < K) v.z = p[4 * q + 2]; }
            }
            a[2 * q] = h ? v.y : v.x;
            a[2 * q + 1] = h ? v.w : v.z;
        }
    }
    // exp(s - lse) = exp2(s log2(e) - lse log2(e)): lse log2(e) as hi + lo (48 bits), so that a score of 90 costs no more than one near 0
    auto split = [](float x, float& hi, float& lo) {
        hi = __fmul_rn(x, kFsmLog2eHi);
        lo = fmaf(x, kFsmLog2eLo, fmaf(x, kFsmLog2eHi, -hi));
    };
    // USER_A: the weight and the scaled lse of the 16 rows this lane holds accumulator elements of (w = 0 beyond ma)
    float wq[16], lhi[16], llo[16];
    if constexpr (USER_A) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t row = row0 + 32 * wave + (q & 3) + 8 * (q >> 2) + 4 * h;
            wq[q] = row < ma ? w[row] : 0.f;
            split(row < ma ? lse[row] : 0.f, lhi[q], llo[q]);
        }
    }

    const int64_t ntiles = (nb + SBN - 1) / SBN;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(B), 0, MODE == 2 ? (int)(uint32_t)(nb * ldb * 4) : 0, 0x00020000);
    float4 stg[NCH];
    for (int qd = 0; qd < 4; ++qd) {
        fsm_quarter_load<NCH, MODE>(B, rsrc, nb, K, ldb, 0, ntiles, qd, tid, stg);
        fsm_quarter_write<NCH, MODE>(Bt, K, qd, tid, stg);
    }
    __syncthreads();

    fsm_f32x16 gacc[NCH];  // the wave's 32 rows x K_PAD output columns
#pragma unroll
    for (int jj = 0; jj < NCH; ++jj)
#pragma unroll
        for (int q = 0; q < 16; ++q) gacc[jj][q] = 0.f;

    for (int64_t tile = 0; tile < ntiles; ++tile) {
        const float* cur = Bt + (int)(tile & 1) * SBN * LDB;
        float* nxt = Bt + (int)((tile + 1) & 1) * SBN * LDB;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            // a quarter of the next tile: requested here, written to the other buffer behind this block's MFMAs
            fsm_quarter_load<NCH, MODE>(B, rsrc, nb, K, ldb, tile + 1, ntiles, j, tid, stg);
            const int64_t col = tile * SBN + 32 * j + l31;   // the swept row this lane holds scores of
            const bool col_ok = col < nb;
            float wc = 0.f, chi = 0.f, clo = 0.f;
            if constexpr (!USER_A) {
                wc = col_ok ? w[col] : 0.f;
                split(col_ok ? lse[col] : 0.f, chi, clo);
            }
            // ---- scores of the wave's 32 rows against the block's 32 swept rows ----
            fsm_f32x16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.f;
            {
                const float* bs = cur + (32 * j + l31) * LDB + h;   // B operand: [k = 2 ks + h][column l31]
                float bq[2][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) bq[0][i] = bs[2 * i];
#pragma unroll
                for (int g4 = 0; g4 < 4 * NCH; ++g4) {
                    if (g4 + 1 < 4 * NCH) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) bq[(g4 + 1) & 1][i] = bs[2 * (4 * (g4 + 1) + i)];
                    }
                    __builtin_amdgcn_sched_barrier(0);  // the reads of the next four k-steps ahead of these four MFMAs
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * g4 + i], bq[g4 & 1][i], acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // ---- P = w exp(s - lse), accumulator layout -> the wave's LDS block ----
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float s = acc[q];
                float wv, hi, lo;
                if constexpr (USER_A) { wv = wq[q]; hi = lhi[q]; lo = llo[q]; } else { wv = wc; hi = chi; lo = clo; }
                float t = fmaf(s, kFsmLog2eHi, -hi);          // exact product, one rounding of the (small) difference
                t = fmaf(s, kFsmLog2eLo, t - lo);
                const float p = (col_ok && wv != 0.f) ? wv * __builtin_amdgcn_exp2f(t) : 0.f;
                pw[((q & 3) + 8 * (q >> 2) + 4 * h) * SLDP + l31] = p;
            }
            wave_lds_sync();
            // ---- G += P . B_block: A operand P[row l31][k = 2 ks + h], B operand B_block[2 ks + h][32 jj + l31] ----
            {
                const float* pa = pw + l31 * SLDP + h;
                const float* bb = cur + (32 * j + h) * LDB + l31;
                float pq[2], bq[2][NCH];
                pq[0] = pa[0];
#pragma unroll
                for (int jj = 0; jj < NCH; ++jj) bq[0][jj] = bb[32 * jj];
#pragma unroll
                for (int ks = 0; ks < 16; ++ks) {
                    if (ks + 1 < 16) {
                        pq[(ks + 1) & 1] = pa[2 * (ks + 1)];
#pragma unroll
                        for (int jj = 0; jj < NCH; ++jj) bq[(ks + 1) & 1][jj] = bb[2 * (ks + 1) * LDB + 32 * jj];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int jj = 0; jj < NCH; ++jj)
                        gacc[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(pq[ks & 1], bq[ks & 1][jj], gacc[jj], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            wave_lds_sync();   // the next block's P writes stay behind these reads
            fsm_quarter_write<NCH, MODE>(nxt, K, j, tid, stg);
        }
        __syncthreads();   // the next tile is whole, and nobody reads this one any more
    }

    // ---- G[row] += the wave's sums; a stationary user row with w = 0 keeps its bits ----
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t row = row0 + 32 * wave + (q & 3) + 8 * (q >> 2) + 4 * h;
        bool live = row < ma;
        if constexpr (USER_A) live = live && wq[q] != 0.f;
        if (live) {
#pragma unroll
            for (int jj = 0; jj < NCH; ++jj) {
                const int c = 32 * jj + l31;
                if (c < K) G[row * ldg + c] += gacc[jj][q];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The positives' term: one wave per segment, 64/G groups of G lanes (k_mse_pass).  acc = -sum of the gathered rows of the entries with
// a value > 0, written as the raw gradient; loss_part[seg] = sum over those entries of (lse[row] - p_k) when loss_part is not NULL.
// ---------------------------------------------------------------------------------------------
constexpr int kFsmUnroll = 4;

template <int G, int NV>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_fsm_pos_pass(
    SegView sv, const int32_t* __restrict__ other, const float* __restrict__ val, const float* __restrict__ X_old,
    const float* __restrict__ Y_old, float* __restrict__ X_out, float* __restrict__ slab, const float* __restrict__ lse,
    float* __restrict__ loss_part) {
    constexpr int NG = 64 / G;
    const int lane = threadIdx.x & 63;
    const int64_t seg = sv.seg0 + (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (seg >= sv.nseg) return;
    const int g = lane & (G - 1), grp = lane / G;
    const auto [row, beg, end] = seg_range(sv, seg);

    Frag<NV> x, acc;
    load_row<G, NV>(x, X_old, row, g);
    zero<NV>(acc);
    const float l_row = loss_part != nullptr ? lse[row] : 0.f;
    float lsum = 0.f;

    for (int64_t k0 = beg + grp; k0 < end; k0 += (int64_t)NG * kFsmUnroll) {
        Raw<NV, float> raw[kFsmUnroll];
        float a[kFsmUnroll];
        int j[kFsmUnroll];
        bool ok[kFsmUnroll];
#pragma unroll
        for (int t = 0; t < kFsmUnroll; ++t) {   // ids and values first, index clamped into the segment (k_mse_pass)
            const int64_t k = k0 + (int64_t)t * NG;
            ok[t] = k < end;
            const int64_t kc = ok[t] ? k : end - 1;
            j[t] = other[kc];
            a[t] = val[kc];
        }
#pragma unroll
        for (int t = 0; t < kFsmUnroll; ++t) load_raw<G, NV>(raw[t], Y_old, j[t], g);
#pragma unroll
        for (int t = 0; t < kFsmUnroll; ++t) {
            Frag<NV> y;
            to_frag<NV>(y, raw[t]);
            const float p = group_allsum<G>(dot_partial<NV>(x, y));
            const bool pos = ok[t] && a[t] > 0.f;   // padded slots, values <= 0 and NaN values: nothing
            lsum += pos ? l_row - p : 0.f;
            axpy<NV>(acc, pos ? -1.0f : 0.f, y);
        }
    }
    across_groups_sum<G, NV>(acc);
    if (loss_part != nullptr) {
        float l = (g == 0) ? lsum : 0.f;   // every lane of a group carries the same terms: take lane 0 of each group
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off, 64);
        if (lane == 0) loss_part[seg] = l;
    }
    if (grp == 0) finish_segment<G, NV, float>(sv, seg, acc, X_old, X_out, slab, row, g, TMF_EPI_GRAD, tmf_adam{});
}

template <int NCH, int MODE>
static int launch_fsm_lse(const float* A, const float* B, int64_t m, int64_t n, int K, int64_t lda, int64_t ldb, float* lse,
                          hipStream_t stream) {
    const size_t lds = sizeof(float) * 3 * SBK * SLD;
    const int64_t blocks = (m + SBM - 1) / SBM;
    TMF_REQUIRE_LAUNCH(blocks, 256, "tmf_fsm_lse_f32");
    hipLaunchKernelGGL((k_fsm_lse<NCH, MODE>), dim3((unsigned)blocks), dim3(256), lds, stream, A, B, m, n, K, lda, ldb, lse);
    return check_launch("tmf_fsm_lse_f32");
}

template <int NCH>
static int launch_fsm_lse_nch(const float* A, const float* B, int64_t m, int64_t n, int K, int64_t lda, int64_t ldb, float* lse,
                              hipStream_t stream) {
    if (K % 4 == 0 && (n + 4 * SBN) * ldb * 4 < ((int64_t)1 << 32))  // 32-bit byte offsets into B
        return launch_fsm_lse<NCH, 2>(A, B, m, n, K, lda, ldb, lse, stream);
    if (K % 4 == 0) return launch_fsm_lse<NCH, 1>(A, B, m, n, K, lda, ldb, lse, stream);
    return launch_fsm_lse<NCH, 0>(A, B, m, n, K, lda, ldb, lse, stream);
}

template <int NCH, int MODE, bool USER_A>
static int launch_fsm_wsum(const float* A, const float* B, int64_t ma, int64_t nb, int K, int64_t lda, int64_t ldb, const float* lse,
                           const float* w, float* G, int64_t ldg, hipStream_t stream) {
    const size_t lds = sizeof(float) * (2 * SBN * (32 * NCH + 1) + 4 * 32 * SLDP);
    static LdsGrant grant;  // per template instance
    if (int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&k_fsm_wsum<NCH, MODE, USER_A>), lds, grant)) return rc;
    const int64_t blocks = (ma + SBM - 1) / SBM;
    TMF_REQUIRE_LAUNCH(blocks, 256, "tmf_fsm_wsum_f32");
    hipLaunchKernelGGL((k_fsm_wsum<NCH, MODE, USER_A>), dim3((unsigned)blocks), dim3(256), lds, stream, A, B, ma, nb, K, lda, ldb, lse,
                       w, G, ldg);
    return check_launch("tmf_fsm_wsum_f32");
}

template <int NCH, bool USER_A>
static int launch_fsm_wsum_nch(const float* A, const float* B, int64_t ma, int64_t nb, int K, int64_t lda, int64_t ldb,
                               const float* lse, const float* w, float* G, int64_t ldg, hipStream_t stream) {
    if (K % 4 == 0 && (nb + 2 * SBN) * ldb * 4 < ((int64_t)1 << 32))  // 32-bit byte offsets into B, the tile past the end included
        return launch_fsm_wsum<NCH, 2, USER_A>(A, B, ma, nb, K, lda, ldb, lse, w, G, ldg, stream);
    return launch_fsm_wsum<NCH, 0, USER_A>(A, B, ma, nb, K, lda, ldb, lse, w, G, ldg, stream);
}

template <bool USER_A>
static int fsm_wsum(const float* A, const float* B, int64_t ma, int64_t nb, int r, int64_t lda, int64_t ldb, const float* lse,
                    const float* w, float* G, int64_t ldg, hipStream_t s) {
    if (r <= 32) return launch_fsm_wsum_nch<1, USER_A>(A, B, ma, nb, r, lda, ldb, lse, w, G, ldg, s);
    if (r <= 64) return launch_fsm_wsum_nch<2, USER_A>(A, B, ma, nb, r, lda, ldb, lse, w, G, ldg, s);
    return launch_fsm_wsum_nch<4, USER_A>(A, B, ma, nb, r, lda, ldb, lse, w, G, ldg, s);
}

static int fsm_check_tables(const char* what, const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda, int64_t ldb) {
    TMF_REQUIRE(A && B && m > 0 && n > 0 && r > 0, "%s: bad arguments", what);
    TMF_REQUIRE(lda >= r && ldb >= r && (lda % 4 == 0) && (ldb % 4 == 0) && ((uintptr_t)A % 16 == 0) && ((uintptr_t)B % 16 == 0),
                "%s: operands must be 16-byte aligned with ld %% 4 == 0", what);
    TMF_REQUIRE(m < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), "%s: too many rows", what);
    if (r > FSM_MAX_COMPONENTS) {
        set_error("%s: supports n_components <= %d (got %d)", what, FSM_MAX_COMPONENTS, r);
        return TMF_E_UNSUPPORTED;
    }
    return TMF_OK;
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_fsm_max_components(void) { return FSM_MAX_COMPONENTS; }

extern "C" int tmf_fsm_lse_f32(const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda, int64_t ldb, float* lse,
                               void* stream) {
    if (m == 0) return TMF_OK;
    if (int rc = fsm_check_tables("tmf_fsm_lse_f32", A, B, m, n, r, lda, ldb)) return rc;
    TMF_REQUIRE(lse, "tmf_fsm_lse_f32: lse is null");
    hipStream_t s = (hipStream_t)stream;
    if (r <= 32) return launch_fsm_lse_nch<1>(A, B, m, n, r, lda, ldb, lse, s);
    if (r <= 64) return launch_fsm_lse_nch<2>(A, B, m, n, r, lda, ldb, lse, s);
    return launch_fsm_lse_nch<4>(A, B, m, n, r, lda, ldb, lse, s);
}

extern "C" int tmf_fsm_wsum_f32(const float* A, const float* B, int64_t ma, int64_t nb, int r, int64_t lda, int64_t ldb,
                                const float* lse, const float* w, int user_is_a, float* G, int64_t ldg, void* stream) {
    if (ma == 0 || nb == 0) return TMF_OK;
    if (int rc = fsm_check_tables("tmf_fsm_wsum_f32", A, B, ma, nb, r, lda, ldb)) return rc;
    TMF_REQUIRE(lse && w && G && ldg >= r, "tmf_fsm_wsum_f32: lse, w or G is null, or ldg < n_components");
    TMF_REQUIRE(user_is_a == 0 || user_is_a == 1, "tmf_fsm_wsum_f32: user_is_a=%d (0: the swept rows are the users, 1: the stationary ones)",
                user_is_a);
    hipStream_t s = (hipStream_t)stream;
    if (user_is_a) return fsm_wsum<true>(A, B, ma, nb, r, lda, ldb, lse, w, G, ldg, s);
    return fsm_wsum<false>(A, B, ma, nb, r, lda, ldb, lse, w, G, ldg, s);
}

extern "C" int tmf_fsm_pos_pass_f32(const tmf_segments* seg, const int32_t* other, const float* val, const float* X_old,
                                    const float* Y_old, float* G_out, float* slab, const float* lse, float* loss_part,
                                    int n_components, void* stream) {
    if (int rc = check_segments(seg)) return rc;
    if (seg->nseg == 0) return TMF_OK;
    TMF_REQUIRE(X_old && Y_old && G_out, "tmf_fsm_pos_pass_f32: null table");
    TMF_REQUIRE(other && val, "tmf_fsm_pos_pass_f32: null entry list");
    TMF_REQUIRE(loss_part == nullptr || lse != nullptr, "tmf_fsm_pos_pass_f32: loss_part without lse");
    if (n_components < 1 || n_components > FSM_MAX_COMPONENTS) {
        set_error("tmf_fsm_pos_pass_f32: supports n_components in [1, %d] (got %d)", FSM_MAX_COMPONENTS, n_components);
        return TMF_E_UNSUPPORTED;
    }
    const RowGeom geom = row_geom(n_components);
    SegView sv = view(seg);
#define CALL(G_, NV_) \
    for_segment_pieces(sv, kWavesPerBlock, [&](unsigned blocks) { \
        hipLaunchKernelGGL((k_fsm_pos_pass<G_, NV_>), dim3(blocks), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, \
                           sv, other, val, X_old, Y_old, G_out, slab, lse, loss_part); \
    })
    TMF_DISPATCH_GEOM(geom, CALL);
#undef CALL
    return check_launch("tmf_fsm_pos_pass_f32");
}
