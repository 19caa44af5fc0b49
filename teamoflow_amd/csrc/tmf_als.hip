// Alternating least squares (EXTENSION): tmf_gram_f32 and tmf_als_solve_rows_f32.
//
// tmf_als_solve_rows_f32 - one workgroup of four waves per solved row.  For the row's stored entries k (column j_k, weight w_k, target
// t_k) it builds  A = G0 + reg I + sum_k w_k y_k y_k^T,  b = sum_k t_k y_k  (y_k = Y[j_k, :r]) and solves A x = b by Cholesky, all fp32:
//   1. Entries are staged in batches of ALS_KB through LDS (the gathered rows zero-padded to RP = 32 ceil(r / 32) columns, w and t);
//      the next batch's rows are already in flight (registers) while this one is consumed.
//   2. The lower 32 x 32 tiles of sum w y y^T accumulate on v_mfma_f32_32x32x2_f32 with the entries as the K dimension - bit for bit
//      an fmaf chain in entry order.  The NT (NT + 1) / 2 tiles are dealt round-robin to the four waves (3, 3, 2, 2 at r = 128);
//      waves 2 and 3, which hold the fewest, also carry b (one column per thread, an fmaf chain in entry order).
//   3. The tiles go through LDS (packed lower triangle, aliasing the staging buffer) into a 2-D cyclic register layout: thread
//      (ty, tx) of 16 x 16 holds A[ty + 16 a][tx + 16 b], a >= b, where G0 and reg are added.
//   4. Right-looking Cholesky, one barrier per column: the owners of column k publish it (double-buffered), every thread rescales the
//      entries it needs by 1 / sqrt(pivot) itself and updates its registers.  b rides along as one more row, so the forward solve
//      L z = b costs nothing extra.  The finished column goes back to the packed triangle in LDS.
//   5. Wave 0 solves L^T x = z from the last row up, z in registers, one readlane per step and the next row of L prefetched.
// Every sum runs in a fixed order and nothing depends on the launch: a row's result is a function of its entries, Y, G0 and reg only.
// A pivot that is not a positive finite number fails the row: x = 0 and *n_failed += 1 (the block's barriers stay uniform, since
// every thread reads the same pivot).
// LDS at r = 128: 33,024 B triangle / staging + 2.5 KB vectors = 35,600 B; registers: 48 accumulator + 32 prefetch, later 36 matrix
// elements - the compiler allocates about 240 in all, so two workgroups share a CU.
//
// tmf_gram_f32 - G = T^T T: blocks of rows give partial [r, r] sums (8 x 8 register tiles, rows staged in LDS), a second kernel adds
// the partials in block order.  No atomics; element (i, j) and (j, i) run the same chain on commuted products, so G is exactly symmetric.
// tmf_gram_wide_f32 - the same for r <= 256: the rows are staged 256 wide and blockIdx.y names one of the four 128 x 128 quadrants.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int ALS_THREADS = 256;
constexpr int ALS_KB = 64;             // entries per staged batch
constexpr int ALS_MAX_BLOCKS = 1 << 22;   // the blocks stride the rows beyond
constexpr int ALS_MAX_R = 128;

typedef float als_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, row-major

// 1 / sqrt(d) for a positive finite d: v_rsq_f32 and one Newton step - a fixed instruction sequence (the same bits for the same d
// on every thread), a handful of dependent instructions where an IEEE square root and division are some sixty, and this value stands
// on the serial path of every column of the factorisation.
__device__ __forceinline__ float als_rsqrt(float d) {
    const float y = __frsqrt_rn(d);
    return y * fmaf(-0.5f * d * y, y, 1.5f);
}

// Registers: about 240 at r = 128 (two workgroups per CU).  Bounds of 168 and 128 registers were compiled and both spill to scratch
// (43 and 82 registers), so the kernel is left unbounded.
template <int NT>
__global__ __launch_bounds__(ALS_THREADS) void k_als_solve_rows(const float* __restrict__ Y, int r, int64_t ldy,
                                                                const float* __restrict__ G0, int64_t ldg,
                                                                const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                const float* __restrict__ w, const float* __restrict__ t, float reg,
                                                                const int32_t* __restrict__ ids, int64_t q, float* __restrict__ X,
                                                                int64_t ldx, int32_t* __restrict__ n_failed) {
    constexpr int RP = 32 * NT;                 // padded width
    constexpr int NB = 2 * NT;                  // 16-wide blocks of the cyclic layout
    constexpr int NTILES = NT * (NT + 1) / 2;   // lower 32 x 32 tiles
    constexpr int SLOTS = (NTILES + 3) / 4;     // tiles per wave
    constexpr int TRI = RP * (RP + 1) / 2;
    constexpr int STAGE = ALS_KB * RP;
    constexpr int MAT = TRI > STAGE ? TRI : STAGE;
    constexpr int NCH = RP / 4;                 // 16-byte chunks per staged row
    constexpr int PASSES = ALS_KB * NCH / ALS_THREADS;   // chunks per thread and batch: chunk tid + 256 ps of the batch, row-major
    static_assert(PASSES * ALS_THREADS == ALS_KB * NCH, "a batch is a whole number of passes");
    constexpr int NV = (RP + 63) / 64;          // columns per lane of the back substitution

    __shared__ __attribute__((aligned(16))) float mat[MAT];   // staged rows, then the packed lower triangle of A / L
    __shared__ float wt[2][ALS_KB];                            // w and t of the staged entries
    __shared__ float colk[2][RP + 1];                          // column k as published (even / odd k), b_k behind it
    __shared__ float vec[RP];                                  // b, then z
    __shared__ float invd[RP];                                 // 1 / L[k][k]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int tx = tid & 15, ty = tid >> 4;

    int tI[SLOTS], tJ[SLOTS];   // this wave's tiles (wave-uniform)
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int ti = wave + 4 * s;
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= ti) ++I;
        tI[s] = I;
        tJ[s] = ti - I * (I + 1) / 2;
    }

    for (int64_t p = blockIdx.x; p < q; p += gridDim.x) {
        const int64_t row = ids ? (int64_t)ids[p] : p;
        const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
        float* __restrict__ xrow = X + row * ldx;
        if (e1 <= e0) {   // no entries: b = 0, so x = 0
            for (int64_t c = tid; c < ldx; c += ALS_THREADS) xrow[c] = 0.f;
            continue;
        }

        // ---- 1, 2: accumulate sum w y y^T (MFMA) and b ----
        als_f32x16 acc[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[s][g] = 0.f;
        float bsum = 0.f;
        float4 pre[PASSES];
        float prew = 0.f, pret = 0.f;
        auto fetch = [&](int64_t base) {
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps) {
                const int chunk = tid + ALS_THREADS * ps;
                const int64_t e = base + chunk / NCH;
                pre[ps] = e < e1 ? load_row_chunk(Y + (int64_t)col[e] * ldy, chunk % NCH, r) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if (tid < ALS_KB) {
                const int64_t e = base + tid;
                prew = e < e1 ? w[e] : 0.f;
                pret = e < e1 ? t[e] : 0.f;
            }
        };
        fetch(e0);
        for (int64_t base = e0; base < e1; base += ALS_KB) {
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps)
                *reinterpret_cast<float4*>(&mat[4 * (tid + ALS_THREADS * ps)]) = pre[ps];
            if (tid < ALS_KB) {
                wt[0][tid] = prew;
                wt[1][tid] = pret;
            }
            __syncthreads();
            if (base + ALS_KB < e1) fetch(base + ALS_KB);
            const int64_t left = e1 - base;
            const int nk = left < ALS_KB ? (int)left : ALS_KB;   // rows [nk, ALS_KB) of the batch are zeros with w = t = 0
#pragma unroll 4
            for (int k = 0; k < nk; k += 2) {   // unrolled so that the LDS reads of several steps are in flight before the first MFMA
                const int kk = k + h;
                const float wk = wt[0][kk];
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    if (wave + 4 * s < NTILES) {
                        const float a = wk * mat[kk * RP + 32 * tI[s] + l31];
                        const float b = mat[kk * RP + 32 * tJ[s] + l31];
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[s], 0, 0, 0);
                    }
                }
            }
            if (tid >= 128 && tid - 128 < RP) {
                const int c = tid - 128;
#pragma unroll 8
                for (int k = 0; k < nk; ++k) bsum = fmaf(wt[1][k], mat[k * RP + c], bsum);
            }
            __syncthreads();
        }

        // ---- 3: tiles -> packed lower triangle -> cyclic registers ----
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            if (wave + 4 * s < NTILES) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int i = 32 * tI[s] + (g & 3) + 8 * (g >> 2) + 4 * h, j = 32 * tJ[s] + l31;
                    if (j <= i) mat[tri(i, j)] = acc[s][g];
                }
            }
        }
        if (tid >= 128 && tid - 128 < RP) vec[tid - 128] = bsum;
        __syncthreads();
        float a[NB][NB], bacc[NB];
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) {
#pragma unroll
            for (int jb = 0; jb <= ib; ++jb) {
                const int i = ty + 16 * ib, j = tx + 16 * jb;
                float v = 0.f;
                if (j <= i && i < r) {
                    v = mat[tri(i, j)];
                    if (G0) v += G0[(int64_t)i * ldg + j];
                    if (i == j) v += reg;
                }
                a[ib][jb] = v;
            }
            bacc[ib] = vec[tx + 16 * ib];
        }
        __syncthreads();

        // ---- 4: Cholesky with b as one more row ----
        bool failed = false;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) {
            for (int kx = 0; kx < 16; ++kx) {
                const int k = 16 * kb + kx;
                if (k >= r) break;
                float* ck = colk[k & 1];
                if (tx == kx) {
#pragma unroll
                    for (int ib = kb; ib < NB; ++ib) ck[ty + 16 * ib] = a[ib][kb];
                    if (ty == 15) ck[RP] = bacc[kb];
                }
                __syncthreads();
                const float d = ck[k];
                if (!(d > 0.f) || !(d <= 3.402823466e38f)) {   // the same value in every thread
                    failed = true;
                    break;
                }
                const float inv = als_rsqrt(d);
                float li[NB], lj[NB];
#pragma unroll
                for (int b = kb; b < NB; ++b) {
                    const int i = ty + 16 * b, j = tx + 16 * b;
                    li[b] = i > k ? ck[i] * inv : 0.f;   // rows up to k are finished: a zero factor leaves them as they are
                    lj[b] = j > k ? ck[j] * inv : 0.f;
                }
#pragma unroll
                for (int ib = kb; ib < NB; ++ib)
#pragma unroll
                    for (int jb = kb; jb <= ib; ++jb) a[ib][jb] = fmaf(-li[ib], lj[jb], a[ib][jb]);
                if (ty == 15) {
                    const float zk = ck[RP] * inv;
#pragma unroll
                    for (int jb = kb; jb < NB; ++jb) bacc[jb] = fmaf(-lj[jb], zk, bacc[jb]);
                    if (tx == kx) {
                        vec[k] = zk;
                        invd[k] = inv;
                    }
                }
                if (tx == kx) {
#pragma unroll
                    for (int ib = kb; ib < NB; ++ib) {
                        const int i = ty + 16 * ib;
                        if (i > k && i < r) mat[tri(i, k)] = li[ib];
                    }
                }
            }
            if (failed) break;
        }
        __syncthreads();

        // ---- 5: L^T x = z, or the failed row ----
        if (failed) {
            for (int64_t c = tid; c < ldx; c += ALS_THREADS) xrow[c] = 0.f;
            if (tid == 0) atomicAdd(n_failed, 1);
        } else {
            for (int64_t c = r + tid; c < ldx; c += ALS_THREADS) xrow[c] = 0.f;
            if (wave == 0) {
                float z[NV], iv[NV], x[NV], lnext[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int c = lane + 64 * v;
                    z[v] = c < r ? vec[c] : 0.f;
                    iv[v] = c < r ? invd[c] : 0.f;
                    x[v] = 0.f;
                    lnext[v] = c < r - 1 ? mat[tri(r - 1, c)] : 0.f;
                }
                for (int k = r - 1; k >= 0; --k) {
                    float lcur[NV];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const int c = lane + 64 * v;
                        lcur[v] = lnext[v];
                        lnext[v] = (k > 0 && c < k - 1) ? mat[tri(k - 1, c)] : 0.f;
                    }
                    float cand = z[0] * iv[0];
                    if (NV == 2 && k >= 64) cand = z[NV - 1] * iv[NV - 1];
                    const float xk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand), k & 63));
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        if (lane + 64 * v == k) x[v] = xk;
                        z[v] = fmaf(-lcur[v], xk, z[v]);   // lcur is zero at and beyond column k
                    }
                }
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int c = lane + 64 * v;
                    if (c < r) xrow[c] = x[v];
                }
            }
        }
        __syncthreads();   // the next row's staging overwrites mat
    }
}

// ---------------------------------------------------------------------------------------------
// Gram matrix
// ---------------------------------------------------------------------------------------------
constexpr int GRAM_THREADS = 256;
constexpr int GRAM_ROWS = 32;          // rows staged at a time
constexpr int GRAM_WIDTH = ALS_MAX_R;  // staged width (zero-padded); tmf_gram_wide_f32 stages twice that
constexpr int GRAM_WIDE_MAX_R = 2 * GRAM_WIDTH;
constexpr int GRAM_MAX_BLOCKS = 512;

inline int64_t gram_rows_per_block(int64_t n_rows) {
    const int64_t per = (n_rows + GRAM_MAX_BLOCKS - 1) / GRAM_MAX_BLOCKS;
    return (per + GRAM_ROWS - 1) / GRAM_ROWS * GRAM_ROWS;
}
inline int64_t gram_blocks(int64_t n_rows) {
    if (n_rows <= 0) return 0;
    const int64_t per = gram_rows_per_block(n_rows);
    return (n_rows + per - 1) / per;
}

// Block b sums rows [b per, (b + 1) per) in row order into part[b][r][r]; thread (ty, tx) holds the 8 x 8 tile at (i0, j0) =
// (8 ty, 8 tx) + 128 (qi, qj), (qi, qj) the quadrant blockIdx.y names (WIDTH = 128: the only one).
template <int WIDTH>
__global__ __launch_bounds__(GRAM_THREADS) void k_gram_partial(const float* __restrict__ T, int64_t n_rows, int r, int64_t ldt,
                                                               int64_t per, float* __restrict__ part) {
    constexpr int Q = WIDTH / GRAM_WIDTH;   // quadrants per side
    __shared__ __attribute__((aligned(16))) float Ts[GRAM_ROWS][WIDTH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = 8 * ty + GRAM_WIDTH * ((int)blockIdx.y / Q), j0 = 8 * tx + GRAM_WIDTH * ((int)blockIdx.y % Q);
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n_rows ? lo + per : n_rows;
    const bool works = i0 < r && j0 < r;
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int64_t base = lo; base < hi; base += GRAM_ROWS) {
        for (int idx = tid; idx < GRAM_ROWS * (WIDTH / 4); idx += GRAM_THREADS) {
            const int k = idx / (WIDTH / 4), c = idx % (WIDTH / 4);
            const int64_t row = base + k;
            const float4 v = row < hi ? load_row_chunk(T + row * ldt, c, r) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(&Ts[k][4 * c]) = v;
        }
        __syncthreads();
        if (works) {
            for (int k = 0; k < GRAM_ROWS; ++k) {   // rows beyond hi are zeros: they add +0
                float x[8], y[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    x[i] = Ts[k][i0 + i];
                    y[i] = Ts[k][j0 + i];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(x[i], y[j], acc[i][j]);
            }
        }
        __syncthreads();
    }
    if (works) {
        float* out = part + (int64_t)blockIdx.x * r * r;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int gi = i0 + i, gj = j0 + j;
                if (gi < r && gj < r) out[gi * r + gj] = acc[i][j];
            }
    }
}

__global__ __launch_bounds__(GRAM_THREADS) void k_gram_combine(const float* __restrict__ part, int64_t blocks, int r,
                                                               float* __restrict__ G, int64_t ldg) {
    const int idx = blockIdx.x * GRAM_THREADS + threadIdx.x;
    if (idx >= r * r) return;
    float s = 0.f;
    for (int64_t b = 0; b < blocks; ++b) s += part[b * r * r + idx];
    G[(int64_t)(idx / r) * ldg + idx % r] = s;
}

inline bool als_reg_valid(float reg) { return reg > 0.f && reg <= 3.402823466e38f; }   // NaN fails the comparison

// tmf_gram_f32 (WIDTH = 128) and tmf_gram_wide_f32 (WIDTH = 256)
template <int WIDTH>
size_t gram_workspace_bytes(int64_t n_rows, int r) {
    if (r < 1 || r > WIDTH) return 0;
    const int64_t blocks = gram_blocks(n_rows);
    return (size_t)(blocks > 0 ? blocks : 1) * (size_t)r * (size_t)r * sizeof(float);
}

template <int WIDTH>
int gram(const char* what, const float* T, int64_t n_rows, int r, int64_t ldt, float* G, int64_t ldg, void* workspace,
         size_t workspace_bytes, void* stream) {
    TMF_REQUIRE(r >= 1 && r <= WIDTH, "%s: r = %d outside [1, %d]", what, r, WIDTH);
    TMF_REQUIRE(n_rows >= 0, "%s: n_rows = %lld", what, (long long)n_rows);
    TMF_REQUIRE(ldt >= r && ldt % 4 == 0, "%s: ldt = %lld must be >= r = %d and a multiple of 4", what, (long long)ldt, r);
    TMF_REQUIRE(ldg >= r, "%s: ldg = %lld must be >= r = %d", what, (long long)ldg, r);
    TMF_REQUIRE(G && (uintptr_t)G % 4 == 0, "%s: G is required", what);
    TMF_REQUIRE(n_rows == 0 || (T && (uintptr_t)T % 16 == 0), "%s: T must be 16-byte aligned", what);
    TMF_REQUIRE(workspace && (uintptr_t)workspace % 4 == 0 && workspace_bytes >= gram_workspace_bytes<WIDTH>(n_rows, r),
                "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, gram_workspace_bytes<WIDTH>(n_rows, r));
    const int64_t blocks = gram_blocks(n_rows);
    if (blocks > 0) {
        constexpr int Q = WIDTH / GRAM_WIDTH;
        hipLaunchKernelGGL(k_gram_partial<WIDTH>, dim3((unsigned)blocks, Q * Q), dim3(GRAM_THREADS), 0, (hipStream_t)stream, T, n_rows, r,
                           ldt, gram_rows_per_block(n_rows), static_cast<float*>(workspace));
        const int rc = check_launch(what);
        if (rc != TMF_OK) return rc;
    }
    hipLaunchKernelGGL(k_gram_combine, dim3((unsigned)((r * r + GRAM_THREADS - 1) / GRAM_THREADS)), dim3(GRAM_THREADS), 0,
                       (hipStream_t)stream, static_cast<const float*>(workspace), blocks, r, G, ldg);
    return check_launch(what);
}

}  // namespace tmf

using namespace tmf;

extern "C" size_t tmf_gram_workspace_bytes(int64_t n_rows, int r) { return gram_workspace_bytes<GRAM_WIDTH>(n_rows, r); }

extern "C" int tmf_gram_f32(const float* T, int64_t n_rows, int r, int64_t ldt, float* G, int64_t ldg, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return gram<GRAM_WIDTH>("tmf_gram_f32", T, n_rows, r, ldt, G, ldg, workspace, workspace_bytes, stream);
}

extern "C" size_t tmf_gram_wide_workspace_bytes(int64_t n_rows, int r) { return gram_workspace_bytes<GRAM_WIDE_MAX_R>(n_rows, r); }

extern "C" int tmf_gram_wide_f32(const float* T, int64_t n_rows, int r, int64_t ldt, float* G, int64_t ldg, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return gram<GRAM_WIDE_MAX_R>("tmf_gram_wide_f32", T, n_rows, r, ldt, G, ldg, workspace, workspace_bytes, stream);
}

extern "C" int tmf_als_solve_rows_f32(const float* Y, int64_t n_other, int r, int64_t ldy, const float* G0, int64_t ldg,
                                      const int64_t* rowptr, const int32_t* col, const float* w, const float* t, float reg,
                                      const int32_t* ids, int64_t q, float* X, int64_t ldx, int32_t* n_failed, void* stream) {
    const char* what = "tmf_als_solve_rows_f32";
    TMF_REQUIRE(r >= 1 && r <= ALS_MAX_R, "%s: r = %d outside [1, %d]", what, r, ALS_MAX_R);
    TMF_REQUIRE(als_reg_valid(reg), "%s: reg = %g must be finite and > 0", what, (double)reg);
    TMF_REQUIRE(ldy >= r && ldy % 4 == 0, "%s: ldy = %lld must be >= r = %d and a multiple of 4", what, (long long)ldy, r);
    TMF_REQUIRE(ldx >= r, "%s: ldx = %lld must be >= r = %d", what, (long long)ldx, r);
    TMF_REQUIRE(!G0 || ldg >= r, "%s: ldg = %lld must be >= r = %d", what, (long long)ldg, r);
    TMF_REQUIRE(q >= 0 && n_other >= 0, "%s: q = %lld, n_other = %lld", what, (long long)q, (long long)n_other);
    if (q == 0) return TMF_OK;
    TMF_REQUIRE(Y && X && rowptr && col && w && t && n_failed, "%s: Y, X, rowptr, col, w, t and n_failed are required", what);
    TMF_REQUIRE((uintptr_t)Y % 16 == 0 && (uintptr_t)X % 16 == 0, "%s: Y and X must be 16-byte aligned", what);
    TMF_REQUIRE(!G0 || (uintptr_t)G0 % 4 == 0, "%s: G0 must be 4-byte aligned", what);
    const int64_t blocks = q < ALS_MAX_BLOCKS ? q : ALS_MAX_BLOCKS;
    TMF_REQUIRE_LAUNCH(blocks, ALS_THREADS, what);
#define TMF_ALS_LAUNCH(NT)                                                                                                      \
    hipLaunchKernelGGL(k_als_solve_rows<NT>, dim3((unsigned)blocks), dim3(ALS_THREADS), 0, (hipStream_t)stream, Y, r, ldy, G0, \
                       ldg, rowptr, col, w, t, reg, ids, q, X, ldx, n_failed)
    switch ((r + 31) / 32) {
        case 1: TMF_ALS_LAUNCH(1); break;
        case 2: TMF_ALS_LAUNCH(2); break;
        case 3: TMF_ALS_LAUNCH(3); break;
        default: TMF_ALS_LAUNCH(4); break;
    }
#undef TMF_ALS_LAUNCH
    return check_launch(what);
}
