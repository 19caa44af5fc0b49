// ReLUEmbedding (embedding_graphs.py:61-87): E = relu(F Wr + b) W, aux width 5 r.  The sparse products F Wr and F^T dZ are
// tmf_feat_pass_f32's; this file is the dense middle of the layer on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): three tall-skinny
// GEMMs with the ReLU folded into their staging or their epilogue, and the fresh-Adam step of W from split-K partials.
// The hidden value is h = max(fl(z + b), 0) and a unit is on where fl(z + b) > 0 - the same expression in every kernel; H is never
// stored.  Contracts in include/tmf.h.
//
// Tiling (k_predict_gemm's): 256 threads = 4 waves in a 2x2 grid, each wave a 64x64 block as 2x2 MFMA tiles; 128 x 128 x 16 block
// panels k-major in LDS.  An operand that is K-contiguous in memory (a row of Z along aux, of G or W along r) is staged transposed,
// one float per store, into a panel of row stride 129; an operand that is already k-major (W[k][n] in the forward product, Z and G
// by table row in the weight gradient) is staged with 16-byte stores into a panel of row stride 132.  Either way the MFMA operand
// read (lane l -> row l & 31 of k = l >> 5) walks consecutive floats.  The next panels are loaded into registers before the MFMA
// loop of the current ones.
#include "tmf_common.h"

namespace tmf {

typedef float relu_f32x16 __attribute__((ext_vector_type(16)));

constexpr int RBM = 128, RBN = 128, RBK = 16;
constexpr int kLdT = RBM + 1;   // panel staged transposed (scalar stores)
constexpr int kLdV = RBM + 4;   // panel staged with float4 stores

constexpr int64_t kDwMinRows = 512;   // table rows per split-K part at least
constexpr int64_t kDwMaxParts = 256;  // parts at most (one tile row of the grid per CU at the widest aux)

inline int64_t relu_rows_per_part(int64_t n_rows) {
    int64_t per = (n_rows + kDwMaxParts - 1) / kDwMaxParts;
    if (per < kDwMinRows) per = kDwMinRows;
    return (per + RBK - 1) / RBK * RBK;
}

inline int64_t relu_part_rows(int64_t n_rows) {
    if (n_rows <= 0) return 0;
    const int64_t per = relu_rows_per_part(n_rows);
    return (n_rows + per - 1) / per;
}

__device__ __forceinline__ float relu_hidden(float z, float b) {
    const float s = z + b;
    return s > 0.f ? s : 0.f;
}

__device__ __forceinline__ float4 relu_hidden4(const float4 z, const float4 b) {
    return make_float4(relu_hidden(z.x, b.x), relu_hidden(z.y, b.y), relu_hidden(z.z, b.z), relu_hidden(z.w, b.w));
}

// columns c .. c + 3 of a float4: those at or beyond `width` become 0 (whatever the table holds there)
__device__ __forceinline__ float4 keep_below(const float4 v, int c, int width) {
    return make_float4(c + 0 < width ? v.x : 0.f, c + 1 < width ? v.y : 0.f, c + 2 < width ? v.z : 0.f, c + 3 < width ? v.w : 0.f);
}

// A panel on its way from memory to LDS: the raw 16-byte pieces a thread loaded (and, for a hidden operand, the bias beside them).
// Loading and finishing are two steps so that nothing touches the loaded registers before the MFMA loop of the previous panels has
// been issued - a use right behind the load would make the wave wait for it there.  No branch surrounds a load either (the compiler
// would wait for each in turn): an address beyond the table is clamped into it and the value replaced when the panel is finished.
struct Staged {
    float4 v[2], bias[2];
};

// ---- K-contiguous operand: X[row][k], 128 rows x 16 k per panel; thread -> rows tid / 4 + 64 h, k-quad tid % 4 ----
template <bool HIDDEN>
__device__ __forceinline__ void load_kcontig(Staged& p, const float* __restrict__ X, int64_t ldx, int64_t row0, int64_t n_rows, int k0,
                                             int K, const float* __restrict__ bias, int tid) {
    const int srow = tid >> 2, kk = k0 + 4 * (tid & 3);
    const int kc = kk < K ? kk : 0;   // kk is a multiple of 4 below K <= ldx, ldx a multiple of 4: the 16 bytes lie inside the row
    if (HIDDEN) p.bias[0] = *reinterpret_cast<const float4*>(bias + kc);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t row = row0 + srow + 64 * h;
        p.v[h] = *reinterpret_cast<const float4*>(X + (row < n_rows ? row : n_rows - 1) * ldx + kc);
    }
}

template <bool HIDDEN>
__device__ __forceinline__ void store_kcontig(float* __restrict__ panel, const Staged& p, int64_t row0, int64_t n_rows, int k0, int K,
                                              int tid) {
    const int srow = tid >> 2, kq = 4 * (tid & 3), kk = k0 + kq;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = srow + 64 * h;
        float4 x = p.v[h];
        if (HIDDEN) x = relu_hidden4(x, p.bias[0]);
        x = keep_below(x, kk, (row0 + r < n_rows && kk < K) ? K : 0);
        panel[(kq + 0) * kLdT + r] = x.x;
        panel[(kq + 1) * kLdT + r] = x.y;
        panel[(kq + 2) * kLdT + r] = x.z;
        panel[(kq + 3) * kLdT + r] = x.w;
    }
}

// ---- k-major operand: X[k][col], 16 k x 128 columns per panel; thread -> k = tid / 16, columns 4 (tid % 16) + 64 h ----
template <bool HIDDEN>
__device__ __forceinline__ void load_kmajor(Staged& p, const float* __restrict__ X, int64_t ldx, int64_t k0, int64_t k_end, int col0,
                                            int width, const float* __restrict__ bias, int tid) {
    const int64_t k = k0 + (tid >> 4);
    const int64_t kc = k < k_end ? k : k_end - 1;   // k_end >= 1
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = col0 + 4 * (tid & 15) + 64 * h;
        const int cc = c < width ? c : 0;   // c is a multiple of 4 below width <= the table's ld, a multiple of 4
        p.v[h] = *reinterpret_cast<const float4*>(X + kc * ldx + cc);
        if (HIDDEN) p.bias[h] = *reinterpret_cast<const float4*>(bias + cc);
    }
}

template <bool HIDDEN>
__device__ __forceinline__ void store_kmajor(float* __restrict__ panel, const Staged& p, int64_t k0, int64_t k_end, int col0, int width,
                                             int tid) {
    const int kl = tid >> 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cl = 4 * (tid & 15) + 64 * h, c = col0 + cl;
        float4 x = p.v[h];
        if (HIDDEN) x = relu_hidden4(x, p.bias[h]);
        *reinterpret_cast<float4*>(panel + kl * kLdV + cl) = keep_below(x, c, (k0 + kl < k_end && c < width) ? width : 0);
    }
}

template <int LDA, int LDB>
__device__ __forceinline__ void mfma_panels(relu_f32x16 (&acc)[2][2], const float* __restrict__ As, const float* __restrict__ Bs,
                                            int wr, int wc, int lane) {
#pragma unroll
    for (int ks = 0; ks < RBK; ks += 2) {
        const int kl = ks + (lane >> 5), rl = lane & 31;
        float af[2], bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = As[kl * LDA + wr * 64 + i * 32 + rl];
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = Bs[kl * LDB + wc * 64 + j * 32 + rl];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
}

__device__ __forceinline__ void zero_acc(relu_f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
}

// C/D map of the 32x32 tile (k_predict_gemm): col = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
#define TMF_RELU_FOR_EACH_ACC(ROW, COL, VAL, ...)                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) { \
        const int COL = wc * 64 + j_ * 32 + (lane & 31);                                               \
        _Pragma("unroll") for (int q_ = 0; q_ < 16; ++q_) {                                            \
            const int ROW = wr * 64 + i_ * 32 + (q_ & 3) + 8 * (q_ >> 2) + 4 * (lane >> 5);            \
            const float VAL = acc[i_][j_][q_];                                                         \
            __VA_ARGS__                                                                                \
        }                                                                                              \
    }

// E[i, c] = sum_a h[i, a] W[a, c] for c < r, 0 for r <= c < ldw.  M = rows, N = ldw, K = aux.
__global__ __launch_bounds__(256) void k_relu_embed(const float* __restrict__ Z, const float* __restrict__ b,
                                                    const float* __restrict__ W, float* __restrict__ E, int64_t n_rows, int aux,
                                                    int r, int ldz, int ldw, int tiles_n) {
    __shared__ __attribute__((aligned(16))) float As[RBK * kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[RBK * kLdV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int64_t row0 = (int64_t)(blockIdx.x / tiles_n) * RBM;
    const int col0 = (int)(blockIdx.x % tiles_n) * RBN;
    relu_f32x16 acc[2][2];
    zero_acc(acc);
    Staged a, w;
    load_kcontig<true>(a, Z, ldz, row0, n_rows, 0, aux, b, tid);
    load_kmajor<false>(w, W, ldw, 0, aux, col0, r, nullptr, tid);
    for (int k0 = 0; k0 < aux; k0 += RBK) {
        store_kcontig<true>(As, a, row0, n_rows, k0, aux, tid);
        store_kmajor<false>(Bs, w, k0, aux, col0, r, tid);
        __syncthreads();
        if (k0 + RBK < aux) {
            load_kcontig<true>(a, Z, ldz, row0, n_rows, k0 + RBK, aux, b, tid);
            load_kmajor<false>(w, W, ldw, k0 + RBK, aux, col0, r, nullptr, tid);
        }
        mfma_panels<kLdT, kLdV>(acc, As, Bs, wr, wc, lane);
        __syncthreads();
    }
    TMF_RELU_FOR_EACH_ACC(rr, cc, val, {
        const int64_t row = row0 + rr;
        const int c = col0 + cc;
        if (row < n_rows && c < ldw) E[row * ldw + c] = val;   // columns r .. ldw: W was staged as zeros there
    })
}

// dZ[i, a] = on(i, a) ? sum_c G[i, c] W[a, c] : 0 for a < aux, 0 for aux <= a < ldz.  M = rows, N = ldz, K = r.
__global__ __launch_bounds__(256) void k_relu_dhidden(const float* __restrict__ G, const float* __restrict__ W,
                                                      const float* __restrict__ Z, const float* __restrict__ b,
                                                      float* __restrict__ dZ, int64_t n_rows, int aux, int r, int ldz, int ldw,
                                                      int tiles_n) {
    __shared__ __attribute__((aligned(16))) float As[RBK * kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[RBK * kLdT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int64_t row0 = (int64_t)(blockIdx.x / tiles_n) * RBM;
    const int col0 = (int)(blockIdx.x % tiles_n) * RBN;
    relu_f32x16 acc[2][2];
    zero_acc(acc);
    uint64_t on = 0;    // bit (2 i + j) 16 + q: the unit behind acc[i][j][q] is on
    if (col0 < aux) {   // the same for the whole workgroup; a tile of padding columns only writes its zeros
        Staged g, w;
        load_kcontig<false>(g, G, ldw, row0, n_rows, 0, r, nullptr, tid);
        load_kcontig<false>(w, W, ldw, col0, aux, 0, r, nullptr, tid);
        // the mask first, from 64 loads that are all in flight at once: addresses clamped into the table instead of branches (a row
        // or column beyond it is never stored), then one compare per element.  An epilogue that loads z where it stores would wait
        // for every load in turn
        float z[2][2][16];
        float bias[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = col0 + wc * 64 + j * 32 + (lane & 31);
            bias[j] = b[c < aux ? c : aux - 1];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = col0 + wc * 64 + j * 32 + (lane & 31);
                const int cz = c < aux ? c : aux - 1;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int64_t row = row0 + wr * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                    z[i][j][q] = Z[(row < n_rows ? row : n_rows - 1) * ldz + cz];
                }
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bool live = col0 + wc * 64 + j * 32 + (lane & 31) < aux;
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (live && z[i][j][q] + bias[j] > 0.f) on |= 1ull << ((2 * i + j) * 16 + q);
            }
        for (int k0 = 0; k0 < r; k0 += RBK) {
            store_kcontig<false>(As, g, row0, n_rows, k0, r, tid);
            store_kcontig<false>(Bs, w, col0, aux, k0, r, tid);
            __syncthreads();
            if (k0 + RBK < r) {
                load_kcontig<false>(g, G, ldw, row0, n_rows, k0 + RBK, r, nullptr, tid);
                load_kcontig<false>(w, W, ldw, col0, aux, k0 + RBK, r, nullptr, tid);
            }
            mfma_panels<kLdT, kLdT>(acc, As, Bs, wr, wc, lane);
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = col0 + wc * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t row = row0 + wr * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                if (row < n_rows && c < ldz) dZ[row * ldz + c] = (on >> ((2 * i + j) * 16 + q)) & 1 ? acc[i][j][q] : 0.f;
            }
        }
}

// part[p][a, c] = sum over the rows i of block p of h[i, a] G[i, c] for a < aux, c < r; 0 for r <= c < ldw.  M = aux, N = ldw,
// K = the rows of the block; both operands are k-major as stored.
__global__ __launch_bounds__(256) void k_relu_dweights(const float* __restrict__ Z, const float* __restrict__ b,
                                                       const float* __restrict__ G, float* __restrict__ part, int64_t n_rows,
                                                       int64_t rows_per, int aux, int r, int ldz, int ldw, int tiles_m, int tiles_n) {
    __shared__ __attribute__((aligned(16))) float As[RBK * kLdV];
    __shared__ __attribute__((aligned(16))) float Bs[RBK * kLdV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int tiles = tiles_m * tiles_n;
    const int64_t p = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x % tiles);
    const int a0 = (t / tiles_n) * RBM, c0 = (t % tiles_n) * RBN;
    const int64_t i0 = p * rows_per;
    const int64_t i1 = i0 + rows_per < n_rows ? i0 + rows_per : n_rows;
    relu_f32x16 acc[2][2];
    zero_acc(acc);
    Staged h, g;
    load_kmajor<true>(h, Z, ldz, i0, i1, a0, aux, b, tid);
    load_kmajor<false>(g, G, ldw, i0, i1, c0, r, nullptr, tid);
    for (int64_t k0 = i0; k0 < i1; k0 += RBK) {
        store_kmajor<true>(As, h, k0, i1, a0, aux, tid);
        store_kmajor<false>(Bs, g, k0, i1, c0, r, tid);
        __syncthreads();
        if (k0 + RBK < i1) {
            load_kmajor<true>(h, Z, ldz, k0 + RBK, i1, a0, aux, b, tid);
            load_kmajor<false>(g, G, ldw, k0 + RBK, i1, c0, r, nullptr, tid);
        }
        mfma_panels<kLdV, kLdV>(acc, As, Bs, wr, wc, lane);
        __syncthreads();
    }
    float* out = part + p * (int64_t)aux * ldw;
    TMF_RELU_FOR_EACH_ACC(rr, cc, val, {
        const int a = a0 + rr;
        const int c = c0 + cc;
        if (a < aux && c < ldw) out[(int64_t)a * ldw + c] = val;
    })
}

// g = sum_p part[p] in the order p = 0, 1, ..; W_out = fresh_adam(W_old, g) for c < r, zeros beyond.  One float4 per lane.
__global__ __launch_bounds__(256) void k_relu_adam_weights(const float4* __restrict__ part, int64_t part_rows,
                                                           const float4* __restrict__ W_old, float4* __restrict__ W_out,
                                                           float4* __restrict__ g_out, int64_t n4, int L4, int r, tmf_adam adam) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t p = 0; p < part_rows; ++p) {
        const float4 v = part[p * n4 + i];
        g.x += v.x;
        g.y += v.y;
        g.z += v.z;
        g.w += v.w;
    }
    const int c = 4 * (int)(i % L4);
    g = keep_below(g, c, r);
    const float4 w = W_old[i];
    const float4 nw = make_float4(adam_fresh(w.x, g.x, adam), adam_fresh(w.y, g.y, adam), adam_fresh(w.z, g.z, adam),
                                  adam_fresh(w.w, g.w, adam));
    W_out[i] = keep_below(nw, c, r);
    if (g_out != nullptr) g_out[i] = g;
}

static inline bool relu_aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace tmf

using namespace tmf;

#define TMF_RELU_GEOMETRY(what)                                                                              \
    const RowGeom ga = row_geom(aux), gr = row_geom(n_components);                                           \
    TMF_REQUIRE(ga.ld > 0, what ": unsupported aux width %d", aux);                                          \
    TMF_REQUIRE(gr.ld > 0, what ": unsupported n_components %d", n_components);                              \
    const int ldz = ga.ld, ldw = gr.ld;                                                                      \
    (void)ldz;                                                                                               \
    (void)ldw

extern "C" int64_t tmf_relu_part_rows(int64_t n_rows) { return relu_part_rows(n_rows); }

extern "C" int tmf_relu_embed_f32(const float* Z, const float* b, const float* W, float* E, int64_t n_rows, int aux,
                                  int n_components, void* stream) {
    TMF_RELU_GEOMETRY("relu_embed");
    TMF_REQUIRE(n_rows >= 0, "relu_embed: n_rows=%lld", (long long)n_rows);
    if (n_rows == 0) return TMF_OK;
    TMF_REQUIRE(Z && b && W && E, "relu_embed: null table");
    TMF_REQUIRE(relu_aligned16(Z) && relu_aligned16(b) && relu_aligned16(W) && relu_aligned16(E),
                "relu_embed: a table is not 16-byte aligned");
    const int64_t tm = (n_rows + RBM - 1) / RBM;
    const int tn = (ldw + RBN - 1) / RBN;
    TMF_REQUIRE_LAUNCH(tm * tn, 256, "relu_embed");
    hipLaunchKernelGGL(k_relu_embed, dim3((unsigned)(tm * tn)), dim3(256), 0, (hipStream_t)stream, Z, b, W, E, n_rows, aux,
                       n_components, ldz, ldw, tn);
    return check_launch("tmf_relu_embed_f32");
}

extern "C" int tmf_relu_dhidden_f32(const float* G, const float* W, const float* Z, const float* b, float* dZ, int64_t n_rows,
                                    int aux, int n_components, void* stream) {
    TMF_RELU_GEOMETRY("relu_dhidden");
    TMF_REQUIRE(n_rows >= 0, "relu_dhidden: n_rows=%lld", (long long)n_rows);
    if (n_rows == 0) return TMF_OK;
    TMF_REQUIRE(G && W && Z && b && dZ, "relu_dhidden: null table");
    TMF_REQUIRE(dZ != Z, "relu_dhidden: dZ and Z are the same table");
    TMF_REQUIRE(relu_aligned16(G) && relu_aligned16(W) && relu_aligned16(Z) && relu_aligned16(b) && relu_aligned16(dZ),
                "relu_dhidden: a table is not 16-byte aligned");
    const int64_t tm = (n_rows + RBM - 1) / RBM;
    const int tn = (ldz + RBN - 1) / RBN;
    TMF_REQUIRE_LAUNCH(tm * tn, 256, "relu_dhidden");
    hipLaunchKernelGGL(k_relu_dhidden, dim3((unsigned)(tm * tn)), dim3(256), 0, (hipStream_t)stream, G, W, Z, b, dZ, n_rows, aux,
                       n_components, ldz, ldw, tn);
    return check_launch("tmf_relu_dhidden_f32");
}

extern "C" int tmf_relu_dweights_f32(const float* Z, const float* b, const float* G, float* part, int64_t part_rows,
                                     int64_t n_rows, int aux, int n_components, void* stream) {
    TMF_RELU_GEOMETRY("relu_dweights");
    TMF_REQUIRE(n_rows >= 0, "relu_dweights: n_rows=%lld", (long long)n_rows);
    TMF_REQUIRE(part_rows == relu_part_rows(n_rows), "relu_dweights: part_rows=%lld, tmf_relu_part_rows gives %lld",
                (long long)part_rows, (long long)relu_part_rows(n_rows));
    if (n_rows == 0) return TMF_OK;
    TMF_REQUIRE(Z && b && G && part, "relu_dweights: null table");
    TMF_REQUIRE(relu_aligned16(Z) && relu_aligned16(b) && relu_aligned16(G) && relu_aligned16(part),
                "relu_dweights: a table is not 16-byte aligned");
    const int tm = (aux + RBM - 1) / RBM, tn = (ldw + RBN - 1) / RBN;
    TMF_REQUIRE_LAUNCH(part_rows * tm * tn, 256, "relu_dweights");
    hipLaunchKernelGGL(k_relu_dweights, dim3((unsigned)(part_rows * tm * tn)), dim3(256), 0, (hipStream_t)stream, Z, b, G, part,
                       n_rows, relu_rows_per_part(n_rows), aux, n_components, ldz, ldw, tm, tn);
    return check_launch("tmf_relu_dweights_f32");
}

extern "C" int tmf_relu_adam_weights_f32(const float* part, int64_t part_rows, const float* W_old, float* W_out, float* g_out,
                                         int aux, int n_components, tmf_adam adam, void* stream) {
    TMF_RELU_GEOMETRY("relu_adam_weights");
    TMF_REQUIRE(part_rows >= 0 && part_rows <= kDwMaxParts, "relu_adam_weights: part_rows=%lld outside [0, %lld]",
                (long long)part_rows, (long long)kDwMaxParts);
    TMF_REQUIRE((part_rows == 0 || part) && W_old && W_out, "relu_adam_weights: null table");
    TMF_REQUIRE(relu_aligned16(part) && relu_aligned16(W_old) && relu_aligned16(W_out) && relu_aligned16(g_out),
                "relu_adam_weights: a table is not 16-byte aligned");
    const int64_t n4 = (int64_t)aux * (ldw / 4);
    hipLaunchKernelGGL(k_relu_adam_weights, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(part), part_rows, reinterpret_cast<const float4*>(W_old),
                       reinterpret_cast<float4*>(W_out), reinterpret_cast<float4*>(g_out), n4, ldw / 4, n_components, adam);
    return check_launch("tmf_relu_adam_weights_f32");
}
