// Unit rows for cosine similarity (tmf_unit_rows_*): out[j] = T[row_j] / ||T[row_j]||, row_j = ids[j] or j - the gather and the
// normalisation in one launch, every source row read once and every output row written once.
//
// A row is held by a GROUP of L lanes, L the power of two that covers its 16-byte chunks (4 fp32 / 8 bf16 elements; at most 64 lanes,
// then up to NV chunks per lane), 64 / L rows per wave; waves stride the q rows.  Per row:
//   amax = max |x|            (butterfly over the group)
//   y = x * 2^sh              sh brings amax into [1, 2): exact, and the squares of a finite row can neither overflow nor all vanish
//   s = sum y^2               fp32: each lane its chunks in column order, then a butterfly - a fixed tree, no atomics
//   out = y / sqrt(s)         IEEE square root and division;  norm = sqrt(s) * 2^-sh
// The tree depends on r alone, so a row's unit vector does not depend on where the row stands or which j asks for it.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int UN_THREADS = 256;   // four waves
constexpr int UN_WAVES = UN_THREADS / 64;
constexpr int UN_MAX_BLOCKS = 2048;   // 8 workgroups per CU; the waves stride the rest

// One 16-byte chunk of a source row as fp32: elements [E c, E c + E), those at or beyond r as zeros WITHOUT being read.
template <int E>
struct UnitChunk {
    float x[E];
};
__device__ __forceinline__ void load_chunk(UnitChunk<4>& k, const float* __restrict__ row, int c, int r) {
    if (4 * c + 4 <= r) {
        const float4 t = *reinterpret_cast<const float4*>(row + 4 * c);
        k.x[0] = t.x; k.x[1] = t.y; k.x[2] = t.z; k.x[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) k.x[e] = 4 * c + e < r ? row[4 * c + e] : 0.f;
    }
}
__device__ __forceinline__ void load_chunk(UnitChunk<8>& k, const __bf16* __restrict__ row, int c, int r) {
    if (8 * c + 8 <= r) {
        const f32x8 w = __builtin_convertvector(*reinterpret_cast<const bf16x8*>(row + 8 * c), f32x8);
#pragma unroll
        for (int e = 0; e < 8; ++e) k.x[e] = w[e];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) k.x[e] = 8 * c + e < r ? (float)row[8 * c + e] : 0.f;
    }
}

// L = 1 << shift lanes per row.  E elements per chunk, NV chunks per lane at L = 64 (E * 64 * NV >= 1024); narrower groups hold one.
template <typename T, int E, int NV>
__global__ __launch_bounds__(UN_THREADS) void k_unit_rows(const T* __restrict__ Tb, int r, int64_t ldt, const int32_t* __restrict__ ids,
                                                          int64_t q, float* __restrict__ out, int64_t ldo, float* __restrict__ norms,
                                                          int shift) {
    const int L = 1 << shift;
    const int lane = threadIdx.x & 63;
    const int g = lane & (L - 1);
    const int64_t rows_per_wave = 64 >> shift;
    const int64_t wave = (int64_t)blockIdx.x * UN_WAVES + (threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * UN_WAVES * rows_per_wave;
    const int nch = (r + E - 1) / E;
    const int64_t span = (int64_t)E * (L < 64 ? L : 64 * NV);   // columns the chunk stores below cover
    for (int64_t j0 = wave * rows_per_wave; j0 < q; j0 += step) {   // wave-uniform: every lane takes part in the shuffles
        const int64_t j = j0 + (lane >> shift);
        const bool live = j < q;
        UnitChunk<E> y[NV];
        float amax = 0.f;
        {
            const T* row = Tb + (live ? (int64_t)(ids ? ids[j] : j) : 0) * ldt;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c = g + L * v;
                if (live && c < nch && (v == 0 || L == 64)) {
                    load_chunk(y[v], row, c, r);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) y[v].x[e] = 0.f;
                }
#pragma unroll
                for (int e = 0; e < E; ++e) amax = fmaxf(amax, fabsf(y[v].x[e]));
            }
        }
        for (int off = L >> 1; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
        int ex = 0;
        frexpf(amax, &ex);          // amax = f * 2^ex, f in [0.5, 1)
        const int sh = 1 - ex;      // amax * 2^sh in [1, 2)
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                y[v].x[e] = ldexpf(y[v].x[e], sh);
                s = fmaf(y[v].x[e], y[v].x[e], s);
            }
        }
        for (int off = L >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);   // x + y == y + x: the group agrees on every bit
        const float nrm = __fsqrt_rn(s);   // in [1, 64) unless the row is zero
        const bool zero = !(amax > 0.f);
        if (live) {
            float* dst = out + j * ldo;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if (v == 0 || L == 64) {
                    const int64_t col = (int64_t)E * (g + L * v);
#pragma unroll
                    for (int h = 0; h < E / 4; ++h) {
                        if (col + 4 * h + 4 <= ldo) {
                            float4 o;
                            o.x = zero ? 0.f : __fdiv_rn(y[v].x[4 * h + 0], nrm);
                            o.y = zero ? 0.f : __fdiv_rn(y[v].x[4 * h + 1], nrm);
                            o.z = zero ? 0.f : __fdiv_rn(y[v].x[4 * h + 2], nrm);
                            o.w = zero ? 0.f : __fdiv_rn(y[v].x[4 * h + 3], nrm);
                            *reinterpret_cast<float4*>(dst + col + 4 * h) = o;
                        }
                    }
                }
            }
            for (int64_t col = span + 4 * g; col + 4 <= ldo; col += 4 * L)   // an output pitch beyond the chunks: zeros
                *reinterpret_cast<float4*>(dst + col) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (norms && g == 0) norms[j] = zero ? 0.f : ldexpf(nrm, -sh);
        }
    }
}

template <typename T, int E, int NV>
static int unit_rows(const char* what, const T* Tb, int64_t n_rows, int r, int64_t ldt, const int32_t* ids, int64_t q, float* out,
                     int64_t ldo, float* norms, void* stream) {
    TMF_REQUIRE(r >= 1 && r <= 1024, "%s: r = %d outside [1, 1024]", what, r);
    TMF_REQUIRE(ldt >= r && ldt % E == 0, "%s: ldt = %lld must be >= r = %d and a multiple of %d", what, (long long)ldt, r, E);
    TMF_REQUIRE(ldo >= r && ldo % 4 == 0, "%s: ldo = %lld must be >= r = %d and a multiple of 4", what, (long long)ldo, r);
    TMF_REQUIRE(q >= 0 && n_rows >= 0, "%s: q = %lld, n_rows = %lld", what, (long long)q, (long long)n_rows);
    if (q == 0) return TMF_OK;
    TMF_REQUIRE(n_rows > 0 && (ids || q <= n_rows), "%s: q = %lld rows asked of a table of %lld", what, (long long)q, (long long)n_rows);
    TMF_REQUIRE(Tb && out, "%s: T and out are required", what);
    TMF_REQUIRE((uintptr_t)Tb % 16 == 0 && (uintptr_t)out % 16 == 0, "%s: T and out must be 16-byte aligned", what);
    const int nch = (r + E - 1) / E;
    int shift = 0;
    while (shift < 6 && (1 << shift) < nch) ++shift;
    const int64_t rows_per_wave = 64 >> shift;
    const int64_t waves = (q + rows_per_wave - 1) / rows_per_wave;
    int64_t blocks = (waves + UN_WAVES - 1) / UN_WAVES;
    if (blocks > UN_MAX_BLOCKS) blocks = UN_MAX_BLOCKS;
    TMF_REQUIRE_LAUNCH(blocks, UN_THREADS, what);
    hipLaunchKernelGGL((k_unit_rows<T, E, NV>), dim3((unsigned)blocks), dim3(UN_THREADS), 0, (hipStream_t)stream, Tb, r, ldt, ids, q,
                       out, ldo, norms, shift);
    return check_launch(what);
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_unit_rows_f32(const float* T, int64_t n_rows, int r, int64_t ldt, const int32_t* ids, int64_t q, float* out,
                                 int64_t ldo, float* norms, void* stream) {
    return unit_rows<float, 4, 4>("tmf_unit_rows_f32", T, n_rows, r, ldt, ids, q, out, ldo, norms, stream);
}

extern "C" int tmf_unit_rows_bf16(const void* T, int64_t n_rows, int r, int64_t ldt, const int32_t* ids, int64_t q, float* out,
                                  int64_t ldo, float* norms, void* stream) {
    return unit_rows<__bf16, 8, 2>("tmf_unit_rows_bf16", static_cast<const __bf16*>(T), n_rows, r, ldt, ids, q, out, ldo, norms, stream);
}
