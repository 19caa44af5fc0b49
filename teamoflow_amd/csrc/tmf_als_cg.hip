// Alternating least squares by conjugate gradients (EXTENSION): tmf_als_cg_rows_f32.  teamoflow_amd/_als.py states the iteration.
//
// A workgroup of four waves takes a BATCH of 32 rows (positions [32 b, 32 b + 32) of ids); group j = tid / 8, eight lanes, owns
// batch row j for the whole solve and holds its x, res, p and A p in registers: lane g of the group has the 16-byte chunks
// g + 8 m of the row (m < NV = RP / 32, RP the width padded to 32, 64, 128 or 256), so a group's load of a gathered Y row is
// contiguous pieces of 128 bytes.  A is never formed; one application  A v = G0 v + reg v + sum_k w_k (y_k . v) y_k  is
//   1. the rows of CG_LONG entries or more, one after the other, by the WHOLE workgroup: the owner publishes v in LDS, group s
//      walks the s-th of 32 equal pieces of the row's entries, and the owner adds the 32 partial sums in piece order;
//   2. every other row by its own group: per entry a gather of y, a dot (an fmaf chain per lane, then the DPP sum over the group's
//      eight lanes - the same bits in each) and an axpy, CG_UN entries' loads in flight at a time;
//   3. G0 V^T for the batch on v_mfma_f32_32x32x2_f32: the vectors go to LDS k-major (pitch 33), wave w owns the output blocks
//      i = 32 (w + 4 s), G0 streams from L2 (element (i, k) is read from the lower triangle), the batch is the N dimension - output
//      column j depends on column j of V alone - and the products come back through the same LDS image.
// The first application also sums b = sum t_k y_k in the same walk.  Every sum runs in a fixed order that depends on the row alone
// (its entries, their count, Y, G0, reg, x0, cg_steps): not on the launch, the position in ids or the rows that share the batch.
// Barriers are uniform: a row that has finished or failed keeps walking the loop with p = 0.
// LDS: 33 RP floats (the k-major image, aliased by the 32 partial sums of a long row) + RP (the published vector) + 512 B.
#include <math.h>

#include "tmf_common.h"

namespace tmf {

constexpr int CG_THREADS = 256;
constexpr int CG_BATCH = 32;              // rows per batch: the N dimension of the MFMA
constexpr int CG_G = 8;                   // lanes per row
constexpr int CG_LONG = 1024;             // entries from which the whole workgroup walks a row
constexpr int CG_PITCH = CG_BATCH + 1;    // pitch of the k-major LDS image
constexpr int CG_MAX_R = 256;
constexpr int CG_MAX_STEPS = 32;
constexpr int CG_MAX_BLOCKS = 1 << 22;    // the blocks stride the batches beyond

typedef float cg_f32x16 __attribute__((ext_vector_type(16)));

// sum_k [w_k (y_k . v)] y_k into acc and, WITH_B, sum_k t_k y_k into bacc over entries [a0, a1), in entry order; lane g of a group.
template <int NV, bool WITH_B>
__device__ __forceinline__ void cg_walk(const float* __restrict__ Y, int64_t ldy, int r, const int32_t* __restrict__ col,
                                        const float* __restrict__ w, const float* __restrict__ t, int64_t a0, int64_t a1, int g,
                                        const Frag<NV>& v, Frag<NV>& acc, Frag<NV>& bacc) {
    constexpr int UN = NV <= 4 ? 4 : 2;   // entries in flight
    for (int64_t e = a0; e < a1; e += UN) {
        Frag<NV> y[UN];
        float wk[UN], tk[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const bool ok = e + u < a1;   // an entry beyond the end: zeros, which add +0
            const float* __restrict__ yr = Y + (int64_t)(ok ? col[e + u] : 0) * ldy;
            wk[u] = ok ? w[e + u] : 0.f;
            tk[u] = (WITH_B && ok) ? t[e + u] : 0.f;
#pragma unroll
            for (int m = 0; m < NV; ++m) y[u].v[m] = ok ? load_row_chunk(yr, g + CG_G * m, r) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const float d = group_allsum<CG_G>(dot_partial(y[u], v));
            axpy(acc, wk[u] * d, y[u]);
            if (WITH_B) axpy(bacc, tk[u], y[u]);
        }
    }
}

template <int NV>
__device__ __forceinline__ float cg_dot(const Frag<NV>& a, const Frag<NV>& b) {
    return group_allsum<CG_G>(dot_partial(a, b));
}

template <int NT>
__global__ __launch_bounds__(CG_THREADS) void k_als_cg_rows(const float* __restrict__ Y, int r, int64_t ldy,
                                                            const float* __restrict__ G0, int64_t ldg,
                                                            const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const float* __restrict__ w, const float* __restrict__ t, float reg,
                                                            const int32_t* __restrict__ ids, int64_t q, const float* X0, int64_t ldx0,
                                                            float* X, int64_t ldx, int cg_steps, int32_t* __restrict__ n_failed) {
    constexpr int RP = 32 * NT;               // padded width
    constexpr int NV = NT;                    // 16-byte chunks per lane and vector
    constexpr int SLOTS = (NT + 3) / 4;       // 32-row output blocks per wave

    __shared__ __attribute__((aligned(16))) float img[RP * CG_PITCH];   // k-major vectors / products; 32 partial sums of a long row
    __shared__ __attribute__((aligned(16))) float pub[RP];              // the vector of the long row being walked
    __shared__ int64_t long_e0[CG_BATCH], long_e1[CG_BATCH];            // entries of the batch's long rows (empty: not long)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int j = tid >> 3, g = tid & (CG_G - 1);

    const int64_t batches = (q + CG_BATCH - 1) / CG_BATCH;
    for (int64_t batch = blockIdx.x; batch < batches; batch += gridDim.x) {
        const int64_t pos = batch * CG_BATCH + j;
        const bool named = pos < q;
        const int64_t row = named ? (ids ? (int64_t)ids[pos] : pos) : 0;
        const int64_t e0 = named ? rowptr[row] : 0, e1 = named ? rowptr[row + 1] : 0;
        const bool live = e1 > e0;
        const bool is_long = e1 - e0 >= CG_LONG;
        if (g == 0) {
            long_e0[j] = is_long ? e0 : 0;
            long_e1[j] = is_long ? e1 : 0;
        }
        __syncthreads();

        // A v for every row of the batch (and b with it the first time): steps 1 - 3 of the header
        auto apply = [&](auto with_b, const Frag<NV>& v, Frag<NV>& out, Frag<NV>& bout) {
            constexpr bool WITH_B = decltype(with_b)::value;
            zero(out);
            if (WITH_B) zero(bout);
            for (int jj = 0; jj < CG_BATCH; ++jj) {   // 1. long rows: the same test in every thread
                const int64_t l0 = long_e0[jj], l1 = long_e1[jj];
                if (l1 <= l0) continue;
                if (j == jj) {
#pragma unroll
                    for (int m = 0; m < NV; ++m) *reinterpret_cast<float4*>(&pub[4 * (g + CG_G * m)]) = v.v[m];
                }
                __syncthreads();
                Frag<NV> vl, part, bpart;
#pragma unroll
                for (int m = 0; m < NV; ++m) vl.v[m] = *reinterpret_cast<const float4*>(&pub[4 * (g + CG_G * m)]);
                zero(part);
                zero(bpart);
                const int64_t piece = (l1 - l0 + CG_BATCH - 1) / CG_BATCH;
                const int64_t a0 = l0 + piece * j < l1 ? l0 + piece * j : l1;
                const int64_t a1 = a0 + piece < l1 ? a0 + piece : l1;
                cg_walk<NV, WITH_B>(Y, ldy, r, col, w, t, a0, a1, g, vl, part, bpart);
#pragma unroll
                for (int m = 0; m < NV; ++m) *reinterpret_cast<float4*>(&img[j * RP + 4 * (g + CG_G * m)]) = part.v[m];
                __syncthreads();
                if (j == jj) {
                    for (int s = 0; s < CG_BATCH; ++s) {
#pragma unroll
                        for (int m = 0; m < NV; ++m) {
                            const float4 a = *reinterpret_cast<const float4*>(&img[s * RP + 4 * (g + CG_G * m)]);
                            out.v[m].x += a.x;
                            out.v[m].y += a.y;
                            out.v[m].z += a.z;
                            out.v[m].w += a.w;
                        }
                    }
                }
                __syncthreads();
                if (WITH_B) {
#pragma unroll
                    for (int m = 0; m < NV; ++m) *reinterpret_cast<float4*>(&img[j * RP + 4 * (g + CG_G * m)]) = bpart.v[m];
                    __syncthreads();
                    if (j == jj) {
                        for (int s = 0; s < CG_BATCH; ++s) {
#pragma unroll
                            for (int m = 0; m < NV; ++m) {
                                const float4 a = *reinterpret_cast<const float4*>(&img[s * RP + 4 * (g + CG_G * m)]);
                                bout.v[m].x += a.x;
                                bout.v[m].y += a.y;
                                bout.v[m].z += a.z;
                                bout.v[m].w += a.w;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            if (live && !is_long) cg_walk<NV, WITH_B>(Y, ldy, r, col, w, t, e0, e1, g, v, out, bout);   // 2.
            if (G0) {   // 3. (a kernel argument: uniform)
#pragma unroll
                for (int m = 0; m < NV; ++m) {
                    const int k = 4 * (g + CG_G * m);
                    img[(k + 0) * CG_PITCH + j] = v.v[m].x;
                    img[(k + 1) * CG_PITCH + j] = v.v[m].y;
                    img[(k + 2) * CG_PITCH + j] = v.v[m].z;
                    img[(k + 3) * CG_PITCH + j] = v.v[m].w;
                }
                __syncthreads();
                cg_f32x16 acc[SLOTS];
#pragma unroll
                for (int s = 0; s < SLOTS; ++s)
#pragma unroll
                    for (int c = 0; c < 16; ++c) acc[s][c] = 0.f;
                if (wave < NT) {
                    for (int kb = 0; kb < NT; ++kb) {
                        // MFMA step c takes k = 32 kb + c from the lower half-wave and k = 32 kb + 16 + c from the upper one
                        const int k0 = 32 * kb + 16 * h;
                        float bk[16];
#pragma unroll
                        for (int c = 0; c < 16; ++c) bk[c] = img[(k0 + c) * CG_PITCH + l31];
#pragma unroll
                        for (int s = 0; s < SLOTS; ++s) {
                            if (wave + 4 * s < NT) {
                                const int i = 32 * (wave + 4 * s) + l31;
                                float ak[16];
#pragma unroll
                                for (int c = 0; c < 16; ++c) {
                                    const int k = k0 + c;
                                    const int hi = i > k ? i : k, lo = i > k ? k : i;   // the lower triangle of G0
                                    ak[c] = hi < r ? G0[(int64_t)hi * ldg + lo] : 0.f;
                                }
#pragma unroll
                                for (int c = 0; c < 16; ++c) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[c], bk[c], acc[s], 0, 0, 0);
                            }
                        }
                    }
                }
                __syncthreads();   // every wave has read the vectors: the products take their place
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    if (wave + 4 * s < NT) {
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            const int i = 32 * (wave + 4 * s) + (c & 3) + 8 * (c >> 2) + 4 * h;
                            img[i * CG_PITCH + l31] = acc[s][c];
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int m = 0; m < NV; ++m) {
                    const int k = 4 * (g + CG_G * m);
                    out.v[m].x += img[(k + 0) * CG_PITCH + j];
                    out.v[m].y += img[(k + 1) * CG_PITCH + j];
                    out.v[m].z += img[(k + 2) * CG_PITCH + j];
                    out.v[m].w += img[(k + 3) * CG_PITCH + j];
                }
                __syncthreads();   // the image is free again
            }
            axpy(out, reg, v);
        };

        Frag<NV> x, res, p, ap;
        zero(x);
        if (live && X0) {
            const float* x0 = X0 + row * ldx0;
#pragma unroll
            for (int m = 0; m < NV; ++m) x.v[m] = load_row_chunk(x0, g + CG_G * m, r);
        }
        apply(std::true_type{}, x, ap, res);   // res holds b
        const float bb = cg_dot(res, res);
        const float stop = fmaxf(1e-14f * bb, 1e-30f);
#pragma unroll
        for (int m = 0; m < NV; ++m) {
            res.v[m].x -= ap.v[m].x;
            res.v[m].y -= ap.v[m].y;
            res.v[m].z -= ap.v[m].z;
            res.v[m].w -= ap.v[m].w;
        }
        p = res;
        float rs = cg_dot(res, res);
        bool active = live, failed = false;
        for (int step = 0; step < cg_steps; ++step) {
            if (active && rs <= stop) active = false;   // fp32 cannot lower the residual further; also rs == 0
            if (!active) zero(p);
            if (!__syncthreads_or(active ? 1 : 0)) break;
            Frag<NV> none;
            apply(std::false_type{}, p, ap, none);
            if (active) {
                const float pap = cg_dot(p, ap);
                if (!(pap > 0.f) || !(pap <= 3.402823466e38f)) {   // the same value in the group's eight lanes
                    failed = true;
                    active = false;
                    zero(x);
                } else {
                    const float a = rs / pap;
                    axpy(x, a, p);
                    axpy(res, -a, ap);
                    const float rs_new = cg_dot(res, res);
                    const float beta = rs_new / rs;
#pragma unroll
                    for (int m = 0; m < NV; ++m) {
                        p.v[m].x = fmaf(beta, p.v[m].x, res.v[m].x);
                        p.v[m].y = fmaf(beta, p.v[m].y, res.v[m].y);
                        p.v[m].z = fmaf(beta, p.v[m].z, res.v[m].z);
                        p.v[m].w = fmaf(beta, p.v[m].w, res.v[m].w);
                    }
                    rs = rs_new;
                }
            }
        }
        if (named) {
            if (!live) zero(x);
            float* xrow = X + row * ldx;
#pragma unroll
            for (int m = 0; m < NV; ++m) {   // columns at and beyond r of x are zeros
                const int c0 = 4 * (g + CG_G * m);
                if (c0 < ldx) *reinterpret_cast<float4*>(xrow + c0) = x.v[m];
            }
            for (int64_t c0 = RP + 4 * g; c0 < ldx; c0 += 4 * CG_G) *reinterpret_cast<float4*>(xrow + c0) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (failed && g == 0) atomicAdd(n_failed, 1);
        }
        __syncthreads();   // the next batch overwrites long_e0 / long_e1
    }
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_als_cg_rows_f32(const float* Y, int64_t n_other, int r, int64_t ldy, const float* G0, int64_t ldg,
                                   const int64_t* rowptr, const int32_t* col, const float* w, const float* t, float reg,
                                   const int32_t* ids, int64_t q, const float* X0, int64_t ldx0, float* X, int64_t ldx, int cg_steps,
                                   int32_t* n_failed, void* stream) {
    const char* what = "tmf_als_cg_rows_f32";
    TMF_REQUIRE(r >= 1 && r <= CG_MAX_R, "%s: r = %d outside [1, %d]", what, r, CG_MAX_R);
    TMF_REQUIRE(cg_steps >= 1 && cg_steps <= CG_MAX_STEPS, "%s: cg_steps = %d outside [1, %d]", what, cg_steps, CG_MAX_STEPS);
    TMF_REQUIRE(reg > 0.f && reg <= 3.402823466e38f, "%s: reg = %g must be finite and > 0", what, (double)reg);
    TMF_REQUIRE(ldy >= r && ldy % 4 == 0, "%s: ldy = %lld must be >= r = %d and a multiple of 4", what, (long long)ldy, r);
    TMF_REQUIRE(ldx >= r && ldx % 4 == 0, "%s: ldx = %lld must be >= r = %d and a multiple of 4", what, (long long)ldx, r);
    TMF_REQUIRE(!X0 || (ldx0 >= r && ldx0 % 4 == 0), "%s: ldx0 = %lld must be >= r = %d and a multiple of 4", what, (long long)ldx0, r);
    TMF_REQUIRE(!G0 || ldg >= r, "%s: ldg = %lld must be >= r = %d", what, (long long)ldg, r);
    TMF_REQUIRE(q >= 0 && n_other >= 0, "%s: q = %lld, n_other = %lld", what, (long long)q, (long long)n_other);
    if (q == 0) return TMF_OK;
    TMF_REQUIRE(Y && X && rowptr && col && w && t && n_failed, "%s: Y, X, rowptr, col, w, t and n_failed are required", what);
    TMF_REQUIRE((uintptr_t)Y % 16 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)X0 % 16 == 0, "%s: Y, X and X0 must be 16-byte aligned",
                what);
    TMF_REQUIRE(!G0 || (uintptr_t)G0 % 4 == 0, "%s: G0 must be 4-byte aligned", what);
    TMF_REQUIRE(!X0 || X0 != X || ldx0 == ldx, "%s: in place (X0 == X) needs ldx0 == ldx", what);
    const int64_t batches = (q + CG_BATCH - 1) / CG_BATCH;
    const int64_t blocks = batches < CG_MAX_BLOCKS ? batches : CG_MAX_BLOCKS;
    TMF_REQUIRE_LAUNCH(blocks, CG_THREADS, what);
#define TMF_CG_LAUNCH(NT)                                                                                                       \
    hipLaunchKernelGGL(k_als_cg_rows<NT>, dim3((unsigned)blocks), dim3(CG_THREADS), 0, (hipStream_t)stream, Y, r, ldy, G0, ldg, \
                       rowptr, col, w, t, reg, ids, q, X0, ldx0, X, ldx, cg_steps, n_failed)
    if (r <= 32) TMF_CG_LAUNCH(1);
    else if (r <= 64) TMF_CG_LAUNCH(2);
    else if (r <= 128) TMF_CG_LAUNCH(4);
    else TMF_CG_LAUNCH(8);
#undef TMF_CG_LAUNCH
    return check_launch(what);
}
