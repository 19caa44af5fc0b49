// BiasedLinearEmbedding over indicator features: E = W + 1 b^T.  The passes of tmf_train.hip / tmf_wmrb.hip read the effective table E
// and emit G = dL/dE under TMF_EPI_GRAD; this file turns G into the step of the [1, r] bias (deterministic column sums, fp64) and
// the step of the raw weights W, and rebuilds E - three streams over [rows, ld] fp32 tables.  Contracts in include/tmf.h.
#include "tmf_common.h"

namespace tmf {

constexpr int kColsumThreads = 256;     // one workgroup of the partial sums: ld/4 lanes across a row, 256 / (ld/4) rows at a time
constexpr int kColsumMaxParts = 1024;   // workgroups of the first stage (four per CU) = rows of `part`
constexpr int kColsumMinRows = 64;      // table rows per workgroup at least: small tables take few workgroups
constexpr int kColsumInFlight = 4;      // 16-byte loads a lane keeps in flight
constexpr int kCombineThreads = 1024;

inline int64_t colsum_rows_per_part(int64_t n_rows) {
    const int64_t even = (n_rows + kColsumMaxParts - 1) / kColsumMaxParts;
    return even > kColsumMinRows ? even : kColsumMinRows;
}

inline int64_t colsum_part_rows(int64_t n_rows) {
    const int64_t per = colsum_rows_per_part(n_rows);
    const int64_t parts = (n_rows + per - 1) / per;
    return parts > 0 ? parts : 1;
}

// Stage 1: workgroup p sums the table rows [p rows_per, (p + 1) rows_per) column by column into part[p][0 .. ld).  Lane (s, c4) owns
// the four columns 4 c4 .. 4 c4 + 3 of the rows s, s + RS, s + 2 RS .. of that range (RS = 256 / (ld/4)), so a wave's load is RS whole
// rows of 16-byte pieces; the RS lanes of a column are then summed in the order s = 0, 1, .. through LDS.  Every order is fixed by
// (n_rows, ld) alone.  The padding columns are summed like the others (whatever they hold) and dropped by the second stage.
__global__ __launch_bounds__(kColsumThreads) void k_bias_colsum_part(const float4* __restrict__ G, int64_t n_rows, int L4,
                                                                     int64_t rows_per, double* __restrict__ part) {
    __shared__ double sh[kColsumThreads * 4];
    const int t = threadIdx.x;
    const int c4 = t & (L4 - 1), s = t / L4, RS = kColsumThreads / L4;
    const int ld = 4 * L4;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per;
    const int64_t r1 = (r0 + rows_per < n_rows) ? r0 + rows_per : n_rows;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t row = r0 + s;
    for (; row + (int64_t)(kColsumInFlight - 1) * RS < r1; row += (int64_t)RS * kColsumInFlight) {   // whole steps: no guard on the loads
        float4 v[kColsumInFlight];
#pragma unroll
        for (int u = 0; u < kColsumInFlight; ++u) v[u] = G[(row + (int64_t)u * RS) * L4 + c4];
#pragma unroll
        for (int u = 0; u < kColsumInFlight; ++u) {
            a0 += (double)v[u].x;
            a1 += (double)v[u].y;
            a2 += (double)v[u].z;
            a3 += (double)v[u].w;
        }
    }
    for (; row < r1; row += RS) {   // the lane's last rows, in the same ascending order
        const float4 v = G[row * L4 + c4];
        a0 += (double)v.x;
        a1 += (double)v.y;
        a2 += (double)v.z;
        a3 += (double)v.w;
    }
    double* mine = sh + (int64_t)s * ld + 4 * c4;
    mine[0] = a0;
    mine[1] = a1;
    mine[2] = a2;
    mine[3] = a3;
    __syncthreads();
    for (int col = t; col < ld; col += kColsumThreads) {
        double tot = 0.0;
        for (int k = 0; k < RS; ++k) tot += sh[k * ld + col];
        part[(int64_t)blockIdx.x * ld + col] = tot;
    }
}

// Stage 2 (one workgroup): column c < r = sum over the rows of `part` - K = 1024 / ld lanes per column take the rows k, k + K, ..
// in ascending order, then lane c adds the K sums in the order k = 0, 1, ..  Columns >= r give zero.  With `b` the fp64 sum is
// rounded to fp32 once (g_b, also stored in g_out) and b takes the fresh-Adam step.
__global__ __launch_bounds__(kCombineThreads) void k_bias_combine(const double* __restrict__ part, int64_t part_rows, int ld, int r,
                                                                  double* __restrict__ colsum, float* __restrict__ b,
                                                                  float* __restrict__ g_out, tmf_adam adam) {
    __shared__ double sh[kCombineThreads];
    const int t = threadIdx.x;
    const int col = t & (ld - 1), k = t / ld, K = kCombineThreads / ld;
    double sum = 0.0;
#pragma unroll 4
    for (int64_t p = k; p < part_rows; p += K) sum += part[p * ld + col];
    sh[t] = sum;
    __syncthreads();
    if (t >= ld) return;
    double tot = 0.0;
    for (int j = 0; j < K; ++j) tot += sh[j * ld + t];
    const bool live = t < r;
    if (colsum != nullptr) colsum[t] = live ? tot : 0.0;
    if (b != nullptr) {
        const float g = live ? (float)tot : 0.f;
        if (g_out != nullptr) g_out[t] = g;
        b[t] = live ? adam_fresh(b[t], g, adam) : 0.f;
    }
}

// W <- fresh-Adam(W, G) in place (the arithmetic of k_adam_rows), E <- W + b, one float4 per lane, grid-stride.  Columns >= r of W
// and E are written as zeros whatever W, G and b hold there.
// L2 = true: the step takes g' = fl(g + fl(l2 w)) (l2_grad, tmf_common.h), w the RAW pre-update weight - the bias is not penalised and
// E plays no part in g'.  L2 = false ignores l2.
template <bool L2>
__global__ __launch_bounds__(256) void k_adam_bias_rows(float4* __restrict__ W, const float4* __restrict__ Gr,
                                                        const float4* __restrict__ b, float4* __restrict__ E, int64_t n4, int L4, int r,
                                                        tmf_adam adam, float l2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i & (int64_t)(L4 - 1));
        const float4 w = W[i];
        float4 g = Gr[i];
        if constexpr (L2) g = make_float4(l2_grad(g.x, w.x, l2), l2_grad(g.y, w.y, l2), l2_grad(g.z, w.z, l2), l2_grad(g.w, w.w, l2));
        const float4 bb = b[c4];
        // all four columns are stepped and the dead ones masked afterwards: whole 16-byte loads, no divergent branch in the sweep
        const float4 nw = make_float4(adam_fresh(w.x, g.x, adam), adam_fresh(w.y, g.y, adam), adam_fresh(w.z, g.z, adam),
                                      adam_fresh(w.w, g.w, adam));
        const float4 ne = make_float4(nw.x + bb.x, nw.y + bb.y, nw.z + bb.z, nw.w + bb.w);
        const int c = 4 * c4;
        const bool l0 = c + 0 < r, l1 = c + 1 < r, l2 = c + 2 < r, l3 = c + 3 < r;
        W[i] = make_float4(l0 ? nw.x : 0.f, l1 ? nw.y : 0.f, l2 ? nw.z : 0.f, l3 ? nw.w : 0.f);
        E[i] = make_float4(l0 ? ne.x : 0.f, l1 ? ne.y : 0.f, l2 ? ne.z : 0.f, l3 ? ne.w : 0.f);
    }
}

static inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace tmf

using namespace tmf;

extern "C" int64_t tmf_bias_colsum_part_rows(int64_t n_rows) {
    return n_rows < 0 ? 0 : colsum_part_rows(n_rows);
}

extern "C" int tmf_bias_colsum_f32(const float* G, int64_t n_rows, int n_components, double* part, int64_t part_rows,
                                   double* colsum, void* stream) {
    const RowGeom geom = row_geom(n_components);
    TMF_REQUIRE(geom.ld > 0, "bias_colsum: unsupported n_components %d", n_components);
    TMF_REQUIRE(n_rows >= 0 && (n_rows == 0 || G) && part, "bias_colsum: bad arguments");
    TMF_REQUIRE(part_rows == colsum_part_rows(n_rows), "bias_colsum: part_rows=%lld, tmf_bias_colsum_part_rows gives %lld",
                (long long)part_rows, (long long)colsum_part_rows(n_rows));
    TMF_REQUIRE(n_rows == 0 || aligned16(G), "bias_colsum: G is not 16-byte aligned");
    hipLaunchKernelGGL(k_bias_colsum_part, dim3((unsigned)part_rows), dim3(kColsumThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(G), n_rows, geom.ld / 4, colsum_rows_per_part(n_rows), part);
    if (colsum != nullptr) {
        hipLaunchKernelGGL(k_bias_combine, dim3(1), dim3(kCombineThreads), 0, (hipStream_t)stream, (const double*)part, part_rows,
                           geom.ld, n_components, colsum, (float*)nullptr, (float*)nullptr, tmf_adam{});
    }
    return check_launch("tmf_bias_colsum_f32");
}

extern "C" int tmf_bias_adam_f32(const double* part, int64_t part_rows, float* b, float* g_out, int n_components, tmf_adam adam,
                                 void* stream) {
    const RowGeom geom = row_geom(n_components);
    TMF_REQUIRE(geom.ld > 0, "bias_adam: unsupported n_components %d", n_components);
    TMF_REQUIRE(part && b && part_rows >= 1, "bias_adam: bad arguments");
    hipLaunchKernelGGL(k_bias_combine, dim3(1), dim3(kCombineThreads), 0, (hipStream_t)stream, part, part_rows, geom.ld, n_components,
                       (double*)nullptr, b, g_out, adam);
    return check_launch("tmf_bias_adam_f32");
}

extern "C" int tmf_adam_bias_rows_f32(float* W, const float* G, const float* b_new, float* E, int64_t n_rows, int n_components,
                                      tmf_adam adam, void* stream) {
    if (n_rows == 0) return TMF_OK;
    const RowGeom geom = row_geom(n_components);
    TMF_REQUIRE(geom.ld > 0, "adam_bias_rows: unsupported n_components %d", n_components);
    TMF_REQUIRE(W && G && b_new && E && n_rows > 0, "adam_bias_rows: bad arguments");
    TMF_REQUIRE(W != E, "adam_bias_rows: W and E are the same table");
    TMF_REQUIRE(aligned16(W) && aligned16(G) && aligned16(b_new) && aligned16(E), "adam_bias_rows: a table is not 16-byte aligned");
    const int64_t n4 = n_rows * (geom.ld / 4);
    const int64_t want = (n4 + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(k_adam_bias_rows<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float4*>(W),
                       reinterpret_cast<const float4*>(G), reinterpret_cast<const float4*>(b_new), reinterpret_cast<float4*>(E), n4,
                       geom.ld / 4, n_components, adam, 0.f);
    return check_launch("tmf_adam_bias_rows_f32");
}

extern "C" int tmf_adam_bias_rows_l2_f32(float* W, const float* G, const float* b_new, float* E, int64_t n_rows, int n_components,
                                         tmf_adam adam, float l2, void* stream) {
    const RowGeom geom = row_geom(n_components);
    TMF_REQUIRE(geom.ld > 0, "adam_bias_rows_l2: unsupported n_components %d", n_components);
    TMF_REQUIRE(l2_valid(l2), "adam_bias_rows_l2: l2=%g is negative or not finite", (double)l2);
    if (n_rows == 0) return TMF_OK;
    TMF_REQUIRE(W && G && b_new && E && n_rows > 0, "adam_bias_rows_l2: bad arguments");
    TMF_REQUIRE(W != E, "adam_bias_rows_l2: W and E are the same table");
    TMF_REQUIRE(aligned16(W) && aligned16(G) && aligned16(b_new) && aligned16(E), "adam_bias_rows_l2: a table is not 16-byte aligned");
    const int64_t n4 = n_rows * (geom.ld / 4);
    const int64_t want = (n4 + 255) / 256;
    hipLaunchKernelGGL(k_adam_bias_rows<true>, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(W), reinterpret_cast<const float4*>(G), reinterpret_cast<const float4*>(b_new),
                       reinterpret_cast<float4*>(E), n4, geom.ld / 4, n_components, adam, l2);
    return check_launch("tmf_adam_bias_rows_l2_f32");
}
