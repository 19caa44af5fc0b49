// The scalar item bias of the table family (scores U[u] . V[i] + b[i]): two passes around the pair step of the sliced user pass, neither
// of which sees a factor table.  tmf_item_bias_add puts b into the scores the scores kernel left (sp of the negatives, pk of the
// interactions) - a stream over sp / R with gathers from a table that stays in the L2s; tmf_item_bias_grad gives item i the sum of
// the weights of its list entries (the item pass's sum with the user row replaced by 1) in fp64, in a fixed order, and steps b.
// Contracts in include/tmf.h.
#include "tmf_common.h"

namespace tmf {

constexpr int kIbThreads = 256;
constexpr int kIbWaves = kIbThreads / 64;      // waves of a workgroup of the partial sums: each takes a unit of its own, no barrier
constexpr int kIbInFlight = 4;                 // weight gathers a lane keeps in flight (every one its own cache line)
constexpr int64_t kIbMaxBlocks = ((int64_t)1 << 32) / kIbThreads - 1;   // workgroups of one launch: < 2^32 work-items
constexpr unsigned kIbAddBlocks = 16384;       // grid-stride workgroups of the add (64 per CU)

static inline bool ib_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// sp[j] += b[R[j]] over the flat [m * S] table - n4 float4 / int4 pieces when both are 16-byte aligned (VEC), the elements behind
// the last whole piece (or all of them) one by one - then pk[k] += b[col[k]].  One fp32 add per score.
template <bool VEC>
__global__ __launch_bounds__(kIbThreads) void k_item_bias_add(const float* __restrict__ b, const int32_t* __restrict__ R,
                                                              float* __restrict__ sp, int64_t total, const int32_t* __restrict__ col,
                                                              float* __restrict__ pk, int64_t nnz) {
    const int64_t gid = (int64_t)blockIdx.x * kIbThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kIbThreads;
    int64_t done = 0;
    if constexpr (VEC) {
        const int64_t n4 = total / 4;
        const int4* R4 = reinterpret_cast<const int4*>(R);
        float4* sp4 = reinterpret_cast<float4*>(sp);
        for (int64_t i = gid; i < n4; i += stride) {
            const int4 id = R4[i];
            float4 v = sp4[i];
            v.x += b[id.x];
            v.y += b[id.y];
            v.z += b[id.z];
            v.w += b[id.w];
            sp4[i] = v;
        }
        done = 4 * n4;
    }
    for (int64_t j = done + gid; j < total; j += stride) sp[j] += b[R[j]];
    for (int64_t k = gid; k < nnz; k += stride) pk[k] += b[col[k]];
}

// Stage 1 of the gradient: one wave per unit.  Unit u < n_lists is chunk 0 of list row u, unit n_lists + k chunk xchunk[k] >= 1 of list
// row xrow[k]; chunk c of a row holds its entries [c chunk, (c + 1) chunk).  Lane l adds the weights of the entries l, l + 64, .. of
// the chunk in ascending order in fp64, the 64 sums meet in a fixed butterfly, and ws[u] gets the chunk's sum (0.0 for an empty row).
__global__ __launch_bounds__(kIbThreads) void k_item_bias_partial(const int64_t* __restrict__ rowptr, int64_t n_lists,
                                                                  const int32_t* __restrict__ ent_w, const float* __restrict__ wbuf,
                                                                  int32_t chunk, const int32_t* __restrict__ xrow,
                                                                  const int32_t* __restrict__ xchunk, int64_t n_units, int64_t unit0,
                                                                  double* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = unit0 + (int64_t)blockIdx.x * kIbWaves + (threadIdx.x >> 6);
    if (unit >= n_units) return;
    int64_t row = unit, c = 0;
    if (unit >= n_lists) {
        row = xrow[unit - n_lists];
        c = xchunk[unit - n_lists];
    }
    const int64_t rend = rowptr[row + 1];
    const int64_t beg = rowptr[row] + c * (int64_t)chunk;
    const int64_t end = (beg + chunk < rend) ? beg + chunk : rend;
    double acc = 0.0;
    int64_t e = beg + lane;
    for (; e + (int64_t)(kIbInFlight - 1) * 64 < end; e += (int64_t)kIbInFlight * 64) {   // whole steps: no guard on the loads
        int32_t id[kIbInFlight];
        float w[kIbInFlight];
#pragma unroll
        for (int q = 0; q < kIbInFlight; ++q) id[q] = ent_w[e + (int64_t)q * 64];
#pragma unroll
        for (int q = 0; q < kIbInFlight; ++q) w[q] = wbuf[id[q]];
#pragma unroll
        for (int q = 0; q < kIbInFlight; ++q) acc += (double)w[q];
    }
    for (; e < end; e += 64) acc += (double)wbuf[ent_w[e]];   // the lane's last entries, in the same ascending order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) ws[unit] = acc;
}

// Stage 2: item i adds chunk 0 of its list rows in block order, then its further chunks in (block, chunk) order - ws[n_lists + k] for
// k in [xptr[i], xptr[i + 1]) - rounds the fp64 sum to fp32 once and takes the epilogue.  A thread per item: the reads of a block's
// chunk sums are consecutive across the items.
__global__ __launch_bounds__(kIbThreads) void k_item_bias_finish(const double* __restrict__ ws, int32_t n_items, int32_t user_chunks,
                                                                 const int64_t* __restrict__ xptr, const float* __restrict__ b_old,
                                                                 float* __restrict__ b_out, int epi, tmf_adam adam) {
    const int64_t i = (int64_t)blockIdx.x * kIbThreads + threadIdx.x;
    if (i >= n_items) return;
    double acc = 0.0;
    for (int32_t blk = 0; blk < user_chunks; ++blk) acc += ws[(int64_t)blk * n_items + i];
    if (xptr != nullptr) {
        const double* extra = ws + (int64_t)user_chunks * n_items;
        for (int64_t k = xptr[i]; k < xptr[i + 1]; ++k) acc += extra[k];
    }
    const float g = (float)acc;
    b_out[i] = epi == TMF_EPI_GRAD ? g : adam_fresh(b_old[i], g, adam);
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_item_bias_add(const float* b, int32_t n_items, const int32_t* R, int64_t n_users, int32_t n_samples, float* sp,
                                 const int32_t* col, int64_t nnz, float* pk, void* stream) {
    TMF_REQUIRE(n_items >= 0 && n_users >= 0 && n_samples >= 0 && nnz >= 0, "item_bias_add: n_items=%d n_users=%lld n_samples=%d nnz=%lld",
                n_items, (long long)n_users, n_samples, (long long)nnz);
    const int64_t total = n_users * (int64_t)n_samples;
    if (total == 0 && nnz == 0) return TMF_OK;
    TMF_REQUIRE(b != nullptr && n_items > 0, "item_bias_add: scores without a bias table (n_items=%d)", n_items);
    TMF_REQUIRE(total == 0 || (R && sp), "item_bias_add: null R / sp for %lld sampled scores", (long long)total);
    TMF_REQUIRE(nnz == 0 || (col && pk), "item_bias_add: null col / pk for %lld interactions", (long long)nnz);
    TMF_REQUIRE(ib_aligned(b, 4) && ib_aligned(R, 4) && ib_aligned(sp, 4) && ib_aligned(col, 4) && ib_aligned(pk, 4),
                "item_bias_add: a pointer is not 4-byte aligned");
    const bool vec = total >= 4 && ib_aligned(R, 16) && ib_aligned(sp, 16);
    const int64_t work = (vec ? total / 4 : total) > nnz ? (vec ? total / 4 : total) : nnz;
    const int64_t want = (work + kIbThreads - 1) / kIbThreads;
    const unsigned blocks = (unsigned)(want < (int64_t)kIbAddBlocks ? (want > 0 ? want : 1) : kIbAddBlocks);
    if (vec) {
        hipLaunchKernelGGL(k_item_bias_add<true>, dim3(blocks), dim3(kIbThreads), 0, (hipStream_t)stream, b, R, sp, total, col, pk, nnz);
    } else {
        hipLaunchKernelGGL(k_item_bias_add<false>, dim3(blocks), dim3(kIbThreads), 0, (hipStream_t)stream, b, R, sp, total, col, pk, nnz);
    }
    return check_launch("tmf_item_bias_add");
}

extern "C" size_t tmf_item_bias_grad_workspace_bytes(int32_t n_items, int32_t user_chunks, int64_t n_extra) {
    if (n_items <= 0 || user_chunks <= 0 || n_extra < 0) return 0;
    return (size_t)((int64_t)n_items * user_chunks + n_extra) * sizeof(double);
}

extern "C" int tmf_item_bias_grad(const int64_t* rowptr_e, int32_t n_items, int32_t user_chunks, const int32_t* ent_w,
                                  const float* wbuf, int32_t chunk, const int32_t* xrow, const int32_t* xchunk, const int64_t* xptr,
                                  int64_t n_extra, const float* b_old, float* b_out, int epi, tmf_adam adam, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    TMF_REQUIRE(n_items >= 0 && user_chunks >= 1 && chunk >= 1 && n_extra >= 0, "item_bias_grad: n_items=%d user_chunks=%d chunk=%d n_extra=%lld",
                n_items, user_chunks, chunk, (long long)n_extra);
    TMF_REQUIRE(epi == TMF_EPI_ADAM || epi == TMF_EPI_GRAD, "item_bias_grad: epi=%d", epi);
    if (n_items == 0) return TMF_OK;
    const int64_t n_lists = (int64_t)n_items * user_chunks;
    TMF_REQUIRE(n_lists < ((int64_t)1 << 31), "item_bias_grad: %lld list rows do not fit the int32 row ids", (long long)n_lists);
    TMF_REQUIRE(rowptr_e && ent_w && wbuf && b_out && workspace, "item_bias_grad: null pointer");
    TMF_REQUIRE(epi == TMF_EPI_GRAD || b_old, "item_bias_grad: TMF_EPI_ADAM without b_old");
    TMF_REQUIRE(n_extra == 0 || (xrow && xchunk && xptr), "item_bias_grad: %lld further chunks without their tables", (long long)n_extra);
    TMF_REQUIRE(workspace_bytes >= tmf_item_bias_grad_workspace_bytes(n_items, user_chunks, n_extra),
                "item_bias_grad: workspace of %zu bytes, tmf_item_bias_grad_workspace_bytes gives %zu", workspace_bytes,
                tmf_item_bias_grad_workspace_bytes(n_items, user_chunks, n_extra));
    TMF_REQUIRE(ib_aligned(workspace, 8), "item_bias_grad: the workspace is not 8-byte aligned");
    double* ws = static_cast<double*>(workspace);
    const int64_t n_units = n_lists + n_extra;
    for (int64_t unit0 = 0; unit0 < n_units; unit0 += kIbMaxBlocks * kIbWaves) {   // a launch carries < 2^32 work-items
        const int64_t want = (n_units - unit0 + kIbWaves - 1) / kIbWaves;
        const unsigned blocks = (unsigned)(want < kIbMaxBlocks ? want : kIbMaxBlocks);
        hipLaunchKernelGGL(k_item_bias_partial, dim3(blocks), dim3(kIbThreads), 0, (hipStream_t)stream, rowptr_e, n_lists, ent_w, wbuf,
                           chunk, xrow, xchunk, n_units, unit0, ws);
    }
    hipLaunchKernelGGL(k_item_bias_finish, dim3((unsigned)((n_items + kIbThreads - 1) / kIbThreads)), dim3(kIbThreads), 0,
                       (hipStream_t)stream, (const double*)ws, n_items, user_chunks, n_extra ? xptr : (const int64_t*)nullptr, b_old,
                       b_out, epi, adam);
    return check_launch("tmf_item_bias_grad");
}
