// The negative table under weighted sampling (tmf_sample_rows_weighted): every user's n_samples distinct items, each draw an item
// with probability q_i / T, the function mf/utils.py random_sampler_device(weights=q) computes, bit for bit, in one launch.
//
// cum [n_items] int64 is the inclusive prefix sum of the weights q_i >= 0 and T = cum[n_items - 1] their total, 1 <= T < 2^33.  The
// row of user u is a function of (seed, u, q) alone.  With counter_hash of mf/utils.py (64-bit wrapping integers) and
//   item(h) = the first i with cum[i] > (h >> 11) mod T      (searchsorted(cum, x, right=True); an item of weight 0 is never drawn)
//   draw:     row[pos] = item(counter_hash(seed, u, pos, 2)), pos < S; the row is sorted ascending
//   redraw:   rnd = 3 .. 258: an element equal to its left neighbour is replaced by item(counter_hash(seed, u, pos, rnd)), pos its
//             place in the SORTED row; the row is sorted again; a row without repeats is a fixed point
//   shuffle:  out[i] = row[ord[i]], ord = the order of (counter_hash(seed, u, pos, 0) >> 1, pos) ascending
// A row that still holds a repeat when round 259 begins sets *failed (the torch function raises there).  The caller admits only
// weights whose S largest hold at most 3/4 of T, so a redraw leaves the row's items with probability >= 1/4 and 256 rounds fail
// with probability <= 0.75^256 per place.
//
// Shape: the row loop both samplers share - tmf_sample_rows.h.  item() is a bisection over cum in global memory: ceil(log2 n_items)
// dependent 8-byte loads (17 at 100K items, whose cum is 800 KB and stays in L2), no LDS beyond the row's, so S = 4096 keeps its
// 56 KB.  The bisection never leaves [0, n_items): whatever cum holds, every id written is a valid one.  T travels as a kernel
// argument - the host reads cum[n_items - 1] once, to refuse a total outside [1, 2^33) before the launch.
#include "tmf_sample_rows.h"

namespace tmf {

constexpr int SRW_FAIL_ROUND = 259;   // redraws run in rounds 3 .. 258

template <int NPAD, int THREADS>
__global__ __launch_bounds__(THREADS) void k_sample_rows_weighted(const int64_t* __restrict__ cum, int32_t n_items, uint64_t total,
                                                                  int64_t n_users, int32_t S, uint64_t seed_add, int64_t user_offset,
                                                                  int32_t* __restrict__ R, int32_t* __restrict__ failed) {
    auto item = [=](uint64_t w) {
        const int64_t x = (int64_t)((w >> 11) % total);
        int32_t lo = 0, hi = n_items - 1;   // cum[hi] > x always: cum[n_items - 1] = total
        while (lo < hi) {
            const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);   // lo <= mid < hi
            if (cum[mid] > x) hi = mid; else lo = mid + 1;
        }
        return (uint32_t)lo;
    };
    sr_rows<NPAD, THREADS, SRW_FAIL_ROUND>(item, n_users, S, seed_add, user_offset, R, failed);
}

template <int NPAD, int THREADS>
static int sample_rows_weighted(const int64_t* cum, int32_t n_items, uint64_t total, int64_t n_users, int32_t S, uint64_t seed_add,
                                int64_t user_offset, int32_t* R, int32_t* failed, void* stream) {
    const int64_t blocks = sr_blocks<NPAD, THREADS>(n_users);
    TMF_REQUIRE_LAUNCH(blocks, THREADS, "tmf_sample_rows_weighted");
    hipLaunchKernelGGL((k_sample_rows_weighted<NPAD, THREADS>), dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, cum, n_items,
                       total, n_users, S, seed_add, user_offset, R, failed);
    return check_launch("tmf_sample_rows_weighted");
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_sample_rows_weighted_supported(int32_t n_items, int32_t n_samples) {
    return n_samples >= 1 && n_samples <= SR_MAX_SAMPLES && n_items >= 1;
}

extern "C" int tmf_sample_rows_weighted(const int64_t* cum, int32_t n_items, int64_t n_users, int32_t n_samples, int64_t seed,
                                        int64_t user_offset, int32_t* R, int32_t* failed, void* stream) {
    TMF_REQUIRE(tmf_sample_rows_weighted_supported(n_items, n_samples),
                "tmf_sample_rows_weighted: n_samples = %d, n_items = %d: needs 1 <= n_samples <= %d and n_items >= 1", n_samples, n_items,
                SR_MAX_SAMPLES);
    TMF_REQUIRE(n_users >= 0 && user_offset >= 0, "tmf_sample_rows_weighted: n_users = %lld, user_offset = %lld", (long long)n_users,
                (long long)user_offset);
    TMF_REQUIRE(cum, "tmf_sample_rows_weighted: cum is required");
    TMF_REQUIRE(failed, "tmf_sample_rows_weighted: failed is required");
    TMF_REQUIRE(R || n_users == 0, "tmf_sample_rows_weighted: R is required");
    if (n_users == 0) return TMF_OK;
    int64_t total = 0;   // the one word of cum the host needs, in stream order
    if (hipMemcpyAsync(&total, cum + (n_items - 1), sizeof(total), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        set_error("tmf_sample_rows_weighted: could not read cum[n_items - 1]");
        return TMF_E_LAUNCH;
    }
    TMF_REQUIRE(total >= 1 && total < ((int64_t)1 << 33), "tmf_sample_rows_weighted: cum[n_items - 1] = %lld: the total weight must lie in [1, 2^33)",
                (long long)total);
    const uint64_t seed_add = sr_seed_add(seed);
#define TMF_SR_WEIGHTED(NPAD, THREADS) \
    return sample_rows_weighted<NPAD, THREADS>(cum, n_items, (uint64_t)total, n_users, n_samples, seed_add, user_offset, R, failed, stream)
    TMF_SR_DISPATCH(n_samples, TMF_SR_WEIGHTED);
}
