// The negative table of a resampling fit (tmf_sample_rows): every user's n_samples distinct items, the function
// mf/utils.py random_sampler_device computes on its rejection branch (2 S <= n_items), bit for bit, in one launch.
//
// The row of user u is a function of (seed, u) alone.  With counter_hash / hash_below of mf/utils.py (64-bit wrapping integers):
//   draw:     row[pos] = hash_below(counter_hash(seed, u, pos, 2), n_items), pos < S; the row is sorted ascending
//   redraw:   rnd = 3 .. 66: an element equal to its left neighbour is replaced by hash_below(counter_hash(seed, u, pos, rnd),
//             n_items), pos its place in the SORTED row; the row is sorted again; a row without repeats is a fixed point
//   shuffle:  out[i] = row[ord[i]], ord = the order of (counter_hash(seed, u, pos, 0) >> 1, pos) ascending
// A row that still holds a repeat when round 66 begins sets *failed (the torch function raises there).
//
// Shape: the row loop both samplers share - tmf_sample_rows.h.
#include "tmf_sample_rows.h"

namespace tmf {

template <int NPAD, int THREADS>
__global__ __launch_bounds__(THREADS) void k_sample_rows(int32_t n_items, int64_t n_users, int32_t S, uint64_t seed_add,
                                                         int64_t user_offset, int32_t* __restrict__ R, int32_t* __restrict__ failed) {
    const uint64_t n = (uint64_t)n_items;
    sr_rows<NPAD, THREADS, 66>([n](uint64_t w) { return (uint32_t)((w >> 11) % n); }, n_users, S, seed_add, user_offset, R, failed);
}

template <int NPAD, int THREADS>
static int sample_rows(int32_t n_items, int64_t n_users, int32_t S, uint64_t seed_add, int64_t user_offset, int32_t* R, int32_t* failed,
                       void* stream) {
    const int64_t blocks = sr_blocks<NPAD, THREADS>(n_users);
    TMF_REQUIRE_LAUNCH(blocks, THREADS, "tmf_sample_rows");
    hipLaunchKernelGGL((k_sample_rows<NPAD, THREADS>), dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, n_items, n_users, S,
                       seed_add, user_offset, R, failed);
    return check_launch("tmf_sample_rows");
}

}  // namespace tmf

using namespace tmf;

extern "C" int tmf_sample_rows_supported(int32_t n_items, int32_t n_samples) {
    return n_samples >= 1 && n_samples <= SR_MAX_SAMPLES && 2 * (int64_t)n_samples <= (int64_t)n_items;
}

extern "C" int tmf_sample_rows(int32_t n_items, int64_t n_users, int32_t n_samples, int64_t seed, int64_t user_offset, int32_t* R,
                               int32_t* failed, void* stream) {
    TMF_REQUIRE(tmf_sample_rows_supported(n_items, n_samples),
                "tmf_sample_rows: n_samples = %d, n_items = %d: needs 1 <= n_samples <= %d and 2 n_samples <= n_items", n_samples, n_items,
                SR_MAX_SAMPLES);
    TMF_REQUIRE(n_users >= 0 && user_offset >= 0, "tmf_sample_rows: n_users = %lld, user_offset = %lld", (long long)n_users,
                (long long)user_offset);
    TMF_REQUIRE(failed, "tmf_sample_rows: failed is required");
    if (n_users == 0) return TMF_OK;
    TMF_REQUIRE(R, "tmf_sample_rows: R is required");
    const uint64_t seed_add = sr_seed_add(seed);
#define TMF_SR_UNIFORM(NPAD, THREADS) return sample_rows<NPAD, THREADS>(n_items, n_users, n_samples, seed_add, user_offset, R, failed, stream)
    TMF_SR_DISPATCH(n_samples, TMF_SR_UNIFORM);
}
