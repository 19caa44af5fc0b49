// The streams of the item-run scores kernel (tmf_wmrb_scores7_*, tmf_wmrb.hip) built on the device, chunk by chunk: what
// _engine.Scores7Plan builds in torch with two global sorts of all E = nnz + n_users * S entries and a third of all steps.
// No global sort is needed because the inputs are sorted where it matters: a user's interactions (col_u inside rowptr_u) and a
// user's negatives (a row of R_sorted) ascend by item, so a chunk = (item slice, group of 256 users) is a merge of at most 512
// sorted lists, and every position of that merge can be found by itself:
//   position P of a chunk's order (item, local user, entry id) lies in the run of the smallest item b with
//   #(entries of the chunk with item <= b) > P - a bisection over b, every probe a sum over the group of two bisections in a
//   user's own lists, whose bounds shrink with the bounds of b - and P - #(item < b) entries of the run, dealt to the users in
//   order (a user's interactions before its negatives), come before it.
// A workgroup owns one SUB-CHUNK = positions [j * slots, (j + 1) * slots) of its chunk.  It finds the two borders as above, which
// gives every user's entries of the sub-chunk as two ranges of consecutive addresses (interactions, negatives): the slots are a
// prefix sum over the users, `place` is written from that alone.  The <= 6144 entries then go through a bitonic sort in LDS by the
// unique key (item, slot) = the chunk's order (32-bit keys where a slice holds fewer than 2^19 items), runs are cut into steps of 4, and a packed scan of the four fill classes gives
// every step its position in item order or in fill order.  Nothing depends on the order in which threads run: no atomics.
// Three calls, with the two totals the host has to read in between (n_sub, n_steps): tmf.h.
#include "tmf_common.h"

namespace tmf {

constexpr int kPlUsers = 256;     // = tmf_wmrb_scores7_users_per_group(), checked at every call: the 8-bit local user
constexpr int kPlThreads = 512;   // threads of a sub-chunk's workgroup: the first kPlUsers own a user each during the bisection
constexpr int kPlWaves = kPlThreads / 64;
constexpr int kPlK = 4;           // users per step
constexpr int kPlScanThreads = 1024;
constexpr int kPlSlotBits = 13;     // a key = (item - first item) << kPlSlotBits | slot
constexpr unsigned kPlSlotMask = (1u << kPlSlotBits) - 1;
constexpr int kPlNarrow = (1 << (32 - kPlSlotBits)) - 1;   // slices of at most this many items sort as 32-bit keys (no key reaches the pad ~0)
constexpr size_t kPlStaticLds = 8192;   // above the static LDS of k_s7plan_sub: the grant counts it with the keys

struct S7PlanArgs {
    const int64_t* rowptr;      // [n_users + 1]
    const int32_t* col;         // [nnz] ascending inside a user
    const int32_t* R;           // [n_users, S] ascending inside a user
    int64_t n_users, n_groups, n_chunks;
    int32_t S, n_items, width, slots, cap;
    const int64_t* chunk_ent;   // [n_chunks + 1]
    const int32_t* chunk_sub;   // [n_chunks + 1]
    int32_t* sub_fill;          // counting pass: [n_sub, 4]
    int64_t* sub_place;         //                [n_sub + 1]
    int64_t* sub_cnt;           //                [n_sub] steps of every sub-chunk (the workspace)
    const int64_t* sub_step;    // writing pass: [n_sub + 1]
    int4* steps;                //               [n_steps + 1]
    int32_t* place;             //               [E] or null
    int32_t fill_order;
};

// first position in [lo, hi) of the ascending a[] with a[p] >= v (hi if none)
__device__ __forceinline__ int lower_i32(const int32_t* __restrict__ a, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// A user's entries of a chunk: interactions [a0, a1) of col, negatives [b0, b1) of the flat R (so b = u * S + pos is the place)
__device__ __forceinline__ void chunk_ranges(const S7PlanArgs& a, int64_t u, int ilo, int ihi, int& a0, int& a1, int& b0, int& b1) {
    const int rlo = (int)a.rowptr[u], rhi = (int)a.rowptr[u + 1];
    a0 = lower_i32(a.col, rlo, rhi, ilo);
    a1 = lower_i32(a.col, a0, rhi, ihi);
    const int slo = (int)(u * a.S), shi = slo + a.S;
    b0 = lower_i32(a.R, slo, shi, ilo);
    b1 = lower_i32(a.R, b0, shi, ihi);
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Exclusive prefix of v over the threads of the workgroup (any number of waves up to 16); total = the sum.  Two barriers.
template <typename T>
__device__ __forceinline__ T block_excl_sum(T v, T* s_wave, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    T incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const T x = s_wave[w];
        if (w < wave) base += x;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return base + incl - v;
}

// The same with max (for values >= -1): the largest v of the threads before this one, -1 if none.
__device__ __forceinline__ int block_excl_max(int v, int* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl = max(incl, o);
    }
    if (lane == 63) s_wave[wave] = incl;
    int before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = -1;
    __syncthreads();
    for (int w = 0; w < wave; ++w) before = max(before, s_wave[w]);
    __syncthreads();
    return before;
}

// entries of every chunk: one workgroup per chunk, a thread per user, four bisections - no entry is touched
__global__ __launch_bounds__(kPlUsers) void k_s7plan_count(S7PlanArgs a, int64_t* __restrict__ cnt) {
    __shared__ long long s_red[kPlUsers / 64];
    const int64_t c = blockIdx.x;
    const int64_t slice = c / a.n_groups, grp = c % a.n_groups;
    const int64_t lo64 = slice * a.width, hi64 = lo64 + a.width;
    const int ilo = (int)lo64, ihi = (int)(hi64 < a.n_items ? hi64 : a.n_items);
    const int64_t u = grp * kPlUsers + threadIdx.x;
    long long mine = 0;
    if (u < a.n_users) {
        int a0, a1, b0, b1;
        chunk_ranges(a, u, ilo, ihi, a0, a1, b0, b1);
        mine = (long long)(a1 - a0) + (b1 - b0);
    }
    mine = wave_sum_i64(mine);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < kPlUsers / 64; ++w) t += s_red[w];
        cnt[c] = t;
    }
}

// out64[i] = in[0] + .. + in[i - 1], out32[i] = the same over ceil(in / div) (either may be null), i = 0 .. n - 1: one workgroup,
// arrays of per-chunk or per-sub-chunk length
__global__ __launch_bounds__(kPlScanThreads) void k_s7plan_scan(const int64_t* __restrict__ in, int64_t n, int64_t div,
                                                                int64_t* __restrict__ out64, int32_t* __restrict__ out32) {
    __shared__ long long s_wave[kPlScanThreads / 64];
    long long carry64 = 0, carry32 = 0;
    for (int64_t i0 = 0; i0 < n; i0 += kPlScanThreads) {
        const int64_t i = i0 + threadIdx.x;
        const long long v = i < n ? in[i] : 0;
        long long tot;
        const long long e = block_excl_sum<long long>(v, s_wave, tot);
        if (out64 && i < n) out64[i] = carry64 + e;
        carry64 += tot;
        if (out32) {
            const long long e32 = block_excl_sum<long long>((v + div - 1) / div, s_wave, tot);
            if (i < n) out32[i] = (int32_t)(carry32 + e32);
            carry32 += tot;
        }
    }
}

// The static LDS of a sub-chunk's workgroup: every user's entries of the sub-chunk (first interaction, interactions, first negative,
// negatives), their prefix sum = the user's first slot, and the scratch of the block sums
struct S7PlanLds {
    int ci[kPlUsers], ni[kPlUsers], cn[kPlUsers], nn[kPlUsers], ubase[kPlUsers + 1];
    long long red[2][2][kPlUsers / 64];
    int wave32[kPlWaves];
    unsigned long long wave64[kPlWaves];
};

// the user of slot s: the last one with ubase <= s
__device__ __forceinline__ int slot_user(const S7PlanLds& sm, int s) {
    int lo = 0, hi = kPlUsers - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sm.ubase[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// What follows the borders, over keys (item - item0) << 13 | slot of type KEY: 32 bits where a slice holds at most
// kPlNarrow items (half the LDS of a workgroup: four of them on a CU instead of two), 64 bits for any span.
template <bool WRITE, typename KEY>
__device__ __forceinline__ void s7plan_finish(const S7PlanArgs& a, S7PlanLds& sm, KEY* keys, int item0, int L, int64_t sub, int64_t place0,
                                              int64_t place1) {
    const int tid = threadIdx.x;
    int Lpad = 1;
    while (Lpad < L) Lpad <<= 1;
    for (int s = tid; s < Lpad; s += kPlThreads) {
        KEY key = ~(KEY)0;
        if (s < L) {
            const int lu = slot_user(sm, s), k = s - sm.ubase[lu];
            int item, pl;
            if (k < sm.ni[lu]) {
                const int e = sm.ci[lu] + k;
                item = a.col[e], pl = ~e;
            } else {
                const int e = sm.cn[lu] + (k - sm.ni[lu]);
                item = a.R[e], pl = e;
            }
            if (WRITE && a.place) a.place[place0 + s] = pl;
            key = ((KEY)(unsigned)(item - item0) << kPlSlotBits) | (KEY)s;
        }
        keys[s] = key;
    }
    __syncthreads();
    // ---- the chunk's order (item, local user, entry id) = ascending (item, slot): unique keys, pads behind all
    for (int k = 2; k <= Lpad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (Lpad >> 1); t += kPlThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const KEY ka = keys[i], kb = keys[l];
                if ((ka > kb) == ((i & k) == 0)) keys[i] = kb, keys[l] = ka;
            }
            __syncthreads();
        }
    // ---- steps: a thread walks PER consecutive positions; a run = positions of one item (equal keys above the slot), cut every kPlK
    const int PER = Lpad > kPlThreads ? Lpad / kPlThreads : 1;
    const int p0 = tid * PER, p1 = (p0 + PER < L) ? p0 + PER : L;
    int last = -1;
    for (int p = p0; p < p1; ++p)
        if (p == 0 || (keys[p - 1] >> kPlSlotBits) != (keys[p] >> kPlSlotBits)) last = p;
    const int carry = block_excl_max(last, sm.wave32);   // the first position of the run that reaches into p0
    unsigned long long mine = 0;
    {
        int rs = carry;
        for (int p = p0; p < p1; ++p) {
            const KEY it = keys[p] >> kPlSlotBits;
            if (p == 0 || (keys[p - 1] >> kPlSlotBits) != it) rs = p;
            if (((p - rs) & (kPlK - 1)) == 0) {
                int fill = 1;
                while (fill < kPlK && p + fill < L && (keys[p + fill] >> kPlSlotBits) == it) ++fill;
                mine += 1ull << (16 * (kPlK - fill));   // four 16-bit counts: fill 4 | 3 | 2 | 1, each <= 6144
            }
        }
    }
    unsigned long long total;
    unsigned long long run = block_excl_sum<unsigned long long>(mine, sm.wave64, total);
    if (!WRITE) {
        if (tid == 0) {
            long long n = 0;
            for (int f = 0; f < kPlK; ++f) {
                const int v = (int)((total >> (16 * f)) & 0xffff);
                a.sub_fill[sub * kPlK + f] = v;
                n += v;
            }
            a.sub_cnt[sub] = n;
            a.sub_place[sub] = place0;
            if (sub == (int64_t)gridDim.x - 1) a.sub_place[sub + 1] = place1;   // = E: the chunks behind the last sub-chunk are empty
        }
        return;
    }
    int cls0[kPlK];   // first step of every class in fill order
    {
        int acc = 0;
        for (int f = 0; f < kPlK; ++f) cls0[f] = acc, acc += (int)((total >> (16 * f)) & 0xffff);
    }
    int4* out = a.steps + a.sub_step[sub];
    int rs = carry;
    for (int p = p0; p < p1; ++p) {
        const KEY k0 = keys[p], it = k0 >> kPlSlotBits;
        if (p == 0 || (keys[p - 1] >> kPlSlotBits) != it) rs = p;
        if (((p - rs) & (kPlK - 1)) != 0) continue;
        unsigned sl[kPlK] = {(unsigned)(k0 & kPlSlotMask), (unsigned)a.cap, (unsigned)a.cap, (unsigned)a.cap};
        unsigned users = (unsigned)slot_user(sm, (int)sl[0]) * 0x01010101u;   // pads repeat the step's first user: a resident row
        int fill = 1;
        while (fill < kPlK && p + fill < L && (keys[p + fill] >> kPlSlotBits) == it) {
            sl[fill] = (unsigned)(keys[p + fill] & kPlSlotMask);
            users = (users & ~(0xffu << (8 * fill))) | ((unsigned)slot_user(sm, (int)sl[fill]) << (8 * fill));
            ++fill;
        }
        const int f = kPlK - fill;
        int idx;
        if (a.fill_order) idx = cls0[f] + (int)((run >> (16 * f)) & 0xffff);
        else idx = (int)((run & 0xffff) + ((run >> 16) & 0xffff) + ((run >> 32) & 0xffff) + ((run >> 48) & 0xffff));
        run += 1ull << (16 * f);
        out[idx] = make_int4((int)it + item0, (int)users, (int)(sl[0] | (sl[1] << 16)), (int)(sl[2] | (sl[3] << 16)));
    }
}

// One sub-chunk per workgroup.  WRITE = false: its steps by fill class, their sum and its first place; WRITE = true: its step
// records (item order or fill order) and its places.
template <bool WRITE>
__global__ __launch_bounds__(kPlThreads) void k_s7plan_sub(S7PlanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // [smallest power of two >= slots] 32- or 64-bit keys
    __shared__ S7PlanLds sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t sub = blockIdx.x;
    // the chunk of the sub-chunk: the last one with chunk_sub[c] <= sub (empty chunks before it share the value)
    int64_t c;
    {
        int64_t lo = 0, hi = a.n_chunks;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)a.chunk_sub[mid] <= sub) lo = mid + 1;
            else hi = mid;
        }
        c = lo - 1;
    }
    const int64_t slice = c / a.n_groups, grp = c % a.n_groups;
    const int64_t lo64 = slice * a.width, hi64 = lo64 + a.width;
    const int ilo = (int)lo64, ihi = (int)(hi64 < a.n_items ? hi64 : a.n_items);
    const int64_t ent0 = a.chunk_ent[c], cnt = a.chunk_ent[c + 1] - ent0;
    int64_t P[2];
    P[0] = (sub - a.chunk_sub[c]) * a.slots;
    P[1] = P[0] + a.slots < cnt ? P[0] + a.slots : cnt;
    const bool to_end = P[1] >= cnt;   // the sub-chunk ends with its chunk: no second border to look for
    const int64_t u = grp * kPlUsers + tid;
    const bool has = tid < kPlUsers && u < a.n_users;
    int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (has) chunk_ranges(a, u, ilo, ihi, a0, a1, b0, b1);

    // ---- the two borders: bisection over the item; [la, ha) / [lb, hb) = the user's entries with vlo <= item <= vhi
    int vlo[2], vhi[2], la[2], ha[2], lb[2], hb[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        vlo[x] = ilo, vhi[x] = ihi - 1;
        la[x] = a0, ha[x] = a1, lb[x] = b0, hb[x] = b1;
    }
    if (to_end) vlo[1] = vhi[1];
    int par = 0;
    while (vlo[0] < vhi[0] || vlo[1] < vhi[1]) {
        int mid[2], ua[2], ub[2];
        long long below[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            mid[x] = vlo[x] + ((vhi[x] - vlo[x]) >> 1);
            ua[x] = la[x], ub[x] = lb[x];
            below[x] = 0;
            if (has && vlo[x] < vhi[x]) {
                ua[x] = lower_i32(a.col, la[x], ha[x], mid[x] + 1);
                ub[x] = lower_i32(a.R, lb[x], hb[x], mid[x] + 1);
                below[x] = (long long)(ua[x] - a0) + (ub[x] - b0);   // the user's entries with item <= mid
            }
            below[x] = wave_sum_i64(below[x]);
        }
        if (lane == 0 && wave < kPlUsers / 64) sm.red[par][0][wave] = below[0], sm.red[par][1][wave] = below[1];
        __syncthreads();
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            long long tot = 0;
            for (int w = 0; w < kPlUsers / 64; ++w) tot += sm.red[par][x][w];
            if (vlo[x] < vhi[x]) {
                if (tot > P[x]) vhi[x] = mid[x], ha[x] = ua[x], hb[x] = ub[x];
                else vlo[x] = mid[x] + 1, la[x] = ua[x], lb[x] = ub[x];
            }
        }
        par ^= 1;   // the next round writes the other buffer: whoever gets there has passed this round's barrier behind every read
    }
    // now [la, ha) / [lb, hb) are the user's entries of the border's item: the entries before the border are those of smaller
    // items and the first P - #(smaller) of the run, which goes user by user, interactions first
    int ci[2], cn[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        long long before = wave_sum_i64(has ? (long long)(la[x] - a0) + (lb[x] - b0) : 0);
        if (lane == 0 && wave < kPlUsers / 64) sm.red[par][x][wave] = before;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        long long before = 0;
        for (int w = 0; w < kPlUsers / 64; ++w) before += sm.red[par][x][w];
        const int xa = ha[x] - la[x], t = xa + (hb[x] - lb[x]);
        long long run;
        const long long pre = block_excl_sum<long long>(t, reinterpret_cast<long long*>(sm.wave64), run);
        long long take = P[x] - before - pre;
        take = take < 0 ? 0 : (take > t ? t : take);
        ci[x] = la[x] + (int)(take < xa ? take : xa);
        cn[x] = lb[x] + (int)(take > xa ? take - xa : 0);
    }
    if (to_end) ci[1] = a1, cn[1] = b1;
    // ---- slots: the users one after the other, a user's interactions before its negatives
    int L;
    {
        const int mine = tid < kPlUsers ? (ci[1] - ci[0]) + (cn[1] - cn[0]) : 0;
        const int base = block_excl_sum<int>(mine, sm.wave32, L);
        if (tid < kPlUsers) {
            sm.ci[tid] = ci[0], sm.ni[tid] = ci[1] - ci[0], sm.cn[tid] = cn[0], sm.nn[tid] = cn[1] - cn[0];
            sm.ubase[tid] = base;
        }
        if (tid == 0) sm.ubase[kPlUsers] = L;
        L = L < (int)(P[1] - P[0]) ? L : (int)(P[1] - P[0]);   // equal by construction: the bound of every index below
    }
    __syncthreads();
    // every item of the sub-chunk is one of its slice, at or behind the first border's: 32-bit keys wherever the slice is narrow
    // enough (the host sizes the key buffer by the same rule)
    const int item0 = vlo[0];
    if (a.width <= kPlNarrow)
        s7plan_finish<WRITE, uint32_t>(a, sm, reinterpret_cast<uint32_t*>(keys), item0, L, sub, ent0 + P[0], ent0 + P[1]);
    else
        s7plan_finish<WRITE, unsigned long long>(a, sm, keys, item0, L, sub, ent0 + P[0], ent0 + P[1]);
}

static LdsGrant g_s7plan_grant[2];

static size_t s7plan_align(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t s7plan_lds(int32_t slots, int32_t width) {
    size_t pad = 1;
    while (pad < (size_t)slots) pad <<= 1;
    return pad * (width <= kPlNarrow ? sizeof(uint32_t) : sizeof(unsigned long long));
}

// the checks every call shares; fills the geometry
static int s7plan_args(S7PlanArgs& a, const char* what, const int64_t* rowptr_u, const int32_t* col_u, const int32_t* R_sorted,
                       int64_t nnz, int64_t n_users, int32_t n_samples, int32_t n_items, int32_t width, int32_t slots) {
    const int cap = tmf_wmrb_scores7_slots();
    TMF_REQUIRE(tmf_wmrb_scores7_users_per_group() == kPlUsers && cap <= (1 << kPlSlotBits), "%s: built for groups of %d users", what, kPlUsers);
    TMF_REQUIRE(nnz >= 0 && n_users >= 0 && n_samples >= 0, "%s: negative size", what);
    TMF_REQUIRE(rowptr_u && (nnz == 0 || col_u) && (n_users * (int64_t)n_samples == 0 || R_sorted), "%s: null list", what);
    TMF_REQUIRE(n_items >= 1 && n_items < (1 << 24), "%s: n_items = %d outside [1, 2^24)", what, n_items);
    TMF_REQUIRE(width >= 1, "%s: width = %d < 1", what, width);
    TMF_REQUIRE(slots >= 1 && slots <= cap, "%s: slots = %d outside [1, %d]", what, slots, cap);
    TMF_REQUIRE(nnz < ((int64_t)1 << 31) && n_users * (int64_t)n_samples < ((int64_t)1 << 31),
                "%s: 2^31 or more interactions or negatives (int32 places)", what);
    a = S7PlanArgs{};
    a.rowptr = rowptr_u, a.col = col_u, a.R = R_sorted;
    a.n_users = n_users, a.S = n_samples, a.n_items = n_items, a.width = width, a.slots = slots, a.cap = cap;
    a.n_groups = (n_users + kPlUsers - 1) / kPlUsers;
    const int64_t n_slices = ((int64_t)n_items + width - 1) / width;
    a.n_chunks = n_slices * a.n_groups;
    TMF_REQUIRE(a.n_chunks < ((int64_t)1 << 31), "%s: %lld chunks (2^31 or more)", what, (long long)a.n_chunks);
    return TMF_OK;
}

}  // namespace tmf

using namespace tmf;

// workspace of tmf_s7plan_chunks (n = chunks) and tmf_s7plan_subs (n = sub-chunks): [counts (n + 1) * 8]
extern "C" size_t tmf_s7plan_workspace_bytes(int64_t n) { return s7plan_align((size_t)((n > 0 ? n : 0) + 1) * 8); }

extern "C" int tmf_s7plan_chunks(const int64_t* rowptr_u, const int32_t* col_u, const int32_t* R_sorted, int64_t nnz,
                                 int64_t n_users, int32_t n_samples, int32_t n_items, int32_t width, int32_t slots,
                                 int64_t* chunk_ent, int32_t* chunk_sub, void* workspace, size_t workspace_bytes, void* stream) {
    S7PlanArgs a;
    if (int rc = s7plan_args(a, "s7plan_chunks", rowptr_u, col_u, R_sorted, nnz, n_users, n_samples, n_items, width, slots)) return rc;
    TMF_REQUIRE(chunk_ent && chunk_sub, "s7plan_chunks: null output");
    TMF_REQUIRE(workspace && workspace_bytes >= tmf_s7plan_workspace_bytes(a.n_chunks), "s7plan_chunks: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int64_t* cnt = static_cast<int64_t*>(workspace);
    if (a.n_chunks > 0) {
        TMF_REQUIRE_LAUNCH(a.n_chunks, kPlUsers, "s7plan_chunks");
        hipLaunchKernelGGL(k_s7plan_count, dim3((unsigned)a.n_chunks), dim3(kPlUsers), 0, s, a, cnt);
    }
    if (hipMemsetAsync(cnt + a.n_chunks, 0, 8, s) != hipSuccess) return check_launch("tmf_s7plan_chunks");
    hipLaunchKernelGGL(k_s7plan_scan, dim3(1), dim3(kPlScanThreads), 0, s, (const int64_t*)cnt, a.n_chunks + 1, (int64_t)slots,
                       chunk_ent, chunk_sub);
    return check_launch("tmf_s7plan_chunks");
}

extern "C" int tmf_s7plan_subs(const int64_t* rowptr_u, const int32_t* col_u, const int32_t* R_sorted, int64_t nnz,
                               int64_t n_users, int32_t n_samples, int32_t n_items, int32_t width, int32_t slots,
                               const int64_t* chunk_ent, const int32_t* chunk_sub, int64_t n_sub, int32_t* sub_fill,
                               int64_t* sub_place, int64_t* sub_step, void* workspace, size_t workspace_bytes, void* stream) {
    S7PlanArgs a;
    if (int rc = s7plan_args(a, "s7plan_subs", rowptr_u, col_u, R_sorted, nnz, n_users, n_samples, n_items, width, slots)) return rc;
    TMF_REQUIRE(chunk_ent && chunk_sub && sub_place && sub_step && (n_sub == 0 || sub_fill), "s7plan_subs: null list");
    TMF_REQUIRE(n_sub >= 0 && n_sub < ((int64_t)1 << 31), "s7plan_subs: n_sub = %lld outside [0, 2^31)", (long long)n_sub);
    TMF_REQUIRE(workspace && workspace_bytes >= tmf_s7plan_workspace_bytes(n_sub), "s7plan_subs: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int64_t* cnt = static_cast<int64_t*>(workspace);
    a.chunk_ent = chunk_ent, a.chunk_sub = chunk_sub, a.sub_fill = sub_fill, a.sub_place = sub_place, a.sub_cnt = cnt;
    if (n_sub > 0) {
        TMF_REQUIRE_LAUNCH(n_sub, kPlThreads, "s7plan_subs");
        const size_t lds = s7plan_lds(slots, width);
        if (int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&k_s7plan_sub<false>), lds + kPlStaticLds, g_s7plan_grant[0])) return rc;
        hipLaunchKernelGGL(k_s7plan_sub<false>, dim3((unsigned)n_sub), dim3(kPlThreads), lds, s, a);
    } else if (hipMemsetAsync(sub_place, 0, 8, s) != hipSuccess) {
        return check_launch("tmf_s7plan_subs");
    }
    if (hipMemsetAsync(cnt + n_sub, 0, 8, s) != hipSuccess) return check_launch("tmf_s7plan_subs");
    hipLaunchKernelGGL(k_s7plan_scan, dim3(1), dim3(kPlScanThreads), 0, s, (const int64_t*)cnt, n_sub + 1, (int64_t)1, sub_step,
                       (int32_t*)nullptr);
    return check_launch("tmf_s7plan_subs");
}

extern "C" int tmf_s7plan_streams(const int64_t* rowptr_u, const int32_t* col_u, const int32_t* R_sorted, int64_t nnz,
                                  int64_t n_users, int32_t n_samples, int32_t n_items, int32_t width, int32_t slots,
                                  const int64_t* chunk_ent, const int32_t* chunk_sub, int64_t n_sub, const int64_t* sub_step,
                                  int64_t n_steps, int32_t fill_order, void* steps, int32_t* place, void* stream) {
    S7PlanArgs a;
    if (int rc = s7plan_args(a, "s7plan_streams", rowptr_u, col_u, R_sorted, nnz, n_users, n_samples, n_items, width, slots)) return rc;
    TMF_REQUIRE(chunk_ent && chunk_sub && sub_step && steps, "s7plan_streams: null list");
    TMF_REQUIRE(n_sub >= 0 && n_sub < ((int64_t)1 << 31) && n_steps >= 0, "s7plan_streams: n_sub = %lld, n_steps = %lld",
                (long long)n_sub, (long long)n_steps);
    TMF_REQUIRE((reinterpret_cast<uintptr_t>(steps) & 15) == 0, "s7plan_streams: steps not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    a.chunk_ent = chunk_ent, a.chunk_sub = chunk_sub, a.sub_step = sub_step, a.steps = static_cast<int4*>(steps), a.place = place;
    a.fill_order = fill_order != 0;
    if (n_sub > 0) {
        TMF_REQUIRE_LAUNCH(n_sub, kPlThreads, "s7plan_streams");
        const size_t lds = s7plan_lds(slots, width);
        if (int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&k_s7plan_sub<true>), lds + kPlStaticLds, g_s7plan_grant[1])) return rc;
        hipLaunchKernelGGL(k_s7plan_sub<true>, dim3((unsigned)n_sub), dim3(kPlThreads), lds, s, a);
    }
    if (hipMemsetAsync(a.steps + n_steps, 0, 16, s) != hipSuccess) return check_launch("tmf_s7plan_streams");   // the record behind the last
    return check_launch("tmf_s7plan_streams");
}
