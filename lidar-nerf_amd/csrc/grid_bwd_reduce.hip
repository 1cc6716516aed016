// grid_bwd_reduce.hip — pass 2 of the bucketed table backward (grid_pool.h), the workspace plan, the walk over chunks
// and the entry points of the bucketed backward.
#include "grid_pool.h"

typedef uint32_t uint4_t __attribute__((ext_vector_type(4)));
typedef uint32_t uint2_t __attribute__((ext_vector_type(2)));

namespace {

// A bucket with many entries (coarse dense levels: every ray passes the same few cells; very large batches) is split
// over up to kMaxSlices workgroups (blockIdx.y).  An unsplit bucket owns its rows and adds its image into the table with
// plain stores; the slices of a split bucket write their 64-bit integer images to the workspace and the slice that
// arrives last adds them up — integers, so the sum does not depend on the order.
// Entries per slice: 512 K keeps every hashed bucket whole up to 4 M points (a chunk).  Measured in round 4 with everything
// else as it is: 384 K the same, 256 K +4 %, 192 K and below 3.5 x (every hashed bucket split, its images through HBM).
// With the dense levels' rows dealt to 64 buckets, slices occur for concentrated batches only; lnh_grid_backward_set_slice_
// entries lowers the length so that tests reach this path with small inputs.
constexpr uint32_t kSliceEntries = 512 * 1024;
constexpr uint32_t kMaxSlices = 16;
uint32_t g_slice_entries = kSliceEntries;  // process-wide (set before sizing the workspace)

__device__ __forceinline__ uint32_t slices_of(uint32_t n_tot, uint32_t per) {
    const uint32_t s = (n_tot + per - 1) / per;
    return s > kMaxSlices ? kMaxSlices : s;
}
// Work items of pass 2 in dispatch order (blockIdx.x): first the EXTRA slices (slice 1.. of every split bucket — known
// only on the device, so the launch carries the host-side upper bound `n_extra` of them and the surplus workgroups
// exit after one look at the cursors), then slice 0 of every bucket of the window, longest first: buckets of the dense
// levels (few rows near the sensor take most entries -> same-address LDS adds), then the hashed levels from the finest
// (no run-merge, most entries) to the coarsest.  The dispatcher hands a free CU the next workgroup in that order, i.e.
// longest-processing-time-first list scheduling; with the plain (bucket, slice) grid the slices of the split buckets
// were dispatched behind everything else and 15 of 16 workgroups were empty, each waiting for a CU with 128 KiB of
// free LDS only to exit.
struct ReduceOrder {
    uint32_t level[LNH_MAX_LEVELS];      // levels of the window in processing order
    uint32_t first[LNH_MAX_LEVELS + 1];  // prefix sum of their bucket counts
    uint32_t n_levels, n_extra, bucket0, n_buckets;  // window: buckets [bucket0, bucket0 + n_buckets)
    uint32_t slice_entries;
};

template <typename T>
__global__ void __launch_bounds__(1024)
k_grid_bwd_reduce(T *__restrict__ grad_table, GridMeta meta, BucketPlan plan, const char *__restrict__ pool_bytes,
                  const uint32_t *__restrict__ cursor, const uint32_t *__restrict__ spill_cursor,
                  uint32_t *__restrict__ done, uint32_t L, ReduceOrder ord, uint32_t table_zero) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(smem_raw);  // [kBucketRows][2] fixed point
    __shared__ uint32_t sh_sum, sh_item[4], sh_wave[2][16];
    constexpr int K = sizeof(T) == 2 ? 24 : 40;  // scale of the fixed-point image (to_fixed)
    typedef v2_t<T> V2;
    // ---- which (bucket, slice) is this workgroup?
    const bool is_extra = blockIdx.x < ord.n_extra;
    uint32_t bid = ord.bucket0, slice = 0, slot0 = 0;
    if (!is_extra) {
        const uint32_t j = blockIdx.x - ord.n_extra;
        uint32_t k = 0;
        for (uint32_t q = 1; q < ord.n_levels; q++)
            if (j >= ord.first[q]) k = q;
        bid = plan.first_bucket[ord.level[k]] + (j - ord.first[k]);
    }
    if (is_extra || slices_of(cursor[bid], ord.slice_entries) > 1) {  // workgroup-uniform
        // block-wide exclusive scan over the window's buckets: extra slices before a bucket (-> which bucket an extra
        // workgroup serves) and image slots before it (-> where a split bucket keeps its slice images)
        const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
        const uint32_t sl = t < ord.n_buckets ? slices_of(cursor[ord.bucket0 + t], ord.slice_entries) : 0u;
        const uint32_t ex = sl > 1 ? sl - 1 : 0u, im = sl > 1 ? sl : 0u;
        const uint32_t in_ex = wave_scan_add_u32(ex), in_im = wave_scan_add_u32(im);
        if (lane == 63) {
            sh_wave[0][wv] = in_ex;
            sh_wave[1][wv] = in_im;
        }
        if (t == 0) sh_item[0] = 0;
        __syncthreads();
        uint32_t ex0 = in_ex - ex, im0 = in_im - im;
        for (uint32_t w = 0; w < wv; w++) {
            ex0 += sh_wave[0][w];
            im0 += sh_wave[1][w];
        }
        if (is_extra ? (ex && blockIdx.x >= ex0 && blockIdx.x < ex0 + ex) : (ord.bucket0 + t == bid)) {
            sh_item[0] = 1;
            sh_item[1] = ord.bucket0 + t;
            sh_item[2] = is_extra ? blockIdx.x - ex0 + 1 : 0u;
            sh_item[3] = im0;
        }
        __syncthreads();
        if (!sh_item[0]) return;  // surplus extra workgroup
        bid = sh_item[1];
        slice = sh_item[2];
        slot0 = sh_item[3];
    }
    uint32_t level = 0;
    for (uint32_t l = 0; l < L; l++)
        if (bid >= plan.first_bucket[l]) level = l;
    const LevelParams lv = meta.lv[level];
    const bool hashed = (lv.flags & (LV_HASH | LV_POW2)) == (LV_HASH | LV_POW2);  // pair rule of the level (pair_row)
    const uint32_t bk = bid - plan.first_bucket[level], cap = plan.cap[level];
    const uint32_t n_tot = cursor[bid];          // every entry reserved for this bucket, pool + spill
    const uint32_t n_all = min(n_tot, cap);      // ... of which in the pool
    const uint32_t slices = slices_of(n_tot, ord.slice_entries);
    if (slice >= slices) return;  // workgroup-uniform (n_tot == 0: nothing to add)
    const uint32_t i_begin = (uint32_t)((uint64_t)n_all * slice / slices);
    const uint32_t i_end = (uint32_t)((uint64_t)n_all * (slice + 1) / slices);
    const uint32_t n = i_end - i_begin;
    const bool il = (plan.interleaved >> level) & 1u;  // rows dealt to the buckets in 128-row groups (bucket_of_row)
    // table row of position r of this bucket's image (>= hashmap_size: no such row)
    auto table_row = [&](uint32_t r) { return row_of_local(r, bk, il); };
    // channel-planar image: acc[row] | acc[kBucketRows + row].  With the two channels of a row interleaved, each
    // 64-bit LDS add of a wave would touch only every other pair of banks and pay twice the conflicts; planar, the 64
    // random rows of an instruction spread over all banks.
    //
    // Element of the image: 64-bit FIXED POINT (ds_add_u64).  fp16 contributions are multiples of 2^-24 and enter exactly
    // (half_to_fixed24); fp32 ones are truncated to 2^-40 each.  Integer sums do not depend on the order of arrival.
    // (Measured and rejected in round 4: a DOUBLE image for fp16 tables — exact as well up to partial sums of 2^29, two
    // conversions per value instead of five VALU operations — runs the pass at 447 us against 330: ds_add_f64 is the slower
    // LDS atomic.  profiles/r04_reduce_levels.txt)
    typedef unsigned long long acc_t;
    acc_t *img = reinterpret_cast<acc_t *>(smem_raw);
    // (the image is cleared inside `stream`, AFTER the first pool loads have been issued: a workgroup's HBM round trip
    //  runs under its 128 KiB of LDS stores instead of behind them)
    auto clear_image = [&]() {
        for (uint32_t i = threadIdx.x; i < kBucketRows * 2; i += blockDim.x) acc[i] = 0ull;
        __syncthreads();
    };
    auto acc_add = [&](uint32_t idx, T v) {
        if constexpr (sizeof(T) == 2) atomicAdd(&img[idx], (unsigned long long)half_to_fixed24(v));
        else atomicAdd(&img[idx], (unsigned long long)(long long)ldexp((double)v, 40));
    };
    // No branch around the LDS adds: a single (code 7) adds ZERO for its absent second corner, to whatever row of the bucket
    // the pair rule yields.  (Per-entry `if`s cost an exec-mask round trip and a wait each; singles are one entry in 128.)
    auto add_entry = [&](auto hashed_c, uint32_t row0, uint32_t code, V2 a, V2 b) {
        constexpr bool HASHED = decltype(hashed_c)::value;
        const bool sgl = code == kCodeSingle;
        if constexpr (sizeof(T) == 2) {
            uint32_t wb = __builtin_bit_cast(uint32_t, b);
            wb = sgl ? 0u : wb;
            b = __builtin_bit_cast(V2, wb);
        } else {
            b[0] = sgl ? (T)0.0f : b[0];
            b[1] = sgl ? (T)0.0f : b[1];
        }
        const uint32_t row1 = (HASHED ? row0 ^ ((2u << code) - 1u) : row0 + 1u) & (kBucketRows - 1);
        acc_add(row0, a[0]);
        acc_add(kBucketRows + row0, a[1]);
        acc_add(row1, b[0]);
        acc_add(kBucketRows + row1, b[1]);
    };
    // One workgroup streams its whole slice [a_begin, a_end) of the level's slots.  The aligned QUADS inside it (4 entries =
    // 4 * sizeof(2 V2) bytes of values in 16-byte loads + 8 bytes of rows) take the main loop, with no per-entry range test;
    // the up to 3 + 3 entries in front of the first and behind the last full quad are added by the first threads, one each.
    auto stream = [&](auto hashed_c) {
        constexpr uint32_t UNROLL = sizeof(T) == 2 ? 2 : 1;  // (fp16: 1 / 2 / 4 quads in flight per lane measure the same)
        constexpr uint32_t VQ = sizeof(V2) * 2 * 4 / 16;     // 16-byte loads per quad: 2 (fp16) / 4 (fp32)
        const char *vbytes = pool_bytes + plan.pool_off[level], *rbytes = pool_bytes + plan.rows_off[level];
        const uint4_t *vals4 = reinterpret_cast<const uint4_t *>(vbytes);
        const uint2_t *rows4 = reinterpret_cast<const uint2_t *>(rbytes);
        const uint32_t a_begin = bk * cap + i_begin, a_end = a_begin + n;  // level-relative slots (< 2^32, checked)
        const uint32_t qf_begin = (a_begin + 3) >> 2, qf_end = a_end >> 2;
        const uint32_t nfull = qf_end > qf_begin ? qf_end - qf_begin : 0u;
        // every lane keeps UNROLL independent quads outstanding (non-temporal loads: the pool is written once and read
        // once), double-buffered: the loads of batch i+1 are in flight while the LDS adds of batch i execute
        const uint32_t stride = blockDim.x * UNROLL;
        uint4_t rv[2][UNROLL][VQ];
        uint2_t rr[2][UNROLL];
        auto fetch = [&](uint32_t j0, uint4_t (&v)[UNROLL][VQ], uint2_t (&r)[UNROLL]) {
#pragma unroll
            for (uint32_t u = 0; u < UNROLL; u++) {
                const uint32_t j = j0 + u * blockDim.x, q = qf_begin + (j < nfull ? j : nfull - 1);  // clamped, unconditional
#pragma unroll
                for (uint32_t w = 0; w < VQ; w++) v[u][w] = __builtin_nontemporal_load(vals4 + (size_t)q * VQ + w);
                r[u] = __builtin_nontemporal_load(rows4 + q);
            }
        };
        if (nfull) fetch(threadIdx.x, rv[0], rr[0]);
        clear_image();
        {
            const uint32_t lo_end = nfull ? qf_begin * 4 : a_end, hi_begin = nfull ? qf_end * 4 : a_end;
            const uint32_t n_lo = lo_end - a_begin, n_hi = a_end - hi_begin;
            if (threadIdx.x < n_lo + n_hi) {
                const uint32_t slot = threadIdx.x < n_lo ? a_begin + threadIdx.x : hi_begin + (threadIdx.x - n_lo);
                const V2 *pv = reinterpret_cast<const V2 *>(vbytes + (size_t)slot * (2 * sizeof(V2)));
                const uint32_t key = *reinterpret_cast<const unsigned short *>(rbytes + (size_t)slot * 2);
                add_entry(hashed_c, key & (kBucketRows - 1), key >> kBucketRowsLog2, pv[0], pv[1]);
            }
        }
        auto consume = [&](uint32_t j0, const uint4_t (&v)[UNROLL][VQ], const uint2_t (&r)[UNROLL]) {
#pragma unroll
            for (uint32_t u = 0; u < UNROLL; u++) {
                if (j0 + u * blockDim.x >= nfull) continue;  // (only in the last round of a lane: one test per quad)
                uint32_t words[VQ * 4];
#pragma unroll
                for (uint32_t w = 0; w < VQ; w++) {
                    words[4 * w] = v[u][w].x; words[4 * w + 1] = v[u][w].y;
                    words[4 * w + 2] = v[u][w].z; words[4 * w + 3] = v[u][w].w;
                }
                const uint32_t rw[2] = {r[u].x, r[u].y};
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    constexpr uint32_t EW = VQ;  // dwords per entry: 2 (fp16: a | b) / 4 (fp32: a0 a1 | b0 b1)
                    V2 a, b;
                    __builtin_memcpy(&a, &words[h * EW], sizeof(V2));
                    __builtin_memcpy(&b, &words[h * EW + EW / 2], sizeof(V2));
                    const uint32_t key = (rw[h >> 1] >> (16 * (h & 1))) & 0xffffu;
                    add_entry(hashed_c, key & (kBucketRows - 1), key >> kBucketRowsLog2, a, b);
                }
            }
        };
        uint32_t j0 = threadIdx.x;
        while (j0 < nfull) {  // unrolled by two so that the buffer index is a compile-time constant
            const uint32_t j1 = j0 + stride;
            if (j1 < nfull) fetch(j1, rv[1], rr[1]);
            consume(j0, rv[0], rr[0]);
            if (j1 >= nfull) break;
            const uint32_t j2 = j1 + stride;
            if (j2 < nfull) fetch(j2, rv[0], rr[0]);
            consume(j1, rv[1], rr[1]);
            j0 = j2;
        }
        // ---- this bucket overflowed its pool: its remaining entries sit somewhere in the level's spill list (among those
        //      of the level's other overflowing buckets).  Each slice filters its share of the list.
        if (n_tot > cap) {  // workgroup-uniform
            const SpillEntry<T> *spill = reinterpret_cast<const SpillEntry<T> *>(pool_bytes + plan.spill_off[level]);
            const uint32_t s_all = min(spill_cursor[level], plan.spill_cap);
            const uint32_t s_begin = (uint32_t)((uint64_t)s_all * slice / slices);
            const uint32_t s_end = (uint32_t)((uint64_t)s_all * (slice + 1) / slices);
            constexpr uint32_t SU = 4;
            for (uint32_t i0 = s_begin + threadIdx.x; i0 < s_end; i0 += blockDim.x * SU) {
                SpillEntry<T> e[SU];
#pragma unroll
                for (uint32_t u = 0; u < SU; u++) {
                    const uint32_t i = i0 + u * blockDim.x;
                    e[u] = spill[i < s_end ? i : s_end - 1];
                }
#pragma unroll
                for (uint32_t u = 0; u < SU; u++) {
                    const uint32_t i = i0 + u * blockDim.x;
                    const uint32_t r = e[u].key & 0x7ffffu;
                    if (i < s_end && bucket_of_row(r, il) == bk)
                        add_entry(hashed_c, local_of_row(r, il), e[u].key >> 29, e[u].a, e[u].b);
                }
            }
        }
    };
    if (hashed) stream(std::true_type{});
    else stream(std::false_type{});
    __syncthreads();
    // image element -> float: the exact integer sum * 2^-K, rounded once
    auto to_float = [&](acc_t q) -> float { return (float)ldexp((double)(long long)q, -K); };
    if (slices == 1) {
        // this workgroup owns the bucket's rows: table += image.  All row loads of a thread are issued before the first
        // use (a load -> add -> store chain per row would cost a memory round trip per row: 8 in a row per thread)
        T *gt = grad_table + (size_t)lv.offset * 2;
        constexpr uint32_t RPT = kBucketRows / 1024;
        Vec<T, 2> cur[RPT];
        // table_zero (workgroup-uniform): the caller has just cleared the gradient and this is its first chunk — the rows
        // hold zeros, nothing to read (27 MB per step and the round trip at the end of every workgroup).  Not so on a level
        // whose spill list ran full: the scatter pass has then added entries straight into the table with device atomics
        // (its last resort), and those rows must be read like any others.
        const bool rows_are_zero = table_zero && spill_cursor[level] <= plan.spill_cap;
#pragma unroll
        for (uint32_t i = 0; i < RPT; i++) {
            const uint32_t row = table_row(threadIdx.x + i * 1024u);
            if (rows_are_zero) {
                cur[i].v[0] = (T)0.0f;
                cur[i].v[1] = (T)0.0f;
            } else {
                cur[i] = load_vec<T, 2>(gt + 2 * (size_t)(row < lv.hashmap_size ? row : 0u));
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < RPT; i++) {
            const uint32_t r = threadIdx.x + i * 1024u, row = table_row(r);
            const acc_t qa = img[r], qb = img[kBucketRows + r];
            if (row < lv.hashmap_size && (qa != (acc_t)0 || qb != (acc_t)0)) {
                cur[i].v[0] = (T)((float)cur[i].v[0] + to_float(qa));
                cur[i].v[1] = (T)((float)cur[i].v[1] + to_float(qb));
                store_vec<T, 2>(gt + 2 * (size_t)row, cur[i]);
            }
        }
    } else {
        // slice image -> workspace (coalesced 16-byte stores of the whole image); the slice that finishes LAST adds the
        // images up (exact sums: the result does not depend on which slice that is) and adds the rows into the table
        if (slot0 + slices > plan.partial_slots) return;  // (never: plan_buckets sizes the region for the worst case)
        char *images = const_cast<char *>(pool_bytes) + plan.partial_off;
        uint4 *dst = reinterpret_cast<uint4 *>(images) + (size_t)(slot0 + slice) * kBucketRows;
        const uint4 *src = reinterpret_cast<const uint4 *>(acc);
        for (uint32_t i = threadIdx.x; i < kBucketRows; i += blockDim.x) dst[i] = src[i];
        __threadfence();  // release (agent scope): this slice's image is visible before its arrival is
        __syncthreads();
        if (threadIdx.x == 0) sh_sum = atomicAdd(&done[bid], 1u);
        __syncthreads();
        if (sh_sum != slices - 1) return;  // workgroup-uniform
        __threadfence();  // acquire: the other slices' images (written by other CUs / XCDs) are read from memory
        const acc_t *simg = reinterpret_cast<const acc_t *>(images) + (size_t)slot0 * kBucketRows * 2;
        T *gt = grad_table + (size_t)lv.offset * 2;
        for (uint32_t r = threadIdx.x; r < kBucketRows; r += blockDim.x) {
            const uint32_t row = table_row(r);
            if (row >= lv.hashmap_size) continue;
            acc_t qa = (acc_t)0, qb = (acc_t)0;
            for (uint32_t sl = 0; sl < slices; sl++) {
                qa += simg[(size_t)sl * kBucketRows * 2 + r];
                qb += simg[(size_t)sl * kBucketRows * 2 + kBucketRows + r];
            }
            if (qa != (acc_t)0 || qb != (acc_t)0) {
                Vec<T, 2> cur = load_vec<T, 2>(gt + 2 * (size_t)row);
                cur.v[0] = (T)((float)cur.v[0] + to_float(qa));
                cur.v[1] = (T)((float)cur.v[1] + to_float(qb));
                store_vec<T, 2>(gt + 2 * (size_t)row, cur);
            }
        }
    }
}

// Host: bucket layout + pool sizing.  Returns the number of bytes of workspace needed:
//   [cursor: one u32 per bucket | spill cursor: one u32 per level | slice arrival counter: one u32 per bucket]
//                                                                      (zeroed by every launch)
//   [pool of every level: value stream | row stream] [spill list of every level] [slice images]
// Pool slots per bucket = even split of the level's expected entries (pair format: B * 2^D / 2, + 1/64 for the pairs
// that travel as two singles; generic level classes: B * 2^D) + 12.5 % + 12 sigma of a Poisson count (hashed levels are
// statistically even; correlated corners of neighbouring samples widen the spread, so the margin is generous) —
// whatever does not fit goes to the level's spill list (1/16 of the level's worst case B * 2^D), and beyond that into the
// table with device atomics.
constexpr uint32_t kCursorAlign = 256;
// the head of the workspace (cursors and arrival counters): what a launch, or a caller that promises LNH_BWD_WS_CLEARED, zeroes
inline uint64_t cursor_head_bytes(uint32_t n_buckets, uint32_t L) {
    return ((uint64_t)(2 * n_buckets + L) * 4 + kCursorAlign - 1) / kCursorAlign * kCursorAlign;
}
// the two sizes the layout takes from the table type, read off the types the kernels store
struct PoolElem {
    uint32_t v2_bytes, spill_bytes;
};
template <typename T>
constexpr PoolElem pool_elem() {
    return {sizeof(v2_t<T>), sizeof(SpillEntry<T>)};
}
inline PoolElem pool_elem(bool fp16) { return fp16 ? pool_elem<half_t>() : pool_elem<float>(); }

uint64_t plan_buckets(BucketPlan &plan, const GridMeta &m, uint32_t L, uint32_t B, uint32_t D, bool plain, PoolElem elem) {
    const uint64_t worst = (uint64_t)B << D;  // worst-case entries of one level (all singles)
    uint64_t bytes = 0;
    uint32_t nbt = 0;
    plan.interleaved = 0;
    for (uint32_t l = 0; l < L; l++) {
        // dense plain levels (k_grid_bwd_scatter_plain's MODE 2 / 3): 128-row groups dealt to up to 64 buckets
        const bool il = plain && dense_paired(m.lv[l].flags, D);
        if (il) plan.interleaved |= 1u << l;
        const uint32_t groups = (m.lv[l].hashmap_size + (1u << kGroupRowsLog2) - 1) >> kGroupRowsLog2;
        const uint32_t nb = il ? std::min<uint32_t>(groups, kMaxBucketsPerLevel)
                               : (m.lv[l].hashmap_size + kBucketRows - 1) / kBucketRows;
        plan.first_bucket[l] = nbt;
        const uint64_t expect = level_is_generic(m.lv[l], D, plain) ? worst : worst / 2 + worst / 128;
        const uint64_t mean = (expect + nb - 1) / nb;
        uint64_t cap = mean + mean / 8 + (uint64_t)(12.0 * sqrt((double)mean)) + 64;
        if (cap > worst) cap = worst;
        if (cap > 0xffffffffull) cap = 0xffffffffull;
        cap &= ~1ull;  // even: with even reservations (k_grid_bwd_scatter_plain) every slot PAIR of a workgroup stays inside a pool
        plan.cap[l] = (uint32_t)cap;
        const uint64_t slots = cap * nb;
        // value stream (2 V2 per slot) | row stream (2 B per slot), each padded so that aligned quad reads stay inside
        plan.pool_off[l] = bytes;
        const uint64_t vals_bytes = (slots * 2 * elem.v2_bytes + 64 + 15) / 16 * 16;
        plan.rows_off[l] = bytes + vals_bytes;
        bytes += vals_bytes + (slots * 2 + 8 + 15) / 16 * 16;
        nbt += nb;
    }
    plan.first_bucket[L] = nbt;
    // spill list of a level: 1/16 of its worst case (every entry of the level overflowing), at least 1 M entries (or the worst case itself: small batches never reach the atomics); what
    // does not fit there either is added with device atomics by the scatter pass itself (see to_global)
    uint64_t spill_cap = std::max<uint64_t>(worst / 16, 1u << 20);
    if (spill_cap > worst) spill_cap = worst;
    plan.spill_cap = spill_cap > 0xffffffffull ? 0xffffffffu : (uint32_t)spill_cap;
    for (uint32_t l = 0; l < L; l++) {
        plan.spill_off[l] = bytes;
        bytes += ((uint64_t)plan.spill_cap * elem.spill_bytes + 15) / 16 * 16;
    }
    // slice images: a split bucket has n > S entries (S = slice length of its level) and ceil(n / S) < 2 n / S slices, so
    // the split buckets of a level together have fewer than 2 * (entries of the level) / S of them
    uint64_t slots = 2 * (worst * L) / g_slice_entries + 1;
    if (slots > (uint64_t)nbt * kMaxSlices) slots = (uint64_t)nbt * kMaxSlices;
    plan.partial_slots = (uint32_t)slots;
    plan.partial_off = bytes;
    bytes += slots * kBucketRows * 2 * sizeof(unsigned long long);
    return cursor_head_bytes(nbt, L) + bytes;
}

// 128 KiB of dynamic LDS needs an opt-in per kernel and DEVICE (a process may drive several devices)
template <typename K>
void allow_big_lds(K kernel, size_t lds) {
    static unsigned long long done = 0;  // bit per device ordinal; the attribute call is idempotent, so a race is harmless
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(__atomic_load_n(&done, __ATOMIC_RELAXED) & bit)) {
        (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        __atomic_fetch_or(&done, bit, __ATOMIC_RELAXED);
    }
}

// Large batches are walked in chunks of at most kChunkPoints points (scatter + reduce per chunk, the table accumulates):
// up to 4 M points a bucket of a hashed level stays within one reduce slice (4 M * 8 / 64 buckets = 512 K entries);
// beyond that every bucket would be cut into slices whose images travel through HBM (measured at 16 384 rays x 832:
// 6.5 ms in one piece vs 4 x 1.2 ms in chunks), and the workspace would grow with the batch.  The sum stays a
// fixed-order, bit-reproducible one: integer per chunk, chunks added to the table in order.
constexpr uint32_t kChunkPoints = 4u << 20;
// `plain` = linear interpolation, align_corners off (the x-pair pool format: 4 entries per point and level); the generic
// level classes emit 8 singles per point and level, so their chunks are half as long — both fit the SAME workspace, whose
// size does not depend on an interpolation mode the sizing call does not know.
__host__ inline uint32_t chunk_points(uint32_t B, bool plain = true) {
    uint32_t n = div_up(B, kChunkPoints);
    if (!plain && B > 65536) n *= 2;
    return n <= 1 ? B : div_up(div_up(B, n), 1024) * 1024;
}

// Shortest chunk the call will use for a batch (256 K points, or the batch itself), and the longest chunk whose plan fits
// `workspace_bytes` (0: not even the shortest does).
constexpr uint32_t kMinChunkPoints = 256u << 10;
__host__ inline uint32_t halve_chunk(uint32_t B, uint32_t step) {
    return div_up(div_up(B, div_up(B, step) * 2), 1024) * 1024;
}
__host__ inline uint32_t min_chunk_points(uint32_t B, bool plain) {
    uint32_t step = chunk_points(B, plain);
    while (step > kMinChunkPoints) step = halve_chunk(B, step);
    return step;
}
uint32_t fit_chunk(BucketPlan &plan, uint32_t B, const GridMeta &m, uint32_t L, bool plain, PoolElem elem,
                   uint64_t workspace_bytes) {
    for (uint32_t step = chunk_points(B, plain);; step = halve_chunk(B, step)) {
        if (plan_buckets(plan, m, L, step, 3, plain, elem) <= workspace_bytes) return step;  // `plan` is that chunk's
        if (step <= kMinChunkPoints) return 0;
    }
}

// One chunk of B points starting at b_begin, in a workspace laid out by `plan` (a full chunk's plan serves the last, shorter one).
template <typename T>
int launch_backward_bucketed_chunk(const T *grad, const float *inputs, T *ge, uint32_t B, uint32_t L, const GridMeta &m,
                                   uint32_t align, uint32_t interp, void *workspace, const BucketPlan &plan, hipStream_t s,
                                   uint32_t level_begin, uint32_t level_end, uint32_t b_begin, uint32_t B_all, int phase,
                                   bool cursors_cleared, bool table_zero) {
    // phase 0: scatter + reduce; 1: (zeroed cursors +) scatter only; 2: reduce only, of a scatter an earlier call has run
    // cursors_cleared: the caller has zeroed the head of the workspace (lnh_grid_backward_workspace_clear_bytes) for this
    // chunk; table_zero: grad_table holds zeros — the reduce pass stores its sums instead of adding them to what it reads
    const uint32_t nbt = plan.first_bucket[L], n_win = level_end - level_begin;
    if (((uint64_t)B << 3) > 0xffffffffull) {
        lnh_set_error("grid backward (bucketed): B = %u is too large for 32-bit pool slots", B);
        return LNH_ERR_UNSUPPORTED;
    }
    for (uint32_t l = 0; l < L; l++)
        if ((uint64_t)plan.cap[l] * (plan.first_bucket[l + 1] - plan.first_bucket[l]) > 0xffffffffull) {
            lnh_set_error("grid backward (bucketed): B = %u is too large for 32-bit pool slots", B);
            return LNH_ERR_UNSUPPORTED;
        }
    for (uint32_t l = 0; l < L; l++)
        if (plan.first_bucket[l + 1] - plan.first_bucket[l] > kMaxBucketsPerLevel) {
            lnh_set_error("grid backward (bucketed): level %u has more than %u buckets", l, kMaxBucketsPerLevel);
            return LNH_ERR_UNSUPPORTED;
        }
    const uint64_t cursor_bytes = cursor_head_bytes(nbt, L);
    uint32_t *cursor = reinterpret_cast<uint32_t *>(workspace);
    uint32_t *spill_cursor = cursor + nbt, *done = spill_cursor + L;
    char *pool = reinterpret_cast<char *>(workspace) + cursor_bytes;
    if (phase != 2 && !cursors_cleared) {
        const int zrc = lnh_zero_async(cursor, cursor_bytes, s, "grid backward (cursor clear)");
        if (zrc != LNH_OK) return zrc;
    }
    if (phase != 2)
        grid_bwd_scatter_launch(sizeof(T) == 2 ? LNH_F16 : LNH_F32, grad, inputs, ge, B, m, plan, pool, cursor, spill_cursor,
                                align, interp, level_begin, level_end, b_begin, B_all, s);
    int rc = lnh_check_launch("lnh_grid_encode_backward_ws(scatter)");
    if (rc || phase == 1) return rc;
    auto k = k_grid_bwd_reduce<T>;
    const size_t lds = (size_t)kBucketRows * 2 * sizeof(unsigned long long);
    allow_big_lds(k, lds);
    ReduceOrder ord;
    ord.bucket0 = plan.first_bucket[level_begin];
    ord.n_buckets = plan.first_bucket[level_end] - ord.bucket0;
    ord.n_levels = 0;
    ord.first[0] = 0;
    auto push = [&](uint32_t l) {
        ord.level[ord.n_levels] = l;
        ord.first[ord.n_levels + 1] = ord.first[ord.n_levels] + plan.first_bucket[l + 1] - plan.first_bucket[l];
        ord.n_levels++;
    };
    for (uint32_t l = level_begin; l < level_end; l++)
        if (!(m.lv[l].flags & LV_HASH)) push(l);
    for (uint32_t l = level_end; l-- > level_begin;)
        if (m.lv[l].flags & LV_HASH) push(l);
    // slices beyond the first: sum over buckets of ceil(n / kSliceEntries) - 1 <= (entries of the window) / kSliceEntries
    const uint64_t extra = std::min<uint64_t>((uint64_t)ord.n_buckets * (kMaxSlices - 1),
                                              (((uint64_t)B << 3) * n_win) / g_slice_entries);
    ord.n_extra = (uint32_t)extra;
    ord.slice_entries = g_slice_entries;
    LNH_LAUNCH(k, dim3(ord.n_extra + ord.n_buckets), dim3(1024), lds, s, ge, m, plan, pool, cursor, spill_cursor, done, L,
               ord, table_zero ? 1u : 0u);
    return lnh_check_launch("lnh_grid_encode_backward_ws(reduce)");
}

// split = 0: the whole backward of the levels [level_begin, level_end).
// split = 1 ("begin"): every chunk but the last completely, then the SCATTER pass of the last chunk (the caller passes all levels).
// split = 2 ("finish"): the REDUCE pass of the last chunk for the levels [level_begin, level_end) — after it the gradient of
//           those levels is final.  A data-parallel caller runs begin once and finish per level window, handing each window
//           to the all-reduce while the next is being reduced: the scatter pass stays in one piece (cut into level windows it
//           loses its level-fastest interleave: 2 windows cost 444 + 453 us against 707 us, profiles/r03_bwd_pipeline.txt).
template <typename T>
int launch_backward_bucketed(const T *grad, const float *inputs, T *ge, uint32_t B, uint32_t L, const GridMeta &m,
                             uint32_t align, uint32_t interp, void *workspace, uint64_t workspace_bytes,
                             hipStream_t s, uint32_t level_begin, uint32_t level_end, int split, uint32_t flags) {
    // flags (lnh_grid_encode_backward_ws_ex): LNH_BWD_WS_CLEARED — the head of the workspace is zero on entry (serves the
    // FIRST chunk's scatter pass); LNH_BWD_TABLE_ZERO — grad_embeddings is zero on entry (serves the first chunk's reduce pass)
    if (level_begin >= level_end) return LNH_OK;
    // The workspace serves one chunk at a time, so a SMALLER workspace than lnh_grid_backward_workspace_size() asks for is
    // not an error: the batch is walked in shorter chunks (fit_chunk halves the chunk until its plan fits; 3.09 GB / 1.60 /
    // 0.91 GB at 4096 rays x 832 cost 897 / 922 / 992 us, profiles/r04_workspace_chunks.txt).  Below the plan of the
    // shortest chunk the call fails and names that size.
    const bool plain = align == 0 && interp == 0;
    BucketPlan plan;
    const uint32_t step = fit_chunk(plan, B, m, L, plain, pool_elem<T>(), workspace_bytes);
    if (step == 0) {
        const uint64_t least = plan_buckets(plan, m, L, min_chunk_points(B, plain), 3, plain, pool_elem<T>());
        lnh_set_error("grid backward: workspace too small (%llu bytes; this batch needs at least %llu — "
                      "lnh_grid_backward_workspace_size_min — and runs fastest with lnh_grid_backward_workspace_size)",
                      (unsigned long long)workspace_bytes, (unsigned long long)least);
        return LNH_ERR_INVALID_ARG;
    }
    if (workspace == nullptr) {
        lnh_set_error("grid backward: workspace too small (%llu < %llu bytes)", (unsigned long long)workspace_bytes,
                      (unsigned long long)plan_buckets(plan, m, L, step, 3, plain, pool_elem<T>()));
        return LNH_ERR_INVALID_ARG;
    }
    for (uint32_t b0 = 0; b0 < B; b0 += step) {
        const bool last = b0 + step >= B;
        if (split == 2 && !last) continue;
        const int phase = last ? split : 0;
        const bool first = b0 == 0;
        const int rc = launch_backward_bucketed_chunk<T>(grad, inputs, ge, std::min(step, B - b0), L, m, align, interp,
                                                         workspace, plan, s, level_begin, level_end, b0, B, phase,
                                                         first && (flags & LNH_BWD_WS_CLEARED),
                                                         first && (flags & LNH_BWD_TABLE_ZERO));
        if (rc) return rc;
    }
    return LNH_OK;
}

// The sizing functions' version of that front (they answer 0, not an error): the geometry of a configuration the bucketed
// backward may serve.
bool bucketed_levels(GridMeta &m, const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                     uint32_t H, uint32_t gridtype, int align_corners) {
    if (!offsets_host || L < 1 || L > LNH_MAX_LEVELS || D != 3 || C != 2 || B == 0) return false;
    return build_meta(m, offsets_host, D, L, S, H, gridtype, align_corners != 0) == 0;
}
// The interpolation mode is not an argument of the sizing functions: they size for the larger of the two pool layouts it
// can select — each with ITS chunk length (`chunk`: chunk_points or min_chunk_points).
uint64_t larger_layout_bytes(const GridMeta &m, uint32_t L, uint32_t B, int align_corners, int dtype,
                             uint32_t (*chunk)(uint32_t, bool)) {
    BucketPlan plan;
    uint64_t need = 0;
    for (int plain = 0; plain <= (align_corners ? 0 : 1); plain++)
        need = std::max(need, plan_buckets(plan, m, L, chunk(B, plain != 0), 3, plain != 0, pool_elem(dtype == LNH_F16)));
    return need;
}

// what the bucketed backward checks before it looks at the level window
int check_bucketed(const void *grad, const float *inputs, const int32_t *offsets_host, const void *grad_embeddings, uint32_t B,
                   uint32_t D, uint32_t C, uint32_t L, int dtype) {
    const int rc = check_common(inputs, offsets_host, B, D, C, L, dtype);
    if (rc) return rc;
    LNH_REQUIRE(grad && grad_embeddings, LNH_ERR_INVALID_ARG, "grid backward: null grad/grad_embeddings");
    LNH_REQUIRE(D == 3 && C == 2, LNH_ERR_UNSUPPORTED,
                "grid backward (bucketed): only D == 3, C == 2 (use lnh_grid_encode_backward otherwise)");
    return LNH_OK;
}

}  // namespace

extern "C" {

uint64_t lnh_grid_backward_workspace_size(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                          float S, uint32_t H, uint32_t gridtype, int align_corners, int dtype) {
    GridMeta m;
    if (!bucketed_levels(m, offsets_host, B, D, C, L, S, H, gridtype, align_corners)) return 0;
    for (uint32_t l = 0; l < L; l++)
        if ((m.lv[l].hashmap_size + kBucketRows - 1) / kBucketRows > kMaxBucketsPerLevel) return 0;
    return larger_layout_bytes(m, L, B, align_corners, dtype, chunk_points);  // the workspace serves one chunk at a time
}

uint64_t lnh_grid_backward_workspace_size_min(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                              float S, uint32_t H, uint32_t gridtype, int align_corners, int dtype) {
    GridMeta m;
    if (lnh_grid_backward_workspace_size(offsets_host, B, D, C, L, S, H, gridtype, align_corners, dtype) == 0 ||
        !bucketed_levels(m, offsets_host, B, D, C, L, S, H, gridtype, align_corners))
        return 0;
    return larger_layout_bytes(m, L, B, align_corners, dtype, min_chunk_points);
}

void lnh_grid_backward_set_slice_entries(uint32_t entries) {
    g_slice_entries = entries == 0 ? kSliceEntries : std::min(std::max(entries, 1024u), kSliceEntries);
}

int lnh_grid_backward_plan_info(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                uint32_t H, uint32_t gridtype, int align_corners, int dtype, uint32_t level,
                                uint32_t *out4) {
    LNH_REQUIRE(out4 && offsets_host, LNH_ERR_INVALID_ARG, "grid backward plan: null argument");
    GridMeta m;
    LNH_REQUIRE(lnh_grid_backward_workspace_size(offsets_host, B, D, C, L, S, H, gridtype, align_corners, dtype) != 0 &&
                    level < L && bucketed_levels(m, offsets_host, B, D, C, L, S, H, gridtype, align_corners),
                LNH_ERR_UNSUPPORTED, "grid backward plan: configuration not served by the bucketed path");
    // (the layout of linear interpolation alone, unlike workspace_size: the plan the usual call runs with)
    BucketPlan plan;
    (void)plan_buckets(plan, m, L, chunk_points(B, align_corners == 0), D, align_corners == 0, pool_elem(dtype == LNH_F16));
    out4[0] = plan.first_bucket[level + 1] - plan.first_bucket[level];
    out4[1] = plan.cap[level];
    out4[2] = kBucketRows;
    out4[3] = g_slice_entries;
    return LNH_OK;
}

// The bucketed backward's one implementation; the four entry points below are forwards to it.
int lnh_grid_encode_backward_ws_ex(const void *grad, const float *inputs, const int32_t *offsets_host, void *grad_embeddings,
                                   uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                   int align_corners, uint32_t interp, int dtype, void *workspace, uint64_t workspace_bytes,
                                   uint32_t level_begin, uint32_t level_end, int split, uint32_t flags, lnh_stream_t stream) {
    LNH_REQUIRE(split >= 0 && split <= 2 && (flags & ~(uint32_t)(LNH_BWD_WS_CLEARED | LNH_BWD_TABLE_ZERO)) == 0,
                LNH_ERR_INVALID_ARG, "grid backward: split must be 0 (whole) / 1 (begin) / 2 (finish), flags LNH_BWD_*");
    int rc = check_bucketed(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, dtype);
    if (rc) return rc;
    if (level_end > L) level_end = L;
    LNH_REQUIRE(level_begin <= level_end, LNH_ERR_INVALID_ARG, "grid backward: need level_begin <= level_end <= L");
    if (B == 0) return LNH_OK;
    GridMeta m;
    if ((rc = resolve_levels(m, offsets_host, D, L, S, H, gridtype, align_corners))) return rc;
    if (split == 1) {  // begin: everything but the last reduce pass, over all levels
        level_begin = 0;
        level_end = L;
    }
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_backward_bucketed<T>((const T *)grad, inputs, (T *)grad_embeddings, B, L, m, align_corners != 0, interp,
                                           workspace, workspace_bytes, (hipStream_t)stream, level_begin, level_end, split, flags);
    });
}

int lnh_grid_encode_backward_ws(const void *grad, const float *inputs, const int32_t *offsets_host,
                                void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                void *workspace, uint64_t workspace_bytes, lnh_stream_t stream) {
    return lnh_grid_encode_backward_ws_ex(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, gridtype, align_corners,
                                          interp, dtype, workspace, workspace_bytes, 0, L, 0, 0, stream);
}

int lnh_grid_encode_backward_ws_begin(const void *grad, const float *inputs, const int32_t *offsets_host,
                                      void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                      uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                      void *workspace, uint64_t workspace_bytes, lnh_stream_t stream) {
    return lnh_grid_encode_backward_ws_ex(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, gridtype, align_corners,
                                          interp, dtype, workspace, workspace_bytes, 0, L, 1, 0, stream);
}

// _ws_levels and _ws_finish REFUSE a window that ends beyond L, where _ws_ex clamps it: they make that one check themselves,
// after the checks that precede the window's in _ws_ex, so that a call wrong in two ways still reports the same error first.
int lnh_grid_encode_backward_ws_levels(const void *grad, const float *inputs, const int32_t *offsets_host,
                                       void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                       uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                       void *workspace, uint64_t workspace_bytes, uint32_t level_begin,
                                       uint32_t level_end, lnh_stream_t stream) {
    const int rc = check_bucketed(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, dtype);
    if (rc) return rc;
    LNH_REQUIRE(level_end <= L, LNH_ERR_INVALID_ARG, "grid backward: need level_begin <= level_end <= L");
    return lnh_grid_encode_backward_ws_ex(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, gridtype, align_corners,
                                          interp, dtype, workspace, workspace_bytes, level_begin, level_end, 0, 0, stream);
}

int lnh_grid_encode_backward_ws_finish(const void *grad, const float *inputs, const int32_t *offsets_host,
                                       void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                       uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                       void *workspace, uint64_t workspace_bytes, uint32_t level_begin, uint32_t level_end,
                                       lnh_stream_t stream) {
    const int rc = check_bucketed(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, dtype);
    if (rc) return rc;
    LNH_REQUIRE(level_end <= L, LNH_ERR_INVALID_ARG, "grid backward: need level_begin <= level_end <= L");
    return lnh_grid_encode_backward_ws_ex(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, gridtype, align_corners,
                                          interp, dtype, workspace, workspace_bytes, level_begin, level_end, 2, 0, stream);
}

uint64_t lnh_grid_backward_workspace_clear_bytes(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                                 float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp,
                                                 int dtype, uint64_t workspace_bytes) {
    GridMeta m;
    if (!bucketed_levels(m, offsets_host, B, D, C, L, S, H, gridtype, align_corners)) return 0;
    // (the layout and chunk the call will run with, for any workspace it accepts; any dtype but LNH_F32 sizes as fp16)
    BucketPlan plan;
    if (fit_chunk(plan, B, m, L, align_corners == 0 && interp == 0, pool_elem(dtype != LNH_F32), workspace_bytes) == 0) return 0;
    return cursor_head_bytes(plan.first_bucket[L], L);
}

}  // extern "C"
