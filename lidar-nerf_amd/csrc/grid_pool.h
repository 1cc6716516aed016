// grid_pool.h — the contract between the two passes of the bucketed backward: bucket layout, pool and spill formats.
//
// Device-scope atomics top out at ~20 G/s on MI355X no matter how the work is spread over XCDs (measured,
// scratch/bench_grid.py), and every LiDAR ray starts in the same few cells around the sensor, which serialises the
// coarse levels on a handful of addresses.  The fast path therefore never adds into HBM atomically:
//   pass 1 (grid_bwd_scatter.hip): per (point, level) the run-merged corner contributions (row, w*g) are appended to
//           the pool of the table BUCKET they belong to (bucket = 8192 consecutive rows of one level); slots are
//           reserved with LDS counters + ONE global atomic per bucket per workgroup, so the pool writes of a
//           workgroup are contiguous per bucket;
//   pass 2 (grid_bwd_reduce.hip): one workgroup per bucket accumulates its pool in a 128 KiB LDS image and adds the
//           touched rows into the gradient table with plain stores — it owns those rows.  The LDS image is 64-bit
//           FIXED POINT: measured on MI355X, ds_add_f32 sustains ~100 G adds/s chip-wide while ds_add_u64 keeps up
//           with the 6 TB/s pool stream (scratch/ldsbench), and integer accumulation makes the sum exact and
//           order-independent (fp16 contributions are multiples of 2^-24, so scale 2^24 loses nothing).
// A bucket whose pool overflows (non-uniform input) sends the excess to the level's SPILL list (full row + value, sized
// for the worst case); pass 2's workgroups of exactly those buckets (cursor > cap) scan the list and add their entries
// into the same fixed-point image.  Buckets with many entries are cut into slices (blockIdx.y of pass 2); the slices'
// integer images are written out and summed by the slice that finishes last.  Every contribution therefore enters ONE
// integer sum per table row, whichever pool / spill slot it landed in: the result does not depend on workgroup arrival
// order, for fp32 tables too (each contribution is truncated to 2^-40 on its own before the sum).
#pragma once
#include "grid_geom.h"

constexpr uint32_t kBucketRowsLog2 = 13;
constexpr uint32_t kBucketRows = 1u << kBucketRowsLog2;
constexpr uint32_t kMaxBucketsPerLevel = 64;

struct BucketPlan {
    uint32_t first_bucket[LNH_MAX_LEVELS + 1];  // prefix sum of buckets per level
    uint32_t cap[LNH_MAX_LEVELS];               // pool slots per bucket of that level
    uint64_t pool_off[LNH_MAX_LEVELS];          // byte offset of that level's pool region (16-byte aligned)
    uint64_t rows_off[LNH_MAX_LEVELS];          // byte offset of the level's 2-byte (row | code << 13) stream
    uint64_t spill_off[LNH_MAX_LEVELS];         // byte offset of the level's spill list (SpillEntry<T>, level-local rows)
    uint64_t partial_off;                       // byte offset of the slice images (kBucketRows * 2 int64 each)
    uint32_t spill_cap;                         // entries per spill list (= worst case of a level: B * 2^D)
    uint32_t partial_slots;
    uint32_t interleaved;                       // bit l: level l maps rows to buckets in 128-row groups (see bucket_of_row)
};

// Pass 1 for the points [b_begin, b_begin + B) of a batch of B_all and the levels [level_begin, level_end): launches the
// scatter kernel(s) the level classes of that window need (grid_bwd_scatter.hip).  dtype (LNH_F32 / LNH_F16) is the type
// behind grad and grad_table; the caller checks the launch.
void grid_bwd_scatter_launch(int dtype, const void *grad, const float *inputs, void *grad_table, uint32_t B,
                             const GridMeta &m, const BucketPlan &plan, char *pool, uint32_t *cursor, uint32_t *spill_cursor,
                             uint32_t align, uint32_t interp, uint32_t level_begin, uint32_t level_end, uint32_t b_begin,
                             uint32_t B_all, hipStream_t s);

namespace {

// ---- pool entries.  One entry carries the contributions of an x-NEIGHBOUR PAIR of corners (c0 = even corner index,
// c1 = c0 | 1): their rows differ in a way a 3-bit code describes, so the pair shares ONE 13-bit row field:
//   hashed power-of-two level:  r1 = r0 ^ ((2 << code) - 1)   (the x term of the hash is the x coordinate itself, so
//                               r0 ^ r1 = x ^ (x + 1) = 2^(t+1) - 1 with t = trailing ones of x; code = t <= 6)
//   every other level:          r1 = r0 + 1                    (dense x stride; code = 0)
//   code 7:                     single — only the first value applies (pairs the code cannot describe: t >= 7, one in
//                               128; a dense pair straddling a bucket boundary; every corner of the generic level
//                               classes: tiled grids, align_corners, smoothstep, non-power-of-two hash tables)
// Pool streams per level: values (two channel pairs: 8 bytes for fp16 tables, 16 for fp32) | 2-byte (row | code << 13):
// 10 bytes per PAIR of corners through HBM instead of 12, and half the LDS rank / stage / row-decode work per corner.
constexpr uint32_t kCodeSingle = 7;
// Dense level indexed in all D dimensions that the paired scatter serves (k_grid_bwd_scatter_plain MODE 2 / 3): the
// default lattice (no wrap needed) or tiny-cuda-nn's (stride res, one wrap: the x pair whose first row is the level's
// last row wraps to row 0 and travels as two singles).
__host__ __device__ inline bool dense_paired(uint32_t flags, uint32_t D) {
    return !(flags & LV_HASH) && (flags & (LV_NOWRAP | LV_WRAP1)) && (flags & 15u) == D;
}

// Rows -> buckets.  Hashed (and generic) levels: bucket = 8192 CONSECUTIVE rows — the hash spreads every batch evenly.
// Dense plain levels: rows are positions in space, every LiDAR ray leaves the same few cells around the sensor, and with
// consecutive rows level 0 is ONE bucket: one workgroup of the reduce pass worked 240 us on its 350 K entries, most of them
// on a handful of rows, while the 64 buckets of a hashed level took 85 us side by side — the whole pass waited for it
// (profiles/r04_reduce_levels.txt).  There the rows are dealt to up to 64 buckets in GROUPS OF 128: bucket = (row >> 7) & 63,
// position inside the bucket's image = (row >> 13) * 128 + (row & 127).  The eight corner rows of a cell differ by 1, R and
// R^2 (R = resolution + 1 >= 17), so the y / z neighbours of a hot cell land in other groups, i.e. other buckets; an x pair
// (r, r + 1) stays inside its group unless r & 127 == 127 (then it travels as two singles, one pair in 128).
constexpr uint32_t kGroupRowsLog2 = 7;
__host__ __device__ inline uint32_t bucket_of_row(uint32_t r, bool il) {
    return il ? (r >> kGroupRowsLog2) & (kMaxBucketsPerLevel - 1) : r >> kBucketRowsLog2;
}
__host__ __device__ inline uint32_t local_of_row(uint32_t r, bool il) {
    return il ? ((r >> kBucketRowsLog2) << kGroupRowsLog2) | (r & ((1u << kGroupRowsLog2) - 1)) : r & (kBucketRows - 1);
}
__host__ __device__ inline uint32_t row_of_local(uint32_t loc, uint32_t bk, bool il) {
    return il ? ((loc >> kGroupRowsLog2) << kBucketRowsLog2) | (bk << kGroupRowsLog2) | (loc & ((1u << kGroupRowsLog2) - 1))
              : (bk << kBucketRowsLog2) | loc;
}

template <typename T>
struct V2Of;
template <>
struct V2Of<half_t> {
    typedef half2_t type;
};
typedef float f32x2_t __attribute__((ext_vector_type(2)));
template <>
struct V2Of<float> {
    typedef f32x2_t type;
};
template <typename T>
using v2_t = typename V2Of<T>::type;

// spill-list entry: level-local row (19 bits) | code << 29, then the two channel pairs
template <typename T>
struct SpillEntry {
    uint32_t key;
    v2_t<T> a, b;
};

// value * 2^24 of an fp16 number as an exact 64-bit integer in 4 VALU operations: x = h * 2^24 is an integer with
// |x| < 2^40, so the double 1.5 * 2^52 + x is exact, its exponent is that of 2^52 and its 52 mantissa bits hold 2^51 + x —
// low word = x mod 2^32, high word = 0x43380000 + floor(x / 2^32).  (The bit-twiddling form — (1024 | m) << (e - 1),
// negate — cost 12 per value and made the reduce pass VALU-bound: 34 VALU operations per pool entry against two
// ds_add_u64.)
// A NON-FINITE value must not vanish in the integer sum: the training step looks for inf / NaN in this table gradient to
// skip an overflowed step.  The high word is therefore taken WHOLE (not its 20 mantissa bits, which are zero for inf and
// cancel for a NaN: a NaN gradient left a finite table): inf / NaN (exponent 0x7ff) give |x| >= 2^61 in multiples of 2^42, so
// a row's sum that holds any count of them short of an exact multiple of 1024 stays beyond 2^42, and the float step of the
// reduce pass rounds it to an infinity of the fp16 table.
__device__ __forceinline__ long long half_to_fixed24(half_t h) {
    const double d = __builtin_fma((double)(float)h, 16777216.0, 6755399441055744.0);
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, d);
    const int hi = (int)(uint32_t)(bits >> 32) - 0x43380000;
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (bits & 0xFFFFFFFFull));
}
// fixed-point images: fp16 contributions are exact multiples of 2^-24; fp32 ones get 2^-40 resolution, +-8e6 of range
template <typename T>
__device__ __forceinline__ void to_fixed(const v2_t<T> &v, long long &qa, long long &qb) {
    if constexpr (sizeof(T) == 2) {
        qa = half_to_fixed24(v[0]);
        qb = half_to_fixed24(v[1]);
    } else {
        qa = (long long)ldexp((double)v[0], 40);
        qb = (long long)ldexp((double)v[1], 40);
    }
}
template <typename T>
__device__ __forceinline__ v2_t<T> make_v2(float a, float b) {
    v2_t<T> r = {(T)a, (T)b};
    return r;
}
// second row of a pair (see above); `hashed` is workgroup-uniform
__device__ __forceinline__ uint32_t pair_row(uint32_t r0, uint32_t code, bool hashed) {
    return hashed ? r0 ^ ((2u << code) - 1u) : r0 + 1u;
}
// true when every corner of the level travels as a single (generic class): 8 entries per point
__host__ __device__ inline bool level_is_generic(const LevelParams &lv, uint32_t D, bool plain) {
    if (plain && (lv.flags & (LV_HASH | LV_POW2)) == (LV_HASH | LV_POW2)) return false;
    if (plain && dense_paired(lv.flags, D)) return false;
    return true;
}

__device__ __forceinline__ void atomic_add_pair(half_t *p, float a, float b) {
    half2_t v = {(half_t)a, (half_t)b};
    __builtin_amdgcn_global_atomic_fadd_v2f16((__attribute__((address_space(1))) half2_t *)p, v);
}
__device__ __forceinline__ void atomic_add_pair(float *p, float a, float b) {
    unsafeAtomicAdd(p, a);
    unsafeAtomicAdd(p + 1, b);
}

}  // namespace
