// grid_bwd_scatter.hip — pass 1 of the bucketed table backward (grid_pool.h): per (point, level) the run-merged corner
// contributions go to the pool of their table bucket.  Two kernels, one per kind of level: k_grid_bwd_scatter_plain for
// the two plain classes (every level of the usual configuration: x-neighbour pairs, 4 entries per point) and
// k_grid_bwd_scatter for the generic classes (8 singles per point); grid_bwd_scatter_launch picks per level window.
#include "grid_pool.h"

namespace {

// ---- scatter pass for the GENERIC level classes (tiled grids, align_corners, smoothstep, non-power-of-two hash tables,
// dense levels that are not indexed in all D dimensions): no code describes the rows of an x-neighbour pair there, so every
// corner travels as a SINGLE (code 7, the second value pair of its entry zero) — eight entries per point.
// One thread = one (point, level): every workgroup reserves its pool slots with ONE global atomic per touched bucket
// for its 1024 points — the cursor atomics are device atomics too (~20 G/s), so fewer, larger reservations matter.
// CAP = LDS staging slots of a workgroup: launched with 6 * 1024, the worst case is 8 * 1024 (no sample of the workgroup
// merges with a neighbour).  Entries beyond CAP bypass the staging and are written to their global slot by the thread
// that holds them.
template <typename T, int D, int CAP>
__global__ void __launch_bounds__(1024)
k_grid_bwd_scatter(const T *__restrict__ grad, const float *__restrict__ inputs, uint32_t B, GridMeta meta,
                   BucketPlan plan, char *__restrict__ pool_bytes, uint32_t *__restrict__ cursor,
                   uint32_t *__restrict__ spill_cursor, uint32_t align, uint32_t interp, uint32_t n_levels,
                   uint32_t level0, uint32_t b_begin, uint32_t B_all, T *__restrict__ grad_table) {
    // this launch handles the points [b_begin, b_begin + B) of a batch of B_all (large batches are walked in chunks)
    constexpr int C = 2, NCORN = 1 << D, NTHREADS = 1024;
    typedef v2_t<T> V2;
    __shared__ uint2 lout[kMaxBucketsPerLevel];           // per bucket: {pool slot - staging slot, staging slots that fit}
    __shared__ uint32_t lsp[kMaxBucketsPerLevel];         // per bucket: spill slot - staging slot of the entries that do not
    __shared__ uint32_t lcnt[kMaxBucketsPerLevel];
    __shared__ uint32_t lstart[kMaxBucketsPerLevel + 1];  // first staging slot per bucket (workgroup-local)
    __shared__ __attribute__((aligned(16))) uint32_t skey[CAP];  // staged entries, bucket-sorted: level-local row
    __shared__ __attribute__((aligned(16))) V2 sval[CAP];
    // level-fastest workgroup order: concurrently resident workgroups work on the same points at different levels
    // (the coordinates stay in L2, the cursor atomics spread over all levels' counters instead of 64 hot words).
    // (A persistent-workgroup variant of this kernel was measured 1.5x SLOWER: the hardware dispatcher overlaps the
    // phases of independent workgroups better than a barrier-separated item loop does.)
    const int lane = threadIdx.x & 63;
    const uint32_t level = level0 + blockIdx.x % n_levels, chunk = blockIdx.x / n_levels;  // window [level0, +n_levels)
    const LevelParams lv = meta.lv[level];
    const uint32_t fb = plan.first_bucket[level], nb = plan.first_bucket[level + 1] - fb, cap = plan.cap[level];
    // the launch covers the whole window: the levels of the two plain classes in it are k_grid_bwd_scatter_plain's
    if (!level_is_generic(lv, (uint32_t)D, align == 0 && interp == 0)) return;
    if (threadIdx.x < kMaxBucketsPerLevel) lcnt[threadIdx.x] = 0;

    V2 val[NCORN];  // (w * g0, w * g1) per corner, already in the pool's element type
    uint32_t row[NCORN];
    bool emit;
    {
        const uint32_t bl = chunk * blockDim.x + threadIdx.x;
        const bool in_range = bl < B;
        const uint32_t bc = b_begin + (in_range ? bl : 0);  // unconditional loads from a clamped index + selects
        float x[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            const float xv = inputs[(size_t)bc * D + d];
            x[d] = in_range ? xv : -1.0f;
        }
        const Vec<T, 2> gv = load_vec<T, 2>(grad + ((size_t)level * B_all + bc) * C);
        Cell<D> cell;
        bool ok = in_range;
#pragma unroll
        for (int d = 0; d < D; d++) ok = ok && !(x[d] < 0.0f || x[d] > 1.0f);
        // Lanes that are not `ok` never emit and never merge with a neighbour (unique key below): instead of zeroing
        // their 8 weights and 8 rows afterwards, they are located at the cube centre (3 selects) with a zero gradient
        // (every value stays finite — the scan multiplies foreign lanes by 0, and 0 * inf would poison a neighbour).
#pragma unroll
        for (int d = 0; d < D; d++) x[d] = ok ? x[d] : 0.5f;
        (void)locate<D>(x, lv, align != 0, interp, cell);
        const float g0 = ok ? (float)gv.v[0] : 0.0f, g1 = ok ? (float)gv.v[1] : 0.0f;
        // a sample whose upstream gradient is exactly zero (fp16 underflow behind an opaque surface, masked-out
        // rays) contributes nothing: it moves no entry of its own through the pool, but within three lanes of a sample
        // that has a gradient it stays a silent member of the run (k_grid_bwd_scatter_plain has the measurements:
        // dropped outright, it cut the runs of a trained field's coarse levels)
        const bool nonzero = ok && (g0 != 0.0f || g1 != 0.0f);
        {
            const unsigned long long in_m = __ballot(ok), nz_m = __ballot(nonzero);
            const unsigned long long nz1_m = nz_m | (nz_m << 1) | (nz_m >> 1);
            ok = ((in_m & (nz1_m | (nz1_m << 2) | (nz1_m >> 2))) >> lane) & 1ull;
        }
        // ---- run-merge inside 16-lane rows: consecutive lanes are consecutive samples of a ray, which share their cell
        //      on the coarser levels.  Runs are cut at DPP row starts (pure-VALU row_shr scan, no cross-row traffic), and
        //      a wave with fewer than kMinMerges mergeable lanes skips the scan altogether — on the fine levels almost
        //      every wave has SOME coincidental pair, and scanning 16 values to save one or two entries does not pay.
        constexpr int kMinMerges = 8;  // (4 / 16 / 24 measured within noise of each other)
        uint32_t key[D];
#pragma unroll
        for (int d = 0; d < D; d++) key[d] = ok ? cell.term[d][0] : 0xffffffffu - lane;
        // dense (coarse) levels: runs span whole waves and every entry lands in the same few buckets, so there the
        // full-wave scan (two extra cross-row steps) is worth its price
        const bool row_local = (lv.flags & LV_HASH) != 0;  // workgroup-uniform
        bool same_prev = row_local ? (lane & 15) != 0 : lane != 0;
#pragma unroll
        for (int d = 0; d < D; d++) {
            // wave_shr:1 (0x138): previous lane across rows
            const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key[d], 0x138, 0xf, 0xf, false);
            same_prev &= (up == key[d]);
        }
        unsigned long long heads = __ballot(!same_prev);
        const bool any_merge = __builtin_popcountll(~heads) >= kMinMerges;  // wave-uniform
        if (!any_merge) heads = ~0ull;
        const unsigned long long below = heads & ((2ull << lane) - 1ull);
        const int run_start = 63 - __builtin_clzll(below);
        const unsigned long long heads_above = (lane == 63) ? 0ull : (heads >> (lane + 1));
        // run tails; a zero-gradient sample that is a run of one emits nothing
        emit = ok && ((lane == 63) || (heads_above & 1ull)) && (nonzero || !((heads >> lane) & 1ull));
        const f32x2_t gg = {g0, g1};
#pragma unroll
        for (uint32_t c = 0; c < (uint32_t)NCORN; c++) {
            // w * (g0, g1) as one packed multiply, narrowed with one packed conversion: float product first, then the
            // per-contribution rounding to the table type, as the reference does (gridencoder.cu:350)
            const f32x2_t p = gg * corner_weight<D>(cell, c);
            val[c] = __builtin_convertvector(p, V2);
            row[c] = corner_row<D>(cell, lv, c);
        }
        if (any_merge) {  // wave-uniform: sum the runs in fp32 (one rounding of the sum when it is stored again)
            const SegScanMask sm = wave_segscan_mask(lane, run_start);
            float vv[2 * NCORN];
#pragma unroll
            for (uint32_t c = 0; c < (uint32_t)NCORN; c++) {
                vv[2 * c] = (float)val[c][0];
                vv[2 * c + 1] = (float)val[c][1];
            }
            row_segscan_add_n(vv, sm);
            if (!row_local) cross_segscan_add_n(vv, sm);
#pragma unroll
            for (uint32_t c = 0; c < (uint32_t)NCORN; c++) val[c] = make_v2<T>(vv[2 * c], vv[2 * c + 1]);
        }
    }
    __syncthreads();
    // ---- reserve pool slots: LDS rank per (bucket), one global atomic per touched bucket per workgroup
    uint32_t rank[NCORN];
#pragma unroll
    for (int c = 0; c < NCORN; c += 2) {  // the even corners
        // On dense (coarse) levels every emitting lane of the wave usually targets the SAME bucket: 64 returning
        // LDS atomics on one counter serialise, so aggregate — one lane adds the population count, the others
        // take their rank from the lane mask.  Mixed buckets (hashed levels) fall back to per-lane atomics.
        const uint32_t bk = row[c] >> kBucketRowsLog2;
        rank[c] = 0;
        if (lv.flags & LV_HASH) {  // workgroup-uniform: hashed level, buckets are mixed -> per-lane atomics
            if (emit) rank[c] = atomicAdd(&lcnt[bk], 1u);
            continue;
        }
        const unsigned long long em = __ballot(emit);
        if (em == 0ull) continue;  // wave-uniform
        const int leader = __builtin_ctzll(em);
        const uint32_t bk0 = __shfl(bk, leader, 64);
        const bool uniform = __ballot(emit && bk != bk0) == 0ull;
        if (uniform) {
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&lcnt[bk0], (uint32_t)__builtin_popcountll(em));
            base = __shfl(base, leader, 64);
            rank[c] = base + (uint32_t)__builtin_popcountll(em & ((1ull << lane) - 1ull));
        } else if (emit) {
            rank[c] = atomicAdd(&lcnt[bk], 1u);
        }
    }
#pragma unroll
    for (int c = 1; c < NCORN; c += 2) {  // the odd corners (the x neighbours): per-lane atomics on every level
        rank[c] = 0;
        if (emit) rank[c] = atomicAdd(&lcnt[row[c] >> kBucketRowsLog2], 1u);
    }
    __syncthreads();
    // global reservation + exclusive scan of the workgroup's bucket counts (first wave: one bucket counter per lane)
    if (threadIdx.x < 64) {
        static_assert(kMaxBucketsPerLevel == 64, "one bucket counter per lane of the first wave");
        const uint32_t n0 = lcnt[lane];
        uint32_t base = 0;
        if ((uint32_t)lane < nb && n0) base = atomicAdd(&cursor[fb + lane], n0);
        const uint32_t incl = wave_scan_add_u32(n0);  // DPP network: no LDS round trips while the atomics are in flight
        const uint32_t st = incl - n0;
        lstart[lane] = st;
        if (lane == 63) lstart[kMaxBucketsPerLevel] = incl;
        // staging slot pos of bucket bk goes to pool slot bk*cap + base + (pos - st) while base + (pos - st) < cap;
        // the `over` entries behind those go to consecutive slots of the level's spill list, reserved with ONE atomic
        // per workgroup (and none at all in the usual case of no overflow)
        const uint32_t fit = base < cap ? min(cap - base, n0) : 0u, over = n0 - fit;
        const uint32_t oincl = wave_scan_add_u32(over);
        uint32_t sp0 = 0;
        if (lane == 63 && oincl) sp0 = atomicAdd(&spill_cursor[level], oincl);
        sp0 = __shfl(sp0, 63, 64);
        lout[lane] = make_uint2((uint32_t)lane * cap + base - st, st + fit);
        lsp[lane] = sp0 + (oincl - over) - (st + fit);
    }
    __syncthreads();
    // pool streams of this level: values [slot][2] | rows [slot] | spill list; byte offsets inside a level fit 32 bits
    // (<= 4 M points per launch), so every store is base (scalar) + 32-bit lane offset — no 64-bit address arithmetic
    char *pvals = pool_bytes + plan.pool_off[level];
    char *prows = pool_bytes + plan.rows_off[level];
    char *spill = pool_bytes + plan.spill_off[level];
    // entry (level-local row r, values a) at staging position `pos` -> its pool slot (bucket-local row | 7 << 13) or, pool
    // full, the spill list; o = lout[] of its bucket
    auto to_global = [&](uint32_t pos, uint32_t r, V2 a, uint2 o) {
        const V2 none = make_v2<T>(0.0f, 0.0f);
        if (pos < o.y) {
            const uint32_t slot = o.x + pos;
            struct Pair { V2 a, b; } pr = {a, none};
            *reinterpret_cast<Pair *>(pvals + slot * (uint32_t)sizeof(Pair)) = pr;
            *reinterpret_cast<unsigned short *>(prows + slot * 2u) =
                (unsigned short)((r & (kBucketRows - 1)) | (kCodeSingle << kBucketRowsLog2));
        } else {
            const uint32_t sp = lsp[r >> kBucketRowsLog2] + pos;
            if (sp < plan.spill_cap) {
                SpillEntry<T> e = {r | (kCodeSingle << 29), a, none};
                *reinterpret_cast<SpillEntry<T> *>(spill + sp * (uint32_t)sizeof(SpillEntry<T>)) = e;
            } else {
                // The spill list is full too (it holds 1/16 of a level's worst case: a batch whose points crowd into a
                // few buckets of a DENSE level without merging): these entries go straight into the table with device
                // atomics — always correct, slow (~20 G/s), and the one place where a sum depends on arrival order.
                T *gt = grad_table + (size_t)lv.offset * 2;
                atomic_add_pair(gt + (size_t)r * 2, (float)a[0], (float)a[1]);
            }
        }
    };
    // ---- stage the entries in LDS grouped by bucket, then stream them out: consecutive lanes write consecutive pool
    //      slots (a per-lane scatter of small stores costs one cache-line transaction per lane)
    if (emit) {
#pragma unroll
        for (int i = 0; i < NCORN; i++) {
            const int c = i < NCORN / 2 ? 2 * i : 2 * (i - NCORN / 2) + 1;  // (even corners first, as they were ranked)
            const uint32_t bk = row[c] >> kBucketRowsLog2, pos = lstart[bk] + rank[c];
            if (pos < (uint32_t)CAP) {
                skey[pos] = row[c];
                sval[pos] = val[c];
            } else {
                to_global(pos, row[c], val[c], lout[bk]);
            }
        }
    }
    __syncthreads();
    // (workgroup-uniform, made scalar: the rounds below stop at it without touching LDS for slots nobody filled)
    const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(lstart[kMaxBucketsPerLevel], (uint32_t)CAP));
    // every thread moves up to CAP / 1024 staged entries: all their LDS reads (entry, then the bucket's slot map) are
    // issued before the first use — one round trip for the batch instead of two dependent ones per entry.  (Moving PAIRS of
    // neighbouring entries per thread — 8-byte LDS reads, one 16-byte value store + one 4-byte row store per pair where both
    // sit in one bucket — was measured slower: 709 vs 677 us; the wide stores land on 8- / 2-byte boundaries.  So was ONE 16-byte
    // LDS record per staged entry instead of three 4-byte arrays: 755 vs 675 us.  Both on the pair format this kernel no
    // longer serves, which staged two value pairs per entry.)
    constexpr int NW = CAP / NTHREADS;
    static_assert(CAP % NTHREADS == 0, "staging slots are dealt to the threads in rounds");
    uint32_t ks[NW];
    V2 as[NW];
    uint2 os[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) {
        if ((uint32_t)i * NTHREADS >= total) break;  // scalar branch
        const uint32_t pos = threadIdx.x + (uint32_t)i * NTHREADS, pc = pos < total ? pos : 0u;
        ks[i] = skey[pc];
        as[i] = sval[pc];
    }
#pragma unroll
    for (int i = 0; i < NW; i++) {
        if ((uint32_t)i * NTHREADS >= total) break;
        os[i] = lout[(ks[i] >> kBucketRowsLog2) & (kMaxBucketsPerLevel - 1)];
    }
#pragma unroll
    for (int i = 0; i < NW; i++) {
        if ((uint32_t)i * NTHREADS >= total) break;
        const uint32_t pos = threadIdx.x + (uint32_t)i * NTHREADS;
        if (pos < total) to_global(pos, ks[i], as[i], os[i]);
    }
}

#ifndef LNH_SCATTER_THREADS
#define LNH_SCATTER_THREADS 1024
#endif
constexpr int kScatterThreads = LNH_SCATTER_THREADS;  // points (= threads) of a scatter workgroup; 5 staging slots each
// Paired write-out (round 5): a workgroup reserves an EVEN number of slots per bucket (an odd count is padded with one
// zero-valued single on the bucket's local row 0, which adds nothing), so every bucket's segment starts at an even staging
// slot AND at an even pool slot; a thread then writes TWO consecutive entries with one 16-byte value store and one 4-byte row
// store (fp16 tables; 2 x 16 + 4 for fp32) instead of two 8-byte and two 2-byte stores, and reads its staging with 8-byte
// LDS loads.  Round 3 tried pairs without the padding (the wide stores landed on 8- / 2-byte boundaries: 709 against 677 us).
// ---- scatter pass for the two PLAIN level classes (hashed power-of-two tables / dense levels, linear interpolation,
// align_corners off — every level of the usual configuration).  Same contract as k_grid_bwd_scatter (which keeps the
// generic classes): same pool format, same cursors, same spill rules; what differs is the instruction budget.  The scatter
// pass is issue-bound (profiles/r03_grid_counters.json: 324 VALU + 168 SALU per wave), so this kernel is written to the
// instruction:
//   * every lane predicate that is a function of wave-wide facts (who continues a run, who emits, the six "take" masks of
//     the segmented scan) lives in SGPR PAIRS: built from two ballots with scalar shifts / ands and handed to the VALU as a
//     v_cndmask source or an exec mask (__builtin_amdgcn_inverse_ballot_w64) — no 64-bit lane arithmetic, no run_start;
//   * the scan executes only the steps the LONGEST run of the wave needs (scalar test on the masks): runs of 2 — the usual
//     case on the middle levels — cost one step instead of four;
//   * the range test is two min3 / max3 + two compares; locate() without its own second range test;
//   * a workgroup whose entries all fit their staging and pool slots (flag from the reserving wave; always, short of
//     adversarial inputs) stages and writes out WITHOUT per-entry tests: the staged key carries the bucket's LDS address
//     pre-shifted (key >> 16) and the pool's 16-bit (row | code << 13) in its low half, so the write-out of an entry is
//     one shift, one LDS read, one add, two shifts and two stores; LDS addresses of the staging reads are immediates;
//   * level / chunk come from a 2-D grid (x = level: the level-fastest order), not from a division.
// (amdgpu_num_sgpr: two 1024-thread workgroups per CU need 8 waves per SIMD, and gfx950 admits 8 only up to 80 SGPRs
//  including VCC / flat-scratch / XNACK — at the 84 the unconstrained allocation took, ONE workgroup per CU ran and the
//  pass took 959 us instead of 682; amdgpu_waves_per_eu: the same for the VGPR side, 64 at most — fp16 tables; fp32 tables
//  stage 100 KB and run one workgroup per CU anyway; profiles/r04_scatter_phases.txt)
template <typename T, int NTHREADS, int CAP>
__global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_num_sgpr(72), amdgpu_waves_per_eu(sizeof(T) == 2 ? 8 : 4)))
k_grid_bwd_scatter_plain(const T *__restrict__ grad, const float *__restrict__ inputs, uint32_t B, GridMeta meta,
                         BucketPlan plan, char *__restrict__ pool_bytes, uint32_t *__restrict__ cursor,
                         uint32_t *__restrict__ spill_cursor, uint32_t level0, uint32_t b_begin, uint32_t B_all,
                         T *__restrict__ grad_table) {
    constexpr int NP = 4;
    typedef v2_t<T> V2;
    struct Pair { V2 a, b; };
    __shared__ uint32_t lcnt[kMaxBucketsPerLevel];
    __shared__ uint32_t lstart[kMaxBucketsPerLevel + 1];  // first staging slot per bucket; [64] = staged entries in all
    __shared__ uint32_t lox[kMaxBucketsPerLevel];          // pool slot - staging slot
    __shared__ uint32_t lofit[kMaxBucketsPerLevel];        // first staging slot of the bucket that does NOT fit its pool
    __shared__ uint32_t lsp[kMaxBucketsPerLevel];          // spill slot - staging slot of those
    __shared__ uint32_t lflag;                             // 1: everything fits staging and pool (the fast path)
    // staged key: bits 0-12 bucket-local row | 13-15 code | 16-23 bucket * 4
    __shared__ __attribute__((aligned(16))) uint32_t skey[CAP];
    // (the two value pairs of an entry in ONE 8-byte LDS record — one write per entry, one 16-byte read per written-out slot
    //  pair — was measured in round 5: 766 against 531 us, the random 8-byte LDS writes of the staging conflict; round 3 saw
    //  the same with a 16-byte record)
    __shared__ __attribute__((aligned(16))) V2 sa[CAP], sb[CAP];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t level = level0 + blockIdx.x, chunk = blockIdx.y;
    const LevelParams lv = meta.lv[level];
    const bool cls_hash = (lv.flags & (LV_HASH | LV_POW2)) == (LV_HASH | LV_POW2);
    const bool cls_dense = dense_paired(lv.flags, 3u);
    if (!cls_hash && !cls_dense) return;  // generic class: k_grid_bwd_scatter's level
    const uint32_t fb = plan.first_bucket[level], nb = plan.first_bucket[level + 1] - fb, cap = plan.cap[level];
    auto lds_at = [](uint32_t *base, uint32_t byte_off) -> uint32_t & {
        return *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(base) + byte_off);
    };
    auto body = [&](auto mode_c) {
    constexpr int MODE = decltype(mode_c)::value;  // 1 hashed, 2 dense, 3 dense on tiny-cuda-nn's lattice (stride res, wrap)
    constexpr bool DENSE = MODE >= 2;
    // x neighbour of a dense row: r + 1, wrapped to row 0 past the level's last row on tiny-cuda-nn's lattice (only singles
    // reach the wrap: a pair whose first row is the last row is sent as two singles, see `single` below)
    auto x_next = [&](uint32_t r) -> uint32_t {
        if constexpr (MODE == 3) return r + 1u == lv.hashmap_size ? 0u : r + 1u;
        else return r + 1u;
    };
    LNH_MARK("A load+locate");
    if (tid < kMaxBucketsPerLevel) lcnt[tid] = 0;
    // ---- load (unconditional, clamped index), range test, cell
    const uint32_t bl = chunk * (uint32_t)NTHREADS + tid;
    const bool in_range = bl < B;
    const uint32_t bc = b_begin + (in_range ? bl : 0u);
    const float *px = inputs + (size_t)bc * 3;
    float x0 = px[0], x1 = px[1], x2 = px[2];
    const Vec<T, 2> gv = load_vec<T, 2>(grad + ((size_t)level * B_all + bc) * 2);
    __syncthreads();  // (the zeroed counters; the loads above stay in flight across it)
    // !(x < 0 || x > 1) per coordinate (gridencoder.cu:158-163), as max3 / min3: a NaN coordinate drops out of both
    bool ok = in_range & !(__builtin_fmaxf(__builtin_fmaxf(x0, x1), x2) > 1.0f) &
              !(__builtin_fminf(__builtin_fminf(x0, x1), x2) < 0.0f);
    const float g0 = (float)gv.v[0], g1 = (float)gv.v[1];
    // A sample whose upstream gradient is exactly zero contributes nothing.  It is not moved through the pool ON ITS OWN (see
    // emit_m below), but it stays a silent member of a run of same-cell neighbours: dropped outright — as rounds 3-4 did — it
    // CUT that run.  A field that has trained for a few hundred steps has such samples sprinkled along every ray: the coarse
    // levels' entry counts went from 0.47 M to 1.7 M (level 0) with them, one bucket of level 0 past its pool share and into
    // two slices, and the reduce pass from 310 to 680 us (profiles/r05_reduce_drift.txt).  Its zeros add nothing to a sum.
    bool nonzero;
    if constexpr (sizeof(T) == 2) {
        uint32_t raw;
        __builtin_memcpy(&raw, &gv, 4);
        nonzero = (raw & 0x7fff7fffu) != 0u;
    } else {
        nonzero = (g0 != 0.0f) | (g1 != 0.0f);
    }
    // Lanes that are not `ok` never emit and never join a run (masks below); they only must stay FINITE, because the scan
    // multiplies foreign lanes by 0: out-of-range coordinates are replaced by the cube centre.
    x0 = ok ? x0 : 0.5f;
    x1 = ok ? x1 : 0.5f;
    x2 = ok ? x2 : 0.5f;
    const float sc = lv.scale;
    const float p0 = fmaf(x0, sc, 0.5f), p1 = fmaf(x1, sc, 0.5f), p2 = fmaf(x2, sc, 0.5f);
    const float f0 = floorf(p0), f1 = floorf(p1), f2 = floorf(p2);
    const uint32_t c0 = (uint32_t)f0, c1 = (uint32_t)f1, c2 = (uint32_t)f2;
    const float fr0 = p0 - f0, fr1 = p1 - f1, fr2 = p2 - f2;
    LNH_MARK("B rows");
    // ---- rows of the four even corners (pair p = y + 2 z holds corners 2p, 2p + 1)
    uint32_t r0[NP];
    uint32_t xm = 0;       // hashed: r1 = r0 ^ xm
    bool single[NP];       // the pair travels as two singles
    uint32_t codesh;       // hashed: code << 13 of all four pairs
    if constexpr (MODE == 1) {
        const uint32_t m = lv.hashmap_size - 1u;
        const uint32_t ty0 = c1 * prime_of(1), ty1 = ty0 + prime_of(1), tz0 = c2 * prime_of(2), tz1 = tz0 + prime_of(2);
        r0[0] = ((ty0 ^ tz0) ^ c0) & m;
        r0[1] = ((ty1 ^ tz0) ^ c0) & m;
        r0[2] = ((ty0 ^ tz1) ^ c0) & m;
        r0[3] = ((ty1 ^ tz1) ^ c0) & m;
        xm = (c0 ^ (c0 + 1u)) & m;  // 2^(t+1) - 1, t = trailing ones of x
        const uint32_t t_hash = (uint32_t)__builtin_popcount(xm) - 1u;
        const bool sg = t_hash >= kCodeSingle;
#pragma unroll
        for (int p = 0; p < NP; p++) single[p] = sg;
        codesh = (sg ? kCodeSingle : t_hash) << kBucketRowsLog2;
    } else {
        const uint32_t R = MODE == 3 ? lv.resolution : lv.resolution + 1u, RR = R * R;
        const uint32_t base = c0 + c1 * R + c2 * RR;
        r0[0] = base;
        r0[1] = base + R;
        r0[2] = base + RR;
        r0[3] = base + R + RR;
        if constexpr (MODE == 3) {  // idx <= res + res^2 + res^3 < 2 * rows: one compare-and-subtract is the modulo
#pragma unroll
            for (int p = 0; p < NP; p++) r0[p] = r0[p] >= lv.hashmap_size ? r0[p] - lv.hashmap_size : r0[p];
        }
#pragma unroll
        for (int p = 0; p < NP; p++)  // r0 + 1 opens the next 128-row group, i.e. another bucket (bucket_of_row)
            single[p] = (r0[p] & ((1u << kGroupRowsLog2) - 1)) == (1u << kGroupRowsLog2) - 1;
        if constexpr (MODE == 3) {  // the straddling pair: its second row wraps to row 0
#pragma unroll
            for (int p = 0; p < NP; p++) single[p] |= r0[p] == lv.hashmap_size - 1u;
        }
        codesh = 0;
    }
    LNH_MARK("C masks");
    // ---- run-merge masks (SGPR pairs).  A lane CONTINUES the run of its lower neighbour when both are ok and lie in the
    //      same cell; hashed levels cut runs at 16-lane row starts (row-local scan), dense levels scan the whole wave.
    const bool same = ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)c0, 0x138, 0xf, 0xf, false) == c0) &
                      ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)c1, 0x138, 0xf, 0xf, false) == c1) &
                      ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)c2, 0x138, 0xf, 0xf, false) == c2);
    // members of runs: every in-range sample with a non-zero gradient, and a zero-gradient one within THREE LANES of such a
    // sample — the bridge inside a run (zero stretches of up to six samples are bridged from both ends); the long zero
    // stretches behind a surface, and whole waves of them, stay out of the masks, the scan and the pool as they always did.
    // Measured on fixed patterns (profiles/r05_reduce_drift.txt; backward = scatter + reduce, us): zeros sprinkled over 30 /
    // 50 / 70 % of the samples — dropped outright 1478 / - / 1696, every sample a member 791 / 712 / 633, this rule 786 / 708 /
    // 638; the far 50 / 85 % of every ray zero — 622 / 421, 692 / 570, 619 / 430.
    const unsigned long long in_m = __builtin_amdgcn_ballot_w64(ok);
    const unsigned long long nz_m = __builtin_amdgcn_ballot_w64(nonzero) & in_m;
    const unsigned long long nz1_m = nz_m | (nz_m << 1) | (nz_m >> 1);
    const unsigned long long ok_m = in_m & (nz1_m | (nz1_m << 2) | (nz1_m >> 2));
    constexpr unsigned long long kRowStarts = MODE == 1 ? 0x0001000100010001ull : 1ull;
    unsigned long long cont = __builtin_amdgcn_ballot_w64(same) & ok_m & (ok_m << 1) & ~kRowStarts;
    constexpr int kMinMerges = 8;  // a wave with fewer mergeable lanes skips the scan (4 / 16 / 24 measured within noise)
    if (__builtin_popcountll(cont) < kMinMerges) cont = 0ull;
    // run tails; a zero-gradient sample that continues nobody's run (a run of one) emits nothing
    const unsigned long long emit_m = ok_m & ~(cont >> 1) & (nz_m | cont);
    const bool emit = __builtin_amdgcn_inverse_ballot_w64(emit_m);
    LNH_MARK("F rank");
    // ---- rank inside the workgroup's (bucket) counters
    uint32_t bk4[NP], rank[NP], rank_x[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        // bucket * 4 = LDS byte offset of its counter (hashed: 8192 consecutive rows; dense: 128-row groups dealt to 64)
        bk4[p] = (r0[p] >> ((MODE == 1 ? kBucketRowsLog2 : kGroupRowsLog2) - 2)) & 0xfcu;
        rank[p] = 0;
        rank_x[p] = 0;
    }
    bool any_single = false;
#pragma unroll
    for (int p = 0; p < NP; p++) any_single |= single[p];
    const bool wave_singles = __builtin_amdgcn_ballot_w64(emit && any_single) != 0ull;  // wave-uniform, rare
    // The returning LDS atomics are issued BEFORE the value arithmetic: the LDS atomic unit retires ~3 lanes per clock and
    // CU (29 cycles per wave instruction here), the two resident workgroups of a CU run phase-locked, so nobody else hides
    // that time — the wave's own ~100 VALU instructions of weights / products / scan do (profiles/r04_scatter_phases.txt).
    // per-lane returning atomics.  (Dense levels: a wave emits a few run tails, and with the rows dealt to 64 buckets in
    // 128-row groups their four pairs go to four buckets — the wave-aggregated rank of round 3, one atomic for a whole
    // wave on the level's single bucket, has nothing left to aggregate and cost ~50 VALU instructions per wave.)
    if (emit) {
#pragma unroll
        for (int p = 0; p < NP; p++) rank[p] = atomicAdd(&lds_at(lcnt, bk4[p]), 1u);
    }
    if (wave_singles) {  // the second corners of pairs that travel as two singles
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const uint32_t r1 = MODE == 1 ? (r0[p] ^ xm) : x_next(r0[p]);
            if (emit && single[p]) rank_x[p] = atomicAdd(&lcnt[bucket_of_row(r1, DENSE)], 1u);
        }
    }
    LNH_MARK("D values");
    // ---- w * (g0, g1) per corner: float product, then the per-contribution rounding to the table type (gridencoder.cu:350).
    //      (Summing the fp32 PRODUCTS of a merged run and rounding once — 24 conversions less per scanning lane — was built
    //      in round 4 and dropped: 844 us against 838 for the backward, i.e. nothing, and rows whose every addend underflows
    //      in fp16 then hold a tiny sum where the reference and the oracle hold 0.)
    V2 val[8];
    {
        const float wx0 = 1.0f - fr0, wy0 = 1.0f - fr1, wz0 = 1.0f - fr2;
        const float wxy[4] = {wx0 * wy0, fr0 * wy0, wx0 * fr1, fr0 * fr1};
        const f32x2_t gg = {g0, g1};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float w = wxy[c & 3] * ((c & 4) ? fr2 : wz0);
            const f32x2_t p = gg * w;
            val[c] = __builtin_convertvector(p, V2);
        }
    }
    LNH_MARK("E scan");
    if (cont != 0ull) {  // wave-uniform: sum the runs in fp32 (one rounding of the sum when it is stored again)
        // take masks of the scan steps: step s adds the value 2^s lanes below iff the lanes (lane - 2^s, lane] all continue
        const unsigned long long k0 = cont, k1 = k0 & (k0 << 1), k2 = k1 & (k1 << 2), k3 = k2 & (k2 << 4);
        float vv[16];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            vv[2 * c] = (float)val[c][0];
            vv[2 * c + 1] = (float)val[c][1];
        }
        {
            const float m0 = __builtin_amdgcn_inverse_ballot_w64(k0) ? 1.0f : 0.0f;
            segscan_step_n<0>(vv, m0);
        }
        if (k1 != 0ull) {  // a run of 3 or more somewhere in the wave
            const float m1 = __builtin_amdgcn_inverse_ballot_w64(k1) ? 1.0f : 0.0f;
            segscan_step_n<1>(vv, m1);
            if (k2 != 0ull) {
                const float m2 = __builtin_amdgcn_inverse_ballot_w64(k2) ? 1.0f : 0.0f;
                segscan_step_n<2>(vv, m2);
                if (k3 != 0ull) {
                    const float m3 = __builtin_amdgcn_inverse_ballot_w64(k3) ? 1.0f : 0.0f;
                    segscan_step_n<3>(vv, m3);
                }
            }
        }
        if constexpr (DENSE) {
            // cross-row steps: lanes of rows 1, 3 (then 2, 3) whose run began before their row (before lane 32) take the
            // sum the last lane of the preceding row (lane 31) holds.  pre = lanes whose whole row prefix continues.
            unsigned long long pre = cont;
            pre &= (pre << 1) | 0x0001000100010001ull;
            pre &= (pre << 2) | 0x0003000300030003ull;
            pre &= (pre << 4) | 0x000f000f000f000full;
            pre &= (pre << 8) | 0x00ff00ff00ff00ffull;
            const unsigned long long k4 = pre & 0xffff0000ffff0000ull;
            const unsigned long long k5 = (pre & 0x0000ffff00000000ull) | (((pre >> 47) & 1ull) ? (pre & 0xffff000000000000ull) : 0ull);
            if (k4 != 0ull) {
                const float m4 = __builtin_amdgcn_inverse_ballot_w64(k4) ? 1.0f : 0.0f;
                segscan_step_n<4>(vv, m4);
            }
            if (k5 != 0ull) {  // (not nested: a run may cross the lane 31 | 32 boundary only)
                const float m5 = __builtin_amdgcn_inverse_ballot_w64(k5) ? 1.0f : 0.0f;
                segscan_step_n<5>(vv, m5);
            }
        }
#pragma unroll
        for (int c = 0; c < 8; c++) val[c] = make_v2<T>(vv[2 * c], vv[2 * c + 1]);
    }
    __syncthreads();
    LNH_MARK("G reserve");
    // ---- global reservation, in two halves around the staging pass: the first wave ISSUES one returning global atomic per
    //      touched bucket and publishes the workgroup-local exclusive scan of the counts (all the staging needs); the
    //      atomics' round trip (~66 us of the pass when it was waited for here) runs under the staging of all 16 waves, and
    //      the first wave turns the returned bases into pool / spill offsets only afterwards.
    uint32_t rs_n0 = 0, rs_base = 0, rs_st = 0, rs_incl = 0;
    bool pad_unstaged = false;  // (paired write-out) this lane's padding entry lies beyond the staging area
    if (tid < 64) {
        static_assert(kMaxBucketsPerLevel == 64, "one bucket counter per lane of the first wave");
        const uint32_t cnt = lcnt[lane];
        rs_n0 = (cnt + 1u) & ~1u;  // slots reserved: even
        if (lane < nb && rs_n0) rs_base = atomicAdd(&cursor[fb + lane], rs_n0);
        rs_incl = wave_scan_add_u32(rs_n0);  // DPP network: no LDS round trips while the atomics are in flight
        rs_st = rs_incl - rs_n0;
        lstart[lane] = rs_st;
        if (lane == 63) lstart[kMaxBucketsPerLevel] = rs_incl;
        if (cnt & 1u) {  // the padding entry: a single with zero values on the bucket's local row 0
            const uint32_t q = rs_st + cnt;
            if (q < (uint32_t)CAP) {
                skey[q] = (kCodeSingle << kBucketRowsLog2) | (lane << 18);
                sa[q] = make_v2<T>(0.0f, 0.0f);
                sb[q] = make_v2<T>(0.0f, 0.0f);
            } else {
                pad_unstaged = true;
            }
        }
    }
    __syncthreads();
    LNH_MARK("H stage");
    // pool streams of this level: values [slot][2] | rows [slot] | spill list; byte offsets inside a level fit 32 bits
    // (<= 4 M points per launch), so every store is base (scalar) + 32-bit lane offset
    char *pvals = pool_bytes + plan.pool_off[level];
    char *prows = pool_bytes + plan.rows_off[level];
    const uint32_t total_all = (uint32_t)__builtin_amdgcn_readfirstlane((int)lstart[kMaxBucketsPerLevel]);
    const uint32_t total = min(total_all, (uint32_t)CAP);
    const bool all_staged = total_all <= (uint32_t)CAP;  // workgroup-uniform; false only for adversarial inputs
    auto key_of = [&](uint32_t r, uint32_t csh) {  // staged key of level-local row r, code << 13
        return local_of_row(r, DENSE) | csh | (bucket_of_row(r, DENSE) << 18);
    };
    static_assert(CAP % 2 == 0, "staging slots are written out in pairs");
    // ---- stage in bucket order.  Needs the workgroup-local scan only.  An entry whose position lies beyond the staging
    //      area (more than CAP entries in the workgroup: every x coordinate = 127 mod 128, ...) stays in its thread's
    //      registers and is written to its global slot by that thread after the bases have arrived.
    uint32_t pos[NP], pos_x[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) pos[p] = pos_x[p] = 0;
    auto stage = [&](auto checked_c) {  // (unswitched by hand: the usual, unchecked copy has no per-entry test)
        constexpr bool CHECKED = decltype(checked_c)::value;
        if (emit) {
#pragma unroll
            for (int p = 0; p < NP; p++) pos[p] = lds_at(lstart, bk4[p]);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                pos[p] += rank[p];
                const uint32_t csh = MODE == 1 ? codesh : (single[p] ? kCodeSingle << kBucketRowsLog2 : 0u);
                if (!CHECKED || pos[p] < (uint32_t)CAP) {
                    skey[pos[p]] = local_of_row(r0[p], DENSE) | (csh | (bk4[p] << 16));
                    sa[pos[p]] = val[2 * p];
                    sb[pos[p]] = val[2 * p + 1];
                }
            }
        }
        if (wave_singles && emit) {  // the second corners of pairs that travel as two singles
#pragma unroll
            for (int p = 0; p < NP; p++)
                if (single[p]) {
                    const uint32_t r1 = MODE == 1 ? (r0[p] ^ xm) : x_next(r0[p]);
                    pos_x[p] = lstart[bucket_of_row(r1, DENSE)] + rank_x[p];
                    if (!CHECKED || pos_x[p] < (uint32_t)CAP) {
                        skey[pos_x[p]] = key_of(r1, kCodeSingle << kBucketRowsLog2);
                        sa[pos_x[p]] = val[2 * p + 1];
                        sb[pos_x[p]] = make_v2<T>(0.0f, 0.0f);
                    }
                }
        }
    };
    if (all_staged) stage(std::false_type{});
    else stage(std::true_type{});
    // ---- second half of the reservation (first wave): staging slot pos of bucket bk goes to pool slot bk * cap + base +
    //      (pos - st) while base + (pos - st) < cap; the `over` entries behind those go to consecutive slots of the level's
    //      spill list, reserved with ONE atomic per workgroup (and none at all in the usual case of no overflow)
    if (tid < 64) {
        const uint32_t fit = rs_base < cap ? min(cap - rs_base, rs_n0) : 0u, over = rs_n0 - fit;
        const uint32_t oincl = wave_scan_add_u32(over);
        uint32_t sp0 = 0;
        if (lane == 63 && oincl) sp0 = atomicAdd(&spill_cursor[level], oincl);
        sp0 = (uint32_t)__builtin_amdgcn_readlane((int)sp0, 63);
        lox[lane] = lane * cap + rs_base - rs_st;
        lofit[lane] = rs_st + fit;
        lsp[lane] = sp0 + (oincl - over) - (rs_st + fit);
        if (lane == 63) lflag = oincl == 0u ? 1u : 0u;  // 1: every entry of the workgroup has a pool slot
    }
    __syncthreads();
    LNH_MARK("I writeout");
    const bool fits = __builtin_amdgcn_readfirstlane((int)lflag) != 0;
    if (fits) {
        // ---- write out in PAIRS of slots (see "Paired write-out" above): slot pair (2j, 2j + 1) of the staging area belongs
        //      to one bucket and goes to an even pool slot; all LDS reads of a thread before the first use
        constexpr int NW2 = (CAP + 2 * NTHREADS - 1) / (2 * NTHREADS);
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        struct V2x2 { V2 v[2]; };
        u32x2 ks2[NW2];
        V2x2 as2[NW2], bs2[NW2];
        uint32_t dl2[NW2];
#pragma unroll
        for (int i = 0; i < NW2; i++) {
            if ((uint32_t)i * 2 * NTHREADS >= total) break;  // scalar branch
            const uint32_t q = 2 * (tid + (uint32_t)i * NTHREADS);
            const uint32_t qc = q < (uint32_t)CAP ? q : 0u;  // (CAP is a multiple of 2: a pair never straddles the end)
            ks2[i] = *reinterpret_cast<const u32x2 *>(&skey[qc]);
            as2[i] = *reinterpret_cast<const V2x2 *>(&sa[qc]);
            bs2[i] = *reinterpret_cast<const V2x2 *>(&sb[qc]);
        }
#pragma unroll
        for (int i = 0; i < NW2; i++) {
            if ((uint32_t)i * 2 * NTHREADS >= total) break;
            dl2[i] = lds_at(lox, (ks2[i][0] >> 16) & 0xffu);
        }
#pragma unroll
        for (int i = 0; i < NW2; i++) {
            if ((uint32_t)i * 2 * NTHREADS >= total) break;
            const uint32_t q = 2 * (tid + (uint32_t)i * NTHREADS);
            if (q < total) {  // (total is even: the pair is whole)
                const uint32_t slot = dl2[i] + q;
                struct Pair2 { V2 a0, b0, a1, b1; };
                Pair2 pr = {as2[i].v[0], bs2[i].v[0], as2[i].v[1], bs2[i].v[1]};
                *reinterpret_cast<Pair2 *>(pvals + slot * (uint32_t)sizeof(Pair)) = pr;
                *reinterpret_cast<uint32_t *>(prows + slot * 2u) = (ks2[i][0] & 0xffffu) | (ks2[i][1] << 16);
            }
        }
        if (all_staged) return;
    }
    LNH_MARK("J general");
    // ---- the general path: a bucket beyond its pool share (spill list, then atomics), entries beyond the staging area
    char *spill = pool_bytes + plan.spill_off[level];
    auto to_global = [&](uint32_t q, uint32_t k, V2 a, V2 b2) {
        const uint32_t bo = k >> 16;  // bucket * 4
        if (q < lds_at(lofit, bo)) {
            const uint32_t slot = lds_at(lox, bo) + q;
            Pair pr = {a, b2};
            *reinterpret_cast<Pair *>(pvals + slot * (uint32_t)sizeof(Pair)) = pr;
            *reinterpret_cast<unsigned short *>(prows + slot * 2u) = (unsigned short)k;
        } else {
            const uint32_t sp = lds_at(lsp, bo) + q;
            const uint32_t rr = row_of_local(k & (kBucketRows - 1), k >> 18, DENSE), cd = (k >> kBucketRowsLog2) & 7u;
            if (sp < plan.spill_cap) {
                SpillEntry<T> e = {rr | (cd << 29), a, b2};
                *reinterpret_cast<SpillEntry<T> *>(spill + sp * (uint32_t)sizeof(SpillEntry<T>)) = e;
            } else {
                // The spill list is full too (it holds 1/16 of a level's worst case): these entries go straight into the
                // table with device atomics — always correct, slow, and the one place where a sum depends on arrival order.
                T *gt = grad_table + (size_t)lv.offset * 2;
                atomic_add_pair(gt + (size_t)rr * 2, (float)a[0], (float)a[1]);
                if (cd != kCodeSingle)
                    atomic_add_pair(gt + (size_t)pair_row(rr, cd, MODE == 1) * 2, (float)b2[0], (float)b2[1]);
            }
        }
    };
    if (!fits)
        for (uint32_t q = tid; q < total; q += NTHREADS) to_global(q, skey[q], sa[q], sb[q]);
    if (pad_unstaged)  // (first wave: the padding entry of a bucket whose segment ends beyond the staging area)
        to_global(rs_st + rs_n0 - 1u, (kCodeSingle << kBucketRowsLog2) | (lane << 18), make_v2<T>(0.0f, 0.0f),
                  make_v2<T>(0.0f, 0.0f));
    if (!all_staged) {
        if (emit) {
#pragma unroll
            for (int p = 0; p < NP; p++)
                if (pos[p] >= (uint32_t)CAP)
                    to_global(pos[p], key_of(r0[p], MODE == 1 ? codesh : (single[p] ? kCodeSingle << kBucketRowsLog2 : 0u)),
                              val[2 * p], val[2 * p + 1]);
        }
        if (wave_singles && emit) {
#pragma unroll
            for (int p = 0; p < NP; p++)
                if (single[p] && pos_x[p] >= (uint32_t)CAP)
                    to_global(pos_x[p], key_of(MODE == 1 ? (r0[p] ^ xm) : x_next(r0[p]), kCodeSingle << kBucketRowsLog2),
                              val[2 * p + 1], make_v2<T>(0.0f, 0.0f));
        }
    }
    };
#ifdef LNH_ONLY_MODE  // tools/isa_sections.py: one body per census
    body(std::integral_constant<int, LNH_ONLY_MODE>{});
#else
    if (cls_hash) body(std::integral_constant<int, 1>{});
    else if (lv.flags & LV_WRAP1) body(std::integral_constant<int, 3>{});
    else body(std::integral_constant<int, 2>{});
#endif
}

}  // namespace

void grid_bwd_scatter_launch(int dtype, const void *grad, const float *inputs, void *grad_table, uint32_t B,
                             const GridMeta &m, const BucketPlan &plan, char *pool, uint32_t *cursor, uint32_t *spill_cursor,
                             uint32_t align, uint32_t interp, uint32_t level_begin, uint32_t level_end, uint32_t b_begin,
                             uint32_t B_all, hipStream_t s) {
    // 1024 threads x 1 point: the per-workgroup cost that matters is the one returning device atomic per touched
    // bucket (measured: 256- and 512-thread workgroups are 2.3x / 1.5x slower); 5 staged pair entries per thread keep
    // the LDS staging at 60 KiB (two workgroups per CU).  The generic kernel (8 singles per point) stages 6 per thread.
    const uint32_t n_win = level_end - level_begin;
    const bool plain = align == 0 && interp == 0;
    bool generic = false, any_plain = false;
    for (uint32_t l = level_begin; l < level_end; l++) {
        const bool g = level_is_generic(m.lv[l], 3, plain);
        generic |= g;
        any_plain |= !g;
    }
    (void)with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        // the plain classes' levels and the generic ones are served by their own kernel (a workgroup of the other kernel's
        // level exits at once); the usual configuration has plain levels only
        if (any_plain)
            LNH_LAUNCH((k_grid_bwd_scatter_plain<T, kScatterThreads, 5 * kScatterThreads>), dim3(n_win, div_up(B, kScatterThreads)),
                       dim3(kScatterThreads), 0, s, (const T *)grad, inputs, B, m, plan, pool, cursor, spill_cursor, level_begin,
                       b_begin, B_all, (T *)grad_table);
        if (generic)
            LNH_LAUNCH((k_grid_bwd_scatter<T, 3, 6144>), dim3(div_up(B, 1024) * n_win), dim3(1024), 0, s, (const T *)grad, inputs,
                       B, m, plan, pool, cursor, spill_cursor, align, interp, n_win, level_begin, b_begin, B_all, (T *)grad_table);
        return LNH_OK;
    });
}
