// grid_forward.hip — encode forward of the grid encoder for gfx950 (MI355X), and the corner-index debug kernel.
//
// Organised for CDNA4 (level geometry: grid_geom.h):
//   * one launch whose workgroup ids run through the levels one after the other (FwdSched), so the chip works
//     level-major and every XCD's 4 MiB L2 holds the ~2 MiB fp16 table of the level in flight; the finest hashed levels
//     each share their turn with one small coarse level;
//   * 64 consecutive lanes = 64 consecutive sample points (consecutive samples along a LiDAR ray): coarse-level
//     corner gathers of a wave hit a few cache lines; the [L,B,C] output store is a fully coalesced 256 B / wave.
#include "grid_geom.h"

namespace {

struct RowMap {
    uint32_t T_cur, T_tot, slot_off, B_all;
    uint32_t kind;  // how b0 / T_cur is taken (make_row_map): ROW_DIV per lane, ROW_UNIFORM on the scalar unit, ROW_SHIFT
    uint32_t aux;   // ROW_UNIFORM: floor(2^32 / T_cur); ROW_SHIFT: log2(T_cur)
};
enum { ROW_DIV = 0, ROW_UNIFORM = 1, ROW_SHIFT = 2 };
constexpr uint32_t kFwdThreads = 256;  // points (= threads) of a forward workgroup

// floor(2^32 / d) clamped to 32 bits: mul_hi(n, .) is n / d or one less for every 32-bit n (n / d - n * m / 2^32 < 1), so a
// workgroup-uniform quotient costs one scalar multiply-high and one compare — the scalar unit has no divide.
inline uint32_t recip32(uint32_t d) { return (uint32_t)std::min<uint64_t>((1ull << 32) / d, 0xffffffffull); }
__device__ __forceinline__ uint32_t div_recip(uint32_t n, uint32_t d, uint32_t recip, uint32_t &rem) {
    uint32_t q = (uint32_t)(((uint64_t)n * recip) >> 32);
    rem = n - q * d;
    if (rem >= d) {
        q++;
        rem -= d;
    }
    return q;
}

// Forward schedule: which (level, chunk) the workgroup with linear id w works on.  The ids are cut into slots of `chunks`
// workgroups; the first 2 * n_pairs slots are PAIRS (two slots each), the rest single levels in ascending order.  Inside a
// pair the two levels alternate in blocks of G = 2^g_log2 consecutive ids (a multiple of 8: consecutive workgroups are dealt
// round-robin to the 8 XCDs, so every XCD sees both levels), the `tail` chunks past the last whole block following as two
// runs.  A pair joins a level bound by distinct-line requests to L2 (fine hashed) with one that hardly loads L2 (dense or
// low hashed: it streams positions in and features out): run one after the other, each leaves the other's unit idle;
// side by side about 60 % of the coarse level's time disappears (profiles/forward_level_pairs.txt).  n_pairs = 0 is the
// level-major order of a (chunks, L) launch.
struct FwdSched {
    uint32_t chunks, chunks_recip;  // workgroups per level, recip32 of it
    uint32_t n_pairs, g_log2;
    uint32_t full_end, tail;     // ids of a pair below full_end alternate in whole blocks; tail = chunks % G
    uint32_t n_blocks;           // full_end / G
    uint32_t lv[LNH_MAX_LEVELS];  // slot -> level (slots 2p, 2p + 1: the levels of pair p)
};
struct FwdSlot {
    uint32_t level, chunk;
};
// scalar arithmetic only: w is workgroup-uniform
__device__ __forceinline__ FwdSlot fwd_slot(const FwdSched &s, uint32_t w) {
    // (selects, not branches: every field of the schedule is then fetched by the kernel's first scalar loads)
    uint32_t rem;
    const uint32_t q = div_recip(w, s.chunks, s.chunks_recip, rem);
    const uint32_t r = (q & 1u) * s.chunks + rem;  // id inside the pair, 0 .. 2 * chunks - 1
    const uint32_t blk = r >> s.g_log2;            // whole blocks: even ones to the first level, odd ones to the second
    const uint32_t chunk_b = ((blk >> 1) << s.g_log2) + (r & ((1u << s.g_log2) - 1u));
    const uint32_t rr = r - s.full_end;  // the tail: `tail` chunks of the first level, then of the second (rr < 2 * tail)
    const uint32_t first = q & ~1u, second = q | 1u, half = s.full_end >> 1;
    const bool whole = blk < s.n_blocks, pair = q < 2 * s.n_pairs, tail2 = rr >= s.tail;
    const uint32_t slot_b = (blk & 1u) ? second : first;
    const uint32_t slot_t = tail2 ? second : first, chunk_t = tail2 ? half + rr - s.tail : half + rr;
    return FwdSlot{s.lv[pair ? (whole ? slot_b : slot_t) : q], pair ? (whole ? chunk_b : chunk_t) : rem};
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int D, int C, bool DYDX>
__global__ void __launch_bounds__(kFwdThreads)
k_grid_forward(const float *__restrict__ inputs, const T *__restrict__ table, T *__restrict__ outputs,
               T *__restrict__ dy_dx, uint32_t B, uint32_t L, GridMeta meta, uint32_t align_rt, uint32_t interp_rt,
               RowMap map, FwdSched sched) {
    const FwdSlot slot = fwd_slot(sched, blockIdx.x);
    const uint32_t base = slot.chunk * kFwdThreads;  // workgroup-uniform
    const uint32_t b0 = base + threadIdx.x;
    if (b0 >= B) return;
    {  // (tools/probe_variants.py "fusion" turns this block into a loop over the levels: the encode -> MLP fusion probe)
    const uint32_t level = slot.level;
    const LevelParams lv_rt = meta.lv[level];
    // optional row map: launch index b0 = r*T_cur + j addresses row r*T_tot + slot_off + j of buffers holding
    // B_all rows (coarse and fine samples of a ray side by side); identity when T_cur == 0.  The division is per lane only
    // where it has to be: a workgroup inside one ray (T_cur a multiple of its threads) takes r on the scalar unit, a
    // power-of-two T_cur that divides the workgroup takes it with a shift.
    uint32_t b = b0;
    if (map.T_cur) {
#ifdef LNH_FWD_ONLY_MAP  // tools/isa_sections.py: one row-map path per census
        const uint32_t kind = LNH_FWD_ONLY_MAP;
#else
        const uint32_t kind = map.kind;
#endif
        if (kind == ROW_UNIFORM) {
            uint32_t j0;
            const uint32_t r = div_recip(base, map.T_cur, map.aux, j0);
            b = r * map.T_tot + map.slot_off + j0 + threadIdx.x;
        } else if (kind == ROW_SHIFT) {
            b = (b0 >> map.aux) * map.T_tot + map.slot_off + (b0 & (map.T_cur - 1u));
        } else {
            b = (b0 / map.T_cur) * map.T_tot + map.slot_off + b0 % map.T_cur;
        }
    }
    const uint32_t Bs = map.T_cur ? map.B_all : B;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = inputs[(size_t)b * D + d];
    const T *tab = table + (size_t)lv_rt.offset * C;
    T *out = outputs + ((size_t)level * Bs + b) * C;
    // The level class is workgroup-uniform.  The two classes that make up the usual configuration (hashed power-of-two
    // level / dense level indexed in all D dimensions, both with linear interpolation and align_corners = false) get
    // their own straight-line copy of the body with the flags as compile-time constants, and so does the dense level of
    // tiny-cuda-nn's lattice (MODE 3: stride res, one wrap); everything else takes the generic copy with run-time branches.
    auto body = [&](auto mode_c) {
    constexpr int MODE = decltype(mode_c)::value;
    LevelParams lv = lv_rt;
    if constexpr (MODE == 1) lv.flags = LV_HASH | LV_POW2;
    if constexpr (MODE == 2) lv.flags = LV_NOWRAP | (uint32_t)D;
    if constexpr (MODE == 3) lv.flags = LV_RSTRIDE | LV_WRAP1 | (uint32_t)D;
    const uint32_t align = MODE ? 0u : align_rt, interp = MODE ? 0u : interp_rt;
    Cell<D> cell;
    Vec<T, C> res;
#pragma unroll
    for (int ch = 0; ch < C; ch++) res.v[ch] = (T)0.0f;
    const bool ok = locate<D>(x, lv, align != 0, interp, cell);
    if (ok) {
        // issue all 2^D gathers before consuming any of them
        Vec<T, C> g[1 << D];
        if constexpr (D == 3 && C == 2) {
            // The x-neighbours of a cell edge lie close together in the table: rows r0, r0 + 1 when the x term is dense,
            // and r1 = r0 ^ (2^(t+1) - 1) on a hashed level (the x term of the hash is x itself; t = trailing ones of the
            // x coordinate).  Measured on MI355X (A/B builds over tools/bench_grid.py): a wave's gather costs per DISTINCT
            // line per INSTRUCTION — a second instruction touching the lines of the first still costs a third of a miss
            // (tag look-up), its width (4 / 8 / 16 bytes per lane) costs nothing — so each (y,z) corner pair is fetched
            // with one wide load wherever its two rows share an aligned block.
            const bool hash = lv.flags & LV_HASH;
            const bool x_dense = MODE == 3 || (!hash && (lv.flags & 15u) >= 1 && (lv.flags & LV_NOWRAP));
            const bool hash_pair = hash && (lv.flags & LV_POW2);   // level-uniform
            const bool x_odd = cell.term[0][0] & 1u;               // per lane
            // All loads first, every use after the loop, and no per-lane branch around a load: a consumer (or the end of
            // a divergent region) pins an s_waitcnt and serialises the four (y,z) iterations into dependent round trips.
            // Lanes that need no second load read row 0 instead (one broadcast line): selecting the address keeps the
            // load unconditional.
            //
            // Hashed level, 4-byte rows: the aligned block of FOUR rows (16 bytes) around r0 also holds r1 for t <= 1,
            // i.e. for 3 lanes in 4; the others fetch r1 on its own (540 -> 505 us per 3.41 M points against the 2-row
            // blocks below; without the second load at all: 445 us).
            if constexpr (sizeof(T) * C == 4) {
            if (hash_pair) {
                Vec<T, 8> blk[4];
                Vec<T, C> solo[4];
                uint32_t r0s[4], r1s[4];
                const uint32_t xm = cell.term[0][0] ^ cell.term[0][1];   // 2^(t+1) - 1 (before the table mask)
                const bool far = (xm & (lv.hashmap_size - 1)) > 3u;
#pragma unroll
                for (uint32_t yz = 0; yz < 4; yz++) {
                    const uint32_t c0 = yz << 1;
                    const uint32_t r0 = corner_row<D>(cell, lv, c0);
                    const uint32_t r1 = corner_row<D>(cell, lv, c0 | 1u);
                    r0s[yz] = r0;
                    r1s[yz] = r1;
                    blk[yz] = load_vec<T, 8>(tab + (size_t)(r0 & ~3u) * C);
                    solo[yz] = load_vec<T, C>(tab + (size_t)(far ? r1 : 0u) * C);  // (probe anchor: tools/probe_variants.py "gather")
                }
#pragma unroll
                for (uint32_t yz = 0; yz < 4; yz++) {
                    const uint32_t c0 = yz << 1, c1 = c0 | 1u;
                    uint32_t w[4], so;
                    __builtin_memcpy(w, &blk[yz], 16);
                    __builtin_memcpy(&so, &solo[yz], 4);
                    const uint32_t i0 = r0s[yz] & 3u, i1 = r1s[yz] & 3u;
                    const uint32_t a0 = (i0 & 2u) ? ((i0 & 1u) ? w[3] : w[2]) : ((i0 & 1u) ? w[1] : w[0]);
                    const uint32_t a1 = (i1 & 2u) ? ((i1 & 1u) ? w[3] : w[2]) : ((i1 & 1u) ? w[1] : w[0]);
                    const uint32_t b1 = far ? so : a1;
                    __builtin_memcpy(&g[c0], &a0, 4);
                    __builtin_memcpy(&g[c1], &b1, 4);
                }
            }
            }
            if (!(sizeof(T) * C == 4 && hash_pair)) {
            //   pair[yz]: the aligned row pair holding corner c0 (hashed levels) / rows r0, r0+1 (dense x)
            //   solo[yz]: corner c1 on its own, fetched only where it is not the sibling of c0 (hashed level, odd x)
            //   (MODE 3, tiny-cuda-nn lattice: r0 + 1 wraps to row 0 when r0 is the level's last row — the one straddling
            //   pair; its lanes read the pair block one row lower and take c1 from solo = row 0, which every lane reads)
            Vec<T, 4> pair[4];
            Vec<T, C> solo[4];
            uint32_t r0s[4];
#pragma unroll
            for (uint32_t yz = 0; yz < 4; yz++) {
                const uint32_t c0 = yz << 1, c1 = c0 | 1u;
                const uint32_t r0 = corner_row<D>(cell, lv, c0);
                r0s[yz] = r0;
                if constexpr (MODE == 3) {
                    const bool strad = r0 == lv.hashmap_size - 1u;
                    pair[yz] = load_vec<T, 4>(tab + (size_t)(strad ? r0 - 1u : r0) * C);
                    solo[yz] = load_vec<T, C>(tab);
                } else if (x_dense || hash_pair) {
                    pair[yz] = load_vec<T, 4>(tab + (size_t)(x_dense ? r0 : (r0 & ~1u)) * C);
                    // lanes whose c1 IS the sibling read row 0 instead (one broadcast line): selecting the address
                    // keeps the load unconditional — an exec-masked load would be waited for at the end of its branch
                    if (hash_pair)
                        solo[yz] = load_vec<T, C>(tab + (size_t)(x_odd ? corner_row<D>(cell, lv, c1) : 0u) * C);
                } else {
                    g[c0] = load_vec<T, C>(tab + (size_t)r0 * C);
                    g[c1] = load_vec<T, C>(tab + (size_t)corner_row<D>(cell, lv, c1) * C);
                }
            }
            if constexpr (MODE == 3) {
#pragma unroll
                for (uint32_t yz = 0; yz < 4; yz++) {
                    const uint32_t c0 = yz << 1, c1 = c0 | 1u;
                    const bool strad = r0s[yz] == lv.hashmap_size - 1u;
                    g[c0].v[0] = strad ? pair[yz].v[2] : pair[yz].v[0];
                    g[c0].v[1] = strad ? pair[yz].v[3] : pair[yz].v[1];
                    g[c1].v[0] = strad ? solo[yz].v[0] : pair[yz].v[2];
                    g[c1].v[1] = strad ? solo[yz].v[1] : pair[yz].v[3];
                }
            } else if (x_dense || hash_pair) {
#pragma unroll
                for (uint32_t yz = 0; yz < 4; yz++) {
                    const uint32_t c0 = yz << 1, c1 = c0 | 1u;
                    const bool swap = hash_pair && (r0s[yz] & 1u);  // hashed, r0 odd: its sibling r0 ^ 1 is the lower row
                    const bool own = hash_pair && x_odd;
                    g[c0].v[0] = swap ? pair[yz].v[2] : pair[yz].v[0];
                    g[c0].v[1] = swap ? pair[yz].v[3] : pair[yz].v[1];
                    g[c1].v[0] = own ? solo[yz].v[0] : (swap ? pair[yz].v[0] : pair[yz].v[2]);
                    g[c1].v[1] = own ? solo[yz].v[1] : (swap ? pair[yz].v[1] : pair[yz].v[3]);
                }
            }
            }
        } else {
#pragma unroll
            for (uint32_t c = 0; c < (1u << D); c++)
                g[c] = load_vec<T, C>(tab + (size_t)corner_row<D>(cell, lv, c) * C);
        }
#pragma unroll
        for (uint32_t c = 0; c < (1u << D); c++) {
            const float w = corner_weight<D>(cell, c);
            // accumulate in the table type, one rounding per corner (gridencoder.cu:173,198)
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                float acc = fmaf(w, (float)g[c].v[ch], (float)res.v[ch]);
                // keep the fp32 rounding of the fma visible: without this hipcc fuses fma+narrowing into
                // v_fma_mixlo_f16 (ONE rounding), while the reference rounds to fp32 and then to fp16
                if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(acc));
                res.v[ch] = (T)acc;
            }
        }
    }
    store_vec<T, C>(out, res);
    if constexpr (DYDX) {
        // gridencoder.cu:214-262: d out / d x for every input dimension, layout [B, L, D, C]
        T *dd = dy_dx + (((size_t)b * L + level) * D) * C;
#pragma unroll
        for (int gd = 0; gd < D; gd++) {
            Vec<T, C> rg;
#pragma unroll
            for (int ch = 0; ch < C; ch++) rg.v[ch] = (T)0.0f;
            if (ok) {
#pragma unroll
                for (uint32_t k = 0; k < (1u << (D - 1)); k++) {
                    float w = lv.scale;
                    uint32_t corner = 0;
#pragma unroll
                    for (int nd = 0; nd < D - 1; nd++) {
                        const int d = (nd >= gd) ? nd + 1 : nd;
                        if ((k >> nd) & 1) {
                            w *= cell.frac[d];
                            corner |= 1u << d;
                        } else {
                            w *= 1.0f - cell.frac[d];
                        }
                    }
                    Vec<T, C> gl = load_vec<T, C>(tab + (size_t)corner_row<D>(cell, lv, corner) * C);
                    Vec<T, C> gr = load_vec<T, C>(tab + (size_t)corner_row<D>(cell, lv, corner | (1u << gd)) * C);
#pragma unroll
                    for (int ch = 0; ch < C; ch++) {
                        T diff = (T)(gr.v[ch] - gl.v[ch]);
                        rg.v[ch] = (T)((float)rg.v[ch] + w * (float)diff * cell.deriv[gd]);
                    }
                }
            }
            store_vec<T, C>(dd + gd * C, rg);
        }
    }
    };
    const bool plain = align_rt == 0 && interp_rt == 0;
#ifdef LNH_FWD_ONLY_MODE  // tools/isa_sections.py: one class per census
    (void)plain;
    body(std::integral_constant<int, LNH_FWD_ONLY_MODE>{});
#else
    if (plain && (lv_rt.flags & (LV_HASH | LV_POW2)) == (LV_HASH | LV_POW2)) body(std::integral_constant<int, 1>{});
    else if (plain && !(lv_rt.flags & LV_HASH) && (lv_rt.flags & LV_NOWRAP) && (lv_rt.flags & 15u) == (uint32_t)D)
        body(std::integral_constant<int, 2>{});
    else if (plain && !(lv_rt.flags & LV_HASH) && (lv_rt.flags & LV_WRAP1) && (lv_rt.flags & 15u) == (uint32_t)D)
        body(std::integral_constant<int, 3>{});
    else body(std::integral_constant<int, 0>{});
#endif
    }  // level
}

// Debug kernel for the bit-exact index contract.
template <int D>
__global__ void __launch_bounds__(256)
k_grid_indices(const float *__restrict__ inputs, uint32_t *__restrict__ out, uint32_t B, uint32_t C, GridMeta meta,
               uint32_t align) {
    const uint32_t level = blockIdx.y;
    const LevelParams lv = meta.lv[level];
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = inputs[(size_t)b * D + d];
    Cell<D> cell;
    const bool ok = locate<D>(x, lv, align != 0, 0, cell);
    uint32_t *o = out + ((size_t)level * B + b) * (1u << D);
#pragma unroll
    for (uint32_t c = 0; c < (1u << D); c++) o[c] = ok ? corner_row<D>(cell, lv, c) * C : 0xffffffffu;
}

RowMap make_row_map(uint32_t T_cur, uint32_t T_tot, uint32_t slot_off, uint32_t B_all) {
    RowMap map{T_cur, T_tot, slot_off, B_all, ROW_DIV, 0};
    if (T_cur && T_cur % kFwdThreads == 0) {
        map.kind = ROW_UNIFORM;
        map.aux = recip32(T_cur);
    } else if (T_cur && (T_cur & (T_cur - 1)) == 0) {
        map.kind = ROW_SHIFT;
        while ((1u << map.aux) < T_cur) map.aux++;
    }
    return map;
}

// Forward schedule knobs, process-wide (lnh_grid_forward_set_schedule; first read from LNH_FWD_SCHEDULE = "pairs[,block]").
// The defaults are what profiles/forward_level_pairs.txt measured on MI355X: blocks of 32 workgroups (8: slower than
// level-major order, 128: the same), and by default (kFwdAuto) a pair forms only where the fine level's resolution is at
// least kFwdMinRatio times its partner's — pairs at ratios 2048 .. 35 each take 7 to 10 us off 3.41 M points, the pair at
// ratio 13 nothing, those at 4.6 and 2.1 (two levels of the same kind) ADD 4 and 2 us.
constexpr uint32_t kFwdAuto = 0xffffffffu, kFwdBlockDefault = 32, kFwdMinRatio = 32;
uint32_t g_fwd_pairs = kFwdAuto, g_fwd_block_log2 = 5;
bool g_fwd_env_read = false;

void set_fwd_schedule(uint32_t max_pairs, uint32_t block) {
    if (block == 0) block = kFwdBlockDefault;
    uint32_t lg = 3;  // G: a power of two, 8 .. 1024
    while (lg < 10 && (1u << lg) < block) lg++;
    g_fwd_pairs = max_pairs;
    g_fwd_block_log2 = lg;
    g_fwd_env_read = true;
}

// 1 hashed power-of-two level, 2 / 3 dense level (reference / tiny-cuda-nn lattice), 0 generic: k_grid_forward's classes
int fwd_level_class(const LevelParams &p, uint32_t D, bool plain) {
    if (!plain) return 0;
    if ((p.flags & (LV_HASH | LV_POW2)) == (LV_HASH | LV_POW2)) return 1;
    if (!(p.flags & LV_HASH) && (p.flags & 15u) == D) return (p.flags & LV_NOWRAP) ? 2 : (p.flags & LV_WRAP1) ? 3 : 0;
    return 0;
}

// Pairs: the finest hashed level with the coarsest level, the next finest with the next coarsest, ... — at most g_fwd_pairs
// of them (kFwdAuto: as many as pass the resolution ratio), as long as the fine one is of the plain hashed class and
// neither is of the generic class.  Everything else runs alone in ascending order; no pair at all = level-major order.
FwdSched build_fwd_schedule(const GridMeta &m, uint32_t B, uint32_t D, uint32_t L, bool plain) {
    if (!g_fwd_env_read) {
        g_fwd_env_read = true;
        if (const char *e = getenv("LNH_FWD_SCHEDULE")) {
            unsigned pairs = 0, block = 0;
            if (sscanf(e, "%u,%u", &pairs, &block) >= 1) set_fwd_schedule(pairs, block);
        }
    }
    FwdSched s{};
    s.chunks = div_up(B, kFwdThreads);
    s.chunks_recip = recip32(s.chunks);
    s.g_log2 = g_fwd_block_log2;
    s.tail = s.chunks & ((1u << s.g_log2) - 1u);
    s.full_end = 2u * (s.chunks - s.tail);
    s.n_blocks = s.full_end >> s.g_log2;
    bool paired[LNH_MAX_LEVELS] = {};
    uint32_t n = 0;
    if (L >= 2) {
        for (uint32_t lo = 0, hi = L - 1; lo < hi && s.n_pairs < g_fwd_pairs; lo++, hi--) {
            if (fwd_level_class(m.lv[hi], D, plain) != 1 || fwd_level_class(m.lv[lo], D, plain) == 0) break;
            if (g_fwd_pairs == kFwdAuto && m.lv[hi].resolution < (uint64_t)kFwdMinRatio * m.lv[lo].resolution) break;
            s.lv[n++] = hi;
            s.lv[n++] = lo;
            paired[hi] = paired[lo] = true;
            s.n_pairs++;
        }
    }
    for (uint32_t l = 0; l < L; l++)
        if (!paired[l]) s.lv[n++] = l;
    return s;
}

template <typename T, int D>
int launch_forward_c(const float *inputs, const T *emb, T *out, T *dy_dx, uint32_t B, uint32_t C, uint32_t L,
                     const GridMeta &m, uint32_t align, uint32_t interp, hipStream_t s, RowMap map = make_row_map(0, 0, 0, 0)) {
    const FwdSched sched = build_fwd_schedule(m, B, D, L, align == 0 && interp == 0);
    dim3 grid(sched.chunks * /* levels */ L), block(kFwdThreads);
    const int rc = with_channels(C, [&](auto c) {
        constexpr int CC = decltype(c)::value;
        if (dy_dx)
            LNH_LAUNCH((k_grid_forward<T, D, CC, true>), grid, block, 0, s, inputs, emb, out, dy_dx, B, L, m, align, interp, map,
                       sched);
        else
            LNH_LAUNCH((k_grid_forward<T, D, CC, false>), grid, block, 0, s, inputs, emb, out, dy_dx, B, L, m, align, interp, map,
                       sched);
        return LNH_OK;
    });
    return rc ? rc : lnh_check_launch("lnh_grid_encode_forward");
}

}  // namespace

extern "C" {

int lnh_grid_encode_forward(const float *inputs, const void *embeddings, const int32_t *offsets_host, void *outputs,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void *dy_dx,
                            uint32_t gridtype, int align_corners, uint32_t interp, int dtype, lnh_stream_t stream) {
    int rc = check_common(inputs, offsets_host, B, D, C, L, dtype);
    if (rc) return rc;
    LNH_REQUIRE(embeddings && outputs, LNH_ERR_INVALID_ARG, "grid forward: null embeddings/outputs");
    if (B == 0) return LNH_OK;
    GridMeta m;
    if ((rc = resolve_levels(m, offsets_host, D, L, S, H, gridtype, align_corners))) return rc;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_dim(D, [&](auto d) {
            return launch_forward_c<T, decltype(d)::value>(inputs, (const T *)embeddings, (T *)outputs, (T *)dy_dx, B, C, L, m,
                                                           align_corners != 0, interp, (hipStream_t)stream);
        });
    });
}

int lnh_grid_encode_forward_mapped_ex(const float *inputs_all, const void *embeddings, const int32_t *offsets_host,
                                      void *outputs_all, uint32_t B, uint32_t T_cur, uint32_t T_tot, uint32_t slot_off,
                                      uint32_t B_all, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                      int dtype, lnh_stream_t stream) {
    int rc = check_common(inputs_all, offsets_host, B, 3, C, L, dtype);
    if (rc) return rc;
    LNH_REQUIRE(embeddings && outputs_all, LNH_ERR_INVALID_ARG, "grid forward (mapped): null embeddings/outputs");
    LNH_REQUIRE(T_cur >= 1 && slot_off + T_cur <= T_tot && B % T_cur == 0 && (uint64_t)(B / T_cur) * T_tot <= B_all,
                LNH_ERR_INVALID_ARG, "grid forward (mapped): inconsistent row map");
    if (B == 0) return LNH_OK;
    LNH_REQUIRE(gridtype == kGridHash || gridtype == kGridTcnn, LNH_ERR_INVALID_ARG,
                "grid forward (mapped): gridtype must be 0 (hash) or 2 (tiny-cuda-nn lattice), got %u", gridtype);
    GridMeta m;
    if ((rc = resolve_levels(m, offsets_host, 3, L, S, H, gridtype, 0))) return rc;
    const RowMap map = make_row_map(T_cur, T_tot, slot_off, B_all);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_forward_c<T, 3>(inputs_all, (const T *)embeddings, (T *)outputs_all, nullptr, B, C, L, m, 0, 0,
                                      (hipStream_t)stream, map);
    });
}

int lnh_grid_encode_forward_mapped(const float *inputs_all, const void *embeddings, const int32_t *offsets_host,
                                   void *outputs_all, uint32_t B, uint32_t T_cur, uint32_t T_tot, uint32_t slot_off,
                                   uint32_t B_all, uint32_t C, uint32_t L, float S, uint32_t H, int dtype,
                                   lnh_stream_t stream) {
    return lnh_grid_encode_forward_mapped_ex(inputs_all, embeddings, offsets_host, outputs_all, B, T_cur, T_tot, slot_off,
                                             B_all, C, L, S, H, kGridHash, dtype, stream);
}

void lnh_grid_forward_set_schedule(uint32_t max_pairs, uint32_t block) {
    set_fwd_schedule(max_pairs, max_pairs == kFwdAuto ? 0 : block);
}

int lnh_grid_corner_indices(const float *inputs, const int32_t *offsets_host, uint32_t *out_idx, uint32_t B,
                            uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                            int align_corners, lnh_stream_t stream) {
    int rc = check_common(inputs, offsets_host, B, D, C, L, LNH_F32);
    if (rc) return rc;
    LNH_REQUIRE(out_idx, LNH_ERR_INVALID_ARG, "grid indices: null output");
    if (B == 0) return LNH_OK;
    GridMeta m;
    if ((rc = resolve_levels(m, offsets_host, D, L, S, H, gridtype, align_corners))) return rc;
    rc = with_dim(D, [&](auto d) {
        LNH_LAUNCH((k_grid_indices<decltype(d)::value>), dim3(div_up(B, 256), L), dim3(256), 0, (hipStream_t)stream, inputs,
                   out_idx, B, C, m, (uint32_t)(align_corners != 0));
        return LNH_OK;
    });
    return rc ? rc : lnh_check_launch("lnh_grid_corner_indices");
}

}  // extern "C"
