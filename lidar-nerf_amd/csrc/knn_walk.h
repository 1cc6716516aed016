// knn_walk.h — the part of the k-nearest-neighbour search (knn.hip) that one thread runs for one query, written so that it also
// compiles as plain C++: tools/knn_walk_host.cpp runs exactly this code on the host, under the address and undefined-behaviour
// sanitizers, against a brute-force search.  Nothing here launches anything.
#pragma once
#include "cell_grid.h"

LNH_HD uint32_t knn_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
LNH_HD float knn_float(uint32_t b) { return __builtin_bit_cast(float, b); }
LNH_HD int knn_imin(int a, int b) { return a < b ? a : b; }
LNH_HD int knn_imax(int a, int b) { return a > b ? a : b; }
LNH_HD uint32_t knn_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The k smallest keys seen, ascending, in registers: every index below is a compile-time constant.  The array has K >= k slots;
// the first K - k hold 0, smaller than every key (a key carries index + 1), so they never move, the k slots behind them hold the
// answer and the k-th key is always the LAST slot: no slot is ever chosen at run time (that would send the array to scratch).
template <int K>
struct KnnBest {
    unsigned long long key[K];
    LNH_HD void clear(uint32_t k) {
#pragma unroll
        for (int j = 0; j < K; j++) key[j] = (uint32_t)j + k < (uint32_t)K ? 0ull : ~0ull;
    }
    LNH_HD void insert(unsigned long long k) {
        if (k < key[K - 1]) {
#pragma unroll
            for (int j = K - 1; j > 0; j--) key[j] = k < key[j - 1] ? key[j - 1] : (k < key[j] ? k : key[j]);
            key[0] = k < key[0] ? k : key[0];
        }
    }
    LNH_HD unsigned long long kth() const { return key[K - 1]; }
};

// (bits of d2) << 32 | (index + 1): the order of the contract's key (index < 2^31)
LNH_HD unsigned long long knn_key(float px, float py, float pz, uint32_t index, const float (&q)[3]) {
    const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
    const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
    return (unsigned long long)knn_bits(d2) << 32 | (index + 1u);
}

// a row of the cloud sorted by cell: the point and the bits of its original index
struct alignas(16) KnnRow {
    float x, y, z, w;
};

struct KnnArgs {
    const float *__restrict__ points;
    const float *__restrict__ box;
    const uint32_t *__restrict__ cell_start;
    const KnnRow *__restrict__ sorted;
    const float *__restrict__ slabs;
    const float *__restrict__ queries;
    const uint8_t *__restrict__ valid;
    const float *__restrict__ values;
    int32_t *__restrict__ indices;
    float *__restrict__ dist2;
    float *__restrict__ mean;
    uint32_t N, nx, ny, nz, Q, k;
};

// the walk of one query with finite coordinates: on return `best` holds the answer
template <int K>
LNH_HD void knn_walk(const KnnArgs &A, const float (&q)[3], KnnBest<K> &best) {
    const float inf = knn_float(0x7f800000u);
    const uint32_t N = A.N;
    const uint32_t nx = A.nx, ny = A.ny, nz = A.nz;
    if (nx * ny * nz == 1) {
        for (uint32_t i = 0; i < N; i++)
            best.insert(knn_key(A.points[(size_t)i * 3], A.points[(size_t)i * 3 + 1], A.points[(size_t)i * 3 + 2], i, q));
    } else {
        const CellGrid g = cell_grid(A.box, nx, ny, nz);
        const int cx = (int)cell_of(q[0], g.lo[0], g.inv[0], nx), cy = (int)cell_of(q[1], g.lo[1], g.inv[1], ny),
                  cz = (int)cell_of(q[2], g.lo[2], g.inv[2], nz);
        const uint32_t S = nx + ny + nz;
        const float *smin_x = A.slabs, *smin_y = A.slabs + nx, *smin_z = A.slabs + nx + ny;
        const float *pmax_x = A.slabs + S, *pmax_y = pmax_x + nx, *pmax_z = pmax_x + nx + ny;
        // lower bound of |p_a - q_a| for the points of slab s along an axis (0 for the query's own slab)
        auto gap = [](const float *__restrict__ smin, const float *__restrict__ pmax, int s, int c, float qa) -> float {
            return s > c ? fmaxf(smin[s] - qa, 0.0f) : (s < c ? fmaxf(qa - pmax[s], 0.0f) : 0.0f);
        };
        const int rmax = knn_imax(knn_imax(knn_imax(cx, (int)nx - 1 - cx), knn_imax(cy, (int)ny - 1 - cy)), knn_imax(cz, (int)nz - 1 - cz));
        for (int r = 0; r <= rmax; r++) {
            const int x0 = knn_imax(cx - r, 0), x1 = knn_imin(cx + r, (int)nx - 1), y0 = knn_imax(cy - r, 0), y1 = knn_imin(cy + r, (int)ny - 1);
            const int z0 = knn_imax(cz - r, 0), z1 = knn_imin(cz + r, (int)nz - 1);
            for (int x = x0; x <= x1; x++) {
                const float gx = gap(smin_x, pmax_x, x, cx, q[0]), gx2 = gx * gx;
                const bool edge_x = x == cx - r || x == cx + r;
                for (int y = y0; y <= y1; y++) {
                    const float gy = gap(smin_y, pmax_y, y, cy, q[1]), gxy2 = gx2 + gy * gy;
                    const unsigned long long kth = best.kth();
                    const float kth_d2 = knn_float((uint32_t)(kth >> 32));
                    const bool held = kth != ~0ull;
                    if (held && kth_d2 < gxy2) continue;  // every point of the column is farther than the k-th
                    const uint32_t col = ((uint32_t)x * ny + (uint32_t)y) * nz;
                    // the cells of this column that belong to shell r: all of [z0, z1] on the shell's x / y faces (one
                    // contiguous run), otherwise the two cells at distance r along z (r >= 1 there)
                    const bool face = edge_x || y == cy - r || y == cy + r;
                    for (int part = 0; part < (face ? 1 : 2); part++) {
                        const int za = face ? z0 : (part == 0 ? cz - r : cz + r), zb = face ? z1 : za;
                        if (za < 0 || zb > (int)nz - 1) continue;
                        if (!face) {
                            const float gz = gap(smin_z, pmax_z, za, cz, q[2]);
                            if (held && kth_d2 < gxy2 + gz * gz) continue;
                        }
                        const uint32_t e0 = knn_umin(A.cell_start[col + (uint32_t)za], N), e1 = knn_umin(A.cell_start[col + (uint32_t)zb + 1], N);
                        for (uint32_t e = e0; e < e1; e++) {  // (clamped to the buffer)
                            const KnnRow row = A.sorted[e];
                            best.insert(knn_key(row.x, row.y, row.z, knn_bits(row.w), q));
                        }
                    }
                }
            }
            // the stopping test: the nearest an untested point can be
            float gmin = inf;
            bool more = false;
            if (cx + r + 1 <= (int)nx - 1) more = true, gmin = fminf(gmin, fmaxf(smin_x[cx + r + 1] - q[0], 0.0f));
            if (cx - r - 1 >= 0) more = true, gmin = fminf(gmin, fmaxf(q[0] - pmax_x[cx - r - 1], 0.0f));
            if (cy + r + 1 <= (int)ny - 1) more = true, gmin = fminf(gmin, fmaxf(smin_y[cy + r + 1] - q[1], 0.0f));
            if (cy - r - 1 >= 0) more = true, gmin = fminf(gmin, fmaxf(q[1] - pmax_y[cy - r - 1], 0.0f));
            if (cz + r + 1 <= (int)nz - 1) more = true, gmin = fminf(gmin, fmaxf(smin_z[cz + r + 1] - q[2], 0.0f));
            if (cz - r - 1 >= 0) more = true, gmin = fminf(gmin, fmaxf(q[2] - pmax_z[cz - r - 1], 0.0f));
            if (!more) break;
            const unsigned long long kth = best.kth();
            if (kth != ~0ull && knn_float((uint32_t)(kth >> 32)) < gmin * gmin) break;
        }
    }
}
