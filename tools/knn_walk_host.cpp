// knn_walk_host.cpp — the per-query walk of the k-nearest-neighbour search (lidar-nerf_amd/csrc/knn_walk.h, the code the kernel
// runs) on the host, against a brute-force search, for a run under the address and undefined-behaviour sanitizers:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/knn_walk_host.cpp -o knn_walk_host
//   ./knn_walk_host
// The grid is built serially with the same cell function; every array is allocated at its exact size, so a read or a write of the
// walk outside cell_start, the sorted rows or the slab arrays is reported.  Exit status 0: every case equal to brute force.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../lidar-nerf_amd/csrc/knn_walk.h"

namespace {

struct Index {
    std::vector<float> points, box, slabs;
    std::vector<uint32_t> cell_start;
    KnnRow *sorted = nullptr;
    uint32_t N = 0, n[3] = {1, 1, 1};
    ~Index() { std::free(sorted); }
};

void build(Index &ix, const std::vector<float> &points, uint32_t nx, uint32_t ny, uint32_t nz) {
    const float inf = std::numeric_limits<float>::infinity();
    ix.points = points, ix.N = (uint32_t)(points.size() / 3), ix.n[0] = nx, ix.n[1] = ny, ix.n[2] = nz;
    ix.box.assign(8, 0.0f);
    for (int a = 0; a < 3; a++) ix.box[a] = inf, ix.box[3 + a] = -inf;
    for (uint32_t i = 0; i < ix.N; i++)
        for (int a = 0; a < 3; a++) ix.box[a] = fminf(ix.box[a], points[i * 3 + a]), ix.box[3 + a] = fmaxf(ix.box[3 + a], points[i * 3 + a]);
    const CellGrid g = cell_grid(ix.box.data(), nx, ny, nz);
    const uint32_t cells = nx * ny * nz, S = nx + ny + nz, off[3] = {0, nx, nx + ny};
    std::vector<uint32_t> cell(ix.N), count(cells, 0);
    std::vector<float> lo(S, inf), hi(S, -inf);
    for (uint32_t i = 0; i < ix.N; i++) {
        uint32_t c[3];
        for (int a = 0; a < 3; a++) {
            c[a] = cell_of(points[i * 3 + a], g.lo[a], g.inv[a], g.n[a]);
            lo[off[a] + c[a]] = fminf(lo[off[a] + c[a]], points[i * 3 + a]);
            hi[off[a] + c[a]] = fmaxf(hi[off[a] + c[a]], points[i * 3 + a]);
        }
        cell[i] = (c[0] * ny + c[1]) * nz + c[2];
        count[cell[i]]++;
    }
    ix.slabs.assign(2 * S, 0.0f);
    for (int a = 0; a < 3; a++) {
        float m = inf;
        for (uint32_t i = g.n[a]; i-- > 0;) m = fminf(m, lo[off[a] + i]), ix.slabs[off[a] + i] = m;
        m = -inf;
        for (uint32_t i = 0; i < g.n[a]; i++) m = fmaxf(m, hi[off[a] + i]), ix.slabs[S + off[a] + i] = m;
    }
    ix.cell_start.assign(cells + 1, 0);
    for (uint32_t c = 0; c < cells; c++) ix.cell_start[c + 1] = ix.cell_start[c] + count[c];
    std::free(ix.sorted);
    ix.sorted = (KnnRow *)std::aligned_alloc(16, sizeof(KnnRow) * ix.N);
    std::vector<uint32_t> cursor(cells, 0);
    for (uint32_t i = ix.N; i-- > 0;) {  // (backwards: the order inside a cell must not matter)
        const uint32_t slot = ix.cell_start[cell[i]] + cursor[cell[i]]++;
        ix.sorted[slot] = KnnRow{points[i * 3], points[i * 3 + 1], points[i * 3 + 2], knn_float(i)};
    }
}

template <int K>
bool check(const Index &ix, const float (&q)[3], uint32_t k) {
    KnnArgs A = {};
    A.points = ix.points.data(), A.box = ix.box.data(), A.cell_start = ix.cell_start.data(), A.sorted = ix.sorted;
    A.slabs = ix.slabs.data(), A.N = ix.N, A.nx = ix.n[0], A.ny = ix.n[1], A.nz = ix.n[2], A.Q = 1, A.k = k;
    KnnBest<K> best;
    best.clear(k);
    knn_walk<K>(A, q, best);
    std::vector<unsigned long long> all(ix.N);
    for (uint32_t i = 0; i < ix.N; i++) all[i] = knn_key(ix.points[i * 3], ix.points[i * 3 + 1], ix.points[i * 3 + 2], i, q);
    std::sort(all.begin(), all.end());
    for (uint32_t j = 0; j < k; j++) {
        const unsigned long long want = j < ix.N ? all[j] : ~0ull;
        if (best.key[K - k + j] != want) return false;
    }
    for (uint32_t j = 0; j + k < (uint32_t)K; j++)
        if (best.key[j] != 0ull) return false;
    return true;
}

bool check_k(const Index &ix, const float (&q)[3], uint32_t k) {
    if (k == 1) return check<1>(ix, q, k);
    if (k <= 4) return check<4>(ix, q, k);
    if (k == 5) return check<5>(ix, q, k);
    if (k <= 8) return check<8>(ix, q, k);
    if (k == 9) return check<9>(ix, q, k);
    return check<16>(ix, q, k);
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    const uint32_t grids[][3] = {{1, 1, 1}, {2, 3, 5}, {8, 8, 8}, {17, 19, 16}, {1, 1, 64}, {33, 1, 2}};
    unsigned long long cases = 0, bad = 0;
    for (int cloud = 0; cloud < 6; cloud++) {
        std::vector<float> p;
        const uint32_t n = cloud == 5 ? 1 : 700;
        for (uint32_t i = 0; i < n; i++) {
            float x = uni(rng) * 10 - 3, y = uni(rng) * 4, z = uni(rng) * 7 + 100;
            if (cloud == 1) x = floorf(x), y = floorf(y), z = floorf(z);           // a lattice full of ties
            if (cloud == 2 && i >= n / 2) x = p[(i - n / 2) * 3], y = p[(i - n / 2) * 3 + 1], z = p[(i - n / 2) * 3 + 2];  // duplicates
            if (cloud == 3) z = 2.5f;                                              // a flat cloud
            if (cloud == 4 && i % 7 == 0) x += 500.0f, y -= 300.0f;                // a far-away cluster
            p.push_back(x), p.push_back(y), p.push_back(z);
        }
        for (const auto &gr : grids) {
            Index ix;
            build(ix, p, gr[0], gr[1], gr[2]);
            for (int t = 0; t < 60; t++) {
                const uint32_t i = (uint32_t)(rng() % n);
                float q[3] = {p[i * 3], p[i * 3 + 1], p[i * 3 + 2]};
                if (t % 4 == 1) q[0] += 1e-3f * (uni(rng) - 0.5f), q[2] -= 1e-3f * uni(rng);
                if (t % 4 == 2) q[0] = uni(rng) * 10 - 3, q[1] = uni(rng) * 4, q[2] = uni(rng) * 7 + (cloud == 3 ? -4.0f : 100.0f);
                if (t % 4 == 3) q[0] = (uni(rng) - 0.5f) * 4000.0f, q[1] = (uni(rng) - 0.5f) * 4000.0f, q[2] = (uni(rng) - 0.5f) * 4000.0f;
                if (t == 59) q[0] = 3e38f, q[1] = -3e38f;  // d2 overflows: +inf on both sides of every comparison
                for (uint32_t k = 1; k <= 16; k++) {
                    cases++;
                    if (!check_k(ix, q, k)) {
                        bad++;
                        std::printf("MISMATCH cloud %d grid %u x %u x %u query %d k %u\n", cloud, gr[0], gr[1], gr[2], t, k);
                    }
                }
            }
        }
    }
    std::printf("%llu cases, %llu mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
