// nvs_ssim_tile_host.cpp — the tile / halo indexing and the arithmetic of the 1-D SSIM kernel (lidar-nerf_amd/csrc/
// nvs_ssim_tile.h, the code k_nvs_ssim runs) on the host, tile by tile as the kernel's workgroups walk them, against a direct
// evaluation of the cropped sequence, for a run under the address and undefined-behaviour sanitizers:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/nvs_ssim_tile_host.cpp -o nvs_ssim_tile_host
//   ./nvs_ssim_tile_host
// Every array is allocated at its exact size (the images H * W, a tile's staging buffers at what the tile stages), so a read
// outside the image or a window that leaves the staged elements is reported.  Exit status 0: every case equal.
#include <cstdio>
#include <random>
#include <vector>

#include "../lidar-nerf_amd/csrc/nvs_ssim_tile.h"

namespace {

struct Case {
    uint32_t H, W, r0, c0, h, w;
};

// what the kernel's grid computes: per tile a sum over its positions in thread order, then the sums in tile order
double by_tiles(const Case &c, const std::vector<float> &gt, const std::vector<float> &pd, double c1, double c2, uint32_t tiles) {
    const NvsSeq seq{c.r0, c.c0, c.h, c.w, c.W, c.h * c.w};
    double total = 0.0;
    for (uint32_t t = 0; t < tiles; t++) {  // (tiles: sized for the capacity H * W, so some own nothing)
        const uint32_t staged = nvs_tile_staged(seq.n, t), owned = nvs_tile_positions(seq.n, t);
        if (owned == 0) continue;
        std::vector<float> sx(staged), sy(staged);  // exact size: a window past the staged elements is an overflow
        for (uint32_t e = 0; e < staged; e++) {
            const uint32_t p = nvs_seq_pixel(seq, t * kNvsTile + e);
            sx[e] = nvs_clamp_depth(gt.at(p));
            sy[e] = nvs_clamp_depth(pd.at(p));
        }
        double part = 0.0;
        for (uint32_t i = 0; i < owned; i++) part += nvs_ssim_at(sx.data() + i, sy.data() + i, c1, c2);
        total += part;
    }
    return total;
}

double direct(const Case &c, const std::vector<float> &gt, const std::vector<float> &pd, double c1, double c2) {
    std::vector<float> x, y;
    for (uint32_t r = 0; r < c.h; r++)
        for (uint32_t q = 0; q < c.w; q++) {
            x.push_back(nvs_clamp_depth(gt[(c.r0 + r) * c.W + c.c0 + q]));
            y.push_back(nvs_clamp_depth(pd[(c.r0 + r) * c.W + c.c0 + q]));
        }
    double total = 0.0, part = 0.0;
    for (uint32_t i = 0; i + kNvsWin <= x.size(); i++) {
        part += nvs_ssim_at(x.data() + i, y.data() + i, c1, c2);
        if ((i + 1) % kNvsTile == 0 || i + kNvsWin == x.size()) total += part, part = 0.0;  // (the kernel's grouping)
    }
    return total;
}

}  // namespace

int main() {
    std::mt19937 rng(2024);
    std::uniform_real_distribution<float> uni(0.0f, 90.0f);
    const Case cases[] = {
        {1, 7, 0, 0, 1, 7}, {1, 8, 0, 0, 1, 8}, {3, 5, 0, 0, 3, 5}, {6, 16, 0, 0, 6, 16}, {23, 37, 0, 0, 23, 37},
        {1, kNvsTile + 6, 0, 0, 1, kNvsTile + 6}, {1, kNvsTile + 5, 0, 0, 1, kNvsTile + 5}, {1, kNvsTile + 7, 0, 0, 1, kNvsTile + 7},
        {1, 2 * kNvsTile + 7, 0, 0, 1, 2 * kNvsTile + 7}, {66, 1030, 0, 0, 66, 1030},
        {23, 37, 0, 0, 5, 9}, {23, 37, 0, 28, 5, 9}, {23, 37, 18, 0, 5, 9}, {23, 37, 18, 28, 5, 9}, {23, 37, 4, 3, 1, 7},
        {23, 37, 22, 30, 1, 7}, {66, 1030, 3, 100, 60, 700}, {23, 37, 2, 2, 2, 3}, {5, 5, 0, 0, 0, 0}};
    unsigned bad = 0, n_cases = 0;
    for (const Case &c : cases) {
        std::vector<float> gt((size_t)c.H * c.W), pd((size_t)c.H * c.W);
        for (auto &v : gt) v = uni(rng);
        for (auto &v : pd) v = uni(rng);
        double c1, c2;
        nvs_ssim_constants(1e-3f, 80.0f, c1, c2);
        const uint32_t cap_tiles = nvs_tiles(c.H * c.W) ? nvs_tiles(c.H * c.W) : 1u;
        const double a = by_tiles(c, gt, pd, c1, c2, cap_tiles), b = direct(c, gt, pd, c1, c2);
        const uint32_t n = c.h * c.w;
        uint32_t owned = 0;
        for (uint32_t t = 0; t < cap_tiles; t++) owned += nvs_tile_positions(n, t);
        n_cases++;
        if (!(a == b) || owned != nvs_positions(n) || nvs_tiles(n) > cap_tiles) {
            bad++;
            std::printf("MISMATCH %u x %u window %u x %u at (%u, %u): %.17g vs %.17g, %u positions owned of %u\n", c.H, c.W, c.h, c.w,
                        c.r0, c.c0, a, b, owned, nvs_positions(n));
        }
    }
    std::printf("%u cases, %u mismatches\n", n_cases, bad);
    return bad ? 1 : 0;
}
