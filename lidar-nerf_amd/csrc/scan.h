// scan.h — the two integer scans of the count / scan / fill features, once:
//   workgroup_scan  exclusive scan of any number of values by ONE workgroup of kScanThreads threads, in tiles of kScanTile with a
//                   total carried from tile to tile (k_march_scan, k_fpa_scan, k_mc_scan, k_rc_scan, k_knn_scan)
//   block_scan_256  exclusive scan of one value per thread over a workgroup of 256 threads (marching cubes)
// Integer sums only: whatever the order of the additions, the result is the same bits.
#pragma once
#include <type_traits>

#include "common.h"

constexpr uint32_t kScanThreads = 1024, kScanPerThread = 4, kScanTile = kScanThreads * kScanPerThread;

// inclusive scan across the 64 lanes of a wave, and the value of one lane: what workgroup_scan asks of a type it sums (a caller
// with a type of its own overloads the two next to it).  32 bits go over the DPP network, 64 bits through __shfl_up (the 64-bit
// instance reads the wave totals from LDS and needs no scan_lane).
__device__ __forceinline__ uint32_t scan_wave(uint32_t v) { return wave_scan_add_u32(v); }
__device__ __forceinline__ uint32_t scan_lane(uint32_t v, uint32_t lane) { return (uint32_t)__shfl((int)v, (int)lane, 64); }
__device__ __forceinline__ unsigned long long scan_wave(unsigned long long v) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// Exclusive scan of load(0) ... load(n - 1), starting at `base`: store(i, base + load(0) + ... + load(i - 1)) for every i < n;
// returns base + the sum of all n, the same value in every thread.  Every thread of the workgroup (kScanThreads of them) must
// call it.  Sum is the type the values are added in inside a tile, Carry the type of the offsets and of the running total: a
// Carry wider than Sum is for tiles whose totals fit Sum while their sum over the tiles may not; a store that keeps 32 bits of
// a 64-bit offset keeps the low ones (it wraps).  load(i, live) is called with i < n always: behind the end it is called for
// i = n - 1 with live = false and its value is dropped, so the four loads of a thread stand outside any branch and are in flight
// together; a load that also counts something counts only where live.
template <typename Carry, typename Sum = Carry, typename Load, typename Store>
__device__ __forceinline__ Carry workgroup_scan(uint32_t n, Carry base, Load load, Store store) {
    constexpr uint32_t kWaves = kScanThreads / 64;
    __shared__ Sum s_wave[kWaves];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Carry carry = base;  // base + the totals of the tiles in front of this one: the same in every thread
    for (uint32_t tile = 0; tile < n; tile += kScanTile) {
        const uint32_t first = tile + threadIdx.x * kScanPerThread;  // kScanPerThread consecutive values per thread
        Sum c[kScanPerThread], mine = Sum();
#pragma unroll
        for (uint32_t k = 0; k < kScanPerThread; k++) {
            const bool live = first + k < n;
            const Sum v = load(min(first + k, n - 1), live);  // (never past the end; no branch around the load)
            c[k] = live ? v : Sum();
            mine += c[k];
        }
        const Sum incl = scan_wave(mine);
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        // every wave forms its own exclusive prefix of the kWaves wave totals and the tile's total
        Sum wave_off, tile_total;
        if constexpr (sizeof(Sum) == sizeof(uint32_t) * 2 && std::is_integral<Sum>::value) {
            // 64 bits: broadcast reads of the totals (a second __shfl_up scan is slower: 12 more ds_bpermute in a row)
            wave_off = tile_total = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; w++) {
                const Sum x = s_wave[w];
                wave_off += w < wv ? x : Sum();
                tile_total += x;
            }
        } else {
            const Sum wt = lane < kWaves ? s_wave[lane] : Sum();
            const Sum wincl = scan_wave(wt);
            wave_off = scan_lane(wincl - wt, wv), tile_total = scan_lane(wincl, kWaves - 1);
        }
        Carry off = carry + (wave_off + (incl - mine));
#pragma unroll
        for (uint32_t k = 0; k < kScanPerThread; k++) {
            if (first + k < n) store(first + k, off);
            off += c[k];
        }
        carry += tile_total;
        __syncthreads();  // s_wave is rewritten by the next tile
    }
    return carry;
}

// exclusive scan over the 256 threads of a workgroup; `total` = the sum.  s_wave: 4 words of LDS.
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t *s_wave, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t incl = wave_scan_add_u32(v);
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    const uint32_t w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
    total = w0 + w1 + w2 + w3;
    return incl - v + (wv > 0 ? w0 : 0u) + (wv > 1 ? w1 : 0u) + (wv > 2 ? w2 : 0u);
}
