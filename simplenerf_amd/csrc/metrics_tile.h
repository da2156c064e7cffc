// Tile / halo arithmetic of the SSIM kernel (metrics.hip), in a header of its own so that a plain C++ program can walk the same
// tiles on the host (tests/native/ssim_tile_test.cpp: bounds under AddressSanitizer, source indices against scipy's).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SNERF_TILE_FN __host__ __device__ __forceinline__
#else
#define SNERF_TILE_FN inline
#endif

namespace snerf {
namespace ssim_tile {

constexpr int kRadius = 5;   // int(truncate * sigma + 0.5) = int(3.5 * 1.5 + 0.5)
constexpr int kTaps = 2 * kRadius + 1;
constexpr int kTileW = 32, kTileH = 16;                                   // output pixels of one workgroup
constexpr int kInW = kTileW + 2 * kRadius, kInH = kTileH + 2 * kRadius;   // its input region: 42 x 26 pixels
constexpr int kInPitch = 3 * kInW + 2;                                    // bytes per LDS input row (128): 3 channels interleaved

// scipy.ndimage mode='reflect' (d c b a | a b c d) for -n <= i < 2n, then clamped: rows / columns further out exist only in
// ragged tiles, where they feed output pixels outside the image that are never stored or summed.
SNERF_TILE_FN int reflect_index(int i, int n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// Source row / column of local row / column `local` (0 .. kInH / kInW) of the tile that starts at `origin`.
SNERF_TILE_FN int source_index(int origin, int local, int n) { return reflect_index(origin - kRadius + local, n); }

}  // namespace ssim_tile
}  // namespace snerf
