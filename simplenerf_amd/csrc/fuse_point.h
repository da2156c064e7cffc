// The point of a pixel that the point-cloud export (fuse.hip) and the depth-map normals (normals.hip) share: simplenerf_fuse.h's
// validity of a depth and P = inv(E)[:3] [d inv(K) (x, y, 1); 1].  Both files call the SAME device functions, so a pixel's point in
// the cloud is, bit for bit, the point its normal was formed from: a rule changed here changes for both.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

#include "simplenerf_fuse.h"

namespace snerf {
namespace fusepoint {

constexpr int kCamera = SNERF_FUSE_CAMERA_DOUBLES;
constexpr int kInvK = 0, kInvE = 9, kE = 21, kK = 33;     // offsets in a view's row of the camera table
static_assert(kK + 9 == kCamera, "the camera row is inv(K) | inv(E)[:3] | E[:3] | K");

__device__ __forceinline__ bool valid_depth(float d) { return d > 0.0f && d <= FLT_MAX; }     // (false for a NaN)

// out = m[:3] . [p; 1] for a row-major 3x4 m
__device__ __forceinline__ void affine(const double* __restrict__ m, const double p[3], double out[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = ((m[4 * a] * p[0] + m[4 * a + 1] * p[1]) + m[4 * a + 2] * p[2]) + m[4 * a + 3];
}

// P of source pixel (x, y) with depth d of the view whose camera row is `cam`
__device__ __forceinline__ void unproject(const double* __restrict__ cam, int x, int y, double d, double P[3]) {
    double c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = d * ((cam[kInvK + 3 * a] * (double)x + cam[kInvK + 3 * a + 1] * (double)y) + cam[kInvK + 3 * a + 2]);
    affine(cam + kInvE, c, P);
}

}  // namespace fusepoint
}  // namespace snerf
