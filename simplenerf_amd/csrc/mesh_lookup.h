// The grid and the projection that the surface export (mesh.hip) and the field export (field.hip) share: simplenerf_mesh.h's GRID
// and the part of its LOOKUP that reads no depth -- a point's depth in a view and the pixel it lands on.  Both files call the SAME
// device functions, so a node that a view of the one sees is seen by the other: a rule changed here changes for both.  The argument
// checks of the grid are here too.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "snerf_common.h"
#include "simplenerf_mesh.h"
#include "sort_plan.h"

namespace snerf {
namespace mesh {

constexpr int kCamera = SNERF_FUSE_CAMERA_DOUBLES;
constexpr int kEi = 9, kE = 21, kK = 33;                       // offsets of inv(E)[:3], E[:3] and K in a view's row of the camera table
static_assert(kK + 9 == kCamera, "the camera row is inv(K) | inv(E)[:3] | E[:3] | K");

struct Grid {
    double voxel_size, lo[3];
    int n[3];
    long long nodes;                // nx ny nz; 7 nodes <= 2^31 - 1
};

__device__ __forceinline__ void node_index(const Grid& g, long long n, int at[3]) {
    at[0] = (int)(n % g.n[0]);
    const long long row = n / g.n[0];
    at[1] = (int)(row % g.n[1]);
    at[2] = (int)(row / g.n[1]);
}

// THE LOOKUP of P in view u up to, and not including, the depth read: false when not c_z > 0 or the pixel lies outside the frame;
// else *c_z is P's depth in the view and (*ix, *iy) the pixel, integral values inside the frame.
__device__ __forceinline__ bool view_pixel(const double* __restrict__ cameras, int u, int height, int width, const double P[3], double* c_z,
                                           double* ix, double* iy) {
    const double* E = cameras + (long long)u * kCamera + kE;
    const double* K = cameras + (long long)u * kCamera + kK;
    double c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = ((E[4 * a] * P[0] + E[4 * a + 1] * P[1]) + E[4 * a + 2] * P[2]) + E[4 * a + 3];
    if (!(c[2] > 0.0)) return false;
    const double q0 = (K[0] * c[0] + K[1] * c[1]) + K[2] * c[2];
    const double q1 = (K[3] * c[0] + K[4] * c[1]) + K[5] * c[2];
    const double q2 = (K[6] * c[0] + K[7] * c[1]) + K[8] * c[2];
    const double x = rint(q0 / q2), y = rint(q1 / q2);
    if (!(x >= 0.0 && x < (double)width && y >= 0.0 && y < (double)height)) return false;     // (a NaN fails every comparison)
    *c_z = c[2];
    *ix = x;
    *iy = y;
    return true;
}

// SNERF_OK with *g filled, or the status the call returns (message set)
inline int grid_of(const char* what, double voxel_size, double lo_x, double lo_y, double lo_z, int nx, int ny, int nz, Grid* g) {
    SNERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: extents %d x %d x %d, each must be at least 1", what, nx, ny, nz);
    SNERF_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "%s: voxel_size %g, expected a finite number > 0", what, voxel_size);
    SNERF_REQUIRE(std::isfinite(lo_x) && std::isfinite(lo_y) && std::isfinite(lo_z), "%s: the bound (%g, %g, %g) is not finite", what, lo_x,
                  lo_y, lo_z);
    const long long limit = sortplan::kMaxCount / SNERF_MESH_KEYS_PER_NODE, xy = (long long)nx * ny;
    if (xy > limit || xy * nz > limit)
        return snerf::fail(SNERF_E_UNSUPPORTED, "%s: extents %d x %d x %d exceed the limit 7 nx ny nz <= 2^31 - 1", what, nx, ny, nz);
    g->voxel_size = voxel_size;
    g->lo[0] = lo_x; g->lo[1] = lo_y; g->lo[2] = lo_z;
    g->n[0] = nx; g->n[1] = ny; g->n[2] = nz;
    g->nodes = xy * nz;
    return SNERF_OK;
}

inline unsigned node_blocks(long long count) { return (unsigned)((count + sortplan::kBlock - 1) / sortplan::kBlock); }

}  // namespace mesh
}  // namespace snerf
