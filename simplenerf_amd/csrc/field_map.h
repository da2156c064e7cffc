// THE INPUT MAP of simplenerf_field.h and the pull-back of a gradient through it (simplenerf_gradient.h), shared by the field export
// (field.hip) and the normal maps (normals.hip).  Both files call the SAME device functions, so a sample's normal along a ray is
// pulled back exactly as a vertex's is: a rule changed here changes for both.  fp64, no fused multiply-adds.
#pragma once

#include <hip/hip_runtime.h>

namespace snerf {
namespace fieldmap {

struct InputMap {
    int ndc;
    double cx, cy, near;
};

// THE INPUT MAP: Q of P, and whether P is in front (always, without ndc)
__device__ __forceinline__ bool input_point(const InputMap& m, const double P[3], double Q[3]) {
    if (!m.ndc) {
        Q[0] = P[0]; Q[1] = P[1]; Q[2] = P[2];
        return true;
    }
    if (!(P[2] <= -m.near)) {       // (a NaN is not in front)
        Q[0] = 0.0; Q[1] = 0.0; Q[2] = 0.0;
        return false;
    }
    Q[0] = (m.cx * P[0]) / P[2];
    Q[1] = (m.cy * P[1]) / P[2];
    Q[2] = 1.0 + (2.0 * m.near) / P[2];
    return true;
}

// G = J^T g at the scene point P (g itself without ndc), and whether P is in front
__device__ __forceinline__ bool pull_back(const InputMap& m, const double P[3], const double g[3], double G[3]) {
    G[0] = g[0]; G[1] = g[1]; G[2] = g[2];
    if (!m.ndc) return true;
    G[0] = (m.cx / P[2]) * g[0];
    G[1] = (m.cy / P[2]) * g[1];
    G[2] = -((((m.cx * P[0]) * g[0] + (m.cy * P[1]) * g[1]) + (2.0 * m.near) * g[2]) / (P[2] * P[2]));
    return P[2] <= -m.near;       // (a NaN is not in front)
}

// m = |G|, and whether a normal can be formed from it
__device__ __forceinline__ bool usable_length(const double G[3], double* length) {
    const double n = sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
    *length = n;
    return n > 0.0 && n < INFINITY;     // (a NaN length fails both comparisons)
}

}  // namespace fieldmap
}  // namespace snerf
