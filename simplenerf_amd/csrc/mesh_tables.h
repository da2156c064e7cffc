// The tables of the marching-tetrahedra extraction (mesh.hip, simplenerf_mesh.h), in a header of its own so that a plain C++ program
// can print them on the host (tests/native/mesh_tables_host.cpp; tests/test_mesh_host.py compares them with the table generated from
// the sentences of the rule, tests/mesh_reference.py).  No HIP types.
//
// A cell splits into the six Kuhn tetrahedra; tetrahedron T belongs to the T-th permutation (a, b, c) of the axes in lexicographic
// order and has the vertices m0 = the cell's origin, m1 = m0 + e_a, m2 = m1 + e_b, m3 = m2 + e_c.  A vertex is written as its
// offset code in the cell, bit 0 = x, bit 1 = y, bit 2 = z.  The case of a tetrahedron is the 4-bit number whose bit m is set when
// vertex m is negative.  A triangle is three tetrahedron edges (m, m'), m < m', each coded 4 m + m'; the order of the three is the
// winding: for node values of +-1 the normal (v1 - v0) x (v2 - v0) looks from the negative nodes to the positive ones.  The rows of
// the even permutations (xyz, yzx, zxy) are equal, those of the odd ones their mirror images.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SNERF_MESH_TABLE static __device__ const
#else
#define SNERF_MESH_TABLE static const
#endif

namespace snerf {
namespace mesh {

constexpr int kTetrahedra = 6;
constexpr int kCases = 16;
constexpr int kKeysPerNode = 7;       // the edge types that start at a node: a key is 7 n(A) + type

struct TetCase {
    unsigned char triangles;          // 0, 1 or 2
    unsigned char edge[6];            // 3 per triangle, 4 m + m'
};

// the offset codes of the four vertices of every tetrahedron
SNERF_MESH_TABLE unsigned char kTetVertex[kTetrahedra][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};

// type of an edge from the offset code of B - A: (1,0,0) 0, (0,1,0) 1, (0,0,1) 2, (1,1,0) 3, (1,0,1) 4, (0,1,1) 5, (1,1,1) 6
SNERF_MESH_TABLE unsigned char kTypeOfOffset[8] = {0, 0, 1, 3, 2, 4, 5, 6};      // ([0] is no edge)
SNERF_MESH_TABLE unsigned char kOffsetOfType[kKeysPerNode] = {1, 2, 4, 3, 5, 6, 7};

SNERF_MESH_TABLE TetCase kTetCase[kTetrahedra][kCases] = {
    {   /* tetrahedron 0: xyz */
        {0, { 0,  0,  0,  0,  0,  0}}, {1, { 1,  2,  3,  0,  0,  0}}, {1, { 1,  7,  6,  0,  0,  0}}, {2, { 2,  3,  7,  2,  7,  6}},
        {1, { 2,  6, 11,  0,  0,  0}}, {2, { 1, 11,  3,  1,  6, 11}}, {2, { 1,  7, 11,  1, 11,  2}}, {1, { 3,  7, 11,  0,  0,  0}},
        {1, { 3, 11,  7,  0,  0,  0}}, {2, { 1,  2, 11,  1, 11,  7}}, {2, { 1, 11,  6,  1,  3, 11}}, {1, { 2, 11,  6,  0,  0,  0}},
        {2, { 2,  6,  7,  2,  7,  3}}, {1, { 1,  6,  7,  0,  0,  0}}, {1, { 1,  3,  2,  0,  0,  0}}, {0, { 0,  0,  0,  0,  0,  0}}},
    {   /* tetrahedron 1: xzy */
        {0, { 0,  0,  0,  0,  0,  0}}, {1, { 1,  3,  2,  0,  0,  0}}, {1, { 1,  6,  7,  0,  0,  0}}, {2, { 2,  7,  3,  2,  6,  7}},
        {1, { 2, 11,  6,  0,  0,  0}}, {2, { 1,  3, 11,  1, 11,  6}}, {2, { 1, 11,  7,  1,  2, 11}}, {1, { 3, 11,  7,  0,  0,  0}},
        {1, { 3,  7, 11,  0,  0,  0}}, {2, { 1, 11,  2,  1,  7, 11}}, {2, { 1,  6, 11,  1, 11,  3}}, {1, { 2,  6, 11,  0,  0,  0}},
        {2, { 2,  7,  6,  2,  3,  7}}, {1, { 1,  7,  6,  0,  0,  0}}, {1, { 1,  2,  3,  0,  0,  0}}, {0, { 0,  0,  0,  0,  0,  0}}},
    {   /* tetrahedron 2: yxz */
        {0, { 0,  0,  0,  0,  0,  0}}, {1, { 1,  3,  2,  0,  0,  0}}, {1, { 1,  6,  7,  0,  0,  0}}, {2, { 2,  7,  3,  2,  6,  7}},
        {1, { 2, 11,  6,  0,  0,  0}}, {2, { 1,  3, 11,  1, 11,  6}}, {2, { 1, 11,  7,  1,  2, 11}}, {1, { 3, 11,  7,  0,  0,  0}},
        {1, { 3,  7, 11,  0,  0,  0}}, {2, { 1, 11,  2,  1,  7, 11}}, {2, { 1,  6, 11,  1, 11,  3}}, {1, { 2,  6, 11,  0,  0,  0}},
        {2, { 2,  7,  6,  2,  3,  7}}, {1, { 1,  7,  6,  0,  0,  0}}, {1, { 1,  2,  3,  0,  0,  0}}, {0, { 0,  0,  0,  0,  0,  0}}},
    {   /* tetrahedron 3: yzx */
        {0, { 0,  0,  0,  0,  0,  0}}, {1, { 1,  2,  3,  0,  0,  0}}, {1, { 1,  7,  6,  0,  0,  0}}, {2, { 2,  3,  7,  2,  7,  6}},
        {1, { 2,  6, 11,  0,  0,  0}}, {2, { 1, 11,  3,  1,  6, 11}}, {2, { 1,  7, 11,  1, 11,  2}}, {1, { 3,  7, 11,  0,  0,  0}},
        {1, { 3, 11,  7,  0,  0,  0}}, {2, { 1,  2, 11,  1, 11,  7}}, {2, { 1, 11,  6,  1,  3, 11}}, {1, { 2, 11,  6,  0,  0,  0}},
        {2, { 2,  6,  7,  2,  7,  3}}, {1, { 1,  6,  7,  0,  0,  0}}, {1, { 1,  3,  2,  0,  0,  0}}, {0, { 0,  0,  0,  0,  0,  0}}},
    {   /* tetrahedron 4: zxy */
        {0, { 0,  0,  0,  0,  0,  0}}, {1, { 1,  2,  3,  0,  0,  0}}, {1, { 1,  7,  6,  0,  0,  0}}, {2, { 2,  3,  7,  2,  7,  6}},
        {1, { 2,  6, 11,  0,  0,  0}}, {2, { 1, 11,  3,  1,  6, 11}}, {2, { 1,  7, 11,  1, 11,  2}}, {1, { 3,  7, 11,  0,  0,  0}},
        {1, { 3, 11,  7,  0,  0,  0}}, {2, { 1,  2, 11,  1, 11,  7}}, {2, { 1, 11,  6,  1,  3, 11}}, {1, { 2, 11,  6,  0,  0,  0}},
        {2, { 2,  6,  7,  2,  7,  3}}, {1, { 1,  6,  7,  0,  0,  0}}, {1, { 1,  3,  2,  0,  0,  0}}, {0, { 0,  0,  0,  0,  0,  0}}},
    {   /* tetrahedron 5: zyx */
        {0, { 0,  0,  0,  0,  0,  0}}, {1, { 1,  3,  2,  0,  0,  0}}, {1, { 1,  6,  7,  0,  0,  0}}, {2, { 2,  7,  3,  2,  6,  7}},
        {1, { 2, 11,  6,  0,  0,  0}}, {2, { 1,  3, 11,  1, 11,  6}}, {2, { 1, 11,  7,  1,  2, 11}}, {1, { 3, 11,  7,  0,  0,  0}},
        {1, { 3,  7, 11,  0,  0,  0}}, {2, { 1, 11,  2,  1,  7, 11}}, {2, { 1,  6, 11,  1, 11,  3}}, {1, { 2,  6, 11,  0,  0,  0}},
        {2, { 2,  7,  6,  2,  3,  7}}, {1, { 1,  7,  6,  0,  0,  0}}, {1, { 1,  2,  3,  0,  0,  0}}, {0, { 0,  0,  0,  0,  0,  0}}},
};

}  // namespace mesh
}  // namespace snerf
