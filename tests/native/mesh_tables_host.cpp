// The tables of the marching-tetrahedra extraction (simplenerf_amd/csrc/mesh_tables.h) printed by a plain C++ program: the text the
// kernels of mesh.hip index, compiled for the host.  tests/test_mesh_host.py compares the output with the tables generated from the
// sentences of the rule (tests/mesh_reference.py).
//
//   mesh_tables_host
//
// Output, one line each: "vertex T c0 c1 c2 c3" (6), "type code type" (7, codes 1..7), "offset type code" (7),
// "case T case triangles e0 .. e5" (96).
#include <cstdio>

#include "../../simplenerf_amd/csrc/mesh_tables.h"

int main() {
    using namespace snerf::mesh;
    for (int t = 0; t < kTetrahedra; ++t)
        std::printf("vertex %d %d %d %d %d\n", t, kTetVertex[t][0], kTetVertex[t][1], kTetVertex[t][2], kTetVertex[t][3]);
    for (int code = 1; code < 8; ++code) std::printf("type %d %d\n", code, kTypeOfOffset[code]);
    for (int type = 0; type < kKeysPerNode; ++type) std::printf("offset %d %d\n", type, kOffsetOfType[type]);
    for (int t = 0; t < kTetrahedra; ++t)
        for (int c = 0; c < kCases; ++c) {
            const TetCase& entry = kTetCase[t][c];
            std::printf("case %d %d %d", t, c, entry.triangles);
            for (int e = 0; e < 6; ++e) std::printf(" %d", entry.edge[e]);
            std::printf("\n");
        }
    return 0;
}
