// The field export (simplenerf_field.h): the nodes of a grid, or a point set, mapped into the MLP's input space and marked with the
// views that saw them, and the densities the MLP returns there turned into the signed volume mesh.hip extracts a surface from.
//
// snerf_field_grid_points, one launch: a thread per node of the block (x fastest; the camera rows are uniform over a wave) maps its
//   node and counts the views that see it.
// snerf_field_point_views, one launch: a thread per point maps it, picks the nearest view that sees it and writes the unit
//   direction from that view's centre.
// snerf_field_values, one launch: a thread per element.
// snerf_field_normals (simplenerf_gradient.h), one launch: a thread per point pulls the density's MLP-space gradient back through
//   the input map and writes the unit outward normal.
// The projection and the grid are mesh.hip's own device functions (mesh_lookup.h).  No atomics, one owner per output element, fp64
// throughout (the library is built with -ffp-contract=off).
// Bound: the first two by the fp64 divide rate (two divisions per view and point), the third by memory (9 bytes an element).
#include <cmath>

#include "snerf_common.h"
#include "simplenerf_field.h"
#include "simplenerf_gradient.h"
#include "mesh_lookup.h"
#include "field_map.h"
#include "sort_plan.h"

namespace {

using namespace snerf::sortplan;
using namespace snerf::mesh;
using namespace snerf::fieldmap;      // THE INPUT MAP and its pull-back: shared with normals.hip

struct Cameras {
    const double* table;
    int views, height, width;       // views == 0 when the frames have no pixel
};

// grid (ceil(count / kBlock))
__global__ void __launch_bounds__(kBlock) field_grid_points_kernel(Grid g, long long first_node, long long count, Cameras f, InputMap m,
                                                                   float* __restrict__ mlp_points, unsigned char* __restrict__ weight) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    int at[3];
    node_index(g, first_node + i, at);
    double P[3], Q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) P[a] = g.lo[a] + g.voxel_size * (double)at[a];
    const bool in_front = input_point(m, P, Q);
    int seen = 0;
    if (in_front) {
        for (int u = 0; u < f.views; ++u) {
            double c_z, ix, iy;
            if (view_pixel(f.table, u, f.height, f.width, P, &c_z, &ix, &iy)) ++seen;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) mlp_points[3 * i + a] = (float)Q[a];
    weight[i] = (unsigned char)seen;
}

// grid (ceil(count / kBlock)); f.views >= 1
__global__ void __launch_bounds__(kBlock) field_point_views_kernel(const float* __restrict__ points, long long count, Cameras f, InputMap m,
                                                                   float* __restrict__ mlp_points, float* __restrict__ view_dirs,
                                                                   unsigned char* __restrict__ view) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const double P[3] = {(double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2]};
    double Q[3];
    const bool in_front = input_point(m, P, Q);
    int chosen = -1;
    double nearest = 0.0;
    if (in_front) {
        for (int u = 0; u < f.views; ++u) {
            double c_z, ix, iy;
            if (!view_pixel(f.table, u, f.height, f.width, P, &c_z, &ix, &iy)) continue;
            if (chosen < 0 || c_z < nearest) {      // (strictly: equal depths keep the lower index)
                chosen = u;
                nearest = c_z;
            }
        }
    }
    const double* Ei = f.table + (long long)(chosen < 0 ? 0 : chosen) * kCamera + kEi;
    double v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = P[a] - Ei[4 * a + 3];
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mlp_points[3 * i + a] = (float)Q[a];
        view_dirs[3 * i + a] = n == 0.0 ? 0.0f : (float)(v[a] / n);
    }
    view[i] = (unsigned char)(chosen < 0 ? SNERF_FIELD_NO_VIEW : chosen);
}

// grid (ceil(count / kBlock))
__global__ void __launch_bounds__(kBlock) field_values_kernel(const float* __restrict__ sigma, const unsigned char* __restrict__ weight,
                                                              long long count, double level, float* __restrict__ tsdf) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const double s = (double)sigma[i];
    double value = 1.0;
    if (weight[i] != 0 && s == s) value = fmin(1.0, fmax(-1.0, (level - s) / level));
    tsdf[i] = (float)value;
}

// grid (ceil(count / kBlock)): the MLP-space gradient pulled back through the input map, negated and normalised (simplenerf_gradient.h)
__global__ void __launch_bounds__(kBlock) field_normals_kernel(const float* __restrict__ points, const float* __restrict__ grad, long long count,
                                                               InputMap m, float* __restrict__ normals) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const double P[3] = {(double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2]};
    const double g[3] = {(double)grad[3 * i], (double)grad[3 * i + 1], (double)grad[3 * i + 2]};
    double G[3], n;
    const bool in_front = pull_back(m, P, g, G);
    const bool usable = usable_length(G, &n) && in_front;
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = usable ? (float)(-G[a] / n) : 0.0f;
}

// SNERF_OK with *f's extents and *m filled, or the status the call returns (message set)
int views_of(const char* what, int views, int least, int height, int width, int ndc, double cx, double cy, double near, Cameras* f,
             InputMap* m) {
    SNERF_REQUIRE(height >= 0 && width >= 0, "%s: views of %d x %d", what, height, width);
    SNERF_REQUIRE(views >= least && views <= SNERF_FUSE_MAX_VIEWS, "%s: %d views, expected %d..%d", what, views, least, SNERF_FUSE_MAX_VIEWS);
    if (ndc) {
        SNERF_REQUIRE(std::isfinite(cx) && std::isfinite(cy), "%s: ndc parameters cx %g, cy %g are not finite", what, cx, cy);
        SNERF_REQUIRE(near > 0.0 && std::isfinite(near), "%s: ndc near %g, expected a finite number > 0", what, near);
    }
    f->views = (long long)height * width > 0 ? views : 0;       // (frames without pixels see nothing)
    f->height = height;
    f->width = width;
    m->ndc = ndc ? 1 : 0;
    m->cx = ndc ? cx : 0.0;
    m->cy = ndc ? cy : 0.0;
    m->near = ndc ? near : 0.0;
    return SNERF_OK;
}

}  // namespace

extern "C" int snerf_field_grid_points(double voxel_size, double lo_x, double lo_y, double lo_z, int nx, int ny, int nz, long long first_node,
                                       long long count, const double* cameras, int views, int height, int width, int ndc, double cx,
                                       double cy, double near, float* mlp_points, unsigned char* weight, snerf_stream_t stream) {
    Grid g;
    int status = grid_of("field_grid_points", voxel_size, lo_x, lo_y, lo_z, nx, ny, nz, &g);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(first_node >= 0 && count >= 0 && first_node <= g.nodes && count <= g.nodes - first_node,
                  "field_grid_points: nodes %lld .. %lld + %lld of a grid of %lld", first_node, first_node, count, g.nodes);
    Cameras f;
    InputMap m;
    status = views_of("field_grid_points", views, 0, height, width, ndc, cx, cy, near, &f, &m);
    if (status != SNERF_OK) return status;
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(mlp_points && weight && (views == 0 || cameras), "field_grid_points: NULL pointer");
    f.table = cameras;
    hipLaunchKernelGGL(field_grid_points_kernel, dim3(node_blocks(count)), dim3(kBlock), 0, (hipStream_t)stream, g, first_node, count, f, m,
                       mlp_points, weight);
    return snerf::check_launch("field_grid_points");
}

extern "C" int snerf_field_point_views(const float* points, long long count, const double* cameras, int views, int height, int width, int ndc,
                                       double cx, double cy, double near, float* mlp_points, float* view_dirs, unsigned char* view,
                                       snerf_stream_t stream) {
    SNERF_REQUIRE(count >= 0, "field_point_views: count %lld", count);
    Cameras f;
    InputMap m;
    const int status = views_of("field_point_views", views, 1, height, width, ndc, cx, cy, near, &f, &m);
    if (status != SNERF_OK) return status;
    if (count > kMaxCount) return snerf::fail(SNERF_E_UNSUPPORTED, "field_point_views: count %lld exceeds 2^31 - 1", count);
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(points && cameras && mlp_points && view_dirs && view, "field_point_views: NULL pointer");
    f.table = cameras;
    hipLaunchKernelGGL(field_point_views_kernel, dim3(node_blocks(count)), dim3(kBlock), 0, (hipStream_t)stream, points, count, f, m,
                       mlp_points, view_dirs, view);
    return snerf::check_launch("field_point_views");
}

extern "C" int snerf_field_values(const float* sigma, const unsigned char* weight, long long count, double level, float* tsdf,
                                  snerf_stream_t stream) {
    SNERF_REQUIRE(count >= 0, "field_values: count %lld", count);
    SNERF_REQUIRE(level > 0.0 && std::isfinite(level), "field_values: level %g, expected a finite number > 0", level);
    if (count > kMaxCount) return snerf::fail(SNERF_E_UNSUPPORTED, "field_values: count %lld exceeds 2^31 - 1", count);
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(sigma && weight && tsdf, "field_values: NULL pointer");
    hipLaunchKernelGGL(field_values_kernel, dim3(node_blocks(count)), dim3(kBlock), 0, (hipStream_t)stream, sigma, weight, count, level, tsdf);
    return snerf::check_launch("field_values");
}

extern "C" int snerf_field_normals(const float* points_scene, const float* grad_mlp, long long count, int ndc, double cx, double cy, double near,
                                   float* normals, snerf_stream_t stream) {
    SNERF_REQUIRE(count >= 0, "field_normals: count %lld", count);
    Cameras f;
    InputMap m;
    const int status = views_of("field_normals", 0, 0, 0, 0, ndc, cx, cy, near, &f, &m);
    if (status != SNERF_OK) return status;
    if (count > kMaxCount) return snerf::fail(SNERF_E_UNSUPPORTED, "field_normals: count %lld exceeds 2^31 - 1", count);
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(points_scene && grad_mlp && normals, "field_normals: NULL pointer");
    hipLaunchKernelGGL(field_normals_kernel, dim3(node_blocks(count)), dim3(kBlock), 0, (hipStream_t)stream, points_scene, grad_mlp, count, m,
                       normals);
    return snerf::check_launch("field_normals");
}
