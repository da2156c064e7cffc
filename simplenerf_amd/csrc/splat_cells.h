// Cell, clip and list-walk arithmetic of the visibility-mask splat (visibility_mask.hip), in a header of its own so that a plain C++
// program can walk the same cells on the host (tests/native/splat_cells_test.cpp: bounds under AddressSanitizer, sums against a
// brute-force scatter).
//
// The splat (the reference's Warper.bilinear_splatting) works on a grid padded by one cell on every side: a source pixel at the padded
// position (X, Y) adds its weight to the four cells (floor | ceil X, floor | ceil Y), each clipped to [0, w + 1] x [0, h + 1], and the
// border cells are cropped away afterwards.  Floor and ceil are taken BEFORE the position is clipped.  An interior cell (1..h, 1..w) can
// only be reached by a source whose UNCLIPPED floor cell lies in [0, h] x [0, w] (a clipped value inside 1..n is the unclipped one, and
// ceil - floor <= 1), so sources are keyed by that cell, every other source goes to one discard key that is never walked, and a
// destination (r, c) reads at most the four lists (r, c), (r - 1, c), (r, c - 1), (r - 1, c - 1).
//
// Unpinned sources -- a non-finite X, Y or Z, or a floor outside int32, which the reference feeds to an undefined astype('int') --
// contribute nothing: they take the discard key too.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SNERF_SPLAT_FN __host__ __device__ __forceinline__
#else
#define SNERF_SPLAT_FN inline
#endif

namespace snerf {
namespace splat {

// Keys of one view: (h + 1)(w + 1) floor cells, row-major over [0, h] x [0, w], then the discard key.
SNERF_SPLAT_FN int cell_keys(int h, int w) { return (h + 1) * (w + 1); }
SNERF_SPLAT_FN int keys_per_view(int h, int w) { return cell_keys(h, w) + 1; }
SNERF_SPLAT_FN int cell_key(int fy, int fx, int w) { return fy * (w + 1) + fx; }

SNERF_SPLAT_FN bool is_finite(double v) { return v - v == 0.0; }   // false for inf and nan

// A pinned coordinate: finite, with floor and ceil well inside int32.
SNERF_SPLAT_FN bool pinned(double v) { return is_finite(v) && v > -2147483000.0 && v < 2147483000.0; }

SNERF_SPLAT_FN int clip_int(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
SNERF_SPLAT_FN double clip_double(double v, double hi) { return v < 0.0 ? 0.0 : (v > hi ? hi : v); }

// Key of the source at padded position (X, Y) with transformed depth Z.
SNERF_SPLAT_FN int source_key(double X, double Y, double Z, int h, int w) {
    if (!pinned(X) || !pinned(Y) || !is_finite(Z)) return cell_keys(h, w);
    const double fx = floor(X), fy = floor(Y);
    if (fx < 0.0 || fx > (double)w || fy < 0.0 || fy > (double)h) return cell_keys(h, w);
    return cell_key((int)fy, (int)fx, w);
}

// One axis of a pinned source: clipped floor and ceil cells, and the proximity weights of the two (Warper.py:123-140).
struct Axis {
    int lo, hi;            // clip(floor v), clip(ceil v): equal for an integer v, and then both weights are 1
    double w_lo, w_hi;     // 1 - (v' - lo), 1 - (hi - v') with v' = clip(v)
};

SNERF_SPLAT_FN Axis axis_of(double v, int n) {   // n = w or h: cells 0 .. n + 1
    Axis a;
    a.lo = clip_int((int)floor(v), n + 1);
    a.hi = clip_int((int)ceil(v), n + 1);
    const double c = clip_double(v, (double)(n + 1));
    a.w_lo = 1.0 - (c - (double)a.lo);
    a.w_hi = 1.0 - ((double)a.hi - c);
    return a;
}

// The reference's depth weight divisor exp(L / max L * 50), L = log(1 + clip(Z, 0, 1000)).
SNERF_SPLAT_FN double log_depth(double Z) { return log(1.0 + (Z < 0.0 ? 0.0 : (Z > 1000.0 ? 1000.0 : Z))); }
SNERF_SPLAT_FN double depth_divisor(double Z, double max_log_depth) { return exp(log_depth(Z) / max_log_depth * 50.0); }

// What a pinned source at (X, Y) adds to the padded cell (r, c): `zw` += Z * weight, `ws` += weight for each of its four corners
// that IS (r, c), in the order nw, sw, ne, se (a source on an integer position adds all four).  `divisor`: depth_divisor of it.
SNERF_SPLAT_FN void add_source(double X, double Y, double Z, double divisor, int r, int c, int h, int w, double& zw, double& ws) {
    const Axis ax = axis_of(X, w), ay = axis_of(Y, h);
    const bool x_lo = ax.lo == c, x_hi = ax.hi == c, y_lo = ay.lo == r, y_hi = ay.hi == r;
    if (y_lo && x_lo) { const double k = ay.w_lo * ax.w_lo / divisor; zw += Z * k; ws += k; }
    if (y_hi && x_lo) { const double k = ay.w_hi * ax.w_lo / divisor; zw += Z * k; ws += k; }
    if (y_lo && x_hi) { const double k = ay.w_lo * ax.w_hi / divisor; zw += Z * k; ws += k; }
    if (y_hi && x_hi) { const double k = ay.w_hi * ax.w_hi / divisor; zw += Z * k; ws += k; }
}

// The lists an interior padded cell (r, c), 1 <= r <= h, 1 <= c <= w, reads, in the order they are walked; -> their number (4:
// r - 1 >= 0 and c - 1 >= 0 always hold for an interior cell; r <= h and c <= w keep every key below the discard key).
SNERF_SPLAT_FN int lists_of(int r, int c, int w, int keys[4]) {
    keys[0] = cell_key(r, c, w);
    keys[1] = cell_key(r - 1, c, w);
    keys[2] = cell_key(r, c - 1, w);
    keys[3] = cell_key(r - 1, c - 1, w);
    return 4;
}

}  // namespace splat
}  // namespace snerf
