// Cell and tap arithmetic of the Warper (warp.hip) beyond what the visibility masks need (splat_cells.h), in a header of its own so
// that a plain C++ program can walk it on the host (tests/native/warp_cells_test.cpp: bounds under AddressSanitizer, sums against a
// brute-force scatter and a brute-force padded frame).
//
// The splat of a frame with c channels adds v[ch] * weight per channel where the depth splat adds Z * weight: corner_weights hands
// out the weights add_source (splat_cells.h) computes, in its order.  The backward warp (the reference's
// Warper.bilinear_interpolation) reads the four cells (floor | ceil X, floor | ceil Y) of the frame padded by one cell of zeros
// on every side, floor and ceil taken BEFORE the clip to [0, w + 1] x [0, h + 1], exactly as the splat writes them.
#pragma once

#include "splat_cells.h"

namespace snerf {
namespace splat {

// The weights a pinned source at (X, Y) adds to the padded cell (r, c), one per corner that IS (r, c), in the order nw, sw, ne, se
// (a source on an integer position adds all four, each 1 / divisor); -> their number, 0..4.  The same expressions as add_source.
SNERF_SPLAT_FN int corner_weights(double X, double Y, double divisor, int r, int c, int h, int w, double k[4]) {
    const Axis ax = axis_of(X, w), ay = axis_of(Y, h);
    const bool x_lo = ax.lo == c, x_hi = ax.hi == c, y_lo = ay.lo == r, y_hi = ay.hi == r;
    int n = 0;
    if (y_lo && x_lo) k[n++] = ay.w_lo * ax.w_lo / divisor;
    if (y_hi && x_lo) k[n++] = ay.w_hi * ax.w_lo / divisor;
    if (y_lo && x_hi) k[n++] = ay.w_lo * ax.w_hi / divisor;
    if (y_hi && x_hi) k[n++] = ay.w_hi * ax.w_hi / divisor;
    return n;
}

// The four taps of the backward warp at the pinned padded position (X, Y), in the order nw, sw, ne, se: the padded cell of each and
// its proximity weight (Warper.py:216-223).
struct Taps {
    int row[4], col[4];
    double prox[4];
};

SNERF_SPLAT_FN Taps taps_of(double X, double Y, int h, int w) {
    const Axis ax = axis_of(X, w), ay = axis_of(Y, h);
    Taps t;
    t.row[0] = ay.lo; t.col[0] = ax.lo; t.prox[0] = ay.w_lo * ax.w_lo;
    t.row[1] = ay.hi; t.col[1] = ax.lo; t.prox[1] = ay.w_hi * ax.w_lo;
    t.row[2] = ay.lo; t.col[2] = ax.hi; t.prox[2] = ay.w_lo * ax.w_hi;
    t.row[3] = ay.hi; t.col[3] = ax.hi; t.prox[3] = ay.w_hi * ax.w_hi;
    return t;
}

// Pixel index (row-major over h x w) of the padded cell (r, c), or -1 for a cell of the zero border (and for anything outside the
// padded grid, which taps_of never returns).
SNERF_SPLAT_FN long long frame_index(int r, int c, int h, int w) {
    if (r < 1 || r > h || c < 1 || c > w) return -1;
    return (long long)(r - 1) * w + (c - 1);
}

// numpy.round(numpy.clip(v, 0, 255)).astype('uint8'): half to even (rint under the default rounding mode); a NaN, whose cast the
// reference leaves undefined, gives 0.
SNERF_SPLAT_FN unsigned char to_image(double v) {
    if (!(v == v)) return 0;
    return (unsigned char)rint(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

}  // namespace splat
}  // namespace snerf
