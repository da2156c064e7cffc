"""The normal maps restated for the tests in the words of simplenerf_amd/csrc/simplenerf_normals.h: rules a-d (the selection of a
render's samples, the compositing of the field's normals, the normals of a depth map, normals as a picture), element by element
in plain Python floats -- IEEE doubles, one operation per step, in the header's order, nothing fused, nothing vectorised -- but
the selected sample's point, which is float32 arithmetic as the header says.  numpy only.

What tests/test_normals_host.py pins on the CPU (the inverse input map against the forward one, a planar slab, a fronto-parallel
plane) and tests/test_gpu_normals.py holds the device to."""
import math

import numpy

E_INV = 9            # offset of inv(E)[:3] in a view's row of the camera table (inv(K) 3x3 | inv(E)[:3] | E[:3] | K)


def _divide(a, b):
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return float(numpy.float64(a) / numpy.float64(b))


def _length(v):
    """m = sqrt((v_x v_x + v_y v_y) + v_z v_z) and whether a normal can be formed from it (m > 0 and finite; a NaN fails)."""
    m = float(numpy.sqrt(numpy.float64((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
    return m, bool(m > 0.0 and m < math.inf)


# ---------------------------------------------------------------------------------------------------------------- a. the selection
def select_ray_samples(origins, dirs, z_vals, weights, min_weight=0.0):
    """snerf_ray_samples_count + snerf_ray_samples_emit -> (offsets int32 (R+1), sample int32 (M), points float32 (M,3))."""
    origins, dirs = numpy.asarray(origins, dtype=numpy.float32), numpy.asarray(dirs, dtype=numpy.float32)
    z_vals, weights = numpy.asarray(z_vals, dtype=numpy.float32), numpy.asarray(weights, dtype=numpy.float32)
    rays, samples = weights.shape
    offsets, sample, points = [0], [], []
    for r in range(rays):
        for i in range(samples):
            if float(weights[r, i]) > float(min_weight):                 # (false for a NaN)
                sample.append(r * samples + i)
                with numpy.errstate(all='ignore'):
                    points.append([origins[r, a] + dirs[r, a] * z_vals[r, i] for a in range(3)])      # float32: product, then sum
        offsets.append(len(sample))
    return (numpy.array(offsets, dtype=numpy.int32), numpy.array(sample, dtype=numpy.int32),
            numpy.array(points, dtype=numpy.float32).reshape(len(sample), 3))


# ---------------------------------------------------------------------------------------------------------------- b. the compositing
def inverse_input_point(Q, ndc):
    """The input map inverted -> (P: three floats, usable: Q_z < 1 and P_z <= -near)."""
    cx, cy, near = (float(v) for v in ndc)
    pz = _divide(2.0 * near, Q[2] - 1.0)
    P = [_divide(Q[0] * pz, cx), _divide(Q[1] * pz, cy), pz]
    return P, bool(Q[2] < 1.0 and pz <= -near)


def pull_back(P, g, ndc):
    """G = J^T g at P, the expression of snerf_field_normals (simplenerf_gradient.h)."""
    cx, cy, near = (float(v) for v in ndc)
    return [_divide(cx, P[2]) * g[0], _divide(cy, P[2]) * g[1],
            -_divide(((cx * P[0]) * g[0] + (cy * P[1]) * g[1]) + (2.0 * near) * g[2], P[2] * P[2])]


def sample_normal(Q, g, ndc=None):
    """-> (n: three floats in fp64, usable) of one selected sample."""
    with numpy.errstate(all='ignore'):
        usable, G = True, list(g)
        if ndc is not None:
            P, usable = inverse_input_point(Q, ndc)
            G = pull_back(P, g, ndc)
        m, formed = _length(G)
        if not (usable and formed):
            return [0.0, 0.0, 0.0], False
        return [_divide(-G[a], m) for a in range(3)], True


def composite_normals(points, grad, offsets, sample, weights, ndc=None):
    """snerf_composite_normals -> (normal float32 (R,3), strength float32 (R))."""
    points, grad = numpy.asarray(points, dtype=numpy.float32), numpy.asarray(grad, dtype=numpy.float32)
    flat = numpy.asarray(weights, dtype=numpy.float32).reshape(-1)
    rays = len(offsets) - 1
    normal, strength = numpy.zeros((rays, 3), dtype=numpy.float32), numpy.zeros((rays,), dtype=numpy.float32)
    for r in range(rays):
        A = [0.0, 0.0, 0.0]
        for k in range(int(offsets[r]), int(offsets[r + 1])):
            n, usable = sample_normal([float(v) for v in points[k]], [float(v) for v in grad[k]], ndc)
            if not usable:
                continue
            w = float(flat[int(sample[k])])
            for a in range(3):
                A[a] = A[a] + w * n[a]
        with numpy.errstate(all='ignore'):
            s, formed = _length(A)
            if formed:
                normal[r] = [numpy.float32(_divide(A[a], s)) for a in range(3)]
                strength[r] = numpy.float32(s)
    return normal, strength


# ---------------------------------------------------------------------------------------------------------------- c. depth normals
def is_valid(depth, mask, v, y, x) -> bool:
    d = depth[v, y, x]
    return bool(numpy.isfinite(d) and d > 0 and (mask is None or mask[v, y, x] != 0))


def point_of(row, x, y, d):
    """P = inv(E)[:3] [d inv(K) (x, y, 1); 1] from a view's row of the camera table, in the fuse's order of operations."""
    c = [d * ((row[3 * a] * float(x) + row[3 * a + 1] * float(y)) + row[3 * a + 2]) for a in range(3)]
    e = row[E_INV:E_INV + 12]
    return [((e[4 * a] * c[0] + e[4 * a + 1] * c[1]) + e[4 * a + 2] * c[2]) + e[4 * a + 3] for a in range(3)]


def _neighbour(depth, mask, row, v, x, y, d, edge_threshold):
    height, width = depth.shape[1:]
    if not (0 <= x < width and 0 <= y < height) or not is_valid(depth, mask, v, y, x):
        return None
    other = float(depth[v, y, x])
    if edge_threshold is not None and not abs(other - d) <= float(edge_threshold) * d:
        return None
    return point_of(row, x, y, other)


def _tangent(before, after, P):
    if before is None and after is None:
        return None
    if before is not None and after is not None:
        return [after[a] - before[a] for a in range(3)]
    if after is not None:
        return [after[a] - P[a] for a in range(3)]
    return [P[a] - before[a] for a in range(3)]


def depth_normals(depth, cameras, mask=None, edge_threshold=None):
    """snerf_depth_normals -> float32 (V,h,w,3).  ``cameras``: the (V,42) float64 table."""
    depth = numpy.asarray(depth, dtype=numpy.float32)
    cameras = numpy.asarray(cameras, dtype=numpy.float64)
    views, height, width = depth.shape
    out = numpy.zeros((views, height, width, 3), dtype=numpy.float32)
    for v in range(views):
        row = [float(t) for t in cameras[v]]
        centre = [row[E_INV + 4 * a + 3] for a in range(3)]
        for y in range(height):
            for x in range(width):
                if not is_valid(depth, mask, v, y, x):
                    continue
                d = float(depth[v, y, x])
                P = point_of(row, x, y, d)
                tx = _tangent(_neighbour(depth, mask, row, v, x - 1, y, d, edge_threshold),
                              _neighbour(depth, mask, row, v, x + 1, y, d, edge_threshold), P)
                ty = _tangent(_neighbour(depth, mask, row, v, x, y - 1, d, edge_threshold),
                              _neighbour(depth, mask, row, v, x, y + 1, d, edge_threshold), P)
                if tx is None or ty is None:
                    continue
                with numpy.errstate(all='ignore'):
                    c = [tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]]
                    m, formed = _length(c)
                    if not formed:
                        continue
                    n = [_divide(c[a], m) for a in range(3)]
                    facing = (n[0] * (centre[0] - P[0]) + n[1] * (centre[1] - P[1])) + n[2] * (centre[2] - P[2])
                    if facing < 0.0:
                        n = [-t for t in n]
                    out[v, y, x] = [numpy.float32(t) for t in n]
    return out


# ---------------------------------------------------------------------------------------------------------------- d. the picture
def normals_to_u8(normals, rotation=None):
    """snerf_normals_to_u8 -> uint8, the shape of ``normals`` (..., 3).  Integers from the floor on."""
    normals = numpy.asarray(normals, dtype=numpy.float32)
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]] if rotation is None else [[float(t) for t in r] for r in numpy.asarray(rotation)]
    flat = normals.reshape(-1, 3)
    out = numpy.zeros(flat.shape, dtype=numpy.uint8)
    for i in range(len(flat)):
        n = [float(t) for t in flat[i]]
        for a in range(3):
            with numpy.errstate(all='ignore'):
                c = (R[0][a] * n[0] + R[1][a] * n[1]) + R[2][a] * n[2]
                level = 127.5 * (c + 1.0) + 0.5
            if level != level:
                out[i, a] = 0
            elif level >= 256.0:
                out[i, a] = 255
            elif level < 0.0:
                out[i, a] = 0
            else:
                out[i, a] = min(255, max(0, int(math.floor(level))))
    return out.reshape(normals.shape)
