"""The mesh export on the CPU: the marching-tetrahedra table of csrc/mesh_tables.h against the one generated from the rule's
sentences, the restatement (tests/mesh_reference.py) on the analytic scene and on the fixtures -- a closed, oriented surface where
the volume is observed, holes where it is not, exact zeros --, the decision margins that let the GPU tests ask for exact equality,
the PLY writer, the header group of the binding and the native program's fixture."""
import ctypes
import os
import shutil
import subprocess

import numpy
import pytest

from simplenerf_amd import _lib, build, geometry

from . import mesh_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9                       # a node decided closer than this to a rounding tie or to -mu may be left out of a comparison


# ------------------------------------------------------------------------------------------------------------------ the table
@pytest.fixture(scope='module')
def compiled_tables(tmp_path_factory):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert compiler, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('mesh_tables') / 'mesh_tables_host')
    r = subprocess.run([compiler, '-std=c++17', '-O1', os.path.join(REPO, 'tests', 'native', 'mesh_tables_host.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        name, *numbers = line.split()
        rows.setdefault(name, []).append([int(v) for v in numbers])
    return rows


def test_compiled_table_equals_the_generated_one(compiled_tables):
    code = lambda offset: offset[0] | offset[1] << 1 | offset[2] << 2
    assert compiled_tables['vertex'] == [[t] + [code(v) for v in ref.tetrahedron(t)] for t in range(6)]
    assert compiled_tables['type'] == sorted([code(offset), kind] for offset, kind in ref.EDGE_TYPES.items())
    assert compiled_tables['offset'] == [[kind, code(ref.OFFSET_OF_TYPE[kind])] for kind in range(7)]
    table = ref.table()
    assert len(compiled_tables['case']) == 96
    for t, case, count, *edges in compiled_tables['case']:
        want = table[t][case]
        assert count == len(want), (t, case)
        assert edges[:3 * count] == [4 * m + m2 for triangle in want for m, m2 in triangle], (t, case)
        assert edges[3 * count:] == [0] * (6 - 3 * count)
    assert sorted((t, case) for t, case, *_ in compiled_tables['case']) == [(t, case) for t in range(6) for case in range(16)]


def test_generated_table_follows_its_sentences():
    """Counts per case, edges between nodes of different sign only, each such edge used, and the winding of a +-1 field."""
    for t in range(6):
        assert ref.tetrahedron(t)[0] == (0, 0, 0) and ref.tetrahedron(t)[3] == (1, 1, 1)
        for case in range(16):
            triangles = ref.table()[t][case]
            negatives = bin(case).count('1')
            assert len(triangles) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[negatives]
            crossing = {(m, m2) for m in range(4) for m2 in range(m + 1, 4) if (case >> m & 1) != (case >> m2 & 1)}
            assert {edge for triangle in triangles for edge in triangle} == crossing
            if len(triangles) == 1:                                                # the opposite signs: the same triangle, turned over
                assert [(a, c, b) for a, b, c in triangles] == list(ref.table()[t][15 - case])
    assert ref.table()[0] == ref.table()[3] == ref.table()[4] and ref.table()[1] == ref.table()[2] == ref.table()[5]


# ------------------------------------------------------------------------------------------------------------------ the scene
def test_scene_and_its_margins():
    s = ref.scene()
    assert s['depth'].shape == (6, 48, 48) and s['depth'].dtype == numpy.float32 and s['image'].shape == (6, 48, 48, 3)
    hit = s['depth'] != ref.SCENE_MISS
    assert 0.3 < hit.mean() < 0.6 and s['depth'][hit].min() > 2.9 and s['depth'][hit].max() < 4.1
    assert not s['image'][~hit].any() and s['image'][hit].any()
    for extrinsic, eye in zip(s['extrinsics'], ref.SCENE_EYES):
        assert numpy.allclose(numpy.matmul(extrinsic[:3, :3], extrinsic[:3, :3].T), numpy.eye(3), atol=1e-14)
        assert numpy.allclose(numpy.matmul(extrinsic, numpy.append(eye, 1.0))[:3], 0.0, atol=1e-14)
        assert numpy.matmul(extrinsic, [0.0, 0.0, 0.0, 1.0])[2] > 0                  # the origin lies in front of every camera
    tsdf, weight, margins = ref.scene_volume()
    assert tsdf.shape == (25, 25, 25) and tsdf.dtype == numpy.float32 and weight.dtype == numpy.uint8
    # the conditions under which the GPU test asks for the exact volume: no decision within 1e-9 of a tie or of -mu
    assert abs(margins['tie'].min() - 2.0e-6) < 1e-7 and abs(margins['behind'].min() - 9.6e-6) < 1e-7
    assert margins['tie'].min() >= MARGIN and margins['behind'].min() >= MARGIN
    assert abs(numpy.abs(tsdf[weight > 0]).min() - 1.9e-3) < 1e-4
    assert numpy.bincount(weight.ravel(), minlength=7).tolist() == [356, 496, 1233, 4843, 5127, 3380, 190]
    assert (tsdf[weight == 0] == 1.0).all() and tsdf.max() <= 1.0 and tsdf.min() >= -1.0


def test_vectorised_integration_equals_the_looped_one():
    """The whole-slab numpy evaluation (the host side of tools/measure_mesh.py) gives the looped restatement's volume bit for bit:
    x + 0.0 is x, so adding a skipped view's zero changes no sum."""
    s = ref.scene()
    tsdf, weight, _ = ref.scene_volume()
    fast = ref.tsdf_integrate_vectorised(s['depth'], s['extrinsics'], s['intrinsics'], ref.GRID_LO, ref.GRID_VOXEL, ref.GRID_EXTENTS, ref.GRID_MU)
    assert fast[0].tobytes() == tsdf.tobytes() and fast[1].tobytes() == weight.tobytes()


def test_restatement_on_the_scene_gives_a_closed_oriented_surface():
    vertices, triangles, keys, cases = ref.scene_mesh()
    assert vertices.dtype == numpy.float32 and triangles.dtype == numpy.int32 and triangles.min() == 0 and triangles.max() == len(vertices) - 1
    stats = ref.assert_closed_oriented_surface(vertices, triangles)
    assert (stats['vertices'], stats['edges'], stats['faces']) == (3736, 11202, 7468)
    radii = numpy.linalg.norm(vertices.astype(numpy.float64), axis=1)
    assert 0.87 <= radii.min() and radii.max() <= 1.11
    # normals look out of the sphere, from the negative side to the positive one: the enclosed volume is positive, near 4 pi / 3
    p = vertices.astype(numpy.float64)
    volume = (p[triangles[:, 0]] * numpy.cross(p[triangles[:, 1]], p[triangles[:, 2]])).sum() / 6
    assert 0.9 * 4.19 < volume < 1.1 * 4.19, volume
    assert (numpy.diff(keys) > 0).all()


def test_a_short_truncation_leaves_holes():
    vertices, triangles, _, _ = ref.scene_mesh(0.25)
    stats = ref.surface_statistics(vertices, triangles)
    assert (stats['vertices'], stats['faces'], stats['boundary_edges']) == (3500, 6682, 440)
    assert stats['irregular_edges'] == 0 and stats['misoriented'] == 0 and stats['zero_area'] == 0


def test_min_weight_two_and_the_slab_grid():
    vertices, triangles, _, _ = ref.scene_mesh(ref.GRID_MU, 2)
    stats = ref.surface_statistics(vertices, triangles)
    assert 0 < stats['faces'] < 7468 and stats['boundary_edges'] > 0 and stats['misoriented'] == 0
    # 25 x 21 x 23 nodes with lo moved by whole voxels (0.25 = 2 and 0.125 = 1): node positions are the cube's wherever the sums round
    # alike, and every vertex of the sphere lies inside the slab: the same set of positions to an ulp.  (The keys differ; the ORDER does
    # not: a box cut out of a grid keeps the (k, j, i) order of its nodes.)
    slab = ref.scene_mesh(ref.GRID_MU, 1, ref.SLAB_EXTENTS, ref.SLAB_LO)
    cube = ref.scene_mesh()
    assert len(slab[0]) == len(cube[0]) == 3736 and len(slab[1]) == len(cube[1])
    ref.assert_closed_oriented_surface(slab[0], slab[1])
    order = lambda v: v[numpy.lexsort((v[:, 0], v[:, 1], v[:, 2]))]
    assert numpy.abs(order(slab[0]).astype(numpy.float64) - order(cube[0])).max() <= 2.0 ** -22
    assert not numpy.array_equal(slab[2], cube[2]) and numpy.array_equal(slab[1], cube[1])


# ------------------------------------------------------------------------------------------------------------------ other fixtures
def test_random_field_meets_every_case_and_is_consistent_inside():
    tsdf, weight = ref.random_field()
    vertices, triangles, keys, cases = ref.extract_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    assert len(cases) == 96                                                            # the seed is chosen for this
    assert (len(vertices), len(triangles)) == (522, 868)
    violations, looked_at = ref.interior_edge_violations(triangles, keys, ref.FIELD_EXTENTS)
    assert (violations, looked_at) == (0, 2390)
    assert numpy.isfinite(vertices).all() and vertices.min() >= 0 and (vertices.max(axis=0) <= [6, 5, 4]).all()


def test_random_field_with_holes():
    tsdf, weight = ref.random_field(holes=True)
    assert 0.05 < (weight == 0).mean() < 0.25
    vertices, triangles, keys, _ = ref.extract_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    full = ref.extract_mesh(*ref.random_field(), (0.0, 0.0, 0.0), 1.0)
    assert 0 < len(triangles) < len(full[1]) and 0 < len(vertices) < len(full[0])
    assert set(keys.tolist()) < set(full[2].tolist())                                   # fewer complete cells: a subset of the vertices
    assert ref.surface_statistics(vertices, triangles)['misoriented'] == 0


def test_a_plane_through_grid_nodes():
    tsdf, weight = ref.plane_field()
    vertices, triangles, _, _ = ref.extract_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    assert len(vertices) == 63 and (vertices[:, 0] == 3.0).all()
    stats = ref.surface_statistics(vertices, triangles)
    assert (stats['faces'], stats['zero_area']) == (96, 72)
    p = vertices.astype(numpy.float64)
    normals = numpy.cross(p[triangles[:, 1]] - p[triangles[:, 0]], p[triangles[:, 2]] - p[triangles[:, 0]])
    assert (normals[:, 0] >= 0).all() and (normals[:, 1:] == 0).all()                 # the others wind towards +x, the positive side


def test_degenerate_volumes_give_nothing():
    for shape in ((1, 4, 5), (3, 1, 5), (3, 4, 1), (1, 1, 1)):
        tsdf = numpy.where(numpy.arange(numpy.prod(shape)).reshape(shape) % 2 == 0, -0.5, 0.5).astype(numpy.float32)
        vertices, triangles, _, _ = ref.extract_mesh(tsdf, numpy.ones(shape, numpy.uint8), (0.0, 0.0, 0.0), 1.0)
        assert len(vertices) == 0 and len(triangles) == 0
    tsdf, weight = ref.random_field()
    assert [len(a) for a in ref.extract_mesh(numpy.abs(tsdf), weight, (0.0, 0.0, 0.0), 1.0)[:2]] == [0, 0]
    assert [len(a) for a in ref.extract_mesh(tsdf, numpy.zeros_like(weight), (0.0, 0.0, 0.0), 1.0)[:2]] == [0, 0]


def test_restated_colours_of_the_scene():
    colours, views, margins = ref.scene_colours()
    vertices = ref.scene_mesh()[0]
    assert abs(min(margins) - 5.8e-6) < 1e-7 and min(margins) >= MARGIN
    assert int((views == 0).sum()) == 40 and not colours[views == 0].any() and views.max() <= 6
    seen = views > 0
    wanted = numpy.clip(numpy.rint(127.5 + 127.5 * vertices[seen].astype(numpy.float64)), 0, 255)
    assert numpy.abs(colours[seen].astype(numpy.float64) - wanted).max() <= 30        # a neighbouring pixel's colour, a voxel away


# ------------------------------------------------------------------------------------------------------------------ the file
def test_ply_mesh_bytes_parse_back():
    vertices, triangles = ref.scene_mesh()[:2]
    colours = ref.scene_colours()[0]
    data = geometry.ply_mesh_bytes(vertices, colours, triangles)
    header = (b'ply\nformat binary_little_endian 1.0\nelement vertex 3736\nproperty float x\nproperty float y\nproperty float z\n'
              b'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 7468\n'
              b'property list uchar int vertex_indices\nend_header\n')
    assert data.startswith(header) and len(data) == len(header) + 3736 * 15 + 7468 * 13
    assert data[:len(header) + 3736 * 15].replace(b'element face 7468\nproperty list uchar int vertex_indices\n', b'') == \
        geometry.ply_bytes(vertices, colours)
    face = numpy.dtype([('count', 'u1'), ('a', '<i4'), ('b', '<i4'), ('c', '<i4')])
    assert face.itemsize == 13
    faces = numpy.frombuffer(data[len(header) + 3736 * 15:], dtype=face)
    assert (faces['count'] == 3).all()
    assert numpy.array_equal(numpy.stack([faces['a'], faces['b'], faces['c']], axis=1), triangles)
    no_faces = geometry.ply_mesh_bytes(vertices, colours, numpy.zeros((0, 3), numpy.int32))
    assert no_faces == header.replace(b'face 7468', b'face 0') + data[len(header):len(header) + 3736 * 15]
    empty = geometry.ply_mesh_bytes(numpy.zeros((0, 3), numpy.float32), numpy.zeros((0, 3), numpy.uint8), numpy.zeros((0, 3), numpy.int32))
    assert empty == header.replace(b'vertex 3736', b'vertex 0').replace(b'face 7468', b'face 0')
    with pytest.raises(RuntimeError, match='triangles'):
        geometry.ply_mesh_bytes(vertices, colours, triangles.astype(numpy.int64))
    with pytest.raises(RuntimeError, match='triangles'):
        geometry.ply_mesh_bytes(vertices, colours, triangles[:, :2])
    with pytest.raises(RuntimeError, match='points'):
        geometry.ply_mesh_bytes(vertices.astype(numpy.float64), colours, triangles)
    with pytest.raises(RuntimeError, match='colours'):
        geometry.ply_mesh_bytes(vertices, colours.astype(numpy.int32), triangles)


def test_save_ply_mesh_leaves_an_existing_file_alone(tmp_path):
    vertices, triangles = ref.scene_mesh()[:2]
    colours = ref.scene_colours()[0]
    path = tmp_path / 'meshes' / 'scene.ply'
    geometry.save_ply_mesh(path, vertices, colours, triangles)
    assert path.read_bytes() == geometry.ply_mesh_bytes(vertices, colours, triangles)
    geometry.save_ply_mesh(path, vertices, colours, triangles[:5])
    assert path.read_bytes() == geometry.ply_mesh_bytes(vertices, colours, triangles)


# ------------------------------------------------------------------------------------------------------------------ ABI and binding
def test_mesh_header_is_the_bindings_next_group():
    assert [os.path.relpath(path, REPO) for path in _lib.MESH_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_mesh.h')]
    assert set(_lib.MESH_SIGNATURES) == {'snerf_tsdf_integrate', 'snerf_mesh_workspace_bytes', 'snerf_mesh_count', 'snerf_mesh_emit',
                                         'snerf_colour_points'}
    earlier = set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.SWEEP16_SIGNATURES) \
        | set(_lib.PNG_SIGNATURES) | set(_lib.JPEG_SIGNATURES) | set(_lib.FUSE_SIGNATURES)
    assert not earlier & set(_lib.MESH_SIGNATURES)
    grid = [ctypes.c_double] * 4 + [ctypes.c_int] * 3
    assert _lib.MESH_SIGNATURES['snerf_mesh_workspace_bytes'] == (ctypes.c_longlong, [ctypes.c_int] * 3)
    assert _lib.MESH_SIGNATURES['snerf_tsdf_integrate'] == (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + grid + [ctypes.c_double]
                                                            + [ctypes.c_void_p] * 3)
    assert _lib.MESH_SIGNATURES['snerf_mesh_count'] == (ctypes.c_int, [ctypes.c_void_p] * 2 + grid + [ctypes.c_int] + [ctypes.c_void_p] * 3)
    assert _lib.MESH_SIGNATURES['snerf_mesh_emit'] == (ctypes.c_int, [ctypes.c_void_p] * 2 + grid + [ctypes.c_int] + [ctypes.c_void_p] * 5)
    assert _lib.MESH_SIGNATURES['snerf_colour_points'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_void_p] * 4
                                                           + [ctypes.c_int] * 3 + [ctypes.c_double] + [ctypes.c_void_p] * 3)
    assert _lib.C.SNERF_MESH_KEYS_PER_NODE == 7 and _lib.C.SNERF_FUSE_CAMERA_DOUBLES == 42 and _lib.ABI_VERSION == 10


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_mesh_symbols_are_exported():
    build.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.MESH_SIGNATURES:
        assert hasattr(lib, name), name


def test_native_fixture_layout():
    data = ref.native_fixture()
    views, h, w, nx, ny, nz, min_weight = numpy.frombuffer(data[:28], '<i4').tolist()
    assert (views, h, w, nx, ny, nz, min_weight) == (6, 48, 48, 25, 25, 25, 1)
    assert numpy.frombuffer(data[28:76], '<f8').tolist() == [0.125, -1.51, -1.49, -1.503, 0.5, 0.125]
    total, nodes, nv, nt = views * h * w, nx * ny * nz, 3736, 7468
    assert len(data) == 28 + 48 + views * 42 * 8 + total * 4 + total * 3 + nodes * 5 + 16 + nv * 12 + nt * 12 + nv * 4
    at = 76 + views * 42 * 8 + total * 7 + nodes * 5
    assert numpy.frombuffer(data[at:at + 16], '<i8').tolist() == [nv, nt]


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_mesh_abi_program_compiles_and_links(tmp_path):
    """CPU-side half of the native smoke: the new header is valid C++ for an outside consumer and the five symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'mesh_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}',
           os.path.join(REPO, 'tests', 'native', 'mesh_abi_smoke.cpp'), '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip',
           f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe
