"""Numpy restatement of the scene kernels (csrc/scene.hip), operation for operation: what the reference's DataPreprocessor computes
per pixel at start-up (src/data_preprocessors/DataPreprocessor01.py :163-185, :448-478, :929-935).  tests/test_scene_host.py holds it
to the fixtures made by RUNNING the reference (tools/make_golden_scene.py); tests/test_gpu_scene.py uses it where no fixture exists
(points in reversed order, empty inputs)."""
import numpy


def prepare_images(images: numpy.ndarray, white_bkgd: bool) -> numpy.ndarray:
    """(V,h,w,C) uint8 -> (V,h,w,3) float32."""
    f = images.astype(numpy.float32) / numpy.float32(255)
    if not white_bkgd:
        return f[..., :3]
    alpha = f[..., -1:]
    return f[..., :3] * alpha + (numpy.float32(1) - alpha)


def rasterise(x, y, depth, error, view, num_views: int, height: int, width: int, scale=1.0, divisor=1.0):
    """-> (depths, errors), float32 (V*h*w,): the LAST point in input order wins a pixel, -1 where there is none.  Written as an
    explicit loop over points in input order, so that the rule does not rest on numpy's fancy assignment."""
    depths = -numpy.ones((num_views, height, width))
    errors = -numpy.ones((num_views, height, width))
    px = numpy.clip(numpy.round(numpy.asarray(x, dtype=numpy.float64) / divisor), 0, width - 1).astype(numpy.int64)
    py = numpy.clip(numpy.round(numpy.asarray(y, dtype=numpy.float64) / divisor), 0, height - 1).astype(numpy.int64)
    scaled = numpy.asarray(depth, dtype=numpy.float64) * scale
    for p in range(len(px)):
        depths[view[p], py[p], px[p]] = scaled[p]
        errors[view[p], py[p], px[p]] = error[p]
    return depths.reshape(-1).astype(numpy.float32), errors.reshape(-1).astype(numpy.float32)


def pixel_rays_z(intrinsics: numpy.ndarray, poses: numpy.ndarray, height: int, width: int):
    """(oz, dz), float32 (V*h*w,): the z of every pixel's world ray, get_rays' arithmetic (:351-368) in float32."""
    xs, ys = numpy.meshgrid(numpy.arange(width, dtype=numpy.float32), numpy.arange(height, dtype=numpy.float32), indexing='xy')
    homo = numpy.stack([xs, ys, numpy.ones_like(xs)], axis=2)
    oz, dz = [], []
    for k, pose in zip(intrinsics.astype(numpy.float32), poses.astype(numpy.float32)):
        dirs = (numpy.linalg.inv(k)[None, None] @ homo[:, :, :, None])[:, :, :, 0]
        dirs[:, :, 1:] *= -1
        rays_d = numpy.sum(dirs[..., numpy.newaxis, :] * pose[:3, :3], -1)
        dz.append(rays_d[..., 2].astype(numpy.float32))
        oz.append(numpy.full((height, width), pose[2, 3], dtype=numpy.float32))
    return numpy.stack(oz).reshape(-1), numpy.stack(dz).reshape(-1)


def depth_to_ndc(depths: numpy.ndarray, oz: numpy.ndarray, dz: numpy.ndarray, near) -> numpy.ndarray:
    """convert_depth_to_ndc (:455-463) in float32, then -1 where the depth is -1."""
    depths = depths.astype(numpy.float32)
    near = numpy.float32(near)
    tn = -(near + oz) / dz
    oz_prime = oz + tn * dz
    with numpy.errstate(divide='ignore', invalid='ignore'):
        ndc = numpy.float32(1) - oz_prime / (oz_prime + (depths - tn) * dz)
    ndc[depths == -1] = -1
    return ndc.astype(numpy.float32)


CASES = ('ndc_sparse', 'world_dense', 'ndc_both')
SPARSE_CASES, DENSE_CASES = ('ndc_sparse', 'ndc_both'), ('world_dense', 'ndc_both')
COLUMNS = ('x', 'y', 'depth', 'reprojection_error')


def load_case(name: str):
    """-> (fixture arrays, configs, raw_data_dict) of tests/golden/scene_prep_<name>.npz; the raw dictionary is rebuilt in the
    loader's layout, sparse tables as plain dicts of arrays."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', f'scene_prep_{name}.npz')
    with numpy.load(path, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    configs = json.loads(str(g['configs_json']))
    raw = {'frame_nums': g['raw_frame_nums'].copy(),
           'nerf_data': {k: g[f'raw_{k}'].copy() for k in ('images', 'extrinsics', 'intrinsics', 'bounds')}}
    raw['nerf_data']['resolution'] = tuple(int(x) for x in g['raw_resolution'])
    frames = sorted({int(k.split('_')[2]) for k in g if k.startswith('raw_sparse_')})
    if frames:
        raw['sparse_depth_data'] = {f: {c: g[f'raw_sparse_{f}_{c}'].copy() for c in COLUMNS} for f in frames}
    if 'raw_dense_depth_values' in g:
        raw['dense_depth_data'] = {k: g[f'raw_dense_{k}'].copy() for k in ('depth_values', 'depth_weights')}
    return g, configs, raw


def bits(a) -> numpy.ndarray:
    """The float32 bit patterns, for comparisons that must not forgive a -0.0 or a NaN payload."""
    return numpy.ascontiguousarray(numpy.asarray(a, dtype=numpy.float32)).view(numpy.uint32)
