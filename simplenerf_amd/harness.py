"""Minimal counterpart of the reference's Tester call path around the model (last row):
full-frame input batch -> ``model(batch)`` under no_grad -> display post-processing, plus the ray-sharded
multi-GPU variant (one process per GPU, contiguous block of rays per rank, one gather of the per-ray outputs).

Reference call sites restated here: DataPreprocessor.create_test_data (src/data_preprocessors/DataPreprocessor01.py
:807-895), NerfTester.predict_frame (src/Tester01.py:57-66), post_process_image/depth (:1106-1114), and the trainer's two
frame loops, Trainer.run_validation (src/Trainer01.py:109-263) and save_sample_images (:319-350), at the end of this file.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Iterable, Optional, Tuple

import numpy
import torch

from . import _lib, ops
from .models.SimpleNeRFHip01 import global_rows

Tensor = torch.Tensor
DEFAULT_KEYS = ('rgb_fine', 'depth_fine', 'depth_var_fine')
# Stream-capture mode of the two graphed steps below.  torch's default, 'global', makes EVERY thread's capture-unsafe HIP call
# fail while the capture is open -- and with a process group alive, torch.distributed's NCCL watchdog thread polls the events of
# earlier collectives (hipEventQuery) whenever it likes: if a poll falls inside the capture window the watchdog dies with
# hipErrorStreamCaptureUnsupported and takes the process with it (round 5: one of three `bench.py --extras` runs, in the
# rank-share leg, right after an eager all-reduce).  'thread_local' confines the check to the capturing thread, whose calls are
# the stream-ordered launches the capture is there to record.
CAPTURE_MODE = 'thread_local'


def shard_range(num_rays: int, rank: int, world_size: int) -> Tuple[int, int]:
    """Contiguous block partition: rank r owns rays [r*ceil(N/R), min(N, (r+1)*ceil(N/R)))  (SURVEY 8e)."""
    per = -(-num_rays // world_size)
    first = min(num_rays, rank * per)
    return first, min(num_rays, first + per) - first


_columns: Dict[tuple, Tensor] = {}


def _constant_column(value: float, rows: int, device: torch.device) -> Tensor:
    """(rows,1) tensor filled with ``value`` (the near/far columns of a frame's batch are constants: built once per
    value and size, shared read-only between batches instead of being re-filled every step)."""
    key = (value, rows, device)
    col = _columns.get(key)
    if col is None:
        if len(_columns) > 64:
            _columns.clear()
        col = _columns[key] = torch.full((rows, 1), value, dtype=torch.float32, device=device)
    return col


def frame_batch(camera: dict, ndc: bool, device, first_ray: int = 0, num_rays: Optional[int] = None,
                view_camera: Optional[dict] = None, secondary_cameras: Optional[Iterable[dict]] = None) -> Dict[str, Tensor]:
    """Input dictionary for rays [first_ray, first_ray+num_rays) of a frame, generated on the device (K1).

    ``view_camera`` (a dict like ``camera``): ``view_dirs`` are those of that camera's rays through the same pixels -- the
    reference's ``create_test_data(pose, view_pose, ..., view_intrinsic)`` (src/data_preprocessors/DataPreprocessor01.py:832-843).
    ``secondary_cameras``: adds ``rays_o2`` (n, K, 3), every secondary camera's centre repeated per ray (:871-885)."""
    h, w = camera['resolution']
    if num_rays is None:
        num_rays = h * w - first_ray
    batch = ops.generate_rays((h, w), camera['intrinsic'], camera['pose'], camera['near'], ndc, device, first_ray, num_rays)
    if view_camera is not None:
        batch['view_dirs'] = view_directions(camera, view_camera, device, first_ray, num_rays)
    col = lambda v: _constant_column(float(v), num_rays, torch.device(device))
    batch['near'], batch['far'] = col(camera['near']), col(camera['far'])
    if ndc:
        batch['near_ndc'], batch['far_ndc'] = col(camera.get('near_ndc', 0.0)), col(camera.get('far_ndc', 1.0))
    if secondary_cameras is not None:
        import numpy
        centres = numpy.array([numpy.asarray(c['pose'], dtype=numpy.float32)[:3, 3] for c in secondary_cameras],
                              dtype=numpy.float32).reshape(-1, 3)                                                  # (K,3)
        batch['rays_o2'] = torch.from_numpy(centres).to(device)[None].expand(num_rays, -1, -1).contiguous()
    return batch


def view_directions(camera: dict, view_camera: dict, device, first_ray: int = 0, num_rays: Optional[int] = None) -> Tensor:
    """(n,3) unit directions of ``view_camera``'s rays through pixels [first_ray, first_ray+num_rays) of ``camera``'s frame: a ray
    generation of which only the view directions are kept (they do not depend on ``ndc`` or ``near``)."""
    return ops.generate_rays(camera['resolution'], view_camera['intrinsic'], view_camera['pose'], camera['near'], False, device,
                             first_ray, num_rays)['view_dirs']


@torch.no_grad()
def render_rays_blockwise(model, camera: dict, ndc: bool, device, first_ray: int, num_rays: int,
                          keys: Iterable[str] = DEFAULT_KEYS, ray_block: int = 65536, view_camera: Optional[dict] = None) -> Dict[str, Tensor]:
    """Render a ray range in blocks (bounding the per-sample buffers), keeping only ``keys``.  ``view_camera``: as ``frame_batch``."""
    keys = tuple(keys)
    pieces = {k: [] for k in keys}
    # a rank that owns no rays (ceil-division shards of a tiny frame) still runs one zero-ray call, so that its
    # outputs have the right trailing shapes for the gather
    for start in (range(first_ray, first_ray + num_rays, ray_block) if num_rays > 0 else (first_ray,)):
        count = min(ray_block, first_ray + num_rays - start)
        out = model(frame_batch(camera, ndc, device, start, count, view_camera=view_camera))
        for k in keys:
            pieces[k].append(out[k])
    return {k: torch.cat(v, 0) for k, v in pieces.items()}


def gather_rays(local: Dict[str, Tensor], num_rays: int, rank: int, world_size: int, dst: int = 0,
                group=None) -> Optional[Dict[str, Tensor]]:
    """One gather of the per-ray outputs of every rank's block to ``dst`` (all keys packed into one buffer, so it
    is a single collective).  Returns the full-frame tensors on ``dst`` and None elsewhere."""
    import torch.distributed as dist
    per = -(-num_rays // world_size)
    keys = sorted(local)
    # (rows, width) view of each key; a zero-row tensor keeps its trailing shape (reshape(0, -1) is ambiguous)
    cols = [local[k].reshape(local[k].shape[0], int(torch.Size(local[k].shape[1:]).numel())) for k in keys]
    widths = [c.shape[1] for c in cols]
    packed = torch.cat(cols, 1) if cols else torch.empty((0, 0))
    pad = torch.zeros((per, packed.shape[1]), dtype=packed.dtype, device=packed.device)
    pad[:packed.shape[0]] = packed
    bucket = [torch.empty_like(pad) for _ in range(world_size)] if rank == dst else None
    dist.gather(pad, bucket, dst=dst, group=group)
    if rank != dst:
        return None
    full = torch.cat(bucket, 0)[:num_rays]
    out, c0 = {}, 0
    for k, wdt in zip(keys, widths):
        out[k] = full[:, c0:c0 + wdt].reshape((num_rays,) + tuple(local[k].shape[1:]))
        c0 += wdt
    return out


@torch.no_grad()
def render_frame(model, camera: dict, ndc: bool, device, keys: Iterable[str] = DEFAULT_KEYS, rank: int = 0,
                 world_size: int = 1, ray_block: int = 65536, collective: Optional[bool] = None,
                 view_camera: Optional[dict] = None) -> Optional[Dict[str, Tensor]]:
    """Full frame, (h*w, .) per key.  With world_size > 1 every rank renders its block and rank 0 receives the
    frame through one gather (returns None on the other ranks).  ``collective=True`` issues that gather with a single rank
    too (a one-rank process group: the RCCL call path of the multi-GPU run on a one-GPU box).  ``view_camera``: as ``frame_batch``."""
    h, w = camera['resolution']
    n = h * w
    first, count = shard_range(n, rank, world_size)
    local = render_rays_blockwise(model, camera, ndc, device, first, count, keys, ray_block, view_camera)
    if not (world_size > 1 if collective is None else collective):
        return local
    return gather_rays(local, n, rank, world_size)


def to_display(rgb: Tensor, depth: Tensor):
    """clip -> round(255 x) -> uint8 colour; depth clipped at 0 (post_process_image / post_process_depth), fused on
    the device so that a frame is copied to the host as 3 B/pixel."""
    return ops.to_display(rgb, depth)


def retrieve_inference_outputs(configs: dict, resolution, network_outputs: Dict[str, Tensor]) -> dict:
    """What leaves the device after a frame and in what form: DataPreprocessor.retrieve_inference_outputs
    (src/data_preprocessors/DataPreprocessor01.py:897-925).  The reference copies EVERY network output to the host
    (post_process_output, incl. ~1 KB/ray of alpha) and then keeps five of them; here only those five are converted on the
    device (K: snerf_to_display -- uint8 colour, depths clipped at 0) and copied: 3 + 16 B per pixel.

    Returns numpy arrays under the reference's keys, in its order: ``image`` (h,w,3) uint8, ``depth``, ``depth_var``
    (h,w) float32 and, for NDC scenes, ``depth_ndc``, ``depth_var_ndc``; the suffix is ``_fine`` when the model has a
    fine MLP, else ``_coarse`` (:900-905); ``visibility2`` (nf-1, h, w) float32 when the outputs carry it
    (predict_visibility with secondary views, :919-924)."""
    return {k: v.cpu().numpy() for k, v in display_outputs(configs, resolution, network_outputs).items()}


def display_outputs(configs: dict, resolution, network_outputs: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """``retrieve_inference_outputs`` before the copy to the host: the same keys, as device tensors."""
    h, w = int(resolution[0]), int(resolution[1])
    if 'fine_mlp' in configs['model']:
        suffix = '_fine'
    elif 'coarse_mlp' in configs['model']:
        suffix = '_coarse'
    else:
        raise RuntimeError('retrieve_inference_outputs: the model has neither a fine nor a coarse MLP')
    image, depth = ops.to_display(network_outputs[f'rgb{suffix}'].reshape(h * w, 3), network_outputs[f'depth{suffix}'].reshape(h * w))
    out = {'image': image.reshape(h, w, 3), 'depth': depth.reshape(h, w)}
    names = ['depth_var'] + (['depth_ndc', 'depth_var_ndc'] if configs['data_loader']['ndc'] else [])
    for name in names:
        out[name] = ops.to_display(network_outputs[f'rgb{suffix}'].reshape(h * w, 3),
                                   network_outputs[f'{name}{suffix}'].reshape(h * w), colour=False)[1].reshape(h, w)
    if f'visibility2{suffix}' in network_outputs:
        vis2 = network_outputs[f'visibility2{suffix}'].reshape(h, w, -1).permute(2, 0, 1).contiguous()
        out['visibility2'] = vis2.float()                          # post_process_visibility: a float32 cast (:1116-1119)
    return out


@torch.no_grad()
def predict_frame(model, configs: dict, camera: dict, device, rank: int = 0, world_size: int = 1,
                  ray_block: int = 65536, collective: Optional[bool] = None, view_camera: Optional[dict] = None) -> Optional[dict]:
    """NerfTester.predict_frame (src/Tester01.py:57-66): full-frame batch -> model under no_grad -> the five display
    outputs.  Rays are generated on the device per block; with world_size > 1 each rank renders its block of the frame
    and rank 0 receives it through one gather (None on the other ranks).  ``view_camera``: as ``frame_batch``."""
    ndc = bool(configs['data_loader']['ndc'])
    suffix = '_fine' if 'fine_mlp' in configs['model'] else '_coarse'
    keys = [f'rgb{suffix}', f'depth{suffix}', f'depth_var{suffix}'] + ([f'depth_ndc{suffix}', f'depth_var_ndc{suffix}'] if ndc else [])
    frame = render_frame(model, camera, ndc, device, keys, rank, world_size, ray_block, collective, view_camera)
    if frame is None:
        return None
    return retrieve_inference_outputs(configs, camera['resolution'], frame)


NORMALS_RAY_BLOCK = 1 << 14      # rays per block of predict_normals: see its docstring for the arithmetic


def _gradient_field(what: str, model, configs: dict):
    """(model unwrapped, the displayed level's MLP name) of a call that needs ``model.query_gradient``; raises what that would raise
    -- NotImplementedError naming the limit, for a ``predict_visibility`` MLP and for a layered shape -- before the caller renders."""
    model = getattr(model, 'module', model) if isinstance(model, torch.nn.DataParallel) else model
    mlp = 'fine_mlp' if 'fine_mlp' in configs['model'] else 'coarse_mlp'
    if not hasattr(model, 'check_query_gradient'):
        raise NotImplementedError(f'{what}: the model has no query_gradient')
    model.check_query_gradient(mlp)
    return model, mlp


@torch.no_grad()
def predict_normals(model, configs: dict, camera: dict, device, ray_block: int = NORMALS_RAY_BLOCK, min_weight: float = 0.0,
                    gradient_block: int = 1 << 16, edge_threshold: Optional[float] = None) -> dict:
    """The two normal maps of a rendered frame, the standard picture for judging a NeRF's geometry.  The frame is rendered in blocks
    of ``ray_block`` rays at the model's precision with ``retraw=True``, for the displayed level (the fine one when there is one).
    Per block the samples whose weight exceeds ``min_weight`` are selected with the points the MLP saw (the NDC rays and depths for a
    model of NDC rays), ``model.query_gradient`` gives the density's gradient there, and every ray sums weight x unit normal over its
    samples (``geometry.ray_normals``).  ``query_gradient`` is ALWAYS fp32 on the master weights, whatever the model's
    ``hip_precision``: a 16-bit model gets its own weights composited with the fp32 field's normals.  Then the depth normals of the
    frame's own displayed depth map (``geometry.depth_normals`` with the camera's matrices; ``edge_threshold`` as there).  Where the
    two maps disagree, the density is not a surface yet.

    Returns device tensors: 'normal' float32 (h,w,3) and 'normal_strength' float32 (h,w) (the length of the weighted sum: at most
    the sum of the selected weights), 'depth_normal' float32 (h,w,3), both in the scene frame; 'normal_image', 'depth_normal_image'
    uint8 (h,w,3), the maps in the camera's frame as ``geometry.normals_to_u8`` draws them (for ``save_image`` / ``png_files`` /
    ``save_video``); 'depth' float32 (h,w), the displayed depth; and 'selected_fraction', the share of the frame's samples that
    were selected (a float).

    A model that ``query_gradient`` refuses -- a layered MLP shape, ``predict_visibility`` -- is refused here with the same
    NotImplementedError before anything is rendered.  A ``DataParallel`` wrapper is unwrapped.

    ``ray_block``: a block holds the per-sample outputs of ``retraw`` for every level that runs -- alpha, visibility, weights, sigma
    and three colour channels, 7 floats, and the depth: 32 bytes a sample.  A coarse level of 64 samples and a fine one of 64 + 128
    are 256 samples, 8 KB a ray: the default 2^14 rays hold 128 MB, beside the at most ~1.3 GB of one gradient block of 2^16 points
    (20 KB a point) and 16 bytes a selected sample for its index and point."""
    from . import geometry
    model, mlp = _gradient_field('predict_normals', model, configs)
    if isinstance(ray_block, bool) or int(ray_block) != ray_block or int(ray_block) < 1:
        raise RuntimeError(f'ray_block: expected an integer >= 1, got {ray_block}')
    ndc = bool(configs['data_loader']['ndc'])
    suffix = '_fine' if mlp == 'fine_mlp' else '_coarse'
    h, w = (int(v) for v in camera['resolution'])
    n = h * w
    parameters = geometry.ndc_parameters(camera) if ndc else None
    normal = torch.empty((n, 3), dtype=torch.float32, device=device)
    strength = torch.empty((n,), dtype=torch.float32, device=device)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=device)
    depth = torch.empty((n,), dtype=torch.float32, device=device)
    selected = samples = 0
    field = lambda points: model.query_gradient(points, mlp, gradient_block)['grad']
    for start in range(0, n, int(ray_block)):
        count = min(int(ray_block), n - start)
        batch = frame_batch(camera, ndc, device, start, count)
        out = model(batch, retraw=True)
        weights = out[f'weights{suffix}'].reshape(count, -1)
        z_vals = out[f'z_vals{suffix}'].reshape(count, -1)
        rays_o, rays_d = (batch['rays_o_ndc'], batch['rays_d_ndc']) if ndc else (batch['rays_o'], batch['rays_d'])
        normal[start:start + count], strength[start:start + count], kept = geometry.ray_normals(field, rays_o, rays_d, z_vals, weights,
                                                                                                parameters, min_weight)
        rgb[start:start + count] = out[f'rgb{suffix}'].reshape(count, 3)
        depth[start:start + count] = out[f'depth{suffix}'].reshape(count)
        selected += kept
        samples += int(weights.numel())
    depth = ops.to_display(rgb, depth)[1].reshape(h, w)        # the displayed depth: clipped at 0, as predict_frame shows it
    extrinsic, intrinsic = geometry.camera_matrices(camera)
    depth_normal = geometry.depth_normals(depth[None], [extrinsic], [intrinsic], None, edge_threshold)[0]
    normal = normal.reshape(h, w, 3)
    return {'normal': normal, 'normal_strength': strength.reshape(h, w), 'depth_normal': depth_normal,
            'normal_image': geometry.normals_to_u8(normal, camera), 'depth_normal_image': geometry.normals_to_u8(depth_normal, camera),
            'depth': depth, 'selected_fraction': selected / samples if samples else 0.0}


# ---------------------------------------------------------------------------------------------------------------
# static-camera view sweep: the reference's start_testing_static_videos (one pose, the view directions of every camera of a path)
SWEEP_ACTIVATION_BYTES = 8 << 30      # what the saved activations + sweep scratch of one ray block may take on the fast route


def _sweep_levels(model):
    """[(C-ABI level, module)] of the MLPs an eval-mode render runs; the last one is the displayed level."""
    return [(0, model.coarse_model)] + ([(3, model.fine_model)] if model.fine_mlp_needed else [])


# The 16-bit modes whose one-trunk-pass route is on by default: those measured at least 2 x faster than their plain loop at 16 views
# of a 756 x 1008 frame.
SWEEP_HALF_PRECISIONS = (ops.PRECISION_F16, ops.PRECISION_BF16, ops.PRECISION_F16S8, ops.PRECISION_BF16S8)


def _sweep_workspace_query(model):
    """The workspace query of the sweep that reads what ``model``'s precision keeps (None: no sweep does): ``snerf_view_sweep``
    for fp32 activations, ``snerf_view_sweep_half`` for the 16-bit pieces of 'f16' / 'bf16' and their 8-bit variants.  'f16x3'
    keeps fp32 tiles and stays on the plain loop."""
    lib = _lib.load()
    if model.precision == ops.PRECISION_FP32:
        return lib.snerf_view_sweep_workspace_floats
    if model.precision in SWEEP_HALF_PRECISIONS:
        return lib.snerf_view_sweep_half_workspace_floats
    return None


def view_sweep_is_fast(model) -> bool:
    """Whether ``predict_view_sweep`` takes the one-trunk-pass route for ``model``: an fp32, 'f16', 'bf16', 'f16s8' or 'bf16s8' model
    whose displayed MLP is a shape its precision's sweep is built for (the library decides: the workspace query is 0 for every
    other descriptor) and none of whose MLPs predicts visibility."""
    if not hasattr(model, 'coarse_model'):
        return False
    query = _sweep_workspace_query(model)
    if query is None:
        return False
    levels = _sweep_levels(model)
    if any(module.predict_visibility for _, module in levels):
        return False
    desc = ops.mlp_desc(levels[-1][1].mlp_configs)
    return int(query(ctypes.byref(desc), 1, 1, 1)) > 0


def _sweep_ray_block(model, num_views: int) -> int:
    """Rays per block so that the saved activations of every level plus the sweep's scratch stay under SWEEP_ACTIVATION_BYTES
    (8 x 256 at 64 + 128 samples: ~2.6 MB of activations per ray, so ~3000 rays; the allocation is the same in the 16-bit modes,
    whose pieces fill half of it)."""
    lib = _lib.load()
    mcfg = model.configs['model']
    s_c = int(mcfg['coarse_mlp']['num_samples'])
    floats = 0           # of 1024 rays
    for level, module in _sweep_levels(model):
        samples = s_c + (int(mcfg['fine_mlp']['num_samples']) if level == 3 else 0)
        desc = ops.mlp_desc(module.mlp_configs)
        floats += int(lib.snerf_mlp_saved_floats(ctypes.byref(desc), 1024, samples))
    floats += int(_sweep_workspace_query(model)(ctypes.byref(desc), 1024, samples, num_views))     # (the displayed level's)
    return max(32, int(SWEEP_ACTIVATION_BYTES * 1024 // (4 * floats)))


@torch.no_grad()
def predict_view_sweep(model, configs: dict, camera: dict, view_cameras, device, ray_block: Optional[int] = None,
                       keep_device_images: bool = False) -> dict:
    """``camera``'s frame under the view directions of each of ``view_cameras`` (dicts like ``camera``): the eval-mode render of
    the reference's static-camera video (src/Tester01.py start_testing with ``extrinsic_viewcam``), on one rank.

    Returns {'images': (V,h,w,3) uint8 array, 'rgb': (V,h*w,3) float32 on the device, 'depth', 'depth_var' (and, for NDC scenes,
    'depth_ndc', 'depth_var_ndc'): (h,w) float32 arrays} -- the maps do not depend on the view camera and are there once, converted
    as ``retrieve_inference_outputs`` converts them.

    Fast route (``view_sweep_is_fast``): per block of ``ray_block`` rays ONE render that keeps the activations
    (``ops.render_keep_activations`` at the model's precision), ONE ``ops.view_sweep`` (fp32) or ``ops.view_sweep_half`` ('f16',
    'bf16' and their 8-bit variants) over all V cameras and one display conversion per view; everything up
    to the views layer's pre-activation is computed once, not V times.  ``ray_block`` defaults to what keeps a block's saved
    activations and scratch under SWEEP_ACTIVATION_BYTES.  Every other model ('f16x3', layered shapes, predict_visibility)
    takes the plain loop, one ordinary render per view camera (``frame_batch(view_camera=...)``, blocks of ``ray_block`` or 65536
    rays), with the answer in the same form.  ``keep_device_images``: also 'images_device', the (V,h,w,3) uint8 frames as the
    tensor they were converted into."""
    view_cameras = list(view_cameras)
    h, w = int(camera['resolution'][0]), int(camera['resolution'][1])
    n, count = h * w, len(view_cameras)
    ndc = bool(configs['data_loader']['ndc'])
    map_names = ['depth', 'depth_var'] + (['depth_ndc', 'depth_var_ndc'] if ndc else [])
    rgb = torch.empty((count, n, 3), dtype=torch.float32, device=device)
    images = torch.empty((count, n, 3), dtype=torch.uint8, device=device)
    maps: Dict[str, Tensor] = {}
    if not view_sweep_is_fast(model):
        suffix = '_fine' if 'fine_mlp' in configs['model'] else '_coarse'
        keys = [f'rgb{suffix}'] + [f'{name}{suffix}' for name in map_names]
        for v, view_camera in enumerate(view_cameras):
            frame = render_frame(model, camera, ndc, device, keys, ray_block=ray_block or 65536, view_camera=view_camera)
            shown = display_outputs(configs, (h, w), frame)
            rgb[v], images[v] = frame[f'rgb{suffix}'], shown['image'].reshape(n, 3)
            if v == 0:
                maps = {name: shown[name] for name in map_names}
    elif count > 0:
        mcfg = configs['model']
        levels = _sweep_levels(model)
        packed = [None] * 6
        for level, module in levels:
            packed[level] = model._packed_mlp('coarse_model' if level == 0 else 'fine_model', True)
        shown_level, shown_module = levels[-1]
        params = shown_module.abi_params()
        white = bool(mcfg['white_bkgd'])
        block = int(ray_block or _sweep_ray_block(model, count))
        maps = {name: torch.empty((n,), dtype=torch.float32, device=device) for name in map_names}
        for first in range(0, n, block):
            rays = min(block, n - first)
            kept = ops.render_keep_activations(packed, frame_batch(camera, ndc, device, first, rays), ndc, white, bool(mcfg['lindisp']),
                                               int(mcfg['coarse_mlp']['num_samples']),
                                               int(mcfg['fine_mlp']['num_samples']) if shown_level == 3 else 0,
                                               precision=model.precision)
            dirs = torch.stack([view_directions(camera, view_camera, device, first, rays) for view_camera in view_cameras])
            if model.precision == ops.PRECISION_FP32:
                swept = ops.view_sweep(packed[shown_level], params, kept['saved_acts'], kept['weights'], kept['acc'], dirs, white)
            else:
                swept = ops.view_sweep_half(packed[shown_level], params, kept['saved_acts'], kept['weights'], kept['acc'], dirs, white,
                                            model.precision)
            rgb[:, first:first + rays] = swept
            for v in range(count):
                images[v, first:first + rays] = ops.to_display(swept[v], None)[0]
            for name in map_names:
                maps[name][first:first + rays] = ops.to_display(None, kept['outputs'][name], colour=False)[1]
    out = {'images': images.reshape(count, h, w, 3).cpu().numpy(), 'rgb': rgb}
    if keep_device_images:
        out['images_device'] = images.reshape(count, h, w, 3)
    out.update({name: value.reshape(h, w).cpu().numpy() for name, value in maps.items()})
    return out


def save_static_camera_frames(model, configs: dict, preprocessor, extrinsics, out_dirpath, device, png_encoder: str = 'host') -> dict:
    """The frames of the reference's StaticCameraVideo (start_testing_static_videos + Tester.start_testing): ``extrinsics`` (N,4,4)
    raw poses; the frame of ``extrinsics[0]`` under the view cameras ``extrinsics[1:]`` (``predict_view_sweep``), written as
    ``predicted_frames/{i:04}.png`` for i = 0 .. N-2 under ``out_dirpath``.  The mp4 is not written.  Returns the sweep's result.
    ``png_encoder='device'``: all N-1 frames are encoded on the device in one ``png_files`` call."""
    import os
    on_device = _check_png_encoder(png_encoder)
    cameras = [preprocessor.camera(pose) for pose in extrinsics]
    result = predict_view_sweep(model, configs, cameras[0], cameras[1:], device, keep_device_images=on_device)
    if on_device:
        frames = result.pop('images_device')
        directory = os.path.join(os.fspath(out_dirpath), 'predicted_frames')
        os.makedirs(directory, exist_ok=True)
        for i, data in enumerate(png_files(frames) if frames.shape[0] else []):
            with open(os.path.join(directory, f'{i:04}.png'), 'wb') as f:
                f.write(data)
        return result
    for i, image in enumerate(result['images']):
        save_image(os.path.join(os.fspath(out_dirpath), 'predicted_frames', f'{i:04}.png'), image)
    return result


@torch.no_grad()
def evaluate_frames(model, configs: dict, frames, device, rank: int = 0, world_size: int = 1, ray_block: int = 65536,
                    collective: Optional[bool] = None, lpips_weights=None, sorter: str = 'torch') -> Optional[dict]:
    """The reference's QA stage over a test set (src/qa/*), without the frames leaving the device: every frame is rendered
    through the path of ``predict_frame``, converted for display there (uint8 colour, depth clipped at 0) and scored against its
    targets by ``qa.image_metrics`` / ``qa.depth_metrics`` -- only the metrics' scalar sums cross to the host.

    ``frames``: iterable of {'frame_num', 'camera', 'image' (h,w,3) uint8 [, 'depth' (h,w) float32, 'mask' (h,w) bool,
    'depth_scale', 'gt_depth_scale' (the reference's per-side depth factors; default 1)]}, arrays or tensors.  Instead of 'mask' a
    frame may carry 'mask_views': {'depth_train' (T,h,w) float32, 'depth_test' (h,w) float32, 'extrinsics_train' (T,4,4),
    'extrinsic_test' (4,4), 'intrinsics_train' (T,3,3), 'intrinsic_test' (3,3) or None [, 'depth_error_threshold', 'min_views']} --
    the arguments of ``qa.visibility_mask``, which then computes the mask of the masked metrics on the device.
    ``lpips_weights``: a ``qa.LpipsWeights``; every row then also carries LPIPS (and MaskedLPIPS where there is a mask), on the
    backbone the weights were packed for (AlexNet or VGG-16: one per call, under the same keys).
    ``sorter``: 'torch' or 'library', handed to ``qa.visibility_mask`` and ``qa.depth_metrics`` (who sorts and selects: same values).
    Returns {'frames': [{'frame_num': ., metric: value rounded to 4 decimals, ...}], 'average': {metric: value}} with the
    reference's bookkeeping (``qa.summarise``) plus 'unrounded', the per-frame values before rounding.  With world_size > 1 each
    rank renders its block of every frame, rank 0 scores and the other ranks return None."""
    from . import qa
    qa._sorter(sorter)
    ndc = bool(configs['data_loader']['ndc'])
    suffix = '_fine' if 'fine_mlp' in configs['model'] else '_coarse'
    keys = [f'rgb{suffix}', f'depth{suffix}']

    def on_device(value):
        return torch.as_tensor(value).to(device)      # (dtypes are checked by the metric functions, not converted)

    rows = []
    for frame in frames:
        camera = frame['camera']
        h, w = int(camera['resolution'][0]), int(camera['resolution'][1])
        rendered = render_frame(model, camera, ndc, device, keys, rank, world_size, ray_block, collective)
        if rendered is None:
            continue
        image, depth = ops.to_display(rendered[f'rgb{suffix}'].reshape(h * w, 3), rendered[f'depth{suffix}'].reshape(h * w))
        mask = on_device(frame['mask']) if frame.get('mask') is not None else None
        if mask is None and frame.get('mask_views') is not None:
            views = frame['mask_views']
            mask = qa.visibility_mask(on_device(views['depth_train']), on_device(views['depth_test']), views['extrinsics_train'],
                                      views['extrinsic_test'], views['intrinsics_train'], views.get('intrinsic_test'),
                                      float(views.get('depth_error_threshold', 0.05)), int(views.get('min_views', 2)), sorter=sorter)
        row = {'frame_num': frame['frame_num']}
        row.update(qa.image_metrics(image.reshape(h, w, 3), on_device(frame['image']), mask))
        if lpips_weights is not None:
            row.update(qa.lpips_metrics(image.reshape(h, w, 3), on_device(frame['image']), lpips_weights, mask))
        if frame.get('depth') is not None:
            row.update(qa.depth_metrics(depth.reshape(h, w), on_device(frame['depth']),
                                        float(frame.get('depth_scale', 1.0)), float(frame.get('gt_depth_scale', 1.0)), mask, sorter=sorter))
        rows.append(row)
    if rank != 0 and (world_size > 1 if collective is None else collective):
        return None
    table = qa.summarise(rows)
    table['unrounded'] = rows
    return table


def allreduce_gradients(parameters, world_size: int, group=None, force: bool = False) -> None:
    """Training with rays sharded over ranks: average every parameter gradient across ranks with ONE collective
    (all gradients flattened into a single buffer: 2 265 488 floats = 9.06 MB for the 4-MLP model).
    Equivalent to the reference's DataParallel, which gathers the per-device outputs and takes the loss mean over the
    whole batch (src/Trainer01.py:93-96), when every rank holds the same number of rays.  ``force``: issue the collective
    with a single rank too (one-rank process group -- the RCCL call path on a one-GPU box)."""
    if world_size == 1 and not force:
        return
    import torch.distributed as dist
    # EVERY trainable parameter takes part, zeros standing in for a missing gradient: a rank whose shard of a short last
    # batch is empty (or whose loss terms skipped an MLP) must still flatten the same layout as its peers
    params = [p for p in parameters if p.requires_grad]
    if not params:
        return
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat.div_(world_size)
    pieces = [piece.view_as(p) for piece, p in zip(flat.split([p.numel() for p in params]), params)]
    held = [(p, piece) for p, piece in zip(params, pieces) if p.grad is not None]
    if held:     # one multi-tensor copy back into the gradient buffers (their addresses stay: they may be a graph's static ones)
        torch._foreach_copy_([p.grad for p, _ in held], [piece for _, piece in held])
    for p, piece in zip(params, pieces):
        if p.grad is None:
            p.grad = piece.clone()


def train_one_iter(model, loss_computer, optimizer, input_batch: dict, sub_batch_size: Optional[int] = None,
                   world_size: int = 1, group=None, single_pass: bool = False, force_collective: bool = False) -> Dict[str, Tensor]:
    """One optimisation step over ``input_batch`` the way the reference's trainer does it (Trainer.train_one_iter,
    src/Trainer01.py:60-107): gradients cleared, the batch cut into consecutive sub-batches, ``model`` ->
    ``compute_losses`` -> ``TotalLoss.backward()`` per sub-batch (gradients accumulate: the step minimises the SUM of
    the sub-batch means), one ``optimizer.step()``.  With ``world_size`` > 1 the accumulated gradients are averaged
    over ranks by one all-reduce before the step.  Returns the summed loss values as device tensors (the reference
    calls ``.item()`` on each, a host sync per loss per sub-batch; the caller decides when to read them).

    ``single_pass``: the same objective -- every loss still normalised over its own sub-batch, the sub-batch totals
    summed -- with ONE model forward/backward over the whole batch instead of one per sub-batch.  The reference cuts the
    batch because of device memory; the renderer treats rays independently, so evaluating them together changes nothing
    but the number of launches and the gradient-accumulation adds (4096 rows: 10.2 -> 9.1 ms in the 16-bit mode).  Only
    the rounding of the sums differs from the sub-batched run (the draws are keyed by iteration and global row)."""
    optimizer.zero_grad(set_to_none=True)
    n = input_batch['rays_o'].shape[0]
    sub = int(sub_batch_size or n)
    totals: Dict[str, Tensor] = {}
    # global rows (keys of the training draws): the batch's per-row ``global_rows`` tensor is sliced with the other
    # tensors; without it the rows are row_offset + r
    base = int(input_batch.get('row_offset', 0))
    if single_pass and sub < n:
        whole = dict(input_batch)
        output = model(whole)
        # one split per output tensor: its backward is a single concatenation of the sub-batch gradients (slicing per
        # sub-batch would zero-fill and add a full-size gradient per slice)
        pieces = {k: (v.split(sub) if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == n else None)
                  for k, v in output.items()}
        objective = None
        for index, start in enumerate(range(0, n, sub)):
            piece = {}
            for key, value in input_batch.items():
                if isinstance(value, torch.Tensor):
                    piece[key] = value[start:start + sub]
                elif key == 'common_data':
                    piece[key] = dict(value)
                else:
                    piece[key] = value
            piece['row_offset'] = base + start
            out_piece = {k: (pieces[k][index] if pieces[k] is not None else v) for k, v in output.items()}
            losses = loss_computer.compute_losses(piece, out_piece)
            objective = losses['TotalLoss'] if objective is None else objective + losses['TotalLoss']
            for name, entry in losses.items():
                value = entry['loss_value'] if isinstance(entry, dict) else entry
                value = value.detach() if isinstance(value, torch.Tensor) else torch.as_tensor(float(value))
                totals[name] = totals[name] + value if name in totals else value
        objective.backward()
        allreduce_gradients(model.parameters(), world_size, group, force_collective)
        optimizer.step()
        return totals
    for start in range(0, n, sub):
        piece = {}
        for key, value in input_batch.items():
            if isinstance(value, torch.Tensor):
                piece[key] = value[start:start + sub]
            elif key == 'common_data':
                piece[key] = dict(value)
            else:
                piece[key] = value
        piece['row_offset'] = base + start
        losses = loss_computer.compute_losses(piece, model(piece))
        losses['TotalLoss'].backward()
        for name, entry in losses.items():
            value = entry['loss_value'] if isinstance(entry, dict) else entry
            value = value.detach() if isinstance(value, torch.Tensor) else torch.as_tensor(float(value))
            totals[name] = totals[name] + value if name in totals else value
    allreduce_gradients(model.parameters(), world_size, group, force_collective)
    optimizer.step()
    return totals


def _refuse_replicated(model, who: str) -> None:
    if isinstance(model, torch.nn.DataParallel) and len(model.device_ids) > 1:
        raise NotImplementedError(f'{who}: a DataParallel wrapper over several devices replicates the model, scatters the batch and '
                                  f'runs threads on every call, which a captured graph cannot replay -- capture the unwrapped model '
                                  f'(one process per GPU, as bench.py --gpus N runs it)')


class GraphedTrainStep:
    """The device work of one training pass -- weight re-pack, every MLP forward, compositing and resampling, the loss
    table, and the whole backward down to the parameter gradients -- captured ONCE as a HIP graph and replayed per
    iteration (``torch.cuda.graph``; every kernel of the library only enqueues on the current stream, so the capture
    sees them like torch's own).  What changes per iteration stays outside the graph and is written into its static
    inputs first: the batch (copied in), the Philox draws (generated in place by ``model.draw_training_randomness``)
    and, after the replay, the optimiser step.  ~150 launches and their Python glue become one graph launch: the host
    cost of an iteration drops from ~5.4 ms to well under 1 ms, which is what bounds small per-rank batches.

    ``sub_batch_size`` (round 2): the captured work is the reference's iteration exactly -- the batch cut into consecutive
    sub-batches, model -> losses -> backward per sub-batch, gradients accumulated by the backward kernels
    (src/Trainer01.py:82-96) -- so a replay is bit-identical to ``train_one_iter(..., sub_batch_size)`` (same draws too:
    they are generated per sub-batch, each counted as one training forward).  Without it the whole batch is one pass:
    the MSE, sparse-depth and augmentation-depth terms come out the same, the coarse-fine consistency term's patch
    statistics see the whole batch at once and differ by ~10 % (tools/probes/sub_batch_terms.py).  ``p.grad`` of every parameter is a static
    buffer the graph overwrites each replay: do not call ``zero_grad(set_to_none=True)`` between iterations.  The loss
    weights of the iteration are baked into the graph; it is re-captured when ``LossComputer.get_loss_weight`` changes
    them (the shipped schedule: once, at iteration 10000).
    """

    def __init__(self, model, loss_computer, sample_batch: Dict[str, object], warmup: int = 2,
                 sub_batch_size: Optional[int] = None):
        _refuse_replicated(model, 'GraphedTrainStep')
        self.model, self.losses = model, loss_computer
        self.static = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in sample_batch.items() if k != 'common_data'}
        self.common = dict(sample_batch.get('common_data', {}))
        self.n = self.static['rays_o'].shape[0]
        self.device = self.static['rays_o'].device
        self.draws = {k: torch.empty(shape, dtype=torch.float32, device=self.device)
                      for k, shape in model.training_draw_shapes(self.n).items()}
        self.warmup = warmup
        self.sub = int(sub_batch_size) if sub_batch_size else self.n
        self.graph = None
        self.weights_key = None
        self.totals: Dict[str, Tensor] = {}

    @staticmethod
    def _rows(batch, n):
        first, rows = global_rows(batch, n)
        return rows if rows is not None else first

    def _weights(self, iter_num):
        return tuple(self.losses.get_loss_weight(cfg, iter_num) for cfg in self.losses.losses.values())

    def _pass(self):
        totals: Dict[str, Tensor] = {}
        for start in range(0, self.n, self.sub):
            cut = slice(start, start + self.sub)
            self.model.set_random_draws({k: v[cut] for k, v in self.draws.items()})
            piece = {k: (v[cut] if isinstance(v, torch.Tensor) else v) for k, v in self.static.items()}
            piece['common_data'] = dict(self.common)
            losses = self.losses.compute_losses(piece, self.model(piece))
            losses['TotalLoss'].backward()
            for name, entry in losses.items():
                value = (entry['loss_value'] if isinstance(entry, dict) else entry).detach()
                totals[name] = totals[name] + value if name in totals else value
        return totals

    def _draw(self, batch):
        """This iteration's draws into the static buffers: per sub-batch, each counted as one training forward -- what the
        eager sub-batched iteration draws."""
        rows = self._rows(batch, self.n)
        for start in range(0, self.n, self.sub):
            count = min(self.sub, self.n - start)
            part = rows[start:start + count] if isinstance(rows, torch.Tensor) else rows + start
            self.model.draw_training_randomness(count, part, self.device, out={k: v[start:start + count] for k, v in self.draws.items()},
                                                iter_num=batch.get('iter_num'))

    def _capture(self):
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):          # eager warm-up on a side stream, as torch's graph capture requires
            for _ in range(self.warmup):
                self._pass()
        torch.cuda.current_stream(self.device).wait_stream(side)
        for p in self.model.parameters():
            p.grad = None                      # gradients are (re)allocated inside the capture: static addresses
        self.model.invalidate_packed()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode=CAPTURE_MODE):
            self.totals = self._pass()

    def __call__(self, batch: Dict[str, object]) -> Dict[str, Tensor]:
        rows = batch['rays_o'].shape[0]
        if rows != self.n:
            # a short batch at the end of an epoch (the reference's slicing, DataPreprocessor01.py:559-563): the same
            # sub-batched pass as train_one_iter (ceil(rows / sub) model -> losses -> backward rounds, the sub-batch
            # totals summed, draws per sub-batch), launched directly, accumulating into the (zeroed) static gradient
            # buffers so that their addresses survive
            for p in self.model.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            all_rows = self._rows(batch, rows)
            totals: Dict[str, Tensor] = {}
            for start in range(0, rows, self.sub):
                count = min(self.sub, rows - start)
                part = all_rows[start:start + count] if isinstance(all_rows, torch.Tensor) else all_rows + start
                self.model.set_random_draws(self.model.draw_training_randomness(count, part, self.device, iter_num=batch.get('iter_num')))
                piece = {k: (v[start:start + count] if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
                piece['common_data'] = dict(batch.get('common_data', {}))
                losses = self.losses.compute_losses(piece, self.model(piece))
                losses['TotalLoss'].backward()
                for name, entry in losses.items():
                    value = (entry['loss_value'] if isinstance(entry, dict) else entry).detach()
                    totals[name] = totals[name] + value if name in totals else value
            return totals
        for k, v in batch.items():
            if isinstance(v, torch.Tensor):
                self.static[k].copy_(v)
            elif k != 'common_data':
                self.static[k] = v
        self._draw(batch)
        key = self._weights(batch['iter_num'])
        if self.graph is None or key != self.weights_key:
            self._capture()                    # records the work (on these inputs); nothing is computed until the replay
            self.weights_key = key
        self.graph.replay()
        # a replay bypasses the entry points that report an fp16 range violation of an earlier launch: ask here (a host read
        # of a pinned word, no synchronisation -- like the entry points it sees launches that have finished)
        if self.model.precision in ops.FP16_RANGE_PRECISIONS and ops.range_status(clear=True):
            raise ops.Fp16RangeError("GraphedTrainStep: an earlier replay met a value outside the fp16 range (|v| > 65504); its "
                                     "gradients are invalid -- use hip_precision 'fp32' for this model")
        return self.totals


class GraphedIteration:
    """The WHOLE training iteration as ONE HIP graph (round 3): batch assembly (index permutation + ray
    assembly), the training draws, weight re-pack, every MLP forward, compositing / resampling, the loss table, the complete
    backward AND the Adam update -- ``GraphedTrainStep`` replayed only the pass in between, with batch copy, draws and optimiser
    enqueued from Python around it.  What changes from iteration to iteration cannot be a kernel argument of a replayed graph,
    so it lives in device memory: the graph's first node (``snerf_iteration_advance``) copies the next record of a pinned host
    ring -- epoch positions of the pixel and sparse-depth slices, the iteration number that keys the Philox draws, Adam's two
    step-dependent factors with the decayed learning rate folded in -- into the device-resident record that
    ``snerf_shuffled_indices_at`` / ``snerf_random_*_at`` / ``snerf_adam_step_at`` read.  Per iteration the host writes one
    64-byte record and launches one graph: parameters after N iterations are bit-identical to N eager
    ``train_one_iter`` iterations (tests/test_gpu_optim.py).

    A short batch at the end of an epoch (other tensor shapes) runs eagerly into the graph's static gradient buffers, as
    ``GraphedTrainStep`` does; the graph is re-captured when ``LossComputer.get_loss_weight`` changes the loss weights.  The host
    may run at most ``slots - 1`` replays ahead of the device: the slot about to be overwritten is guarded by an event.

    Several ranks (round 4): ``batcher`` built with (rank, world_size) hands every rank its slice of the same global batch, and
    the ONE all-reduce of the flattened gradients (``allreduce_gradients``) is captured between the last sub-batch's backward
    and the Adam update -- RCCL collectives record into a HIP graph like kernels, so a replay still costs the host one record
    and one launch.  It needs the ``nccl`` backend (gloo's collectives run on the host and cannot be captured);
    ``force_collective`` captures the all-reduce with a single rank too (the test of exactly that on a one-GPU box)."""

    def __init__(self, model, loss_computer, optimizer, batcher, lr_decayer=None, sub_batch_size: Optional[int] = None,
                 slots: int = 8, warmup: int = 1, group=None, force_collective: bool = False):
        _refuse_replicated(model, 'GraphedIteration')
        self.world = int(getattr(batcher, 'world_size', 1))
        self.group, self.force_collective = group, bool(force_collective)
        if self.world > 1 or self.force_collective:
            import torch.distributed as dist
            if not dist.is_initialized() or dist.get_backend(group) != 'nccl':
                raise NotImplementedError("GraphedIteration over several ranks captures the gradient all-reduce: it needs an initialised "
                                          "'nccl' (RCCL) process group -- with gloo use GraphedTrainStep + allreduce_gradients")
        if len(optimizer.param_groups) != 1:
            raise NotImplementedError('GraphedIteration replays ONE (step size, bias correction) record: a single parameter group')
        self.model, self.losses, self.opt, self.batcher, self.decayer = model, loss_computer, optimizer, batcher, lr_decayer
        self.device = batcher.device
        self.ring = ops.IterationRing(self.device, slots)
        self.events = [None] * slots
        self.sub = int(sub_batch_size) if sub_batch_size else None
        self.warmup = warmup
        self.graph = None
        self.weights_key = None
        self.totals: Dict[str, Tensor] = {}
        self.wait_seconds = 0.0           # time the host spent waiting for a ring slot (it was >= slots - 1 replays ahead)

    def _weights(self, iter_num):
        return tuple(self.losses.get_loss_weight(cfg, iter_num) for cfg in self.losses.losses.values())

    def _passes(self, batch, draws_at) -> Dict[str, Tensor]:
        """model -> losses -> backward per sub-batch (gradients accumulate in the kernels), totals summed."""
        n = batch['rays_o'].shape[0]
        sub = self.sub or n
        rows = batch['global_rows']
        totals: Dict[str, Tensor] = {}
        for start in range(0, n, sub):
            count = min(sub, n - start)
            self.model.set_random_draws(self.model.draw_training_randomness(count, rows[start:start + count], self.device,
                                                                            iter_num=batch.get('iter_num'), at=draws_at))
            piece = {k: (v[start:start + count] if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
            piece['common_data'] = dict(batch.get('common_data', {}))
            losses = self.losses.compute_losses(piece, self.model(piece))
            losses['TotalLoss'].backward()
            for name, entry in losses.items():
                value = (entry['loss_value'] if isinstance(entry, dict) else entry).detach()
                totals[name] = totals[name] + value if name in totals else value
        return totals

    def _body(self, iter_num: int, whole: bool) -> Dict[str, Tensor]:
        if whole:
            self.ring.advance()
        batch = self.batcher.get_next_batch(iter_num, at=self.ring.current)
        totals = self._passes(batch, self.ring.current)
        if not whole:      # the eager warm-up: which trainable parameters does the backward leave without a gradient?
            self._gradless = [p for p in self.model.parameters() if p.requires_grad and p.grad is None]
        allreduce_gradients(self.model.parameters(), self.world, self.group, self.force_collective)
        if whole:
            self.opt.step_at(self.ring.current)
        return totals

    def _capture(self, iter_num: int):
        # optimiser state must exist BEFORE the capture (created inside it, its zero fill would be replayed every iteration)
        for group in self.opt.param_groups:
            for p in group['params']:
                if p.requires_grad and len(self.opt.state[p]) == 0:
                    self.opt.state[p]['step'] = torch.tensor(0.0, dtype=torch.float32)
                    self.opt.state[p]['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self.opt.state[p]['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):          # eager warm-up on a side stream, as torch's graph capture requires: the pass
            for _ in range(self.warmup):       # only -- no ring advance, no optimiser step
                self._body(iter_num, whole=False)
        torch.cuda.current_stream(self.device).wait_stream(side)
        for p in self.model.parameters():
            p.grad = None                      # gradients are (re)allocated inside the capture: static addresses
        if self.world > 1 or self.force_collective:
            # ... except for parameters the backward never reaches: the all-reduce gives those a zero stand-in (every rank must
            # flatten the same layout), and ASSIGNING ``p.grad`` inside a capture would hand the optimiser a buffer of the graph's
            # private pool that no replay re-creates.  They get their static zero buffer here, before the capture;
            # inside it the all-reduce only copies into buffers that exist.
            for p in getattr(self, '_gradless', ()):
                p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
        self.model.invalidate_packed()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode=CAPTURE_MODE):
            self.totals = self._body(iter_num, whole=True)

    def __call__(self, iter_num: int) -> Dict[str, Tensor]:
        positions = self.batcher.next_positions()
        lr = None
        if self.decayer is not None:
            lr = self.decayer.get_updated_learning_rate(iter_num)
            for group in self.opt.param_groups:
                group['lr'] = lr
        lr = self.opt.param_groups[0]['lr'] if lr is None else lr
        self.last_was_short = not self.batcher.is_full(positions)
        if self.last_was_short:
            # a short batch at the end of an epoch: the same sub-batched pass launched directly into the (zeroed) static
            # gradient buffers, then the ordinary optimiser step
            for p in self.model.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            totals = self._passes(self.batcher.get_next_batch(iter_num, positions=positions), None)
            allreduce_gradients(self.model.parameters(), self.world, self.group, self.force_collective)
            self.opt.step()
            return totals
        key = self._weights(iter_num)
        if self.graph is None or key != self.weights_key:
            self._capture(iter_num)            # records the work; nothing of it runs (and no ring record is consumed) until the replay
            self.weights_key = key
        slot = self.ring.filled % self.ring.slots
        if self.events[slot] is not None and not self.events[slot].query():
            import time
            t0 = time.perf_counter()
            self.events[slot].synchronize()    # the replay that read this slot has finished
            self.wait_seconds += time.perf_counter() - t0
        neg_step_size, bias2_sqrt = self.opt.graph_factors(self.opt.next_count(), lr)
        sparse = positions.get('sparse', (0, 0, 0))
        self.ring.fill(iter_num, positions['pixel'][:2], sparse[:2], neg_step_size, bias2_sqrt)
        self.graph.replay()
        event = torch.cuda.Event()
        event.record()
        self.events[slot] = event
        self.opt.count_step()
        if self.model.precision in ops.FP16_RANGE_PRECISIONS and ops.range_status(clear=True):
            raise ops.Fp16RangeError("GraphedIteration: an earlier replay met a value outside the fp16 range (|v| > 65504); its "
                                     "update is invalid -- use hip_precision 'fp32' for this model")
        return self.totals


# ---------------------------------------------------------------------------------------------------------------
# frame writer: what the reference's Tester does with a predicted frame (src/Tester01.py:69-92), without
# its skimage dependency -- PNG through zlib, .npy through numpy
def _png_bytes(array) -> bytes:
    import struct
    import zlib
    import numpy
    a = numpy.ascontiguousarray(array)
    if a.dtype != numpy.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise RuntimeError(f'PNG writer takes uint8 (h,w) or (h,w,3) arrays, got {a.dtype} {a.shape}')
    h, w = a.shape[:2]
    rows = numpy.concatenate([numpy.zeros((h, 1), dtype=numpy.uint8), a.reshape(h, -1)], axis=1)   # filter type 0 per row
    return _png_container(zlib.compress(rows.tobytes(), 6), h, w, a.ndim == 3)


def _png_container(stream: bytes, h: int, w: int, colour: bool) -> bytes:
    """The file around the zlib stream of an 8-bit grey or RGB image's filtered rows: signature, IHDR, one IDAT, IEND."""
    import struct
    import zlib

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)

    header = struct.pack('>IIBBBBB', w, h, 8, 2 if colour else 0, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', header) + chunk(b'IDAT', stream) + chunk(b'IEND', b'')


PNG_ENCODERS = ('host', 'device')      # 'host': _png_bytes (filter type 0, zlib level 6, one host thread); 'device': png_files


def _check_png_encoder(png_encoder) -> bool:
    """True for 'device'; any value but the two names raises."""
    if png_encoder not in PNG_ENCODERS:
        raise RuntimeError(f"png_encoder: expected 'host' or 'device', got {png_encoder!r}")
    return png_encoder == 'device'


def _device_u8(value, what: str) -> Tensor:
    if not isinstance(value, torch.Tensor) or not value.is_cuda:
        raise RuntimeError(f"{what}: png_encoder='device' encodes tensors that are on the device, got "
                           f"{type(value).__name__}{' on ' + str(value.device) if isinstance(value, torch.Tensor) else ''}; "
                           f"there is no fall-back to the host writer")
    return value


def png_files(images) -> list:
    """The PNG files of ``images`` -- uint8 (K,h,w) grey or (K,h,w,3) RGB on the device -- as K ``bytes``, encoded there: one
    ``ops.png_deflate`` call for all K (adaptive row filters, run-length tokens, one Huffman block per 32 KiB), one copy of the K
    stream lengths to the host, then one copy per stream of exactly its bytes; the container around each stream is ``_png_bytes``'
    (signature, IHDR, one IDAT, IEND; the CRC-32 on the host).  The files decode to the pixels ``_png_bytes`` would store; the bytes
    differ (other filters, another deflate)."""
    images = _device_u8(images, 'png_files')
    streams, sizes = ops.png_deflate(images)
    h, w = int(images.shape[1]), int(images.shape[2])
    return [_png_container(streams[i, :n].cpu().numpy().tobytes(), h, w, images.dim() == 4) for i, n in enumerate(sizes.cpu().tolist())]


def save_image(path, image, png_encoder: str = 'host') -> None:
    """``image``: uint8 (h,w,3) array or tensor (e.g. ``to_display`` output reshaped); ``.png`` or ``.npy`` by suffix.
    ``png_encoder='device'``: a ``.png`` of a tensor on the device is encoded there (``png_files``)."""
    import os
    import numpy
    path = os.fspath(path)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    if _check_png_encoder(png_encoder) and path.endswith('.png'):
        data, = png_files(_device_u8(image, 'save_image')[None])
        with open(path, 'wb') as f:
            f.write(data)
        return
    array = image.cpu().numpy() if isinstance(image, torch.Tensor) else numpy.asarray(image)
    if path.endswith('.png'):
        with open(path, 'wb') as f:
            f.write(_png_bytes(array))
    elif path.endswith('.npy'):
        numpy.save(path, array)
    else:
        raise RuntimeError(f'Unknown image format: {path}')


def save_depth(path, depth, as_png: bool = False, png_encoder: str = 'host') -> None:
    """``depth``: float (h,w); ``.npy`` keeps the values (plus a PNG preview when ``as_png``), ``.png`` stores
    round(depth / depth.max() * 255) like the reference (src/Tester01.py:80-92).  A float32 tensor on the device is converted
    there (``ops.maps_to_u8``: the same bytes) and its preview copied as one byte per pixel -- or, with ``png_encoder='device'``,
    encoded there as well (``png_files``; the depth must be such a tensor)."""
    import os
    import numpy
    path = os.fspath(path)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    on_device = _check_png_encoder(png_encoder)
    if on_device and (_device_u8(depth, 'save_depth').dtype != torch.float32 or depth.dim() != 2):
        raise RuntimeError(f"save_depth: png_encoder='device' takes a float32 (h,w) tensor, got {depth.dtype} {tuple(depth.shape)}")
    if isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32:
        # the preview on the device (snerf_maps_to_u8): one byte per pixel crosses, and the floats only for a .npy
        preview = ops.maps_to_u8(depth.reshape(1, -1), (ops.MAP_SCALE_MAX,))[0].reshape(depth.shape)
        if not on_device:
            preview = preview.cpu().numpy()
        array = depth.cpu().numpy() if path.endswith('.npy') else None
    else:
        array = depth.cpu().numpy() if isinstance(depth, torch.Tensor) else numpy.asarray(depth)
        preview = numpy.round(array / array.max() * 255).astype('uint8')

    def preview_file() -> bytes:
        return png_files(preview[None])[0] if on_device else _png_bytes(preview)

    if path.endswith('.png'):
        with open(path, 'wb') as f:
            f.write(preview_file())
    elif path.endswith('.npy'):
        numpy.save(path, array)
        if as_png:
            with open(os.path.splitext(path)[0] + '.png', 'wb') as f:
                f.write(preview_file())
    else:
        raise RuntimeError(f'Unknown depth format: {path}')


# ---------------------------------------------------------------------------------------------------------------
# videos: what the reference's save_video writes (src/NerfLlffTrainerTester01.py:29-38: 15 frames a second, yuv420p), as
# Motion-JPEG in a RIFF AVI instead of H.264 in an mp4 -- every frame a baseline JPEG whose scan is coded on the device
# (ops.jpeg_scan, csrc/simplenerf_jpeg.h); the markers and the container are written here.
# ITU-T T.81 Annex K.1 in zig-zag order (luminance, chrominance) and Annex K.3 as {class << 4 | id: (codes per length, symbols)}
_JPEG_QUANT_BASE = (
    (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101,
     103, 99),
    (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66) + (99,) * 50)
_JPEG_HUFFMAN = {
    0x00: (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
    0x10: (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]), bytes.fromhex(
        '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a4344454647'
        '48494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba'
        'c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')),
    0x01: (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
    0x11: (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]), bytes.fromhex(
        '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546'
        '4748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8'
        'b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'))}


def _jpeg_header(h: int, w: int, colour: bool, quality: int) -> bytes:
    """Everything of a JFIF file before the entropy-coded segment ``ops.jpeg_scan`` writes: SOI, APP0 (JFIF 1.01, no density), DQT
    (the Annex K tables scaled by ``quality`` with the libjpeg rule), SOF0 (8-bit; Y 2x2, Cb and Cr 1x1 -- or one grey component),
    DHT (the Annex K tables), DRI (one MCU row) and SOS."""
    import struct

    def segment(marker: int, data: bytes) -> bytes:
        return bytes([0xFF, marker]) + struct.pack('>H', len(data) + 2) + data

    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    out = b'\xff\xd8' + segment(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for table in range(2 if colour else 1):
        out += segment(0xDB, bytes([table]) + bytes(min(255, max(1, (t * scale + 50) // 100)) for t in _JPEG_QUANT_BASE[table]))
    components = ((1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)) if colour else ((1, 0x11, 0),)
    out += segment(0xC0, struct.pack('>BHHB', 8, h, w, len(components)) + b''.join(bytes(c) for c in components))
    for key in (0x00, 0x10, 0x01, 0x11) if colour else (0x00, 0x10):
        out += segment(0xC4, bytes([key]) + _JPEG_HUFFMAN[key][0] + _JPEG_HUFFMAN[key][1])
    mcu = 16 if colour else 8
    out += segment(0xDD, struct.pack('>H', (w + mcu - 1) // mcu))
    return out + segment(0xDA, bytes([len(components)]) + b''.join(bytes([c[0], c[2] << 4 | c[2]]) for c in components) + bytes([0, 63, 0]))


def _device_frames(value, what: str) -> Tensor:
    if not isinstance(value, torch.Tensor) or not value.is_cuda:
        raise RuntimeError(f"{what}: the JPEG encoder takes tensors that are on the device, got "
                           f"{type(value).__name__}{' on ' + str(value.device) if isinstance(value, torch.Tensor) else ''}; "
                           f"there is no host encoder to fall back to")
    return value


def jpeg_files(images, quality: int = 90) -> list:
    """The JFIF files of ``images`` -- uint8 (K,h,w) grey or (K,h,w,3) RGB on the device -- as K ``bytes``, encoded there: one
    ``ops.jpeg_scan`` call for all K (YCbCr 4:2:0, integer DCT, Annex K tables at ``quality`` 1..100, a restart interval per MCU
    row), one copy of the K scan lengths to the host, then one copy per scan of exactly its bytes; the markers around each scan
    (``_jpeg_header``, EOI) are written here."""
    images = _device_frames(images, 'jpeg_files')
    scans, sizes = ops.jpeg_scan(images, quality)
    header = _jpeg_header(int(images.shape[1]), int(images.shape[2]), images.dim() == 4, int(quality))
    return [header + scans[i, :n].cpu().numpy().tobytes() + b'\xff\xd9' for i, n in enumerate(sizes.cpu().tolist())]


VIDEO_FRAME_RATE = 15          # save_video, src/NerfLlffTrainerTester01.py:34


def _avi_bytes(frames: list, h: int, w: int, frame_rate) -> bytes:
    """A RIFF AVI of JPEG files as one Motion-JPEG video stream: ``hdrl`` (``avih``, one ``strl`` of ``strh`` 'vids'/'MJPG' and a
    BITMAPINFOHEADER ``strf``), ``movi`` of ``00dc`` chunks padded to even length, ``idx1`` (offsets from the 'movi' tag)."""
    import math
    import struct
    from fractions import Fraction

    def chunk(tag: bytes, data: bytes) -> bytes:
        return tag + struct.pack('<I', len(data)) + data + (b'\0' if len(data) & 1 else b'')

    def riff_list(kind: bytes, data: bytes) -> bytes:
        return b'LIST' + struct.pack('<I', 4 + len(data)) + kind + data

    rate = Fraction(frame_rate).limit_denominator(1000)
    if rate <= 0:
        raise RuntimeError(f'save_video: frame_rate {frame_rate!r} is not positive')
    largest = max((len(f) for f in frames), default=0)
    total = sum(len(f) for f in frames)
    avih = struct.pack('<14I', round(1000000 / rate), math.ceil(total * rate / max(1, len(frames))), 0, 0x10, len(frames), 0, 1, largest, w, h,
                       0, 0, 0, 0)
    strh = struct.pack('<4s4sIHHIIIIIIIi4H', b'vids', b'MJPG', 0, 0, 0, 0, rate.denominator, rate.numerator, 0, len(frames), largest,
                       0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack('<IiiHH4sIiiII', 40, w, h, 1, 24, b'MJPG', w * h * 3, 0, 0, 0, 0)
    movi, index, at = [], [], 4          # (an idx1 offset counts from the 'movi' tag)
    for data in frames:
        index.append(struct.pack('<4sIII', b'00dc', 0x10, at, len(data)))
        movi.append(chunk(b'00dc', data))
        at += len(movi[-1])
    body = (b'AVI ' + riff_list(b'hdrl', chunk(b'avih', avih) + riff_list(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf)))
            + riff_list(b'movi', b''.join(movi)) + chunk(b'idx1', b''.join(index)))
    return b'RIFF' + struct.pack('<I', len(body)) + body


def save_video(path, frames, frame_rate=VIDEO_FRAME_RATE, quality: int = 90) -> None:
    """The reference's ``save_video`` (src/NerfLlffTrainerTester01.py:29-38) as Motion-JPEG: ``frames`` -- uint8 (K,h,w,3) or (K,h,w)
    on the device -- become K baseline JPEG files there (``jpeg_files``: 4:2:0 like the reference's yuv420p) and one RIFF AVI
    (``vids``/``MJPG``) at ``frame_rate`` frames a second on the host.  A file that exists is left alone, as the reference leaves it;
    a file that would reach 2^31 bytes is refused (the container's index and many readers stop there)."""
    import os
    path = os.fspath(path)
    if os.path.exists(path):
        return
    frames = _device_frames(frames, 'save_video')
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        raise RuntimeError(f'save_video: frames must be uint8 (K,h,w) or (K,h,w,3), got {frames.dtype} {tuple(frames.shape)}')
    files = jpeg_files(frames, quality) if frames.shape[0] else []
    data = _avi_bytes(files, int(frames.shape[1]), int(frames.shape[2]), frame_rate)
    if len(data) >= 1 << 31:
        raise RuntimeError(f'save_video: {path} would be {len(data)} bytes; an AVI of 2^31 bytes or more is not written')
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)


def _select_video_frames(frames: Tensor, video_frame_nums) -> Tensor:
    """``video_frames[video_frame_nums]`` (src/NerfLlffTrainerTester01.py:166-167): the listed frames in the listed order, repeats
    and negative indices as numpy takes them."""
    if video_frame_nums is None:
        return frames
    import numpy
    picks = numpy.asarray(video_frame_nums).astype(int).reshape(-1)
    count = int(frames.shape[0])
    if picks.size and (picks.min() < -count or picks.max() >= count):
        raise IndexError(f'video_frame_nums: index {int(picks.max() if picks.max() >= count else picks.min())} is out of bounds for {count} frames')
    return frames[torch.from_numpy(picks % count if count else picks).to(frames.device)]


def save_static_camera_video(model, configs: dict, preprocessor, extrinsics, out_dirpath, device, video_frame_nums=None,
                             quality: int = 90) -> dict:
    """The reference's StaticCameraVideo (start_testing_static_videos, src/NerfLlffTrainerTester01.py:199-228): ``extrinsics``
    (N,4,4) raw poses; the frame of ``extrinsics[0]`` under the view cameras ``extrinsics[1:]`` (``predict_view_sweep``), the N-1
    frames -- or those ``video_frame_nums`` lists, in its order -- written as ``StaticCameraVideo.avi`` under ``out_dirpath``
    (``save_video``: the frames are coded where they were rendered).  The PNG frames are not written
    (``save_static_camera_frames`` writes them).  Returns the sweep's result."""
    import os
    cameras = [preprocessor.camera(pose) for pose in extrinsics]
    result = predict_view_sweep(model, configs, cameras[0], cameras[1:], device, keep_device_images=True)
    frames = _select_video_frames(result.pop('images_device'), video_frame_nums)
    save_video(os.path.join(os.fspath(out_dirpath), 'StaticCameraVideo.avi'), frames, quality=quality)
    return result


@torch.no_grad()
def save_camera_path_video(model, configs: dict, preprocessor, extrinsics, out_dirpath, device, video_frame_nums=None,
                           quality: int = 90) -> dict:
    """The reference's PredictedVideo (start_testing_videos, src/NerfLlffTrainerTester01.py:141-169): each of ``extrinsics[1:]``
    rendered as ``predict_frame`` renders it (the frame stays on the device), the N-1 frames -- or those ``video_frame_nums``
    lists, in its order -- written as ``PredictedVideo.avi`` under ``out_dirpath``.  No PNG frames.  Returns {'images_device':
    the (N-1,h,w,3) uint8 frames as rendered}."""
    import os
    ndc = bool(configs['data_loader']['ndc'])
    suffix = '_fine' if 'fine_mlp' in configs['model'] else '_coarse'
    keys = [f'rgb{suffix}', f'depth{suffix}', f'depth_var{suffix}'] + ([f'depth_ndc{suffix}', f'depth_var_ndc{suffix}'] if ndc else [])
    cameras = [preprocessor.camera(pose) for pose in extrinsics]
    h, w = (int(v) for v in cameras[0]['resolution'])
    frames = torch.empty((max(len(cameras) - 1, 0), h, w, 3), dtype=torch.uint8, device=device)
    for i, camera in enumerate(cameras[1:]):
        frames[i] = display_outputs(configs, camera['resolution'], render_frame(model, camera, ndc, device, keys))['image']
    save_video(os.path.join(os.fspath(out_dirpath), 'PredictedVideo.avi'), _select_video_frames(frames, video_frame_nums), quality=quality)
    return {'images_device': frames}


@torch.no_grad()
def _render_views(what: str, model, configs: dict, cameras, device, depth_range):
    """The renders the geometry exports share: every camera of ``cameras`` (dicts as ``frame_batch`` takes them, one resolution)
    rendered as ``predict_frame`` renders it, the 8-bit images and the depths staying on the device.  -> (images uint8 (V,h,w,3),
    depths float32 (V,h,w), extrinsics, intrinsics (lists of float64 matrices, ``geometry.camera_matrices``), mask: the pixels with
    lo <= depth <= hi of ``depth_range`` = (lo, hi), or None).  Refusals are reported under ``what``."""
    from . import geometry
    cameras = list(cameras)
    if not cameras:
        raise RuntimeError(f'{what}: no cameras')
    ndc = bool(configs['data_loader']['ndc'])
    suffix = '_fine' if 'fine_mlp' in configs['model'] else '_coarse'
    keys = [f'rgb{suffix}', f'depth{suffix}', f'depth_var{suffix}'] + ([f'depth_ndc{suffix}', f'depth_var_ndc{suffix}'] if ndc else [])
    h, w = (int(v) for v in cameras[0]['resolution'])
    images = torch.empty((len(cameras), h, w, 3), dtype=torch.uint8, device=device)
    depths = torch.empty((len(cameras), h, w), dtype=torch.float32, device=device)
    for i, camera in enumerate(cameras):
        if tuple(int(v) for v in camera['resolution']) != (h, w):
            raise RuntimeError(f'{what}: camera {i} has resolution {tuple(camera["resolution"])}, camera 0 has {(h, w)}')
        shown = display_outputs(configs, camera['resolution'], render_frame(model, camera, ndc, device, keys))
        images[i], depths[i] = shown['image'], shown['depth']
    matrices = [geometry.camera_matrices(camera) for camera in cameras]
    mask = None
    if depth_range is not None:
        low, high = (float(v) for v in depth_range)
        mask = (depths >= low) & (depths <= high)
    return images, depths, [m[0] for m in matrices], [m[1] for m in matrices], mask


def _field_normals_of(what: str, field, configs: dict, cameras, points: Tensor) -> Tensor:
    """The unit outward normals of the density field at the float32 (N,3) scene-frame ``points`` of a geometry export:
    ``geometry.field_normals`` with ``model.query_gradient`` (always fp32, blocks of 2^16 points) of the displayed level's MLP --
    ``field`` is ``_gradient_field``'s (model, MLP name).  For a model of NDC rays the warp's (cx, cy, near) come from ``cameras[0]``,
    and every camera must give the same, as ``export_density_mesh`` asks."""
    from . import geometry
    model, mlp = field
    ndc = None
    if bool(configs['data_loader']['ndc']):
        ndc = geometry.ndc_parameters(cameras[0])
        for i, camera in enumerate(cameras):
            if geometry.ndc_parameters(camera) != ndc:
                raise RuntimeError(f'{what}: ndc: camera {i} has (cx, cy, near) = {geometry.ndc_parameters(camera)}, camera 0 has {ndc}; '
                                   f'one NDC warp needs cameras of one resolution, focal length and near plane')
    return geometry.field_normals(lambda q: model.query_gradient(q, mlp, 1 << 16)['grad'], points, ndc)


@torch.no_grad()
def export_point_cloud(model, configs: dict, cameras, path, device, depth_error_threshold: float = 0.02, min_views: int = 1,
                       voxel_size: Optional[float] = None, depth_range=None, normals: bool = False) -> dict:
    """The model's geometry as a point cloud: every camera of ``cameras`` (dicts as ``frame_batch`` takes them, one resolution)
    rendered as ``predict_frame`` renders it -- the 8-bit image and the depth stay on the device --, the depth maps fused
    (``geometry.fuse_depth_maps``: a pixel's point is kept where at least ``min_views`` other views agree with it to
    ``depth_error_threshold`` x their depth), optionally thinned to one point per voxel of ``voxel_size`` (``geometry.voxel_thin``),
    and written to ``path`` as a binary PLY (``geometry.save_ply``: a file that exists is left alone).  ``depth_range`` = (lo, hi):
    only pixels with lo <= depth <= hi are sources or witnesses.  The cloud is in the model's processed scene frame (recentred, and
    scaled by ``translation_scale``); mapping it back to the data set's frame is the caller's.  Returns {'points' float32 (N,3),
    'colours' uint8 (N,3), 'counts' (N): the agreeing views of each point (uint8), or with ``voxel_size`` the points of each voxel
    (int32), 'fused_points': N before thinning, 'images_device' (V,h,w,3), 'depths_device' (V,h,w)}, tensors on the device.
    ``normals=True`` adds 'normals' float32 (N,3): the unit outward normals of the density field at the written points (after the
    thinning; ``_field_normals_of``), and the file's vertices carry them (``x y z nx ny nz red green blue``, 27 bytes a vertex:
    oriented normals, which a Poisson reconstruction needs); the default writes the same bytes as before.  A model that
    ``query_gradient`` refuses is refused before anything is rendered."""
    from . import geometry
    cameras = list(cameras)
    field = _gradient_field('export_point_cloud', model, configs) if normals else None
    images, depths, extrinsics, intrinsics, mask = _render_views('export_point_cloud', model, configs, cameras, device, depth_range)
    points, colours, counts = geometry.fuse_depth_maps(depths, images, extrinsics, intrinsics, depth_error_threshold, min_views, mask)
    fused = int(points.shape[0])
    if voxel_size is not None:
        points, colours, counts = geometry.voxel_thin(points, colours, voxel_size)
    out = {'points': points, 'colours': colours, 'counts': counts, 'fused_points': fused, 'images_device': images,
           'depths_device': depths}
    if normals:
        out['normals'] = _field_normals_of('export_point_cloud', field, configs, cameras, points)
        geometry.save_ply(path, points, colours, out['normals'])
    else:
        geometry.save_ply(path, points, colours)
    return out


@torch.no_grad()
def export_mesh(model, configs: dict, cameras, path, device, voxel_size: float, truncation: Optional[float] = None, bounds=None,
                min_weight: int = 1, colour_tolerance: Optional[float] = None, depth_range=None, normals: bool = False) -> dict:
    """The model's geometry as a triangle mesh: every camera of ``cameras`` rendered as ``export_point_cloud`` renders it, the depth
    maps fused into a truncated signed distance volume of ``voxel_size`` (``geometry.tsdf_volume``; ``truncation`` defaults to four
    voxels), the surface extracted by marching tetrahedra over the cells that at least ``min_weight`` views observed at every corner
    (``geometry.extract_mesh``), its vertices coloured from the frames (``geometry.colour_points``; ``colour_tolerance`` defaults
    to one voxel) and written to ``path`` as a binary PLY (``geometry.save_ply_mesh``: a file that exists is left alone).
    ``bounds`` = ((x0, y0, z0), (x1, y1, z1)) is the box the grid covers; it defaults to the box of all valid pixels' points, padded
    by the truncation.  ``depth_range`` = (lo, hi): only pixels with lo <= depth <= hi are used.  Raises, naming the limit
    7 nx ny nz <= 2^31 - 1, when the grid is too large.  The mesh is in the model's processed scene frame.  Returns {'vertices'
    float32 (Nv,3), 'colours' uint8 (Nv,3), 'views' uint8 (Nv), 'triangles' int32 (Nt,3), 'tsdf' float32 (nz,ny,nx), 'weight' uint8
    (nz,ny,nx), 'lo', 'voxel_size', 'extents' (nx,ny,nz), 'truncation', 'images_device', 'depths_device'}, tensors on the device.
    ``normals=True`` adds 'normals' float32 (Nv,3): the unit outward normals of the density field at the vertices
    (``_field_normals_of``, as ``export_density_mesh`` has them), and the file's vertices carry them (``x y z nx ny nz red green
    blue``); the default writes the same bytes as before.  A model that ``query_gradient`` refuses is refused before anything is
    rendered."""
    from . import geometry
    cameras = list(cameras)
    field = _gradient_field('export_mesh', model, configs) if normals else None
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and math.isfinite(voxel_size)):
        raise RuntimeError(f'export_mesh: voxel_size: expected a finite number > 0, got {voxel_size}')
    truncation = 4.0 * voxel_size if truncation is None else float(truncation)
    colour_tolerance = voxel_size if colour_tolerance is None else float(colour_tolerance)
    images, depths, extrinsics, intrinsics, mask = _render_views('export_mesh', model, configs, cameras, device, depth_range)
    if bounds is None:
        points = geometry.fuse_depth_maps(depths, images, extrinsics, intrinsics, 0.0, 0, mask)[0]
        if points.shape[0] == 0:
            raise RuntimeError('export_mesh: no pixel has a valid depth, so there are no bounds to cover; pass bounds')
        low, high = torch.aminmax(points, dim=0)
        box = torch.cat([low, high]).cpu().numpy().astype(numpy.float64)
        low, high = box[:3] - truncation, box[3:] + truncation
    else:
        low, high = (numpy.asarray(b, dtype=numpy.float64).reshape(3) for b in bounds)
    if not (numpy.isfinite(low).all() and numpy.isfinite(high).all() and (high >= low).all()):
        raise RuntimeError(f'export_mesh: bounds {low.tolist()} .. {high.tolist()} are not a finite box')
    extents = tuple(int(math.floor((high[a] - low[a]) / voxel_size)) + 2 for a in range(3))     # (the last node at or past the bound)
    lo, voxel_size, extents = ops.mesh_grid(low.tolist(), voxel_size, extents)
    tsdf, weight = geometry.tsdf_volume(depths, extrinsics, intrinsics, lo, voxel_size, extents, truncation, mask)
    vertices, triangles = geometry.extract_mesh(tsdf, weight, lo, voxel_size, min_weight)
    colours, views = geometry.colour_points(vertices, depths, images, extrinsics, intrinsics, colour_tolerance, mask)
    out = {'vertices': vertices, 'colours': colours, 'views': views, 'triangles': triangles, 'tsdf': tsdf, 'weight': weight, 'lo': lo,
           'voxel_size': voxel_size, 'extents': extents, 'truncation': truncation, 'images_device': images, 'depths_device': depths}
    if normals:
        out['normals'] = _field_normals_of('export_mesh', field, configs, cameras, vertices)
        geometry.save_ply_mesh(path, vertices, colours, triangles, out['normals'])
    else:
        geometry.save_ply_mesh(path, vertices, colours, triangles)
    return out


@torch.no_grad()
def export_density_mesh(model, configs: dict, cameras, path, device, voxel_size: float, level: float, bounds, min_views: int = 1,
                        point_block: int = 1 << 20, normals: bool = False) -> dict:
    """The model's geometry as a triangle mesh of its density field, without a render: the nodes of a grid of ``voxel_size`` over the
    box ``bounds`` = ((x0, y0, z0), (x1, y1, z1)) (required: there are no depth maps to derive it from; the grid is made as
    ``export_mesh`` makes it) are mapped into the space the finest MLP reads -- the NDC warp when ``configs['data_loader']['ndc']``,
    with ``cameras[0]``'s frame, focal lengths and near plane -- and queried (``model.query``, in blocks of ``point_block``); the
    surface is the level set density = ``level`` (``geometry.density_volume``), extracted by marching tetrahedra over the cells
    whose eight corners at least ``min_views`` of ``cameras`` see (``geometry.extract_mesh``), every vertex coloured by the field
    as the nearest camera that sees it would see it (``geometry.colour_vertices``), written to ``path`` as a binary PLY
    (``geometry.save_ply_mesh``: a file that exists is left alone).  ``cameras`` are dicts as ``frame_batch`` takes them, of one
    resolution; with NDC they must also share the focal lengths and the near plane.  ``level`` is in the model's OWN density units:
    density per unit of the length its MLP's rays are marched in -- scene length for a model of world-space rays, NDC length (the
    whole scene depth is about 1) for a model of NDC rays, where useful levels are therefore far larger.  The mesh is in the model's
    processed scene frame, also for NDC models.  A ``DataParallel`` wrapper is unwrapped.  Raises, naming the limit
    7 nx ny nz <= 2^31 - 1, when the grid is too large.  Returns {'vertices' float32 (Nv,3), 'colours' uint8 (Nv,3), 'views' uint8
    (Nv): the camera each vertex is coloured from (``ops.FIELD_NO_VIEW``: none sees it), 'triangles' int32 (Nt,3), 'sigma', 'tsdf'
    float32 (nz,ny,nx), 'weight' uint8 (nz,ny,nx), 'lo', 'voxel_size', 'extents' (nx,ny,nz), 'level'}, tensors on the device.
    ``normals=True`` adds 'normals' float32 (Nv,3), the unit outward normals from the field's own gradient at the vertices
    (``model.query_gradient``, always fp32, in its own blocks of at most 2^16 points; ``geometry.field_normals``), in the scene
    frame, and the file's vertices carry them (``x y z nx ny nz red green blue``); the default writes the same bytes as before."""
    from . import geometry
    model = getattr(model, 'module', model) if isinstance(model, torch.nn.DataParallel) else model
    cameras = list(cameras)
    if not cameras:
        raise RuntimeError('export_density_mesh: no cameras')
    voxel_size, level = float(voxel_size), float(level)
    if not (voxel_size > 0.0 and math.isfinite(voxel_size)):
        raise RuntimeError(f'export_density_mesh: voxel_size: expected a finite number > 0, got {voxel_size}')
    if not (level > 0.0 and math.isfinite(level)):
        raise RuntimeError(f'export_density_mesh: level: expected a finite number > 0, got {level}')
    mlp = 'fine_mlp' if 'fine_mlp' in configs['model'] else 'coarse_mlp'
    if bool(configs['model'][mlp].get('predict_visibility', False)):
        raise NotImplementedError(f'export_density_mesh: {mlp} has predict_visibility, which point queries are not built for')
    resolution = tuple(int(v) for v in cameras[0]['resolution'])
    for i, camera in enumerate(cameras):
        if tuple(int(v) for v in camera['resolution']) != resolution:
            raise RuntimeError(f'export_density_mesh: camera {i} has resolution {tuple(camera["resolution"])}, camera 0 has {resolution}')
    ndc = None
    if bool(configs['data_loader']['ndc']):
        ndc = geometry.ndc_parameters(cameras[0])
        for i, camera in enumerate(cameras):
            if geometry.ndc_parameters(camera) != ndc:
                raise RuntimeError(f'export_density_mesh: ndc: camera {i} has (cx, cy, near) = {geometry.ndc_parameters(camera)}, camera 0 '
                                   f'has {ndc}; one NDC warp needs cameras of one resolution, focal length and near plane')
    low, high = (numpy.asarray(b, dtype=numpy.float64).reshape(3) for b in bounds)
    if not (numpy.isfinite(low).all() and numpy.isfinite(high).all() and (high >= low).all()):
        raise RuntimeError(f'export_density_mesh: bounds {low.tolist()} .. {high.tolist()} are not a finite box')
    extents = tuple(int(math.floor((high[a] - low[a]) / voxel_size)) + 2 for a in range(3))     # (the last node at or past the bound)
    lo, voxel_size, extents = ops.mesh_grid(low.tolist(), voxel_size, extents)
    matrices = [geometry.camera_matrices(camera) for camera in cameras]
    extrinsics, intrinsics = [m[0] for m in matrices], [m[1] for m in matrices]
    sigma, tsdf, weight = geometry.density_volume(lambda points: model.query(points, None, mlp, point_block)['sigma'], lo, voxel_size,
                                                  extents, extrinsics, intrinsics, resolution, level, ndc, point_block, device)
    vertices, triangles = geometry.extract_mesh(tsdf, weight, lo, voxel_size, min_views)
    colours, views = geometry.colour_vertices(lambda points, dirs: model.query(points, dirs, mlp, point_block)['rgb'], vertices,
                                              extrinsics, intrinsics, resolution, ndc)
    out = {'vertices': vertices, 'colours': colours, 'views': views, 'triangles': triangles, 'sigma': sigma, 'tsdf': tsdf,
           'weight': weight, 'lo': lo, 'voxel_size': voxel_size, 'extents': extents, 'level': level}
    if normals:
        gradient_block = min(int(point_block), 1 << 16)       # (a gradient block holds ~20 KB a point)
        out['normals'] = geometry.field_normals(lambda points: model.query_gradient(points, mlp, gradient_block)['grad'], vertices, ndc)
        geometry.save_ply_mesh(path, vertices, colours, triangles, out['normals'])
    else:
        geometry.save_ply_mesh(path, vertices, colours, triangles)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the trainer's two frame loops (src/Trainer01.py: run_validation :109-263, save_sample_images :319-350)
# per-sample outputs the reference deletes from every chunk before merging (:197-221)
VALIDATION_DROPPED_KEYS = tuple(
    f'{stem}_{level}' for level in ('coarse', 'fine') for stem in (
        'z_vals', 'z_vals_other', 'raw_sigma', 'raw_sigma_other', 'raw_rgb', 'raw_rgb_view_independent', 'raw_rgb_view_dependent',
        'raw_rgb_other', 'raw_rgb_view_independent_other', 'raw_rgb_view_dependent_other', 'raw_visibility', 'raw_visibility2',
        'alpha', 'visibility', 'weights', 'alpha_other', 'visibility_other', 'weights_other', 'rays_d2', 'rays_o2_ndc', 'rays_d2_ndc',
        'rgb_other', 'acc_other', 'depth_other', 'depth_var_other', 'depth_ndc_other', 'depth_var_ndc_other'))


def divide_batch(input_batch: dict, chunk_size: int) -> list:
    """A frame's batch in consecutive chunks (:130-145): what has one row per ray is sliced, ``common_data`` is copied (the loss
    computer unpacks it in place), everything else is shared."""
    n = input_batch['rays_o'].shape[0]
    chunks = []
    for start in range(0, n, chunk_size):
        chunk = {}
        for key, value in input_batch.items():
            if hasattr(value, 'shape') and len(value.shape) > 0 and value.shape[0] == n:
                chunk[key] = value[start:start + chunk_size]
            elif key == 'common_data':
                chunk[key] = dict(value)
            else:
                chunk[key] = value
        chunks.append(chunk)
    return chunks


def merge_chunks(chunks: list) -> dict:
    """The reference's merge of per-chunk dictionaries (:147-172), model outputs and loss dictionaries alike: a tensor of more than
    one element is concatenated along the rays, a one-element tensor (a loss value) becomes the PLAIN mean of the chunks' values --
    a short last chunk weighs as much as a full one -- and dictionaries are merged by the same rule, two levels deep (a loss's
    ``loss_value`` and its ``loss_maps``).  Anything else raises, as there."""
    def merge(values, depth):
        first = values[0]
        if isinstance(first, torch.Tensor):
            if depth == 2 or (depth == 0 and first.numel() > 1):
                return torch.cat(values, dim=0)
            if first.numel() == 1:
                return torch.mean(torch.stack(values))
        elif isinstance(first, dict) and depth < 2:
            return {key: merge([v[key] for v in values], depth + 1) for key in first}
        raise RuntimeError(f'merge_chunks: cannot merge {type(first).__name__} values at depth {depth}')

    return {key: merge([chunk[key] for chunk in chunks], 0) for key in chunks[0]}


def _validation_maps(outputs: dict, losses: Optional[dict], frame_num, frame_nums, iter_label: str):
    """[(file name without suffix, float tensor, is colour)] of one frame, in the reference's order (:233-259)."""
    maps = []
    for level in ('coarse', 'fine'):
        if f'rgb_{level}' not in outputs:
            continue
        stem = f'{frame_num:04}_{level}'
        maps.append((f'predicted_frames/{stem}_{iter_label}', outputs[f'rgb_{level}'], True))
        maps.append((f'predicted_depths/{stem}_{iter_label}', outputs[f'depth_{level}'], False))
        if f'depth_ndc_{level}' in outputs:
            maps.append((f'predicted_depths/{stem}_ndc_{iter_label}', outputs[f'depth_ndc_{level}'], False))
        maps.append((f'predicted_depths_variance/{stem}_{iter_label}', outputs[f'depth_var_{level}'], False))
        if f'depth_var_ndc_{level}' in outputs:
            maps.append((f'predicted_depths_variance/{stem}_ndc_{iter_label}', outputs[f'depth_var_ndc_{level}'], False))
        if f'visibility2_{level}' in outputs:
            for j, other in enumerate(x for x in frame_nums if x != frame_num):
                maps.append((f'predicted_visibilities/{frame_num:04}_{other:04}_{level}_{iter_label}',
                             outputs[f'visibility2_{level}'][:, j], False))
    for entry in (losses or {}).values():
        if isinstance(entry, dict):
            for fullname, loss_map in entry['loss_maps'].items():
                maps.append((f'Losses/{fullname}_{frame_num:04}_{iter_label}', loss_map, False))
    return maps


def _convert_and_write(maps, resolution, frame_num, save_dirpath, keep, write_floats: bool = True, png_encoder: str = 'host') -> None:
    """All maps of a frame through ONE ``ops.maps_to_u8`` call -- the colour as rows of mode 0 (save_image :384-387), every other map
    with mode 1 (save_numpy_array :397-409) -- then the reference's files: a PNG for the colour, ``.npy`` + PNG for the rest
    (``write_floats`` False: the PNG only, as save_sample_images writes).  ``png_encoder='device'``: the PNGs are encoded on the
    device, the frame's colour images in one ``png_files`` call and all its grey maps in a second; the 8-bit maps cross to the host
    only for ``keep``."""
    import os
    import numpy
    h, w = int(resolution[0]), int(resolution[1])
    n = h * w
    rows, modes, spans = [], [], []
    for stem, tensor, colour in maps:
        flat = tensor.detach().reshape(-1).float()
        if flat.numel() != (3 * n if colour else n):
            raise RuntimeError(f'{stem}: {tuple(tensor.shape)} is not a {h}x{w} {"colour frame" if colour else "map"}')
        spans.append((len(modes), flat.numel() // n))
        rows.append(flat)
        modes += [ops.MAP_SCALE_255 if colour else ops.MAP_SCALE_MAX] * (flat.numel() // n)
    on_device = _check_png_encoder(png_encoder)
    floats = torch.cat(rows).reshape(len(modes), n)
    bytes_device = ops.maps_to_u8(floats, modes)[0]
    bytes_host = bytes_device.cpu().numpy() if keep is not None or not on_device else None
    encoded = {}
    if on_device and save_dirpath is not None:
        for colour in (True, False):
            group = [(stem, first, count) for (stem, _, c), (first, count) in zip(maps, spans) if c == colour]
            if group:
                stack = torch.stack([bytes_device[first:first + count].reshape((h, w, 3) if colour else (h, w)) for _, first, count in group])
                encoded.update(zip((stem for stem, _, _ in group), png_files(stack)))
    floats_host = floats.cpu().numpy() if keep is not None or (save_dirpath is not None and write_floats) else None
    for (stem, _, colour), (first, count) in zip(maps, spans):
        shape = (h, w, 3) if colour else (h, w)
        as_u8 = None if bytes_host is None else bytes_host[first:first + count].reshape(shape)
        as_float = None if floats_host is None else floats_host[first:first + count].reshape(shape)
        if keep is not None:
            keep[(frame_num, stem)] = {'float': as_float, 'u8': as_u8}
        if save_dirpath is not None:
            path = os.path.join(os.fspath(save_dirpath), stem)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if not colour and write_floats:
                numpy.save(path + '.npy', as_float)
            with open(path + '.png', 'wb') as f:
                f.write(encoded[stem] if on_device else _png_bytes(as_u8))


def run_validation(model, loss_computer, data_preprocessor, iter_num: int, configs: dict, save_dirpath=None,
                   keep: Optional[dict] = None, png_encoder: str = 'host') -> Dict[str, float]:
    """Trainer.run_validation (src/Trainer01.py:109-263) over every view of ``data_preprocessor`` (a train- or validation-mode
    DataPreprocessor), on one rank: the model goes to eval mode (:184) and back to train mode at the end (:262); every frame's
    ``get_next_batch(iter_num, frame_num)`` is cut into chunks of ``configs['validation_chunk_size']``, each chunk rendered under
    no_grad as ``model(chunk, retraw=True, sec_views_vis=(data_preprocessor.mode == 'train'))`` and scored by
    ``compute_losses(chunk, out, return_loss_maps=configs['validation_save_loss_maps'])``; the per-sample outputs are dropped
    (:197-221) and the chunks merged by ``merge_chunks``.  Returns {loss name: mean over the frames of the frame's merged value}
    as Python floats (:110-122, :260-261); the loss values of a frame cross to the host in one copy.

    ``save_dirpath``: the reference's files under the reference's names (:233-259) -- ``predicted_frames/<frame>_<level>_Iter<n>.png``,
    and ``.npy`` + ``.png`` under ``predicted_depths/``, ``predicted_depths_variance/`` (with ``_ndc`` forms), ``predicted_visibilities/``
    and ``Losses/`` -- the 8-bit images from one ``ops.maps_to_u8`` call per frame, written by this module's PNG writer.
    ``keep``: a dict that receives ``{(frame_num, file name without suffix, relative to save_dirpath): {'float': array, 'u8': array}}``
    for the same arrays, with or without a directory.  ``png_encoder='device'``: the PNGs are encoded on the device (``png_files``: per
    frame one call for its colour images and one for its grey maps) -- the same file names, the same pixels, other bytes.

    A loss list that reads outputs an eval-mode model does not produce fails here as it does in the reference: the augmentation
    models run in training mode only (src/models/SimpleNeRF01.py:170, :186), so PointsAugmentationDepthLoss02 and its siblings index
    a missing key -- every shipped experiment sets ``validation_interval`` beyond ``num_iterations`` (NerfLlffTrainerTester01.py
    :438-441).  A loss whose result carries no ``loss_maps`` (the SparseDepthMSE family) fails with ``validation_save_loss_maps``
    as at :256; CoarseFineConsistencyLoss02 needs ``common_data``, which held-out views do not carry."""
    _check_png_encoder(png_encoder)
    resolution = data_preprocessor.preprocessed_data_dict['nerf_data']['resolution']
    chunk_size = int(configs['validation_chunk_size'])
    with_maps = bool(configs['validation_save_loss_maps'])
    train_data = data_preprocessor.mode == 'train'
    frame_nums = [int(f) for f in data_preprocessor.preprocessed_data_dict['frame_nums']]
    iter_label = f'Iter{iter_num + 1:05}'
    totals: Optional[Dict[str, float]] = None
    model.eval()
    for frame_num in frame_nums:
        outputs, losses = [], []
        for chunk in divide_batch(data_preprocessor.get_next_batch(iter_num, frame_num), chunk_size):
            with torch.no_grad():
                out = model(chunk, retraw=True, sec_views_vis=train_data)
            losses.append(loss_computer.compute_losses(chunk, out, return_loss_maps=with_maps))
            outputs.append({key: value for key, value in out.items() if key not in VALIDATION_DROPPED_KEYS})
        frame_outputs, frame_losses = merge_chunks(outputs), merge_chunks(losses)
        names = list(frame_losses) if totals is None else list(totals)
        values = torch.stack([(frame_losses[name]['loss_value'] if isinstance(frame_losses[name], dict) else frame_losses[name])
                              .detach().reshape(()).float() for name in names]).cpu().tolist()
        if totals is None:
            totals = dict.fromkeys(names, 0.0)
        for name, value in zip(names, values):
            totals[name] += value
        if save_dirpath is not None or keep is not None:
            maps = _validation_maps(frame_outputs, frame_losses if with_maps else None, frame_num, frame_nums, iter_label)
            _convert_and_write(maps, resolution, frame_num, save_dirpath, keep, png_encoder=png_encoder)
    model.train()
    return {name: value / len(frame_nums) for name, value in (totals or {}).items()}


def save_sample_images(model, configs: dict, preprocessors, iter_num: int, save_dirpath, keep: Optional[dict] = None,
                       png_encoder: str = 'host') -> None:
    """Trainer.save_sample_images (:319-350): every view of every preprocessor in ``preprocessors`` (the reference's pair: train,
    validation) rendered from its stored processed pose -- ``create_test_data(pose, preprocess_pose=False)`` of the FIRST
    preprocessor, the model under no_grad in eval mode, the outputs of ``retrieve_inference_outputs`` (8-bit colour, depths clipped
    at 0; ``display_outputs``: they stay on the device) -- and written as PNGs: ``predicted_frames/<frame>_Iter<n>.png``,
    ``predicted_depths[_variance]/<frame>[_ndc]_Iter<n>.png``.  The depth previews come from one ``ops.maps_to_u8`` call per frame, so a
    frame crosses to the host as bytes.  ``keep`` as in ``run_validation`` (the colour has no 'float' entry).
    ``png_encoder='device'``: the PNGs are encoded on the device (``png_files``), the frame crosses as the bytes of its files."""
    import os
    import numpy
    on_device = _check_png_encoder(png_encoder)
    first = preprocessors[0]
    resolution = first.get_model_configs()['resolution']
    iter_label = f'Iter{iter_num:05}'
    model.eval()
    for preprocessor in preprocessors:
        view = preprocessor.preprocessed_data_dict
        for frame_num, pose in zip(view['frame_nums'].tolist(), view['nerf_data']['poses']):
            if pose.shape[0] == 3:
                pose = numpy.concatenate([pose, numpy.array([0, 0, 0, 1], dtype=pose.dtype)[None]], axis=0)
            with torch.no_grad():
                outputs = model(first.create_test_data(pose, preprocess_pose=False))
            predictions = display_outputs(first.configs, resolution, outputs)
            names = [(f'predicted_depths/{frame_num:04}_{iter_label}', 'depth'), (f'predicted_depths/{frame_num:04}_ndc_{iter_label}', 'depth_ndc'),
                     (f'predicted_depths_variance/{frame_num:04}_{iter_label}', 'depth_var'),
                     (f'predicted_depths_variance/{frame_num:04}_ndc_{iter_label}', 'depth_var_ndc')]
            maps = [(stem, predictions[name], False) for stem, name in names if name in predictions]
            _convert_and_write(maps, resolution, frame_num, save_dirpath, keep, write_floats=False, png_encoder=png_encoder)
            stem = f'predicted_frames/{frame_num:04}_{iter_label}'
            image = predictions['image'].cpu().numpy() if keep is not None or not on_device else None
            if keep is not None:
                keep[(frame_num, stem)] = {'u8': image}
            save_image(os.path.join(os.fspath(save_dirpath), stem + '.png'), predictions['image'] if on_device else image, png_encoder)
    model.train()
