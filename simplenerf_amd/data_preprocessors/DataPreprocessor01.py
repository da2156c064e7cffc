"""From what the data loader returns to training batches and test frames, behind the reference's ``DataPreprocessor`` interface
(src/data_preprocessors/DataPreprocessor01.py): ``DataPreprocessor(configs, mode, raw_data_dict=None, model_configs=None)``.

``mode='train'`` takes the loader's ``raw_data_dict`` -- ``frame_nums`` (V,), ``nerf_data`` {``images`` (V,h,w,3|4) uint8,
``extrinsics`` (V,4,4) world-to-camera, ``intrinsics`` (V,3,3), ``bounds`` (2,), ``resolution`` (h,w)} [, ``sparse_depth_data``
{frame number: table with columns x, y, depth, reprojection_error -- a pandas DataFrame or a plain dict of arrays}]
[, ``dense_depth_data`` {``depth_values``, ``depth_weights`` (V,h,w)}] -- and builds the ``scene`` of ``BatchAssembler`` where it
is read:
  * poses: recentred, rescaled and turned to the NeRF axes on the host in float64 (V 4x4 matrices: ``prepare_poses`` below
    restates preprocess_poses :937-976 with compute_average_pose, recenter_poses and convert_pose_to_standard_coordinates, same
    operation order, float32 at the end), near / far by the rules of :144-159;
  * images: uint8 -> float (white background optional) by ``ops.scene_images`` (:929-935);
  * sparse depth: every view's COLMAP points in one upload, rasterised by ``ops.rasterise_sparse_depth`` (:163-185 -- last point in
    input order wins a shared pixel; a frame number absent from the dictionary leaves its view at -1) with the NDC table (:448-452,
    near plane 1) from the same launch;
  * dense depth: ``depth_values * sc`` in the input's own dtype, then float32 (:191, :468); weights pass through;
    ``depth_values_ndc`` by ``ops.depth_table_to_ndc`` with the scene's near (:474-478).
No ray cache is built and nothing per pixel is computed on the host.  ``get_next_batch(iter_num, image_num=None, **kw)`` is the
owned ``BatchAssembler``'s (``indices=`` / ``indices_sparse=`` replay a given order; ``rank`` / ``world_size`` pass through), and
``get_model_configs()`` returns the reference's dictionary (:65-80; JSON-serialisable).

``mode='validation'`` (the held-out views of the reference's trainer, :44-48) takes the loader's dictionary for those views and the
train-mode preprocessor's ``get_model_configs()``, which it returns unchanged: poses by the test-mode rule with the training scene's
``translation_scale`` and ``average_pose``, the loader's ``bounds`` times that scale, near / far by the same rules over THOSE bounds
(:144-159), images on the device, float32 intrinsics -- and no sparse- or dense-depth tables, whatever the loader sections say
(:92-99: train mode only; ``raw_data_dict`` need not carry them).  Its ``get_next_batch(iter_num, image_num)`` is the reference's
validation batch: ``common_data`` empty, no sparse, dense or shared-scene entries (:528-543).

Both modes keep a small host-side ``preprocessed_data_dict`` -- ``frame_nums`` and ``nerf_data`` {``resolution``, ``poses``,
``intrinsics``, ``bounds``, ``near``, ``far`` [, ``near_ndc``, ``far_ndc``], ``average_pose`` [, ``sc``]} -- which with ``mode`` is what
the reference's ``Trainer.run_validation`` and ``save_sample_images`` read of a preprocessor (src/Trainer01.py:180, :187, :333-334).

``create_test_data(pose, preprocess_pose=True, intrinsic=None)`` (any mode with model configs) returns the reference's device batch
(:851-869) for a raw world-to-camera pose: ``rays_o``, ``rays_d``, ``view_dirs``, ``near``, ``far`` [, ``rays_o_ndc``, ``rays_d_ndc``,
``near_ndc``, ``far_ndc``], generated on the device (``harness.frame_batch``).  ``retrieve_inference_outputs`` is the harness's.

Refused by name (NotImplementedError): ``downsampling_factor > 1`` (the reference rescales with skimage's anti-aliased filter, which
this build has no restatement of and no fixture for), ``spherify`` (the reference's own path raises: ``self.normalize`` does not
exist, :1050), ``visibility_prior`` and ``mip_nerf`` loader sections (their losses / radii are not built), ``batching: False``, and
``view_pose`` / ``secondary_poses`` of ``create_test_data`` (rendering under other cameras' view directions is not part of this
build).  Non-finite point coordinates raise ValueError (the reference casts them to an undefined integer).  The caller's arrays are
never modified (the reference scales ``bounds`` in place).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy
import torch

from .. import harness, ops
from .BatchAssembler01 import BatchAssembler

POINT_COLUMNS = ('x', 'y', 'depth', 'reprojection_error')


# ------------------------------------------------------------------------------------------------------ host side: poses
def compute_average_pose(poses: numpy.ndarray) -> numpy.ndarray:
    """World-to-camera average of (V,4,4) world-to-camera poses (:992-1017): mean camera centre, summed z and y axes."""
    unit = lambda a: a / numpy.linalg.norm(a)
    to_world = numpy.transpose(poses[:, :3, :3], axes=[0, 2, 1])
    centres = -to_world @ poses[:, :3, 3:]
    centre = numpy.mean(centres, axis=0)[:, 0]
    z = unit(unit(to_world[:, :3, 2].sum(0)))      # the reference normalises the summed axis twice (:1013, then viewmatrix :997)
    up = to_world[:, :3, 1].sum(0)
    x = unit(numpy.cross(up, z))
    y = unit(numpy.cross(z, x))
    c2w = numpy.concatenate([numpy.stack([x, y, z, centre], 1), numpy.array([0, 0, 0, 1])[None]], axis=0)
    return numpy.linalg.inv(c2w)


def to_standard_coordinates(poses: numpy.ndarray) -> numpy.ndarray:
    """(x,-y,-z) of Colmap / RE10K -> NeRF's (x,y,z): r -> p.T r p, t -> p t with p = diag(1,-1,-1) (:983-989, :1020-1030)."""
    p = numpy.eye(3)
    p[1, 1] = p[2, 2] = -1
    return numpy.stack([numpy.concatenate([numpy.concatenate([p.T @ m[:3, :3] @ p, p @ m[:3, 3:]], axis=1), m[3:]], axis=0)
                        for m in poses])


def _own_bounds(bounds) -> numpy.ndarray:
    """A copy in the caller's floating dtype (the reference scales the loader's array in place, in its dtype)."""
    bounds = numpy.array(bounds)
    return bounds if numpy.issubdtype(bounds.dtype, numpy.floating) else bounds.astype(numpy.float64)


def prepare_poses(poses, bounds=None, *, train_mode: bool, bd_factor=None, recenter: bool = True, translation_scale=None,
                  average_pose=None) -> dict:
    """preprocess_poses (:937-976) on copies: ``poses`` (V,4,4) world-to-camera -> {'poses': (V,4,4) float32 processed
    camera-to-world, 'average_pose' [, 'sc', 'bounds']}.  Train mode derives the scale from ``bounds[0] * bd_factor`` (1 without a
    factor) and the average pose from the poses (identity without ``recenter``); test mode is given both."""
    poses = numpy.array(poses, dtype=numpy.float64)
    out = {}
    if train_mode:
        if bounds is not None:
            bounds = _own_bounds(bounds)
            sc = 1. / (float(bounds[0]) * bd_factor) if bd_factor is not None else 1
            poses[:, :3, 3] *= sc
            out['sc'], out['bounds'] = sc, bounds * sc
        average_pose = compute_average_pose(poses) if recenter else numpy.eye(4)
    else:
        poses[:, :3, 3] *= translation_scale
        if bounds is not None:
            out['bounds'] = _own_bounds(bounds) * translation_scale
        average_pose = numpy.array(average_pose, dtype=numpy.float64)
    out['average_pose'] = average_pose
    centred = average_pose[None] @ numpy.linalg.inv(poses)          # recenter_poses (:979-981)
    out['poses'] = to_standard_coordinates(centred).astype(numpy.float32)
    return out


def near_far(bounds, ndc: bool, bd_factor) -> dict:
    """The near / far rules of preprocess_raw_nerf_data (:144-159) over the scaled bounds."""
    if not ndc:
        return {'near': float(bounds[0] * .9), 'far': float(bounds[1] * 1.)}
    return {'near': float(bounds[0] * (bd_factor if bd_factor is not None else 1)), 'far': float(bounds[1]),
            'near_ndc': 0., 'far_ndc': 1.}


# ------------------------------------------------------------------------------------------------------ host side: the rest
def refuse_unbuilt(configs: dict) -> None:
    loader = configs['data_loader']
    if loader.get('downsampling_factor', 1) > 1:
        raise NotImplementedError("downsampling_factor > 1: the reference rescales images and depth maps with skimage's anti-aliased "
                                  "filter, which is not restated here; downsample the data set instead")
    if loader.get('spherify', False):
        raise NotImplementedError("spherify: the reference's own spherify_poses raises (self.normalize does not exist); not built")
    if 'visibility_prior' in loader:
        raise NotImplementedError('visibility_prior: the visibility losses are not built, so their masks and weights are not loaded')
    if 'mip_nerf' in loader:
        raise NotImplementedError('mip_nerf: ray radii are not built')
    if not loader.get('batching', True):
        raise NotImplementedError('batching: False: only random batches over all views are built (the reference calls its own '
                                  'uncached path unmaintained)')


def collect_points(raw_data_dict: dict) -> Dict[str, numpy.ndarray]:
    """The sparse-depth points of all views in input order: float64 x, y, depth, reprojection_error and the int32 view (position
    in ``frame_nums``) of each.  A frame number without an entry contributes none."""
    tables = raw_data_dict.get('sparse_depth_data', {})
    column = lambda table, name: numpy.asarray(table[name].to_numpy() if hasattr(table[name], 'to_numpy') else table[name],
                                               dtype=numpy.float64).reshape(-1)
    parts = {name: [numpy.zeros((0,))] for name in POINT_COLUMNS}
    views = [numpy.zeros((0,), dtype=numpy.int32)]
    for view, frame_num in enumerate(numpy.asarray(raw_data_dict['frame_nums']).tolist()):
        if frame_num not in tables:
            continue
        table = tables[frame_num]
        for name in POINT_COLUMNS:
            parts[name].append(column(table, name))
        views.append(numpy.full(parts['x'][-1].shape, view, dtype=numpy.int32))
    points = {name: numpy.concatenate(chunks) for name, chunks in parts.items()}
    points['view'] = numpy.concatenate(views)
    if len({a.shape[0] for a in points.values()}) != 1:
        raise ValueError('sparse_depth_data: the columns of a frame have different lengths')
    for name in ('x', 'y'):
        if not numpy.isfinite(points[name]).all():
            raise ValueError(f'sparse_depth_data: non-finite {name} coordinates (the reference casts them to an undefined integer)')
    return points


def prepare_host(configs: dict, raw_data_dict: dict, mode: str = 'train', model_configs: Optional[dict] = None) -> dict:
    """Everything that is decided on the host, from copies of the loader's arrays: processed poses, float32 intrinsics, scale,
    bounds, average pose, near / far and -- with a ``sparse_depth`` loader section -- the concatenated points."""
    loader = configs['data_loader']
    nerf = raw_data_dict['nerf_data']
    train = mode == 'train'
    if train:
        host = prepare_poses(nerf['extrinsics'], nerf['bounds'], train_mode=True, bd_factor=loader['bd_factor'],
                             recenter=bool(loader['recenter_camera_poses']))
    else:
        host = prepare_poses(nerf['extrinsics'], nerf['bounds'], train_mode=False, translation_scale=model_configs['translation_scale'],
                             average_pose=model_configs['average_pose'])
    host.update(near_far(host['bounds'], bool(loader['ndc']), loader['bd_factor']))
    host['resolution'] = [int(x) for x in nerf['resolution']]
    host['intrinsics'] = numpy.array(nerf['intrinsics']).astype(numpy.float32)
    host['frame_nums'] = numpy.array(raw_data_dict['frame_nums'])
    if train and 'sparse_depth' in loader:
        host['points'] = collect_points(raw_data_dict)
    return host


def create_model_configs(host: dict, ndc: bool, mode: str = 'train') -> dict:
    """The dictionary the reference saves next to a model (:65-80)."""
    model_configs = {
        'resolution': list(host['resolution']),
        'bounds': host['bounds'].tolist(),
        'translation_scale': host.get('sc', 1),
        f'{mode}_frame_nums': host['frame_nums'].tolist(),
        'intrinsic': numpy.mean(host['intrinsics'], axis=0).tolist(),
        'average_pose': host['average_pose'].tolist(),
        'near': host['near'],
        'far': host['far'],
    }
    if ndc:
        model_configs['near_ndc'], model_configs['far_ndc'] = host['near_ndc'], host['far_ndc']
    return model_configs


def host_view(host: dict, ndc: bool) -> dict:
    """``preprocessed_data_dict`` as far as the reference's trainer reads it (src/Trainer01.py:180, :187, :333-334): the frame numbers
    and the per-view host values.  Nothing per pixel: images, rays and depth tables live on the device (``scene``)."""
    names = ['resolution', 'poses', 'intrinsics', 'bounds', 'near', 'far'] + (['near_ndc', 'far_ndc'] if ndc else []) + ['average_pose']
    nerf = {name: host[name] for name in names}
    if 'sc' in host:
        nerf['sc'] = host['sc']
    return {'frame_nums': host['frame_nums'], 'nerf_data': nerf}


# ------------------------------------------------------------------------------------------------------ the class
class DataPreprocessor:
    def __init__(self, configs: dict, mode: str, raw_data_dict: Optional[dict] = None, model_configs: Optional[dict] = None,
                 device=None, rank: int = 0, world_size: int = 1):
        self.configs = configs
        self.mode = mode.lower()
        loader = configs['data_loader']
        refuse_unbuilt(configs)
        self.ndc = bool(loader['ndc'])
        self.bd_factor = loader['bd_factor']
        self.sparse_depth_needed = 'sparse_depth' in loader
        self.dense_depth_needed = 'dense_depth' in loader
        if device is None:
            devices = configs.get('device', [0])
            first = devices[0] if isinstance(devices, (list, tuple)) else devices
            device = first if isinstance(first, (str, torch.device)) else f'cuda:{int(first)}'
        self.device = torch.device(device)
        self.raw_data_dict = raw_data_dict
        self.model_configs = model_configs
        self.scene = self.assembler = self.preprocessed_data_dict = None
        if self.mode in ('train', 'validation'):
            if self.mode == 'train':
                host = prepare_host(configs, raw_data_dict, 'train')
                self.model_configs = create_model_configs(host, self.ndc, 'train')
            else:
                if model_configs is None:
                    raise RuntimeError("mode 'validation': needs the train-mode preprocessor's get_model_configs()")
                # the sparse / dense loader sections are train-mode only (:92-99): no table is built, none need be given
                self.sparse_depth_needed = self.dense_depth_needed = False
                host = prepare_host(configs, raw_data_dict, 'validation', model_configs)
            self.scene = self.build_scene(host, raw_data_dict)
            self.assembler = BatchAssembler(configs, self.scene, device=self.device, rank=rank, world_size=world_size, mode=self.mode)
            self.preprocessed_data_dict = host_view(host, self.ndc)

    def get_model_configs(self):
        return self.model_configs

    # -------------------------------------------------------------------------------------------------- the scene, on the device
    def build_scene(self, host: dict, raw_data_dict: dict) -> dict:
        if self.device.type != 'cuda':
            raise RuntimeError(f'DataPreprocessor: the scene is built on the GPU (there is no CPU path), got device {self.device}')
        dev = self.device
        h, w = host['resolution']
        views = host['poses'].shape[0]
        images = numpy.ascontiguousarray(raw_data_dict['nerf_data']['images'])
        if images.dtype != numpy.uint8 or images.shape[:3] != (views, h, w):
            raise RuntimeError(f'images: expected uint8 ({views}, {h}, {w}, 3 or 4), got {images.dtype} {images.shape}')
        poses = torch.from_numpy(host['poses']).to(dev)
        intrinsics = torch.from_numpy(host['intrinsics']).to(dev)
        scene = {'poses': poses, 'intrinsics': intrinsics, 'resolution': (h, w), 'frame_nums': host['frame_nums'].tolist(),
                 'images': ops.scene_images(torch.from_numpy(images).to(dev), bool(self.configs['model']['white_bkgd']))}
        scene.update({k: host[k] for k in ('near', 'far', 'near_ndc', 'far_ndc') if k in host})
        table = ops.camera_table(intrinsics, poses, (h, w)) if self.ndc else None
        if self.sparse_depth_needed:
            p = host['points']
            tables = ops.rasterise_sparse_depth(p['x'], p['y'], p['depth'], p['reprojection_error'], p['view'], views, (h, w),
                                                scale=host['sc'], table=table, near=1.0, device=dev)    # near 1: :450
            scene.update(sparse_depths=tables['depths'], sparse_errors=tables['errors'], sparse_depths_ndc=tables.get('depths_ndc'))
        if self.dense_depth_needed:
            dense = raw_data_dict['dense_depth_data']
            depths = (numpy.asarray(dense['depth_values']) * host['sc']).astype(numpy.float32)     # in the input's dtype first
            weights = numpy.asarray(dense['depth_weights']).astype(numpy.float32)
            if depths.shape != (views, h, w) or weights.shape != (views, h, w):
                raise RuntimeError(f'dense_depth_data: expected ({views}, {h}, {w}) maps, got {depths.shape} and {weights.shape}')
            scene['dense_depths'] = torch.from_numpy(depths).to(dev).reshape(-1)
            scene['dense_depth_weights'] = torch.from_numpy(weights).to(dev).reshape(-1)
            if self.ndc:
                scene['dense_depths_ndc'] = ops.depth_table_to_ndc(scene['dense_depths'], table, (h, w), host['near'])
        return scene

    # -------------------------------------------------------------------------------------------------- batches
    def get_next_batch(self, iter_num: int, image_num: Optional[int] = None, **kwargs):
        if self.assembler is None:
            raise RuntimeError(f"get_next_batch: mode '{self.mode}' has no scene (construct with mode='train' or 'validation')")
        return self.assembler.get_next_batch(iter_num, image_num, **kwargs)

    # -------------------------------------------------------------------------------------------------- inference
    def camera(self, pose: numpy.ndarray, intrinsic: Optional[numpy.ndarray] = None, preprocess_pose: bool = True) -> dict:
        """The camera dict of ``harness.frame_batch`` for a raw pose (``preprocess_pose``: recentred and scaled like the training
        poses) or an already processed one, with the scene's intrinsic unless one is given."""
        if self.model_configs is None:
            raise RuntimeError('create_test_data: no model configs (train mode derives them; other modes are given them)')
        cfg = self.model_configs
        if preprocess_pose:
            processed = prepare_poses(numpy.asarray(pose)[None], train_mode=False, translation_scale=cfg['translation_scale'],
                                      average_pose=cfg['average_pose'])['poses'][0]
        else:
            processed = numpy.asarray(pose).astype(numpy.float32)
        intrinsic = numpy.array(cfg['intrinsic'] if intrinsic is None else intrinsic).astype(numpy.float32)
        camera = {'resolution': tuple(int(x) for x in cfg['resolution']), 'intrinsic': intrinsic, 'pose': processed,
                  'near': cfg['near'], 'far': cfg['far']}
        if self.ndc:
            camera.update(near_ndc=cfg['near_ndc'], far_ndc=cfg['far_ndc'])
        return camera

    def create_test_data(self, pose: numpy.ndarray, view_pose=None, secondary_poses=None, preprocess_pose: bool = True,
                         intrinsic: Optional[numpy.ndarray] = None, view_intrinsic=None, secondary_intrinsics=None):
        if view_pose is not None or view_intrinsic is not None:
            raise NotImplementedError("create_test_data(view_pose=...): rendering a pose under another camera's view directions is "
                                      "not part of this call -- use harness.frame_batch(self.camera(pose), ndc, device, "
                                      "view_camera=self.camera(view_pose, view_intrinsic)) or harness.predict_view_sweep")
        if secondary_poses is not None or secondary_intrinsics is not None:
            raise NotImplementedError('create_test_data(secondary_poses=...): secondary-view origins (rays_o2) are not built by this '
                                      'call -- use harness.frame_batch(..., secondary_cameras=[self.camera(p) for p in secondary_poses])')
        return harness.frame_batch(self.camera(pose, intrinsic, preprocess_pose), self.ndc, self.device)

    def retrieve_inference_outputs(self, network_outputs: dict):
        return harness.retrieve_inference_outputs(self.configs, self.model_configs['resolution'], network_outputs)
