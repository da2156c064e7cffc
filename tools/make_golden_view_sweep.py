#!/usr/bin/env python3
"""Golden vectors for the static-camera view sweep, made by RUNNING THE REFERENCE (DataPreprocessor.create_test_data with a view
camera and secondary cameras, SimpleNeRF in eval mode) on the CPU.

    SIMPLENERF_REFERENCE_SRC=<reference checkout>/src PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_view_sweep.py

tests/golden/view_sweep.npz holds, for the NDC scene ``scene_prep_ndc_sparse`` and the world-space, white-background scene
``scene_prep_world_dense`` (their saved model configs, at a 7 x 11 frame: 77 rays, no multiple of 32), under the keys ``<case>_...``:
  pose, view_poses (3), view_intrinsics (3: the first is a camera of its own, the others the scene's), secondary_poses (2),
  secondary_intrinsics (2), model_configs_json (the scene's, at the small resolution)
  batch_<key>        create_test_data(pose, view_poses[0], secondary_poses, True, intrinsic, view_intrinsics[0], secondary_intrinsics)
  view_dirs          (3, 77, 3): create_test_data's view_dirs under each view camera
  seed, ovr_*, fine_equals_coarse   the weights: synth.synth_state_dict(seed) + calibrated density head, fine = coarse (the
                     'consistent' recipe of tools/make_golden.py: it keeps the resampled depths off sample_pdf's discontinuity)
  out_<key>          the eval outputs (retraw=True) that do not depend on the view camera, asserted equal over the three runs
                     (z_vals, weights, acc, depths), and out_rgb_fine (3, 77, 3) per view camera
skimage is stubbed as in tools/make_golden_scene.py (downsampling_factor is 1).
"""
import json
import os
import sys
import types

import numpy
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ['SIMPLENERF_REFERENCE_SRC'])       # the src/ directory of a checkout of the reference
for name in ('skimage', 'skimage.io', 'skimage.transform'):
    sys.modules.setdefault(name, types.ModuleType(name))

from data_preprocessors.DataPreprocessor01 import DataPreprocessor  # noqa: E402  (the reference)
from models.SimpleNeRF01 import SimpleNeRF  # noqa: E402  (the reference)

from simplenerf_amd import synth  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
RESOLUTION = (7, 11)
CASES = (('ndc', 'ndc_sparse', 301), ('world', 'world_dense', 302))
SHARED = ('z_vals_coarse', 'z_vals_fine', 'weights_coarse', 'weights_fine', 'acc_coarse', 'acc_fine', 'depth_fine', 'depth_var_fine',
          'depth_ndc_fine', 'depth_var_ndc_fine')
torch.set_num_threads(8)


def camera_pose(rng, spread):
    pose = numpy.eye(4)
    pose[:3, :3] = synth._rotation(*(spread * rng.standard_normal(3)))
    pose[:3, 3] = [0.3 * rng.standard_normal(), 0.2 * rng.standard_normal(), 0.1 * rng.standard_normal()]
    return pose


def calibrate_density(model, batch):
    """tools/make_golden.py's calibration of the coarse density head: its pre-activation on this batch re-centred on the median and
    scaled so that the 90th percentile maps to sigma = 30 (a random field is otherwise almost transparent)."""
    head = model.coarse_model.pts_output_linear
    seen = []
    hook = head.register_forward_hook(lambda m, i, o: seen.append(o[..., 0].detach()))
    with torch.no_grad():
        model(batch)
    hook.remove()
    raw = torch.cat([c.reshape(-1) for c in seen])
    median = raw.median()
    gain = 30.0 / (torch.quantile(raw[:200000], 0.9) - median)
    with torch.no_grad():
        head.weight[0] *= gain
        head.bias[0] = gain * (head.bias[0] - median)
    return {'ovr_coarse_model.pts_output_linear.weight': head.weight.detach().clone(),
            'ovr_coarse_model.pts_output_linear.bias': head.bias.detach().clone()}


def main():
    arrays = {}
    for tag, scene, seed in CASES:
        with numpy.load(os.path.join(OUT, f'scene_prep_{scene}.npz'), allow_pickle=False) as z:
            scene_configs = json.loads(str(z['configs_json']))
            saved = json.loads(str(z['model_configs_json']))
        h, w = RESOLUTION
        saved['resolution'] = [h, w]
        saved['intrinsic'] = [[14.0, 0.0, w / 2], [0.0, 13.5, h / 2], [0.0, 0.0, 1.0]]
        tester = DataPreprocessor(scene_configs, mode='test', model_configs=saved)
        rng = numpy.random.RandomState(seed)
        pose = camera_pose(rng, 0.05)
        view_poses = [camera_pose(rng, 0.3) for _ in range(3)]
        own = numpy.array([[11.0, 0.0, w / 2 + 0.75], [0.0, 12.5, h / 2 - 0.5], [0.0, 0.0, 1.0]])
        scene_intrinsic = numpy.array(saved['intrinsic'])
        view_intrinsics = [own, scene_intrinsic, scene_intrinsic]
        secondary_poses = [camera_pose(rng, 0.1) for _ in range(2)]
        secondary_intrinsics = [scene_intrinsic, own]

        batch = tester.create_test_data(pose, view_poses[0], secondary_poses, True, scene_intrinsic, view_intrinsics[0],
                                        secondary_intrinsics)
        view_batches = [tester.create_test_data(pose, vp, None, True, scene_intrinsic, vi) for vp, vi in zip(view_poses, view_intrinsics)]
        assert torch.equal(view_batches[0]['view_dirs'], batch['view_dirs'])
        plain = tester.create_test_data(pose, None, None, True, scene_intrinsic)
        assert not torch.equal(plain['view_dirs'], batch['view_dirs']) and torch.equal(plain['rays_d'], batch['rays_d'])

        ndc = bool(scene_configs['data_loader']['ndc'])
        configs = synth.with_overrides(synth.make_configs('config2'), white_bkgd=bool(scene_configs['model']['white_bkgd']))
        configs['data_loader']['ndc'] = ndc
        model = SimpleNeRF(configs, None)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()})
        model.eval()
        overrides = calibrate_density(model, view_batches[0])
        model.fine_model.load_state_dict(model.coarse_model.state_dict())          # the 'consistent' recipe: fine = coarse
        with torch.no_grad():
            outs = [model(b, retraw=True) for b in view_batches]
        for key in SHARED:
            if key in outs[0]:
                assert all(torch.equal(o[key], outs[0][key]) for o in outs[1:]), key
                arrays[f'{tag}_out_{key}'] = outs[0][key].numpy()
        assert not torch.equal(outs[0]['rgb_fine'], outs[1]['rgb_fine'])
        arrays[f'{tag}_out_rgb_fine'] = numpy.stack([o['rgb_fine'].numpy() for o in outs])
        print(f'{tag}: acc_fine mean {float(outs[0]["acc_fine"].mean()):.3f}, colour spread over the view cameras '
              f'{float((outs[0]["rgb_fine"] - outs[1]["rgb_fine"]).abs().max()):.3f}')

        arrays.update({f'{tag}_seed': numpy.int64(seed), f'{tag}_fine_equals_coarse': numpy.int64(1),
                       f'{tag}_pose': pose, f'{tag}_view_poses': numpy.stack(view_poses),
                       f'{tag}_view_intrinsics': numpy.stack(view_intrinsics), f'{tag}_secondary_poses': numpy.stack(secondary_poses),
                       f'{tag}_secondary_intrinsics': numpy.stack(secondary_intrinsics), f'{tag}_intrinsic': scene_intrinsic,
                       f'{tag}_model_configs_json': numpy.array(json.dumps(saved)),
                       f'{tag}_scene_configs_json': numpy.array(json.dumps(scene_configs)),
                       f'{tag}_view_dirs': numpy.stack([b['view_dirs'].numpy() for b in view_batches])})
        arrays.update({f'{tag}_{k}': v.numpy() for k, v in overrides.items()})
        arrays.update({f'{tag}_batch_{k}': v.numpy() for k, v in batch.items()})
    path = os.path.join(OUT, 'view_sweep.npz')
    numpy.savez_compressed(path, **arrays)
    print(f'{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays')


if __name__ == '__main__':
    main()
