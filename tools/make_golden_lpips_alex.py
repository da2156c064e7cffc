#!/usr/bin/env python3
"""Record what the AlexNet LPIPS path returns on an MI355X: tests/golden/lpips_alex_sums.npz, which tests/test_gpu_lpips_vgg.py
compares bit for bit (the VGG-16 path shares csrc/lpips.hip with it and must not move its results).
    python tools/make_golden_lpips_alex.py [out.npz]
Per seeded case of tests/lpips_reference.py (SHAPES, random_images, random_weights): the five float64 layer sums of
ops.lpips_sums, plain and with the case's mask.  Recorded at the commit before the VGG-16 backbone was added; regenerate it only
when the AlexNet arithmetic is changed on purpose."""
import os
import sys

import numpy
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from simplenerf_amd import ops, qa  # noqa: E402
from tests import lpips_reference  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'tests', 'golden', 'lpips_alex_sums.npz')
    dev = torch.device('cuda', 0)
    weights = qa.LpipsWeights(lpips_reference.random_weights(), dev)
    arrays = {}
    for h, w in lpips_reference.SHAPES:
        gt, image, mask = (torch.as_tensor(a).to(dev) for a in lpips_reference.random_images(h, w))
        arrays[f'plain_{h}x{w}'] = ops.lpips_sums(gt, image, weights.packed).cpu().numpy()
        arrays[f'masked_{h}x{w}'] = ops.lpips_sums(gt, image, weights.packed, mask).cpu().numpy()
        print(h, w, arrays[f'plain_{h}x{w}'].tolist(), arrays[f'masked_{h}x{w}'].tolist())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    numpy.savez(out, **arrays)
    print('wrote', out)


if __name__ == '__main__':
    main()
