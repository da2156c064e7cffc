#!/usr/bin/env python3
"""Soak of the side-by-side levels (csrc/render.hip): N training iterations at 512 rows per batch (32 768 coarse samples per
sub-batch call: every level side by side), eager, on a given build of the library; prints the final loss, the PSNR of a training
view and a SHA-256 of every parameter.  Run once on each of two builds of the library (profiles/r05_soak_side_by_side.jsonl: the
shipped one and a build whose levels ran in order): identical arithmetic in another stream arrangement must give the SAME
hash -- a race between levels would not.
    usage: soak_side_by_side.py <lib.so> [iterations] [precision]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402
from simplenerf_amd import _lib  # noqa: E402

_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from simplenerf_amd import harness, optim, synth  # noqa: E402
from simplenerf_amd.data_preprocessors.BatchAssembler01 import BatchAssembler  # noqa: E402
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402
import train_demo  # noqa: E402

iters = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
precision = sys.argv[3] if len(sys.argv) > 3 else 'f16'
dev = torch.device('cuda', 0)
cfg = synth.training_configs(precision, num_rays=384, num_sparse=128, seed=4)
cfg['model']['hip_host_binding'] = 'ctypes'
cfg['sub_batch_size'] = 256
cfg['losses'] = synth.loss_configs(iter_weighted=False)
scene = synth.training_scene(0, 3, 96, 128, sparse_fraction=0.02)
torch.manual_seed(4)
model = get_model(cfg, None).to(dev).train()
batcher, losses = BatchAssembler(cfg, scene, dev), LossComputer(cfg)
opt = optim.Adam(list(model.parameters()), lr=5e-4, betas=(0.9, 0.999))
first = last = None
for it in range(iters):
    totals = harness.train_one_iter(model, losses, opt, batcher.get_next_batch(it), cfg['sub_batch_size'])
    if it == 0:
        first = float(totals['TotalLoss'])
last = float(totals['TotalLoss'])
torch.cuda.synchronize()
digest = hashlib.sha256()
for p in model.parameters():
    digest.update(p.detach().cpu().numpy().tobytes())
print(json.dumps({'lib': os.path.basename(sys.argv[1]), 'precision': precision, 'iterations': iters, 'first_loss': first, 'last_loss': last,
                  'psnr_view0': train_demo.psnr_of_view(model, scene, 0), 'parameters_sha256': digest.hexdigest()}))
