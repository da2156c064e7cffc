"""The headline step in the 16-bit modes with the render as ONE launch (configs['model']['hip_fused_render'],
render_fused_m16_kernel in csrc/render_fused.hip) against the six-launch path, in one process: for each precision the two arms
alternate for several rounds (same weights, same rays), each round timed over a block of steps with the board's power and
shader clock sampled (bench_secondary.BoardSampler, as in bench.py --extras).  One JSON line per (precision, arm, round), then
one summary line per precision.

    python tools/probes/time_fused16.py [--precisions bf16,f16] [--rounds 5] [--steps 200] [--arm both|fused|plain]

`--arm fused` runs the fused arm alone (a rocprofv3 --kernel-trace --stats run of it)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
import bench_secondary  # noqa: E402


def timed_block(renderer, steps, device):
    sampler = bench_secondary.BoardSampler(device.index or 0)
    with torch.no_grad(), sampler:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            renderer.local()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    return elapsed, sampler.summary()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', default='bf16,f16')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--arm', default='both', choices=('both', 'fused', 'plain'))
    args = ap.parse_args()
    device = torch.device('cuda', 0)
    arms = {'both': (False, True), 'fused': (True,), 'plain': (False,)}[args.arm]
    for precision in args.precisions.split(','):
        renderers = {fused: bench.HipRenderer(precision, device, 0, 1, 'headline', collective=False, fused=fused) for fused in arms}
        with torch.no_grad():
            for r in renderers.values():
                for _ in range(args.warmup):
                    r.local()
        if len(arms) == 2:       # same outputs in both arms
            a, b = renderers[False].local(), renderers[True].local()
            assert all(torch.equal(a[k], b[k]) for k in a), 'fused and six-launch outputs differ'
        per_arm = {fused: [] for fused in arms}
        for rnd in range(args.rounds):
            for fused in (arms if rnd % 2 == 0 else arms[::-1]):
                elapsed, board = timed_block(renderers[fused], args.steps, device)
                rays_s = bench.RAYS_PER_GPU * args.steps / elapsed
                per_arm[fused].append(rays_s)
                print(json.dumps({'precision': precision, 'arm': 'fused' if fused else 'six_launch', 'round': rnd, 'steps': args.steps,
                                  'rays_per_s': rays_s, 'ms_per_step': elapsed / args.steps * 1e3, 'board': board}), flush=True)
        summary = {'precision': precision, 'kind': 'headline', 'rays_per_step': bench.RAYS_PER_GPU}
        for fused, vals in per_arm.items():
            summary['fused' if fused else 'six_launch'] = {'median_rays_per_s': statistics.median(vals), 'min': min(vals), 'max': max(vals)}
        if len(arms) == 2:
            summary['fused_over_six_launch'] = summary['fused']['median_rays_per_s'] / summary['six_launch']['median_rays_per_s']
        print(json.dumps(summary), flush=True)
        del renderers


if __name__ == '__main__':
    main()
