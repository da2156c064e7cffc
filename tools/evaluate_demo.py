#!/usr/bin/env python3
"""The reference's third stage on one MI355X: train the synthetic 3-view plane scene briefly (tools/train_demo.py), render every
view, and score the frames on the device with ``harness.evaluate_frames`` -- RMSE / PSNR / SSIM of the 8-bit frame and
RMSE / MAE / SROCC of the depth against the scene's true depth, plain and masked, per frame and averaged with the reference's
rounding.  The masks are the reference's visibility masks, computed on the device from the other views' true depths and cameras
(``qa.visibility_mask`` through the frames' 'mask_views').
    python tools/evaluate_demo.py [iterations]         (SNERF_PREC, SNERF_SEED as in tools/train_demo.py)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_demo  # noqa: E402


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    _, table = train_demo.run(iters, os.environ.get('SNERF_PREC', 'fp32'), False, int(os.environ.get('SNERF_SEED', '0')),
                              with_scores=True)
    names = list(table['average'])
    print('frame  ' + ' '.join(f'{n:>11}' for n in names))
    for row in table['frames']:
        print(f"{row['frame_num']:>5}  " + ' '.join(f'{row[n]:>11.4f}' for n in names))
    print('  avg  ' + ' '.join(f"{table['average'][n]:>11.4f}" for n in names))


if __name__ == '__main__':
    main()
