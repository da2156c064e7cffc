"""The 16-bit view sweep's formula (simplenerf_amd/csrc/simplenerf_sweep16.h) in numpy: the decoder of the saved `feature` pieces,
written from the header's layout text, the operands rounded to the mode's format with torch's casts (round to nearest even), and the
formula itself -- tests/view_sweep_reference.py's, which runs in float32 or float64 on operands given to it."""
import numpy
import torch

from tests import view_sweep_reference as ref

FORMATS = {'f16': torch.float16, 'bf16': torch.bfloat16}


def rounded(a, mode: str) -> numpy.ndarray:
    """r(): float32 -> the mode's 16-bit format, to nearest even -> float32."""
    return torch.from_numpy(numpy.ascontiguousarray(a, dtype=numpy.float32)).to(FORMATS[mode]).float().numpy()


def block_rows(mlp_cfg: dict) -> int:
    """R of the header: rows of 32 x 16 bit per 32-sample block."""
    depth, width, views_width = mlp_cfg['points_net_depth'], mlp_cfg['points_net_width'], mlp_cfg['views_net_width']
    mask_tiles = depth * width // 32 + views_width // 32
    return 96 + (depth + 1) * width + views_width + 4 * ((mask_tiles + 1) // 2)


def saved_feature(saved: numpy.ndarray, mlp_cfg: dict, n: int, s: int, mode: str) -> numpy.ndarray:
    """(n,S,W) float32 feature vectors out of 16-bit saved activations (a float32 array as the library hands it out).  Block b's
    feature tensor starts at row b R + 96 + D W; piece k (1 KiB) holds features 16 k .. 16 k + 15; slot 2 j + h of a piece (16
    bytes) is lane (j, h), whose element e is feature 16 k + 8 (e >> 2) + 4 h + (e & 3) of sample j of the block."""
    depth, width = mlp_cfg['points_net_depth'], mlp_cfg['points_net_width']
    rows = block_rows(mlp_cfg)
    blocks = (n * s + 31) // 32
    halves = torch.from_numpy(numpy.ascontiguousarray(saved)).view(torch.int16)[:((blocks - 1) * rows + 96 + depth * width + width) * 32]
    out = numpy.empty((blocks * 32, width), dtype=numpy.float32)
    e = numpy.arange(8)
    for b in range(blocks):
        first = (b * rows + 96 + depth * width) * 32
        pieces = halves[first:first + width * 32].view(FORMATS[mode]).float().numpy().reshape(width // 16, 32, 2, 8)    # [k][j][h][e]
        for k in range(width // 16):
            for h in range(2):
                out[32 * b:32 * b + 32, 16 * k + 8 * (e >> 2) + 4 * h + (e & 3)] = pieces[k, :, h, :]
    return out[:n * s].reshape(n, s, width)


def settled_directions(view_dirs: numpy.ndarray, degree: int, mode: str) -> numpy.ndarray:
    """``view_dirs`` (float32) with the few components moved whose encoding cannot be rounded to 16 bits the same way by everyone.
    The encoding is an fp32 quantity, and two correct fp32 sines differ by an ulp; where one lies that close to the midpoint of two
    16-bit neighbours, the device and this file may round it to different neighbours, 2^-9 (bf16) or 2^-12 (f16) apart -- far more
    than any summation order moves the colour.  Such a component is moved by 2^-10 until every sine and cosine of it keeps 2^-20
    (16 fp32 ulps at 1) of distance from every midpoint.  The inputs change, for the device and the restatement alike; nothing else."""
    dirs = numpy.array(view_dirs, dtype=numpy.float32)
    fmt = FORMATS[mode]
    for _ in range(64):
        x = dirs.astype(numpy.float64)
        close = numpy.zeros(dirs.shape, dtype=bool)
        for k in range(degree):
            for value in (numpy.sin(x * 2.0 ** k), numpy.cos(x * 2.0 ** k)):
                near = torch.from_numpy(value).to(fmt)
                bits = near.view(torch.int16)
                for step in (1, -1):
                    other = (bits + step).view(fmt).double().numpy()
                    middle = 0.5 * (near.double().numpy() + other)
                    close |= numpy.isfinite(middle) & (numpy.abs(value - middle) < 2.0 ** -20 * numpy.maximum(numpy.abs(value), 2.0 ** -4))
        if not close.any():
            return dirs
        dirs[close] += numpy.float32(2.0 ** -10)
    raise AssertionError('view directions did not settle')


def view_sweep(w_v, b_v, w_o, b_o, feature, weights, view_dirs, acc=None, white_bkgd=False, mode='bf16', dtype=numpy.float64):
    """out (V,n,3): tests/view_sweep_reference.view_sweep on W_v and the encoded directions rounded to ``mode``; the encoding is
    formed in float32 whatever ``dtype`` is (it is an fp32 quantity on the device), every later operation runs in ``dtype``."""
    cast = lambda a: numpy.asarray(a).astype(dtype)
    width = feature.shape[-1]
    degree = (w_v.shape[1] - width - 3) // 6
    w_v = rounded(w_v, mode)
    encoded = rounded(ref.encode(numpy.asarray(view_dirs, dtype=numpy.float32), degree), mode)
    w_v, b_v, w_o, b_o, feature, weights, encoded = (cast(a) for a in (w_v, b_v, w_o[:3], b_o[:3], feature, weights, encoded))
    u = b_v + encoded @ w_v[:, width:].T                                      # (V,n,Wv)
    g = feature @ w_v[:, :width].T                                            # (n,S,Wv)
    hidden = numpy.maximum(g[None] + u[:, :, None, :], dtype(0))              # (V,n,S,Wv)
    pre = hidden @ w_o.T + b_o
    rgb = dtype(1) / (dtype(1) + numpy.exp(-pre))
    out = (weights[None, :, :, None] * rgb).sum(2, dtype=dtype)
    if white_bkgd:
        out = out + (dtype(1) - cast(acc))[None, :, None]
    return out
