"""Decoder of the fp32 / f16x3 training forward's saved tensor -- test infrastructure, never imported by the package.

Layout (simplenerf_amd/csrc/mlp_plan.h:61-75): per 32-sample wave block, act_rows rows of 32 floats, one row per feature and one
column per sample, features in natural (reference) order:

    pe[64] | pev[32] | h_1 .. h_D [width each] | feature [width] | h_v [views_width] | mask words

The mask words are the ReLU sign bits of every hidden tile, 16 bits per lane and tile, two tiles per dword, one dword-row of 64
lanes = 2 rows of 32 floats: dword (t >> 1, lane = sample + 32 half), bit 16 (t & 1) + r <-> feature 32 u + (r & 3) + 8 (r >> 2) +
4 half of tile t = l (width / 32) + u (then the views layer's tiles), as tests/test_gpu_grads.py:136-154 reads them.

`decode_fused32` returns the dictionary tests/test_gpu_rounding.py::decode_fused returns for the 16-bit modes, so that
fused_records(..., rounding_ref.EXACT), reference_grads and rounding_ref.backward give a float64 reference with the kernel's own
activations and ReLU masks.
"""
import torch

from tests import wgrad_plan


def decode_fused32(saved, cfg, total, blocks=None):
    """-> {'samples': indices of the decoded samples, 'pe', 'h': [h_1 .. h_D], 'mask': [bool per layer], and for a view-dependent MLP
    'pev', 'feature', 'hv', 'vmask'}: float64 (rows, features), one row per real sample.  `blocks`: the wave blocks to decode,
    gathered on the device before anything moves to the host (default: all of them)."""
    p = wgrad_plan.rows_of(cfg)
    D, W, vw = p.depth, p.width, p.views_width
    rows, act_mask, tiles = p.act_rows(), p.act_mask(), p.mask_tiles()
    pairs = (tiles + 1) // 2
    all_blocks = (total + 127) // 128 * 4                    # whole workgroups of the forward (mlp_backward.hip:1026)
    assert saved.dtype == torch.float32 and all_blocks * rows * 32 <= saved.numel(), (saved.numel(), rows, total)
    blk = saved[:all_blocks * rows * 32].reshape(all_blocks, rows, 32)
    index = torch.arange(-(-total // 32)) if blocks is None else torch.as_tensor(list(blocks), dtype=torch.int64)
    assert index.numel() == 0 or (0 <= int(index.min()) and int(index.max()) < all_blocks), (blocks, all_blocks)
    blk = blk[index.to(blk.device)].cpu()
    nb = index.numel()
    samples = (index[:, None] * 32 + torch.arange(32)).reshape(-1)
    live = samples < total

    def region(r0, nfeat, keep):
        return blk[:, r0:r0 + nfeat].permute(0, 2, 1).reshape(nb * 32, nfeat)[live][:, :keep].double().contiguous()

    words = blk[:, act_mask:act_mask + 2 * pairs].contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    words = words.reshape(nb, pairs, 2, 32)                                                 # pair, half, sample

    def masks(t0, ntiles):
        out = torch.zeros(nb, 32, ntiles * 32, dtype=torch.bool)
        for u in range(ntiles):
            t = t0 + u
            for h in range(2):
                for r in range(16):
                    out[:, :, 32 * u + (r & 3) + 8 * (r >> 2) + 4 * h] = ((words[:, t >> 1, h, :] >> (16 * (t & 1) + r)) & 1).bool()
        return out.reshape(nb * 32, ntiles * 32)[live]

    dec = {'samples': samples[live], 'pe': region(p.act_pe(), 64, p.full_pe),
           'h': [region(p.act_h(l + 1), W, W) for l in range(D)], 'mask': [masks(l * (W // 32), W // 32) for l in range(D)]}
    if p.view_dependent:
        dec['pev'] = region(p.act_pev(), 32, p.views_pe)
        dec['feature'] = region(p.act_feature(), W, W)
        dec['hv'] = region(p.act_hv(), vw, vw)
        dec['vmask'] = masks(D * (W // 32), vw // 32)
    return dec
