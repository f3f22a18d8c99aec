"""fp32 UNet forward for latent sizes that are not multiples of 8 (resolutions that are multiples of 8 but not of 64).

oracle.nets.unet_forward upsamples with scale_factor=2, which only matches the skips when every level halves exactly.  The reference
(diffusers 0.12 UNet2DConditionModel) sets forward_upsample_size when a side is not a multiple of 2^3, and every non-final up block then
upsamples with interpolate(size=skip.shape[-2:], mode="nearest").  This module restates only the top-level forward with that rule; the
blocks are oracle.nets' own.  For h % 8 == 0 it computes exactly what oracle.nets.unet_forward computes.
"""
import torch
import torch.nn.functional as F

from oracle.nets import _conv, _gn, _linear, _resnet, _transformer, timestep_embedding


def level_sizes(h):
    """Spatial size of the four UNet levels for latent size h: stride-2, pad-1 downsamplers give ceil(n / 2)."""
    out = [h]
    for _ in range(3):
        out.append((out[-1] + 1) // 2)
    return out


def unet_forward(sd, sample, timestep, ctx, return_trace=False):
    """UNet2DConditionModel forward, sample [N,9,h,w] f32, timestep scalar, ctx [N,14,768] -> [N,4,h,w]; any h, w >= 1."""
    eps = 1e-5
    trace = {}
    n = sample.shape[0]
    temb = timestep_embedding(timestep).expand(n, -1)
    temb = _linear(sd, "time_embedding.linear_2", F.silu(_linear(sd, "time_embedding.linear_1", temb)))
    x = _conv(sd, "conv_in", sample)
    skips = [x]
    for i in range(4):
        for j in range(2):
            x = _resnet(sd, f"down_blocks.{i}.resnets.{j}", x, temb, eps)
            if i < 3:
                x = _transformer(sd, f"down_blocks.{i}.attentions.{j}", x, ctx)
            skips.append(x)
        if i < 3:
            x = _conv(sd, f"down_blocks.{i}.downsamplers.0.conv", x, stride=2, padding=1)
            skips.append(x)
    trace["down"] = x
    x = _resnet(sd, "mid_block.resnets.0", x, temb, eps)
    x = _transformer(sd, "mid_block.attentions.0", x, ctx)
    x = _resnet(sd, "mid_block.resnets.1", x, temb, eps)
    trace["mid"] = x
    for i in range(4):
        for j in range(3):
            x = torch.cat([x, skips.pop()], dim=1)
            x = _resnet(sd, f"up_blocks.{i}.resnets.{j}", x, temb, eps)
            if i > 0:
                x = _transformer(sd, f"up_blocks.{i}.attentions.{j}", x, ctx)
        if i < 3:
            x = F.interpolate(x, size=skips[-1].shape[-2:], mode="nearest")  # the next skip's size: 2 n or 2 n - 1
            x = _conv(sd, f"up_blocks.{i}.upsamplers.0.conv", x)
        trace[f"up{i}"] = x
    trace["up"] = x
    x = _conv(sd, "conv_out", F.silu(_gn(sd, "conv_norm_out", x, eps)))
    return (x, trace) if return_trace else x
