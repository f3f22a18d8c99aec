"""Option fp8_operands, the accuracy question of DESIGN.md 4, answered on the CPU: the fp32 oracle with e4m3 rounding (power-of-two
scale, amax * 2 / 448) applied to ONE operand of the merged ff.net.2 / proj_out contraction -- the residual stream y3 or the GEGLU output
f -- in every transformer block, 64^2 x 8 stamps / 8 steps, against the unmodified oracle.   python tools/fp8_operands_emulate.py"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from diffusiontexturepainting_amd import weights as W, synthetic
from oracle import nets, pipeline

def q8(t):
    s = 2.0 ** math.ceil(math.log2(max(t.abs().max().item(), 1e-30) * 2.0 / 448.0))
    return (t / s).clamp(-448, 448).to(torch.float8_e4m3fn).float() * s

MODE = {"y3": False, "f": False}
def _transformer(sd, p, x, ctx, heads=nets.UNET_HEADS):
    b, c, h, w = x.shape
    res = x
    y = nets._conv(sd, p + ".proj_in", nets._gn(sd, p + ".norm", x, 1e-6), padding=0)
    y = y.permute(0, 2, 3, 1).reshape(b, h * w, c)
    t = p + ".transformer_blocks.0"
    n = nets._ln(sd, t + ".norm1", y)
    y = y + nets._attention(sd, t + ".attn1", n, n, heads)
    y = y + nets._attention(sd, t + ".attn2", nets._ln(sd, t + ".norm2", y), ctx, heads)
    f = nets._linear(sd, t + ".ff.net.0.proj", nets._ln(sd, t + ".norm3", y))
    a, g = f.chunk(2, dim=-1)
    hdn = a * F.gelu(g)
    y3 = q8(y) if MODE["y3"] else y
    hdn = q8(hdn) if MODE["f"] else hdn
    y = y3 + nets._linear(sd, t + ".ff.net.2", hdn)
    y = y.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return nets._conv(sd, p + ".proj_out", y, padding=0) + res
orig = nets._transformer
sd = dict(unet=W.synthetic_unet(2), lora=W.synthetic_lora(2), vae=W.synthetic_vae(2))
ow = dict(unet=nets.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"])
st = dict(steps=8, context_pad=5, tg_steps=4, cfg_weight=2.0, tg_weight=1.0)
canvas, brush, lat, eps = synthetic.make_stamp_batch(8, 64, 31)
cond, uncond = synthetic.make_conditioning(32)
ref = pipeline.generate_raw(ow, brush, cond, uncond, canvas, lat, eps, **st)
nets._transformer = _transformer
for mode in ({"y3": True, "f": False}, {"y3": False, "f": True}):
    MODE.update(mode)
    got = pipeline.generate_raw(ow, brush, cond, uncond, canvas, lat, eps, **st)
    print(mode, "max |emulated - oracle| = %.2e" % (got - ref).abs().max().item(), flush=True)
