"""The launch programs of a library, for a line-by-line diff against another build of it (a host-side refactor must not change them):

    python tools/program_dump.py OUTDIR            DTP_LIB=tools/ab/libdtp_head.so python tools/program_dump.py REFDIR
    diff -r -x '*.csv' OUTDIR REFDIR               (both arms on one $DTP_TUNE_CACHE, the reference first: the tuner then picks the same tiles)

Per handle kind OUTDIR/<kind>.unet.kl and <kind>.all.kl hold the `kind,label` columns of dtp_profile_dump after one UNet evaluation and after
one VAE encode + decode more (the .csv files keep the times).  Kinds: 128^2, 256^2, 256^2 with each switch of the GroupNorm claim path
(csrc/builder.hip) set alone, 256^2 with option fp8_linear, 512^2, and n = 6 at 256^2 / 128^2.  Synthetic weights; prints the claim
markers of every kind's UNet program (tests/test_gpu_engine.py CLAIM_PRESENT)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusiontexturepainting_amd import weights as W  # noqa: E402
from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
SW = ["DTP_NO_FUSE_REDUCE_GN", "DTP_NO_GN_EPILOGUE", "DTP_NO_REDUCE_IN_CONCAT_GN", "DTP_NO_GNA_LNLIN", "DTP_NO_FOLD_GN"]
MARKERS = ["(reduce in gn)", "reduce+gn B=", "reduce(front", "reduce+gn-stats", "(+gn stats)", "gn-apply", "(apply in proj_in)", "gn-fold"]
kinds = [("r128", 128, None, False, 3), ("r256", 256, None, False, 3)] + [("r256_" + s, 256, s, False, 3) for s in SW] + \
        [("r256_fp8", 256, None, True, 3), ("r512_b1", 512, None, False, 3), ("r256_n6", 256, None, False, 6), ("r128_n6", 128, None, False, 6)]
sd = dict(unet=W.synthetic_unet(1), lora=W.synthetic_lora(1), vae=W.synthetic_vae(1))


def kl(path):
    rows = [ln.rstrip("\n").split(",", 4) for ln in open(path).read().splitlines()[1:]]
    return [(r[0], r[4]) for r in rows]


for tag, res, sw, fp8, n in kinds:
    for s in SW:
        os.environ.pop(s, None)
    if sw:
        os.environ[sw] = "1"
    t0 = time.perf_counter()
    m = MI355ConditionalInpainter(res, device=0, weights=sd, max_batch=2 if n > 3 else 1, fp8_linear=fp8)
    t1 = time.perf_counter()
    h = res // 8
    g = torch.Generator().manual_seed(n)
    sample = torch.randn(n, 9, h, h, generator=g)
    ctx = torch.randn(n, 14, 768, generator=g).half()
    m.profile(True)
    m.unet(sample, 301.0, ctx)
    t2 = time.perf_counter()
    m.profile_dump(os.path.join(out, tag + ".unet.csv"))
    img = torch.rand(1, 3, res, res, generator=g) * 2 - 1
    m.vae_encode(img, torch.randn(1, 4, h, h, generator=g))
    m.vae_decode(torch.randn(1, 4, h, h, generator=g))
    m.profile_dump(os.path.join(out, tag + ".all.csv"))
    m.profile(False)
    for part in ("unet", "all"):
        rows = kl(os.path.join(out, tag + "." + part + ".csv"))
        with open(os.path.join(out, tag + "." + part + ".kl"), "w") as f:
            f.writelines(k + "," + lb + "\n" for k, lb in rows)
    labels = [lb for _, lb in kl(os.path.join(out, tag + ".unet.csv"))]
    pres = {mk: sum(mk in lb for lb in labels) for mk in MARKERS}
    print(f"{tag}: create {t1 - t0:.1f} s, unet(first) {t2 - t1:.2f} s, launches unet {len(labels)}; markers {pres}", flush=True)
    del m
    torch.cuda.synchronize()
