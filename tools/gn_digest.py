"""sha256 of the outputs of every GroupNorm op wrapper, for a byte-for-byte A/B of two builds of the library (a change of the launchers that
leaves kernels and launch geometry alone must leave every line alone):

    python tools/gn_digest.py  >  new.txt
    DTP_LIB=tools/ab/libdtp_head.so python tools/gn_digest.py  >  ref.txt       (separate processes; then diff)

The shapes are those of the GroupNorm tests of tests/test_gpu_ops.py (test_groupnorm*, test_reduce_groupnorm*,
test_groupnorm_folded_into_linear, test_groupnorm_applied_on_the_resident_fragments_of_the_linear,
test_groupnorm_stats_with_reduce_then_apply); an entry point the library lacks prints `absent`.  Run the reference twice first: a line it
does not reproduce against itself says nothing about the other build."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diffusiontexturepainting_amd import _lib, ops  # noqa: E402

GROUPNORM = [(3, 64, 320), (2, 256, 640), (1, 1024, 128), (2, 16, 1920), (1, 100, 2560), (2, 64, 256), (1, 64, 512), (3, 4, 960), (1, 4096, 320),
             (2, 2048, 128), (1, 1600, 640), (3, 4096, 320), (3, 1024, 640), (3, 256, 1280), (3, 64, 1280), (1, 16384, 128), (1, 4096, 640), (1, 1024, 1280), (3, 4096, 960)]
APPLY = [(3, 4096, 320), (2, 1024, 640), (1, 512, 1280), (2, 256, 640)]  # the outputs of test_conv3x3_weight_streaming_emits_groupnorm_statistics
REDUCE = [(3, 64, 1280, 8, True, False), (3, 256, 1280, 4, True, True), (3, 1024, 640, 2, True, False), (2, 1024, 640, 3, False, True),
          (1, 4096, 320, 2, True, True), (2, 1600, 960, 2, False, False)]
CONCAT = [(3, 64, 1280, 1280, 5, True, True), (3, 256, 1280, 640, 4, True, False), (2, 256, 1280, 1280, 2, False, True), (3, 16, 1280, 1280, 12, True, True),
          (1, 64, 640, 320, 3, True, False)]
FOLD = [(3, 4096, 320, 320), (2, 1024, 640, 640), (1, 1024, 1280, 1280), (2, 1600, 960, 320)]
RESIDENT = [(3, 4096, 320, 320, 5), (3, 1024, 640, 640, 4), (2, 1024, 320, 320, 1), (1, 256, 640, 640, 10), (8, 128, 320, 320, 3), (3, 1024, 640, 320, 2)]
STATS_APPLY = [(2, 1024, 320, 2, True, True), (1, 1000, 640, 3, False, True), (3, 16, 1280, 4, True, False), (2, 64, 128, 0, False, False)]


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:24]


def main():
    g = torch.Generator().manual_seed(1)

    def f16(*shape):
        return (torch.randn(*shape, generator=g) * 1.5 + 0.5).half().cuda()

    def f32(*shape):
        return (torch.randn(*shape, generator=g) * 0.7).cuda()

    def affine(c):
        return (1 + 0.2 * torch.randn(c, generator=g)).cuda(), (0.2 * torch.randn(c, generator=g)).cuda()

    print(f"# library: {os.environ.get('DTP_LIB') or 'working build'}")
    for b, hw, c in GROUPNORM:
        x, (gamma, beta) = f16(b, hw, c), affine(c)
        for silu in (False, True):
            print(f"groupnorm {(b, hw, c)} silu {int(silu)}: {sha(ops.groupnorm(x, gamma, beta, silu=silu))}", flush=True)
    for b, hw, c in APPLY:  # the apply pass alone, from one chunk of partial sums
        x, (gamma, beta) = f16(b, hw, c), affine(c)
        xf = x.float().view(b, hw, 32, c // 32)
        partial = torch.stack([xf.sum(dim=(1, 3)), (xf * xf).sum(dim=(1, 3))], dim=-1).view(b, 1, 32, 2).contiguous()
        print(f"groupnorm_apply {(b, hw, c)}: {sha(ops.groupnorm_apply(x, gamma, beta, partial, silu=True))}", flush=True)
    for b, hw, c, splits, bias, resid in REDUCE:
        part, (gamma, beta) = f32(splits, b, hw, c), affine(c)
        out = ops.reduce_groupnorm(part, gamma, beta, bias=f32(c) if bias else None, resid=f16(b, hw, c) if resid else None, silu=True)
        print(f"reduce_groupnorm {(b, hw, c, splits, bias, resid)}: {sha(*out)}", flush=True)
    for b, hw, cx, cskip, splits, bias, resid in CONCAT:
        part, (gamma, beta) = f32(splits, b, hw, cx), affine(cx + cskip)
        out = ops.reduce_groupnorm(part, gamma, beta, bias=f32(cx) if bias else None, resid=f16(b, hw, cx) if resid else None, silu=True, skip=f16(b, hw, cskip))
        print(f"reduce_groupnorm over a concatenation {(b, hw, cx, cskip, splits, bias, resid)}: {sha(*out)}", flush=True)
    for b, hw, c, n in FOLD:
        x, wp, (gamma, beta) = f16(b, hw, c), ops.pack_linear(f32(n, c) * c ** -0.5), affine(c)
        print(f"gn_fold_weights {(b, hw, c, n)}: {sha(*ops.gn_fold_weights(x, wp, n, f32(n), gamma, beta))}", flush=True)
    for b, hw, c, n, ranges in RESIDENT:
        x, wp, (gamma, beta) = f16(b, hw, c), ops.pack_linear(f32(n, c) * c ** -0.5), affine(c)
        print(f"gn_linear {(b, hw, c, n, ranges)}: {sha(*ops.gn_linear(x, wp, n, f32(n), gamma, beta, col_ranges=ranges, row_stats=True))}", flush=True)
    have = hasattr(_lib.load(), "dtp_op_groupnorm_stats_apply")
    for b, hw, c, splits, bias, resid in STATS_APPLY:
        gamma, beta = affine(c)
        if splits:
            kw = dict(part=f32(splits, b, hw, c), bias=f32(c) if bias else None, resid=f16(b, hw, c) if resid else None)
        else:
            kw = dict(x=f16(b, hw, c))
        print(f"groupnorm_stats_apply {(b, hw, c, splits, bias, resid)}: {sha(*ops.groupnorm_stats_apply(gamma, beta, **kw)) if have else 'absent'}", flush=True)


if __name__ == "__main__":
    main()
