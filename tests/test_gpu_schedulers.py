"""DPM-Solver++ and LMS samplers in the stamp loop (dtp_set_option "scheduler", `MI355ConditionalInpainter(scheduler=...)`): the
stamp's own step kernel against the reference's captured step() chains, whole stamps against the CPU restatement on the oracle
networks (tests/sched_ref.py), mixed batches, and switching samplers on one handle with graph replay.  One 64^2 context."""
import os

import numpy as np
import pytest
import torch

import sched_ref

pytestmark = pytest.mark.gpu

R = 64
TOL = 1e-2


@pytest.fixture(scope="module")
def sd():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import weights as W
    return dict(unet=W.synthetic_unet(5), lora=W.synthetic_lora(5), vae=W.synthetic_vae(5), clip=W.synthetic_clip(5),
                penc=W.synthetic_patch_encoder(5))


@pytest.fixture(scope="module")
def env(sd):
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from oracle import nets
    model = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=4, scheduler="DPM")
    return dict(model=model, nets=dict(unet=nets.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"]))


def _inputs(b, seed):
    from diffusiontexturepainting_amd import synthetic
    canvas, brush, lat, eps = synthetic.make_stamp_batch(b, R, seed)
    cond, uncond = synthetic.make_conditioning(seed + 1)
    return canvas, brush, cond, uncond, lat, eps


@pytest.mark.parametrize("name,n", [("DPM", 6), ("DPM", 16), ("LMSD", 6), ("LMSD", 12)])
def test_step_kernel_follows_the_reference_chain(golden_dir, name, n):
    from diffusiontexturepainting_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = np.load(os.path.join(golden_dir, f"sched_{name.lower()}.npz"))
    t = ops.scheduler_tables(name, n)
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(g[f"x_{n}"]).to(dev)
    e = torch.from_numpy(g[f"e_{n}"]).to(dev)
    b = x.shape[0]
    hist = torch.zeros(3 * x.numel(), dtype=torch.float32, device=dev)
    for i in range(n):
        # uncond = cond = the captured model output: u + cfg (c - u) is that output exactly
        rows = torch.cat([e[i], e[i]])
        in16 = ops.sched_step(name, t["coefs"][i], t["in_scale"][i + 1], rows, x, hist, [1.0] * b, [0.0] * b, [0] * b, 0, i)
        torch.cuda.synchronize()
        ref = g[f"chain_{n}"][i]
        err = np.max(np.abs(x.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref)))
        assert err <= 1e-5, (name, n, i, err)
        want16 = (x * float(t["in_scale"][i + 1])).half()
        assert torch.equal(in16[:b], want16) and torch.equal(in16[b:], want16)


def test_step_kernel_guidance_rows_and_lms_history():
    """The guidance combine with texture-guided rows mapped through rank / k, and the derivative ring at orders 2..4 (the reference's
    LMS rows are all first order, so the stamp never reaches these)."""
    from diffusiontexturepainting_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(3)
    b, k = 3, 2
    rank = [2, 0, 1]  # stamps 1 and 2 own tg rows 2B + 0 and 2B + 1; stamp 0 has none
    cfg, tg = [1.5, 2.0, 3.0], [0.7, 1.3, 0.4]
    x_cpu = torch.randn(b, 4, 5, 5, generator=gen) * 3
    x = x_cpu.to(dev)
    hist = torch.zeros(3 * x.numel(), dtype=torch.float32, device=dev)
    sig = [10.0, 6.0, 3.5, 2.0, 1.0, 0.4]
    ds = []
    for i in range(5):
        out = torch.randn(2 * b + k, 4, 5, 5, generator=gen)
        u, c = out[:b], out[b:2 * b]
        e = u + torch.tensor(cfg).view(b, 1, 1, 1) * (c - u)
        for s in range(b):
            if rank[s] < k:
                e[s] = e[s] + tg[s] * (out[2 * b + rank[s]] - c[s])
        order = min(i + 1, 4)
        coef = [float(v) for v in torch.randn(order, generator=gen)]
        row = [sig[i], float(order)] + coef + [0.0] * (6 - order)
        d = (x_cpu - (x_cpu - sig[i] * e)) / sig[i]
        ds.append(d)
        x_cpu = x_cpu + sum(cc * dd for cc, dd in zip(coef, reversed(ds[-order:])))
        ops.sched_step("LMSD", row, 0.5, out.to(dev), x, hist, cfg, tg, rank, k, i)
        torch.cuda.synchronize()
        err = (x.cpu() - x_cpu).abs().max().item() / max(1.0, x_cpu.abs().max().item())
        assert err <= 1e-5, (i, err)


def _stamp_vs_oracle(env, name, n, seed, **st):
    m = env["model"]
    canvas, brush, cond, uncond, lat, eps = _inputs(1, seed)
    m.set_conditioning(cond, uncond, brush)
    m.set_scheduler(name)
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, steps=n, **st).cpu()
    assert m.stamp_info()["unet_evals"] == n
    ref = sched_ref.generate_raw(env["nets"], brush, cond, uncond, canvas, lat, eps, scheduler=name, steps=n, **st)
    err = (got - ref).abs().max().item()
    print(f"{name} {n}: vs oracle {err:.2e}")
    assert torch.isfinite(got).all() and err <= TOL


def test_dpm_stamp_lower_order_final(env):
    _stamp_vs_oracle(env, "DPM", 6, 3100, tg_steps=6)


def test_dpm_stamp_second_order_to_the_end(env):
    _stamp_vs_oracle(env, "DPM", 16, 3200, tg_steps=5, cfg_weight=3.0)


def test_lmsd_stamp(env):
    _stamp_vs_oracle(env, "LMSD", 6, 3300, tg_steps=3)


MIXED = [dict(cfg_weight=1.0, tg_weight=0.0, tg_steps=4, context_pad=5),
         dict(cfg_weight=2.0, tg_weight=1.0, tg_steps=4, context_pad=9),
         dict(cfg_weight=4.5, tg_weight=2.0, tg_steps=1, context_pad=17),
         dict(cfg_weight=6.0, tg_weight=2.5, tg_steps=0, context_pad=150)]


def test_dpm_mixed_batch(env):
    m = env["model"]
    n = 4
    ins = [_inputs(1, 3400 + i) for i in range(4)]
    for slot, (_, brush, cond, uncond, _, _) in enumerate(ins):
        m.set_conditioning(cond, uncond, brush, slot=slot)
    canvas, lat = torch.cat([i[0] for i in ins]), torch.cat([i[4] for i in ins])
    eps = torch.cat([i[5] for i in ins], dim=1)
    m.set_scheduler("DPM")
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2, 3], per_stamp=MIXED, steps=n).cpu()
    # tg_evals under DPM with 4 steps: (0, 4, 1, 0) -> k_i = 2, 1, 1, 1 over the 4 evaluations
    assert m.stamp_info()["unet_evals"] == n and m.stamp_unet_rows() == (8 + 2) + 3 * (8 + 1)
    for b, st in enumerate(MIXED):
        _, brush, cond, uncond, _, _ = ins[b]
        ref = sched_ref.generate_raw(env["nets"], brush, cond, uncond, canvas[b:b + 1], lat[b:b + 1], eps[:, b:b + 1], scheduler="DPM",
                                     steps=n, **st)
        solo = m.generate_raw(canvas[b:b + 1], latents=lat[b:b + 1], vae_eps=eps[:, b:b + 1], slots=[b], steps=n, **st).cpu()
        e_ref, e_solo = (got[b:b + 1] - ref).abs().max().item(), (got[b:b + 1] - solo).abs().max().item()
        print(f"stamp {b} {st}: vs oracle {e_ref:.2e}, vs solo {e_solo:.2e}")
        assert e_ref <= TOL and e_solo <= TOL


def test_switching_schedulers_with_graph_replay(env):
    m = env["model"]
    canvas, brush, cond, uncond, lat, eps = _inputs(2, 3500)
    m.set_conditioning(cond, uncond, brush)
    kw = dict(latents=lat, vae_eps=eps, steps=4, tg_steps=2)
    outs = {}
    for i, name in enumerate(["DDIM", "DPM", "LMSD", "DDIM"]):
        m.set_scheduler(name)
        graph = m.generate_raw(canvas, **kw).cpu()
        assert m.stamp_info()["unet_evals"] == (3 if name == "DDIM" else 4)
        try:
            m.set_option("use_graph", 0)
            eager = m.generate_raw(canvas, **kw).cpu()
        finally:
            m.set_option("use_graph", 1)
        assert torch.equal(graph, eager), name
        outs.setdefault(name, []).append(graph)
    assert torch.equal(outs["DDIM"][0], outs["DDIM"][1])
    assert not torch.equal(outs["DPM"][0], outs["LMSD"][0]) and not torch.equal(outs["DPM"][0], outs["DDIM"][0])


def test_unsupported_names_raise(env):
    m = env["model"]
    m.set_scheduler("DPM")
    for name in ("EulerA", "PNDM", "ddim"):
        with pytest.raises(ValueError, match="DDIM, DPM, LMSD"):
            m.set_scheduler(name)
    assert m.scheduler == "DPM"
    from diffusiontexturepainting_amd import _lib
    with pytest.raises(_lib.DtpError, match="scheduler"):
        m.set_option("scheduler", 3)
