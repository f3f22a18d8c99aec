"""DPM-Solver++ and LMS samplers on the CPU: the host schedule tables of libdtp (dtp_scheduler_tables) and the fp32 restatement of
the samplers (tests/sched_ref.py) against fixtures captured from the reference's own schedulers and pipeline
(tools/capture_scheduler_golden.py).  No GPU is touched."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import sched_ref
from oracle import fakes

NS = (2, 4, 6, 8, 10, 12, 16, 20, 25, 50)


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(DPM=np.load(os.path.join(golden_dir, "sched_dpm.npz")), LMSD=np.load(os.path.join(golden_dir, "sched_lmsd.npz")))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30))) if a.size else 0.0


def test_dpm_tables_match_the_reference(lib, gold):
    from diffusiontexturepainting_amd import ops
    g = gold["DPM"]
    for n in NS:
        t = ops.scheduler_tables("DPM", n)
        assert t["evals"] == n and t["init_sigma"] == 1.0
        assert t["timesteps"].tolist() == g[f"timesteps_{n}"].tolist(), n
        c = t["coefs"]
        assert _rel(c[:, 0], g[f"alpha_s_{n}"]) <= 1e-5 and _rel(c[:, 1], g[f"sigma_s_{n}"]) <= 1e-5
        assert _rel(c[:, 3], g[f"first_coef_{n}"]) <= 1e-5
        assert _rel(c[:, 4], g[f"second_coef_{n}"]) <= 1e-5
        assert _rel(c[:, 5], g[f"mid_coef_{n}"]) <= 1e-5
        order = c[:, 2]
        want = [1] + [2] * (n - 2) + [1 if n < 15 else 2] if n > 1 else [1]
        assert order.tolist() == want[:n], n
        second = order > 1.5
        assert _rel(c[second, 6], g[f"inv_r0_{n}"][second]) <= 1e-5
        assert np.all(t["in_scale"] == 1.0) and t["in_scale"].shape == (n + 1,)
    # np.round halves to even: 999 * 5 / 6 = 832.5 -> 832 and 999 / 6 = 166.5 -> 166 (std::lround would give 833 and 167)
    assert ops.scheduler_tables("DPM", 6)["timesteps"].tolist() == [999, 832, 666, 500, 333, 166]


def test_lmsd_tables_match_the_reference(lib, gold):
    from diffusiontexturepainting_amd import ops
    g = gold["LMSD"]
    for n in NS:
        t = ops.scheduler_tables("LMSD", n)
        assert t["evals"] == n
        assert abs(t["init_sigma"] - float(g[f"init_sigma_{n}"])) <= 1e-5 * 14.6146
        assert t["timesteps"].tolist() == g[f"timesteps_{n}"].tolist(), n
        assert _rel(t["in_scale"], g[f"latent_scales_{n}"]) <= 1e-5
        c = t["coefs"]
        assert _rel(c[:, 0], g[f"sigmas_{n}"][:-1]) <= 1e-5
        assert c[:, 1].tolist() == g[f"orders_{n}"].astype(np.float32).tolist()
        assert _rel(c[:, 2:6], g[f"coefs_{n}"]) <= 1e-5
    assert abs(ops.scheduler_tables("LMSD", 20)["init_sigma"] - 14.6146) < 1e-4


def test_ddim_rows_are_todays_coefficients(lib):
    """The DDIM rows are what dtp_stamp has always uploaded: sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev) over
    timesteps[1:], built from dtp_ddim_tables -- bit for bit."""
    from diffusiontexturepainting_amd import ops
    for n in (2, 4, 8, 20, 50, 999):
        ts = (C.c_int64 * n)()
        al = (C.c_float * n)()
        fin = C.c_float()
        assert lib.dtp_ddim_tables(n, ts, al, C.byref(fin)) == 0
        a = np.array(al, dtype=np.float32)
        a_t = a[1:]
        a_prev = np.append(a[2:], np.float32(fin.value)).astype(np.float32)
        one = np.float32(1.0)
        want = np.stack([np.sqrt(one - a_t), np.sqrt(a_t), np.sqrt(a_prev), np.sqrt(one - a_prev)], axis=1)
        t = ops.scheduler_tables("DDIM", n)
        assert t["evals"] == n - 1 and t["init_sigma"] == 1.0
        assert np.array_equal(t["timesteps"], np.array(ts[1:], dtype=np.float32))
        assert np.array_equal(t["coefs"][:, :4], want)
        assert not t["coefs"][:, 4:].any() and np.all(t["in_scale"] == 1.0)


def test_bad_tables_requests_are_rejected(lib):
    ev = C.c_int()
    for sched in (0, 1, 2):
        for steps in (1, 1000):
            assert lib.dtp_scheduler_tables(sched, steps, C.byref(ev), None, None, None, None) != 0
            assert b"steps" in lib.dtp_last_error()
    assert lib.dtp_scheduler_tables(3, 20, C.byref(ev), None, None, None, None) != 0
    assert b"scheduler" in lib.dtp_last_error()
    assert lib.dtp_scheduler_tables(-1, 20, None, None, None, None, None) != 0


def test_unsupported_scheduler_names_raise():
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    assert [_lib.scheduler_id(n) for n in ("DDIM", "DPM", "LMSD")] == [0, 1, 2]
    for name in ("EulerA", "PNDM", "dpm", "Euler", ""):
        with pytest.raises(ValueError, match="DDIM, DPM, LMSD"):
            _lib.scheduler_id(name)
        with pytest.raises(ValueError, match="DDIM, DPM, LMSD"):  # before any device work: no GPU needed to be told
            MI355ConditionalInpainter(64, scheduler=name)


@pytest.mark.parametrize("name", ["DPM", "LMSD"])
def test_restated_step_chains_match_the_reference(gold, name):
    g = gold[name]
    for n in NS:
        s = sched_ref.SCHEDULERS[name](n)
        x = torch.from_numpy(g[f"x_{n}"])
        e = torch.from_numpy(g[f"e_{n}"])
        ref = g[f"chain_{n}"]
        for i in range(n):
            x = s.step(e[i], x, i)
            err = np.max(np.abs(x.numpy() - ref[i]) / np.maximum(1.0, np.abs(ref[i])))
            assert err <= 1e-5, (name, n, i, err)


def test_restated_pipelines_match_the_reference(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "sched_orch_*.npz")))
    assert len(files) == 4
    seen = set()
    for f in files:
        g = np.load(f)
        R, steps, cfg, tg, tg_steps = g["settings"]
        name = str(g["scheduler"])
        seen.add((name, int(steps), float(tg)))
        t = {k: torch.from_numpy(g[k]) for k in ("cond", "uncond", "masked", "mask", "ctx_img", "ctx_mask", "latents")}
        calls = []

        def unet(smp, ts, c):
            calls.append("u")
            return fakes.fake_unet(smp, ts, c)

        trace = []
        out = sched_ref.infer(unet, lambda img, k: fakes.fake_vae_encoder(img), fakes.fake_vae_decoder, t["cond"], t["uncond"],
                              t["masked"], t["mask"], t["ctx_img"], t["ctx_mask"], t["latents"], scheduler=name, steps=int(steps),
                              cfg=float(cfg), tg=float(tg), tg_steps=int(tg_steps), trace=trace)
        assert calls.count("u") == int(g["n_unet"]) == int(steps)  # N evaluations (steps_offset 0)
        tr = torch.stack(trace).numpy()
        assert np.max(np.abs(tr - g["trace"]) / np.maximum(1.0, np.abs(g["trace"]))) <= 1e-5, f
        assert np.max(np.abs(out.numpy() - g["out"])) <= 1e-5, f
    assert seen == {("DPM", 6, 1.0), ("DPM", 16, 1.0), ("LMSD", 6, 1.0), ("LMSD", 12, 0.0)}


def test_restated_tables_agree_with_the_library(lib):
    """The restatement and dtp_scheduler_tables are two statements of the same schedule."""
    from diffusiontexturepainting_amd import ops
    for n in (6, 16, 20):
        d, t = sched_ref.DPM(n), ops.scheduler_tables("DPM", n)
        assert t["timesteps"].tolist() == d.timesteps.tolist()
        l, t = sched_ref.LMSD(n), ops.scheduler_tables("LMSD", n)
        assert _rel(t["coefs"][:, 0], l.sigmas[:-1].numpy()) <= 1e-6
        assert _rel(t["in_scale"], np.array([float(v) for v in l.latent_scales])) <= 1e-6
        assert _rel(t["coefs"][:, 2], np.array([c[0] for c in l.coeffs])) <= 1e-6
