"""Strength < 1 stamps on the CPU: the host schedule of libdtp (dtp_strength_schedule) and the fp32 restatement (tests/strength_ref.py)
against fixtures captured from the reference's own initialize_timesteps, add_noise, step() and InpaintPipeline.infer
(tools/capture_strength_golden.py), and the Python argument checks.  No GPU is touched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import strength_ref
from oracle import fakes

SCHEDS = ("DDIM", "DPM", "LMSD")


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def sched_gold(golden_dir):
    return np.load(os.path.join(golden_dir, "strength_schedule.npz"))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def _schedule(lib, name, steps, strength):
    from diffusiontexturepainting_amd import _lib
    ts, ev, nc = C.c_int(), C.c_int(), (C.c_float * 2)()
    rc = lib.dtp_strength_schedule(_lib.scheduler_id(name), int(steps), C.c_double(strength), C.byref(ts), C.byref(ev), nc)
    return rc, ts.value, ev.value, (nc[0], nc[1])


def test_schedule_matches_the_reference(lib, sched_gold):
    g = sched_gold
    for name in SCHEDS:
        init_sigma = 1.0 if name != "LMSD" else float(strength_ref.LMSD(2).init_noise_sigma)
        n_ok = 0
        for steps, st, t_start, evals, a, b in zip(g[f"{name}_steps"], g[f"{name}_strength"], g[f"{name}_t_start"], g[f"{name}_evals"],
                                                   g[f"{name}_a"], g[f"{name}_b"]):
            rc, ts, ev, nc = _schedule(lib, name, steps, float(st))
            if evals == 0:
                assert rc != 0 and b"strength" in lib.dtp_last_error(), (name, steps, st)
                continue
            assert rc == 0, (name, steps, st, lib.dtp_last_error())
            assert (ts, ev) == (int(t_start), int(evals)), (name, steps, st)
            # the pair is the reference's add_noise(1, 0) / add_noise(0, 1) below strength 1, from the fp32 tables the loop already
            # uses (alphas_cumprod within 1 ulp of torch's cumprod: the tolerance of test_ddim_tables_match_reference_fixture);
            # exactly (0, init_sigma) at 1
            if st < 1.0:
                assert _rel(nc, (a, b)) <= 2.5e-7, (name, steps, st, nc, (a, b))
            else:
                assert nc == (0.0, np.float32(init_sigma)), (name, steps, st, nc)
            n_ok += 1
        assert n_ok >= 60, name


def test_schedule_examples_of_the_issue(lib):
    """DDIM at 20 steps: strength 1 -> t_start 1 / 19 evaluations (today's path), 0.75 -> 5 / 15, 0.5 -> 10 / 10, 0.3 -> 14 / 6."""
    for st, want in ((1.0, (1, 19)), (0.75, (5, 15)), (0.5, (10, 10)), (0.3, (14, 6)), (0.95, (1, 19))):
        rc, ts, ev, _ = _schedule(lib, "DDIM", 20, st)
        assert rc == 0 and (ts, ev) == want, st
    for name in ("DPM", "LMSD"):
        for steps, st in ((20, 0.5), (6, 0.7), (50, 0.35)):
            rc, ts, ev, _ = _schedule(lib, name, steps, st)
            assert rc == 0 and ts == steps - int(steps * st) and ev == int(steps * st)


def test_schedule_uses_the_double_product(lib, sched_gold):
    """int(steps * strength) in double as Python computes it.  The fixture grid holds cases where float32 arithmetic truncates to a
    different integer -- a float32-held strength (0.35 * 20 = 6.9999999 -> 6, not 7) or a float32 product (50 * 0.58 = 29.0, not
    28.999999999999996) -- and the library follows the double one there."""
    g = sched_gold
    held, product = 0, 0
    for name in SCHEDS:
        offset = 1 if name == "DDIM" else 0
        for steps, st, t_start in zip(g[f"{name}_steps"], g[f"{name}_strength"], g[f"{name}_t_start"]):
            steps, st = int(steps), float(st)
            d = int(steps * st)
            f_held, f_prod = int(steps * float(np.float32(st))), int(np.float32(steps) * np.float32(st))
            if d == 0 or (f_held == d and f_prod == d):
                continue
            held += f_held != d
            product += f_prod != d
            rc, ts, _, _ = _schedule(lib, name, steps, st)
            assert rc == 0 and ts == int(t_start) == steps - min(d + offset, steps) + offset, (name, steps, st)
            for f in (f_held, f_prod):
                assert f == d or ts != steps - min(f + offset, steps) + offset, (name, steps, st)
    assert held >= 10 and product >= 2


def test_schedule_errors(lib):
    for st in (0.0, -0.5, 1.0000001, 1.5, float("nan"), float("inf")):
        rc, _, _, _ = _schedule(lib, "DDIM", 20, st)
        assert rc == 1 and b"strength" in lib.dtp_last_error(), st  # DTP_ERR_ARG
    rc, _, _, _ = _schedule(lib, "DDIM", 8, 0.1)  # int(0.8) = 0: no evaluation
    assert rc == 1 and b"strength" in lib.dtp_last_error()
    rc, _, _, _ = _schedule(lib, "LMSD", 6, 0.1)
    assert rc == 1 and b"strength" in lib.dtp_last_error()
    assert lib.dtp_strength_schedule(7, 20, C.c_double(0.5), None, None, None) == 1
    assert lib.dtp_strength_schedule(0, 1, C.c_double(0.5), None, None, None) == 1
    assert lib.dtp_strength_schedule(0, 20, C.c_double(0.5), None, None, None) == 0  # every output may be NULL


def test_ops_strength_schedule(lib):
    from diffusiontexturepainting_amd import ops
    d = ops.strength_schedule("LMSD", 6, 0.5)
    assert d["t_start"] == 3 and d["evals"] == 3 and d["noise_coefs"][0] == 1.0
    t = ops.scheduler_tables("LMSD", 6)
    assert d["noise_coefs"][1] == t["coefs"][3][0]  # sigma[t_start]
    d = ops.strength_schedule("DDIM", 8, 0.5)  # t_start 4 = table row 3
    t = ops.scheduler_tables("DDIM", 8)
    assert d["noise_coefs"] == (t["coefs"][3][1], t["coefs"][3][0])


def test_restated_add_noise_and_chains_match_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "strength_chains.npz"))
    seen = set()
    for k in range(int(g["count"])):
        p = f"{k}_"
        name, n, st, t_start = str(g[p + "name"]), int(g[p + "steps"]), float(g[p + "strength"]), int(g[p + "t_start"])
        s = strength_ref.make(name, n)
        ts, ev = strength_ref.initialize_timesteps(n, st, s.steps_offset)
        assert ts == t_start and ev == g[p + "chain"].shape[0]
        x = s.add_noise(torch.from_numpy(g[p + "z0"]), torch.from_numpy(g[p + "eps"]), t_start)
        ref = g[p + "x_init"]
        assert np.max(np.abs(x.numpy() - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-5, (name, n, st)
        e = torch.from_numpy(g[p + "e"])
        for i in range(ev):
            x = s.step(e[i], x, t_start + i)
            ref = g[p + "chain"][i]
            err = np.max(np.abs(x.numpy() - ref) / np.maximum(1.0, np.abs(ref)))
            assert err <= 1e-5, (name, n, st, i, err)
        seen.add(name)
    assert seen == set(SCHEDS)


def test_dpm_first_evaluation_is_first_order(golden_dir):
    """DPM 20 steps at 0.5 starts at row 10, whose full-table order is 2: the reference runs it first order (a fresh history).
    sched_ref.DPM, which takes the order from the table index, does not follow the captured chain there."""
    import sched_ref
    g = np.load(os.path.join(golden_dir, "strength_chains.npz"))
    k = next(k for k in range(int(g["count"])) if str(g[f"{k}_name"]) == "DPM" and int(g[f"{k}_steps"]) == 20 and
             float(g[f"{k}_strength"]) == 0.5)
    p = f"{k}_"
    t_start = int(g[p + "t_start"])
    x0, e, ref = torch.from_numpy(g[p + "x_init"]), torch.from_numpy(g[p + "e"]), g[p + "chain"][0]
    x = strength_ref.DPM(20).step(e[0], x0, t_start)
    assert np.max(np.abs(x.numpy() - ref)) <= 1e-5
    table = sched_ref.DPM(20)
    table.prev_x0 = torch.zeros_like(x0)
    assert np.max(np.abs(table.step(e[0], x0, t_start).numpy() - ref)) > 1e-3


@pytest.mark.parametrize("name", SCHEDS)
def test_restated_pipeline_matches_the_reference(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"strength_orch_{name.lower()}.npz"))
    R, steps, st, cfg, tg, tg_steps = g["settings"]
    assert str(g["scheduler"]) == name
    t = {k: torch.from_numpy(g[k]) for k in ("cond", "uncond", "masked", "mask", "ctx_img", "ctx_mask", "latents", "init_image")}
    calls = []

    def unet(smp, ts, c):
        calls.append("u")
        return fakes.fake_unet(smp, ts, c)

    trace, start = [], {}
    out = strength_ref.infer(unet, lambda img, k: fakes.fake_vae_encoder(img), fakes.fake_vae_decoder, t["cond"], t["uncond"], t["masked"],
                             t["mask"], t["ctx_img"], t["ctx_mask"], t["latents"], t["init_image"], scheduler=name, steps=int(steps),
                             strength=float(st), cfg=float(cfg), tg=float(tg), tg_steps=int(tg_steps), trace=trace, start=start)
    assert start["t_start"] == int(g["t_start"]) and calls.count("u") == int(g["n_unet"]) == int(g["evals"]) < int(steps)
    assert np.max(np.abs(start["x_init"].numpy() - g["x_init"]) / np.maximum(1.0, np.abs(g["x_init"]))) <= 1e-5
    tr = torch.stack(trace).numpy()
    assert np.max(np.abs(tr - g["trace"]) / np.maximum(1.0, np.abs(g["trace"]))) <= 1e-5, name
    assert np.max(np.abs(out.numpy() - g["out"])) <= 1e-5, name


def test_python_argument_checks():
    from diffusiontexturepainting_amd.inpainter import check_strength_args
    assert check_strength_args(1, None, 2, 8) == 1.0
    assert check_strength_args(0.5, torch.zeros(2, 4, 8, 8), 2, 8) == 0.5
    assert check_strength_args(0.5, False, 2, 8) == 0.5
    assert check_strength_args(1.0, torch.zeros(5), 2, 8) == 1.0  # ignored at strength 1
    for st in (0.0, -1.0, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            check_strength_args(st, None, 1, 8)
    for shape in ((1, 4, 8, 8), (2, 4, 8, 4), (2, 1, 4, 8, 8)):
        with pytest.raises(ValueError, match="init_eps"):
            check_strength_args(0.5, torch.zeros(shape), 2, 8)


def test_generate_signatures_take_strength_and_init_eps():
    import inspect
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter as M
    for fn in (M.generate, M.generate_raw, M.generate_u8):
        ps = inspect.signature(fn).parameters
        assert ps["strength"].default == 1.0 and ps["init_eps"].default is None, fn.__name__
