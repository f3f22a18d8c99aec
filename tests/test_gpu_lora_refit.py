"""LoRA refit of a live handle (dtp_refit_stage / dtp_refit_lora, MI355ConditionalInpainter.set_lora) on the GPU.

The operator test compares lora_refit_kernel with the fp64 value rounded to fp16.  Everything else is bit-exact: a refitted handle must
equal (torch.equal) a FRESH handle created from the same base weights and that LoRA with `up` pre-multiplied by the scale -- both run
the device functions of csrc/weight_math.h.  All handles are 64^2, synthetic weights, max_batch 2, 4 steps, autotune off (the same
heuristic tile choices on every handle); the fresh handles are built once per module, asked for their reference outputs and dropped.
"""
import ctypes as C
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

R = 64
ST = dict(steps=4, context_pad=5, tg_steps=4, cfg_weight=2.0, tg_weight=1.0)
SEEDS = [11, 12]
Q_ID = "painter"  # the client of the server test


def _up(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- 1. operator
CASES = [(320, 320, 4, 0),        # one whole matrix
         (320, 320, 4, 640),      # the third of a stack, N not a multiple of 128
         (1280, 768, 4, 1280),    # K of the cross-attention k / v
         (640, 640, 1, 0),
         (320, 320, 64, 0)]       # four passes over the staged `down` rows


def _ordered(h):
    """fp16 bit patterns as integers ordered like the values (adjacent floats differ by 1)."""
    i = h.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("with_gamma", [False, True], ids=["plain", "gamma"])
@pytest.mark.parametrize("scale", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("N,K,rank,row0", CASES)
def test_operator_against_fp64(N, K, rank, row0, scale, with_gamma):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(N * 7 + K + rank + row0)
    w0 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    up = (torch.randn(N, rank, generator=g) * 0.05).to(dev)
    down = (torch.randn(rank, K, generator=g) * 0.5 / K ** 0.5).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dev) if with_gamma else None
    rows, ldw, guard = _up(row0 + N, 128), _up(K, 64) + 64, 4096
    flat = torch.full((rows * ldw + guard,), 123.0, dtype=torch.float16, device=dev)
    out = flat[: rows * ldw].view(rows, ldw)
    ops.lora_refit(w0, up, down, scale, gamma, out=out, row0=row0)
    torch.cuda.synchronize()
    ref64 = w0.double() + scale * (up.double() @ down.double())
    if gamma is not None:
        ref64 = ref64 * gamma.double()
    ref = ref64.half()
    got = out[row0:row0 + N, :K]
    ulps = (_ordered(got) - _ordered(ref)).abs()
    exact = (ulps == 0).float().mean().item()
    print(f"N={N} K={K} rank={rank} row0={row0} scale={scale} gamma={with_gamma}: max ulp {ulps.max().item()}, exact {exact:.6f}")
    assert torch.isfinite(got.float()).all()
    assert ulps.max().item() <= 1   # fp32 reassociation ~1e-7 relative against a half-ulp of 5e-4: only rounding ties can move
    assert exact >= 0.99            # a tie has probability ~1e-4: a systematic off-by-one fails here
    if scale == 0.0:
        want = (w0 * gamma).half() if gamma is not None else w0.half()
        assert torch.equal(got, want)
    # rows outside [row0, row0 + N), columns >= K and the guard behind the buffer are untouched
    assert (out[:row0] == 123.0).all() and (out[row0 + N:] == 123.0).all()
    assert (out[:, K:] == 123.0).all()
    assert (flat[rows * ldw:] == 123.0).all()


# ----------------------------------------------------------------------------- handles
@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import server as S, synthetic, weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    dev = torch.device("cuda", 0)
    unet = {k: v.to(dev) for k, v in W.synthetic_unet(5).items()}  # shared by every handle (device copies: loaded without a host pass)
    vae = {k: v.to(dev) for k, v in W.synthetic_vae(5).items()}
    a, b = W.synthetic_lora(5), W.synthetic_lora(6)
    part = {k: v for k, v in W.synthetic_state_dict(W.lora_spec(2), 9).items() if ".attn1." in k}  # attn1 only, rank 2
    canvas, brush, lat, eps = synthetic.make_stamp_batch(2, R, seed=3)
    cond, uncond = synthetic.make_conditioning(4)
    g = torch.Generator().manual_seed(8)
    sample, ctx = torch.randn(3, 9, R // 8, R // 8, generator=g), torch.randn(3, 14, 768, generator=g).half()
    seed0, seed1 = S.stamp_seed(0, Q_ID, 0), S.stamp_seed(0, Q_ID, 1)

    def make(lora, **kw):
        m = MI355ConditionalInpainter(R, device=0, weights=dict(unet=unet, vae=vae, lora=lora), max_batch=2, **kw)
        m.set_option("autotune", 0)  # before the first program is built: heuristic tiles, the same on every handle
        m.set_conditioning(cond, uncond, brush)
        return m

    def stamp1(m):
        return m.generate(canvas[:1], latents=lat[:1], vae_eps=eps[:, :1], **ST).cpu()

    def seeded2(m):
        return m.generate(canvas, seeds=SEEDS, **ST).cpu()

    def unet_eval(m):
        return m.unet(sample, 500.0, ctx).cpu()

    def queue_stamp(m, seed):
        return m.generate(canvas[:1], slots=[0], seeds=[seed], **ST).cpu()

    ref = {}
    for name, lora in (("b", b), ("none", None), ("a_half", {k: (v * 0.5 if ".up." in k else v) for k, v in a.items()}), ("part", part)):
        m = make(lora)
        ref[name] = dict(stamp1=stamp1(m))
        if name == "b":
            ref[name].update(seeded2=seeded2(m), unet=unet_eval(m), queue1=queue_stamp(m, seed1))
        del m
        gc.collect()
    A = make(a)
    first = stamp1(A)  # LoRA a as dtp_finalize_weights merged it
    e = dict(A=A, a=a, b=b, part=part, ref=ref, first=first, first_info=A.stamp_info(), queue0=queue_stamp(A, seed0), state=["created"],
             stamp1=stamp1, seeded2=seeded2, unet_eval=unet_eval, make=make, canvas=canvas)
    yield e
    del e["A"], A
    gc.collect()


def _set(env, name, lora, scale=1.0):
    info = env["A"].set_lora(lora, scale)
    env["state"][0] = name
    return info


# ----------------------------------------------------------------------------- 2. swap
def test_swap_and_swap_back(env):
    A = env["A"]
    if env["state"][0] != "created":
        _set(env, "a", env["a"])
    s0 = env["stamp1"](A)  # the slot's cross-attention matrices are cached from here on
    assert torch.equal(s0, env["first"])
    info0 = A.stamp_info()
    rinfo = _set(env, "b", env["b"])
    s1 = env["stamp1"](A)  # the slot is NOT redefined: a stale cross-attention cache would keep LoRA a's attn2 here
    assert not torch.equal(s1, s0)
    assert torch.equal(s1, env["ref"]["b"]["stamp1"])
    assert A.stamp_info() == info0 == env["first_info"]  # nothing re-captured, the same loop
    assert rinfo["matrices"] == 128 and rinfo["launches"] >= 1 and rinfo["ms"] > 0
    print("refit info:", rinfo)
    assert A.lora_scale == 1.0
    _set(env, "a", env["a"])
    assert torch.equal(env["stamp1"](A), env["first"])


# ----------------------------------------------------------------------------- 3. scale
def test_scale_zero_and_none_are_the_base_model(env):
    A = env["A"]
    _set(env, "a0", env["a"], 0.0)
    assert A.lora_scale == 0.0
    assert torch.equal(env["stamp1"](A), env["ref"]["none"]["stamp1"])
    _set(env, "b", env["b"])
    _set(env, "none", None)
    assert torch.equal(env["stamp1"](A), env["ref"]["none"]["stamp1"])


def test_scale_half_is_a_handle_with_up_halved(env):
    A = env["A"]
    _set(env, "a_half", env["a"], 0.5)  # a power of two: scale * (up @ down) == (scale * up) @ down exactly
    assert A.lora_scale == 0.5
    assert torch.equal(env["stamp1"](A), env["ref"]["a_half"]["stamp1"])


# ----------------------------------------------------------------------------- 4. partial dict, other rank
def test_partial_lora_at_another_rank(env):
    A = env["A"]
    _set(env, "b", env["b"])  # every module carries a LoRA before ...
    _set(env, "part", env["part"])  # ... attn1 only, rank 2: attn2 must go back to its base
    assert torch.equal(env["stamp1"](A), env["ref"]["part"]["stamp1"])


# ----------------------------------------------------------------------------- 5. every path reads the new weights
def test_batched_seeded_stamp_and_engine_call_after_a_refit(env):
    A = env["A"]
    _set(env, "b", env["b"])
    assert torch.equal(env["seeded2"](A), env["ref"]["b"]["seeded2"])
    assert torch.equal(env["unet_eval"](A), env["ref"]["b"]["unet"])


# ----------------------------------------------------------------------------- 6. errors
def _stage(m, key, t):
    t = t.float().contiguous()
    shape = (C.c_int64 * t.dim())(*t.shape)
    return m._lib.dtp_refit_stage(m._h, f"lora.{key}".encode(), C.c_void_p(t.data_ptr()), 0, shape, t.dim())


def test_errors_leave_the_handle_untouched(env):
    A, lib = env["A"], env["A"]._lib
    _set(env, "a", env["a"])
    before = env["stamp1"](A)
    p = "mid_block.attentions.0.transformer_blocks.0.attn2.processor.to_v_lora."
    # a wrong-shape up next to good tensors of other modules: nothing may be written
    q = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora."
    assert _stage(A, q + "down.weight", env["b"][q + "down.weight"]) == 0
    assert _stage(A, q + "up.weight", env["b"][q + "up.weight"]) == 0
    assert _stage(A, p + "down.weight", torch.zeros(4, 768)) == 0
    assert _stage(A, p + "up.weight", torch.ones(1280, 5)) == 0
    assert lib.dtp_refit_lora(A._h, C.c_float(1.0)) == 1  # DTP_ERR_ARG
    assert (p + "up.weight").encode() in lib.dtp_last_error()
    assert torch.equal(env["stamp1"](A), before)
    # a down without its up
    assert _stage(A, p + "down.weight", torch.zeros(4, 768)) == 0
    assert lib.dtp_refit_lora(A._h, C.c_float(1.0)) == 4  # DTP_ERR_MISSING
    assert (p + "down.weight").encode() in lib.dtp_last_error()
    # a target that does not exist
    r = "mid_block.attentions.0.transformer_blocks.0.attn7.processor.to_v_lora."
    assert _stage(A, r + "down.weight", torch.zeros(4, 768)) == 0 and _stage(A, r + "up.weight", torch.zeros(1280, 4)) == 0
    assert lib.dtp_refit_lora(A._h, C.c_float(1.0)) == 1
    assert b"attn7" in lib.dtp_last_error()
    # a NaN scale, with a valid set staged
    assert _stage(A, q + "down.weight", env["b"][q + "down.weight"]) == 0 and _stage(A, q + "up.weight", env["b"][q + "up.weight"]) == 0
    assert lib.dtp_refit_lora(A._h, C.c_float(float("nan"))) == 1
    assert b"scale" in lib.dtp_last_error()
    assert torch.equal(env["stamp1"](A), before)
    # nothing stayed staged after the failures: a full refit to LoRA a is still LoRA a
    _set(env, "a", env["a"])
    assert torch.equal(env["stamp1"](A), env["first"])
    # dtp_load_tensor keeps its answer after finalize
    t = torch.zeros(4, 768)
    shape = (C.c_int64 * 2)(4, 768)
    assert lib.dtp_load_tensor(A._h, ("lora." + p + "down.weight").encode(), C.c_void_p(t.data_ptr()), 0, shape, 2) == 3


def test_fp8_handle_refuses_a_refit(env):
    from diffusiontexturepainting_amd._lib import DtpError
    m = env["make"](env["a"], fp8_linear=True)
    try:
        with pytest.raises(DtpError, match="code 3"):  # DTP_ERR_STATE
            m.set_lora(env["b"])
    finally:
        del m
        gc.collect()


# ----------------------------------------------------------------------------- 7. server
def test_queue_refit_between_two_stamps(env):
    from diffusiontexturepainting_amd import server as S, server_io as sio
    A = env["A"]
    _set(env, "a", env["a"])
    q = S.StampQueue(A, max_batch=2, seeded=True, base_seed=0)
    try:
        slot = q.attach(Q_ID)
        assert slot == 0
        q.brush_slots.add(slot)  # the fixture installed slot 0's conditioning directly (no brush encoder in these weights)
        got = []
        jobs = [q.submit(S._Job("stamp", slot, dict(ST), env["canvas"][0], got.append, seed=q.next_stamp_seed(Q_ID))),
                q.refit(env["b"], 1.0, wait=False),
                q.submit(S._Job("stamp", slot, dict(ST), env["canvas"][0], got.append, seed=q.next_stamp_seed(Q_ID)))]
        for j in jobs:
            assert j.done.wait(120) and j.error is None, j.error
        env["state"][0] = "b"
        want = [sio.encode_generated_response(sio.RequestType.RETURN_STAMP, S.torch_to_np(img[0]))
                for img in (env["queue0"], env["ref"]["b"]["queue1"])]
        assert len(got) == 2 and q.batch_sizes == [1, 1]
        assert got[0] == want[0]  # LoRA a's image of the client's stamp 0
        assert got[1] == want[1]  # LoRA b's image of its stamp 1
    finally:
        q.close()
