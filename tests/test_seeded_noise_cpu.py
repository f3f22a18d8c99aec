"""Seeded stamp noise on the CPU: the Philox4x32-10 of libdtp (dtp_philox4x32, the function the noise kernel runs) against the
Random123 known answers and the numpy restatement (tests/noise_ref.py), the restatement's moments, the argument errors of the new
entry points, the `seeds` argument check, and StampServer(seeded=True) on fake models.  No GPU is touched."""
import ctypes as C
import inspect
import logging
import os

import numpy as np
import pytest
import torch

import noise_ref
from diffusiontexturepainting_amd import server as S, server_io as sio
from diffusiontexturepainting_amd.model_base import ConditionalInpainterBase

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_philox_known_answers(lib):
    from diffusiontexturepainting_amd import ops
    for ctr, key, want in KNOWN:
        assert ops.philox4x32(ctr, key) == want, (ctr, key)
        assert tuple(int(v) for v in noise_ref.philox4x32(ctr, key)) == want, (ctr, key)
    assert lib.dtp_philox4x32(None, None, None) == 1  # DTP_ERR_ARG


def test_restatement_words_equal_the_library(lib):
    from diffusiontexturepainting_amd import ops
    rng = np.random.default_rng(20)
    ctr = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(1000, 2), dtype=np.uint64)
    ref = noise_ref.philox4x32(ctr, key)
    for i in range(1000):
        assert ops.philox4x32(ctr[i], key[i]) == tuple(int(v) for v in ref[i]), i
    # the stamp keying: key = (seed lo, seed hi), counter = (q lo, q hi, draw, 0)
    seed = 0xfedcba9876543210
    w = noise_ref.words(seed, 2, 16)
    for q in range(4):
        assert ops.philox4x32((q, 0, 2, 0), (seed & 0xffffffff, seed >> 32)) == tuple(int(v) for v in w[q])


def test_restatement_moments():
    """The bounds of the GPU test, which are stated at n = 2^20, hold there for every (seed, draw) of the issue; at its n = 4 * 8 * 8
    the same bounds are applied in units of the standard error (noise_ref.check_moments): |mean| <= 5e-3 cannot be asked of 256
    values, whose mean has sigma 6e-2."""
    seeds = (0, 1, (1 << 64) - 1)
    for seed in seeds:
        for draw in range(4):
            noise_ref.check_moments(noise_ref.normals(seed, draw, 4 * 8 * 8), (seed, draw, 256))
            noise_ref.check_moments(noise_ref.normals(seed, draw, 1 << 20), (seed, draw, 1 << 20))
    a, b, c = (noise_ref.normals(s, d, 1 << 20) for s, d in ((1, 0), (1, 1), (2, 0)))
    assert abs(noise_ref.correlation(a, b)) <= 1e-2 and abs(noise_ref.correlation(a, c)) <= 1e-2
    # a prefix of a draw is the draw of a smaller tensor: the counter is the element's index, nothing else
    assert np.array_equal(noise_ref.normals(1, 0, 256), a[:256])
    u = noise_ref.uniform(np.array([0, 0xffffffff], dtype=np.uint32))
    assert 0.0 < u[0] == 2.0 ** -25 and u[1] == 1.0 - 2.0 ** -25 < 1.0


def test_new_entry_points_and_their_argument_errors(lib):
    from diffusiontexturepainting_amd import _lib
    for name in ("dtp_stamp_seeded", "dtp_op_stamp_noise", "dtp_philox4x32"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.dtp_abi_version() == 3  # additions only
    st = (_lib.Settings * 1)(_lib.Settings(4, 5, 4, 2.0, 1.0, 0, 0))
    seeds = (C.c_uint64 * 1)(7)
    assert lib.dtp_stamp_seeded(None, None, st, None, 1, C.c_double(1.0), None, 1, None, None) == 1  # DTP_ERR_ARG
    assert b"seeds" in lib.dtp_last_error()
    for strength in (0.0, 1.5, float("nan")):  # dtp_stamp_strength's checks, in its order
        assert lib.dtp_stamp_seeded(None, None, st, seeds, 1, C.c_double(strength), None, 1, None, None) == 1
        assert b"strength" in lib.dtp_last_error()
    for strength in (1.0, 0.5):
        assert lib.dtp_stamp_seeded(None, None, st, seeds, 1, C.c_double(strength), None, 1, None, None) == 3  # DTP_ERR_STATE: no handle
    buf = (C.c_float * 8)()  # never written: every call below is refused before a launch
    for draw, n in ((-1, 8), (4, 8), (0, 0), (0, -4), (0, 6), (3, 7)):
        assert lib.dtp_op_stamp_noise(1, draw, buf, n, None) == 1, (draw, n)
        assert b"dtp_op_stamp_noise" in lib.dtp_last_error()
    assert lib.dtp_op_stamp_noise(1, 0, None, 8, None) == 1


def test_seeds_argument_check():
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter as M, check_seed_args
    top = (1 << 64) - 1
    assert check_seed_args(None, 3) is None
    assert check_seed_args(5, 3) == ([5, 6, 7], True)
    assert check_seed_args(top, 2) == ([top, 0], True)  # seed + b wraps in 64 bits
    assert check_seed_args([9, 0, top], 3, vae_eps=False) == ([9, 0, top], False)
    assert check_seed_args(np.uint64(4), 1) == ([4], True) and check_seed_args(np.array([1, 2]), 2)[0] == [1, 2]
    assert check_seed_args((1, 2), 2, vae_eps=False, init_eps=False, strength=0.5) == ([1, 2], False)
    assert check_seed_args(1, 1, init_eps=False, strength=1.0) == ([1], True)  # init_eps is ignored at strength 1
    for bad in (-1, 1 << 64, [1, -2], [1, 1 << 64], 1.5, "7", True, [1.0, 2.0], [1, True]):
        with pytest.raises(ValueError, match="seeds"):
            check_seed_args(bad, 2)
    with pytest.raises(ValueError, match="3 seeds for 2"):
        check_seed_args([1, 2, 3], 2)
    z = torch.zeros(2, 4, 8, 8)
    for kw in (dict(latents=z), dict(vae_eps=torch.zeros(2, 2, 4, 8, 8)), dict(init_eps=z, strength=0.5), dict(init_eps=z)):
        with pytest.raises(ValueError, match="exclusive"):
            check_seed_args([1, 2], 2, **kw)
    for kw in (dict(vae_eps=False), dict(init_eps=False)):  # one switch for all VAE draws below strength 1
        with pytest.raises(ValueError, match="together"):
            check_seed_args([1, 2], 2, strength=0.5, **kw)
    for fn in (M.generate, M.generate_raw, M.generate_u8):
        assert inspect.signature(fn).parameters["seeds"].default is None, fn.__name__


# ------------------------------------------------------------------------------------------------ server
R = 16
WINDOW = 0.3  # generous gather window: every request submitted back to back is pending while a batch is gathered


class UnseededModel(ConditionalInpainterBase):
    """raw output = the slot's brush colour; generate() takes no `seeds`."""

    def __init__(self):
        super().__init__()
        self.brushes, self.calls = {}, []

    def device(self):
        return torch.device("cpu")

    def resolution(self):
        return R

    def set_brush(self, image, slot=0):
        self.brushes[slot] = image.mean(dim=(1, 2)).view(1, 3, 1, 1).expand(1, 3, R, R).clone()

    def slot_image(self, slot):
        return self.brushes[slot]

    def generate_raw(self, canvas, slots=None, **settings):
        raise NotImplementedError  # the server only calls generate()

    def _out(self, canvas, slots):
        raw = torch.cat([self.brushes[s] for s in slots])
        a = canvas[:, 3:]
        return canvas[:, :3] * a + raw * (1 - a)

    def generate(self, canvas, slots=None, **settings):
        slots = slots or [0] * canvas.shape[0]
        self.calls.append(dict(slots=tuple(slots), kwargs=dict(settings)))
        return self._out(canvas, slots)


class SeededModel(UnseededModel):
    """... and with `seeds`: records which seed every slot's stamp was run with."""

    def generate(self, canvas, slots=None, seeds=None, **settings):
        slots = slots or [0] * canvas.shape[0]
        self.calls.append(dict(slots=tuple(slots), seeds=None if seeds is None else tuple(seeds), kwargs=dict(settings)))
        return self._out(canvas, slots)


def _hdr():
    return sio.encode_inference_settings(steps=3, width=R, context_pad=5, cfg_weight=2.0, tg_weight=1.0, tg_steps=3)


def _brush(colour):
    img = np.zeros((R, R, 4), np.uint8)
    img[..., :3] = colour
    return sio.encode_request_type(sio.RequestType.NEW_BRUSH_IMAGE) + _hdr() + sio.encode_new_brush_image_request(img)


def _stamp():
    return sio.encode_request_type(sio.RequestType.NEW_STAMP) + _hdr() + sio.image_to_binary(np.zeros((R, R, 4), np.uint8))


CLIENTS = {3: (200, 0, 0), 11: (0, 200, 0)}
BASE = 0x1234


def _server(model, **kw):
    srv = S.StampServer([model], max_batch=8, gather_window_s=WINDOW, **kw)
    for k, col in CLIENTS.items():
        srv.on_message(k, _brush(col), lambda _f: None, wait=True)
    model.calls.clear()
    return srv


def _seeds_by_client(srv, model):
    """client -> the seeds of its stamps in order, read back from the model's calls through the slot table."""
    q = srv.queues[0]
    by_slot = {slot: k for k, slot in q.clients.items()}
    got = {k: [] for k in CLIENTS}
    for call in model.calls:
        assert call["seeds"] is not None and len(call["seeds"]) == len(call["slots"])
        for slot, seed in zip(call["slots"], call["seeds"]):
            got[by_slot[slot]].append(seed)
    return got


def test_splitmix64_and_the_seed_derivation():
    # the first outputs of splitmix64 from state 0 (Vigna's reference implementation): the function of the state after one increment
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF
    assert S.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert S.stamp_seed(BASE, 3, 2) == S.splitmix64(BASE ^ (3 << 32) ^ 2)
    assert S.stamp_seed(0, (1 << 40) + 5, 0) == S.splitmix64(((1 << 72) + (5 << 32)) & ((1 << 64) - 1))  # 64-bit state
    assert S.stamp_seed(0, "kit-7", 1) == S.stamp_seed(0, "kit-7", 1) != S.stamp_seed(0, "kit-8", 1)  # text ids: a stable hash
    assert len({S.stamp_seed(BASE, c, n) for c in range(8) for n in range(8)}) == 64


def test_seeded_server_gives_a_stamp_its_seed_however_it_is_batched(caplog):
    want = {k: [S.stamp_seed(BASE, k, n) for n in range(2)] for k in CLIENTS}
    frames = {}
    # (a) both clients pending together: batched; then each client's second stamp, batched again
    m = SeededModel()
    srv = _server(m, seeded=True, base_seed=BASE)
    with caplog.at_level(logging.DEBUG, logger=S.logger.name):
        for _ in range(2):
            jobs = [srv.on_message(k, _stamp(), lambda f, k=k: frames.setdefault(("a", k), []).append(f)) for k in CLIENTS]
            assert all(j.done.wait(10) for j in jobs)
    assert srv.queues[0].batch_sizes == [2, 2]
    assert _seeds_by_client(srv, m) == want
    assert any(f"{want[3][0]:#018x}" in r.getMessage() for r in caplog.records if r.levelno == logging.DEBUG)
    srv.close()
    # (b) one by one, client after client
    m = SeededModel()
    srv = _server(m, seeded=True, base_seed=BASE)
    for k in CLIENTS:
        for _ in range(2):
            srv.on_message(k, _stamp(), lambda f, k=k: frames.setdefault(("b", k), []).append(f), wait=True)
    assert srv.queues[0].batch_sizes == [1, 1, 1, 1]
    assert _seeds_by_client(srv, m) == want
    srv.close()
    # (c) interleaved: 3, 11, 3 pending at once -- the client's second stamp ends the batch (equal settings: it is simply next)
    m = SeededModel()
    srv = _server(m, seeded=True, base_seed=BASE, mixed_settings=True)
    jobs = [srv.on_message(k, _stamp(), lambda f, k=k: frames.setdefault(("c", k), []).append(f)) for k in (3, 11, 3, 11)]
    assert all(j.done.wait(10) for j in jobs)
    assert _seeds_by_client(srv, m) == want
    srv.close()
    # the seed does not travel: the replies are the same bytes in all three runs
    for k in CLIENTS:
        assert frames[("a", k)] == frames[("b", k)] == frames[("c", k)] and len(frames[("a", k)]) == 2
    # a client that detaches and comes back starts at stamp 0 again
    m = SeededModel()
    srv = _server(m, seeded=True, base_seed=BASE)
    srv.on_message(3, _stamp(), lambda _f: None, wait=True)
    srv.close_client(3)
    srv.on_message(3, _brush(CLIENTS[3]), lambda _f: None, wait=True)
    m.calls.clear()
    srv.on_message(3, _stamp(), lambda _f: None, wait=True)
    assert m.calls[-1]["seeds"] == (want[3][0],)
    srv.close()


def test_unseeded_server_passes_no_seeds():
    m = SeededModel()
    srv = _server(m)
    jobs = [srv.on_message(k, _stamp(), lambda _f: None) for k in CLIENTS]
    assert all(j.done.wait(10) for j in jobs)
    assert m.calls and all(c["seeds"] is None and "seeds" not in c["kwargs"] for c in m.calls)
    assert all(j.seed is None for j in jobs)
    srv.close()
    m = UnseededModel()  # ... and a model without `seeds` serves as before
    srv = _server(m)
    srv.on_message(3, _stamp(), lambda _f: None, wait=True)
    assert len(m.calls) == 1 and "seeds" not in m.calls[0]["kwargs"]
    srv.close()


def test_seeded_needs_a_model_that_takes_seeds():
    with pytest.raises(TypeError, match="seeds"):
        S.StampServer([UnseededModel()], seeded=True)
    with pytest.raises(TypeError, match="seeds"):
        S.StampQueue(UnseededModel(), seeded=True)
