"""LoRA refit without a GPU: the three entry points exist and are bound, refuse a NULL handle with a message, set_lora checks its
dict against weights.lora_spec before it touches the handle, and the queue runs a refit between two batches (fake model)."""
import ctypes as C
import os
import threading

import pytest
import torch

from diffusiontexturepainting_amd import server as S, weights as W

REFIT_SYMBOLS = ("dtp_refit_stage", "dtp_refit_lora", "dtp_last_refit_info")


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_refit_symbols_exist_and_are_bound(lib):
    from diffusiontexturepainting_amd import _lib
    for name in REFIT_SYMBOLS + ("dtp_op_lora_refit",):
        assert name in _lib.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype is _lib.SYMBOLS[name][0], name
    assert lib.dtp_abi_version() == 3


def test_null_handle_is_an_argument_error_with_a_message(lib):
    data = (C.c_float * 4)()
    shape = (C.c_int64 * 2)(2, 2)
    name = b"lora.x.processor.to_q_lora.down.weight"
    m, n, ms = C.c_int(), C.c_int(), C.c_float()
    calls = {
        "dtp_refit_stage": lambda: lib.dtp_refit_stage(None, name, data, 0, shape, 2),
        "dtp_refit_lora": lambda: lib.dtp_refit_lora(None, 1.0),
        "dtp_last_refit_info": lambda: lib.dtp_last_refit_info(None, C.byref(m), C.byref(n), C.byref(ms)),
    }
    for sym, call in calls.items():
        assert call() == 1, sym  # DTP_ERR_ARG
        msg = lib.dtp_last_error()
        assert msg and sym.encode() in msg, (sym, msg)


def _bare_model():
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    return object.__new__(MI355ConditionalInpainter)  # no handle: set_lora must refuse a bad dict before it needs one


def test_set_lora_rejects_a_wrong_key_by_name():
    m = _bare_model()
    good = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.down.weight"
    bad = "down_blocks.0.attentions.0.transformer_blocks.0.attn3.processor.to_q_lora.up.weight"
    with pytest.raises(ValueError, match="attn3"):
        m.set_lora({good: torch.zeros(4, 320), bad: torch.zeros(320, 4)})


def test_set_lora_rejects_a_wrong_shape_by_name():
    m = _bare_model()
    p = "mid_block.attentions.0.transformer_blocks.0.attn2.processor.to_k_lora."
    with pytest.raises(ValueError, match="to_k_lora.up.weight"):
        m.set_lora({p + "down.weight": torch.zeros(2, 768), p + "up.weight": torch.zeros(1280, 3)})
    with pytest.raises(ValueError, match="to_k_lora.down.weight"):  # K of the cross-attention k is the context width, not 1280
        m.set_lora({p + "down.weight": torch.zeros(2, 1280), p + "up.weight": torch.zeros(1280, 2)})


def test_check_lora_for_refit_accepts_partial_dicts_at_any_rank():
    full = W.lora_spec(2)
    part = {k: torch.zeros(v) for k, v in full.items() if ".attn1." in k}
    assert 0 < len(part) < len(full)
    assert W.check_lora_for_refit(part) == 2
    assert W.check_lora_for_refit({}) is None
    assert W.check_lora_for_refit({k: torch.zeros(v) for k, v in W.lora_spec(7).items()}) == 7


class _FakeModel:
    """What StampQueue needs of a model, plus set_lora: every stamp is painted with the current LoRA's tag."""

    def __init__(self):
        self.tag, self.calls, self.slots = 0.25, [], {}

    def resolution(self):
        return 8

    def device(self):
        return torch.device("cpu")

    def set_brush(self, img, slot=0):
        self.slots[slot] = torch.zeros(1, 3, 8, 8)

    def slot_image(self, slot):
        return self.slots[slot]

    def set_lora(self, lora, scale=1.0):
        if lora == "broken":
            raise ValueError("lora: no such file")
        self.calls.append(("refit", lora, scale))
        self.tag = lora["tag"] * scale

    def generate(self, canvas, slots=None, **settings):
        self.calls.append(("stamp", len(canvas)))
        return torch.full((canvas.shape[0], 3, 8, 8), self.tag)


def test_queue_refit_runs_between_two_batches_in_arrival_order():
    m = _FakeModel()
    q = S.StampQueue(m, max_batch=4, gather_window_s=0.05)
    try:
        slot = q.attach("a")
        got, hold = [], threading.Event()
        brush = q.submit(S._Job("brush", slot, {}, torch.zeros(3, 8, 8), lambda b: hold.wait(5)))  # the worker is busy while the rest queues up
        first = q.submit(S._Job("stamp", slot, dict(steps=4), torch.zeros(4, 8, 8), got.append))
        refit = q.refit(dict(tag=1.0), 0.5, wait=False)
        second = q.submit(S._Job("stamp", slot, dict(steps=4), torch.zeros(4, 8, 8), got.append))
        hold.set()
        for j in (brush, first, refit, second):
            assert j.done.wait(10)
        assert refit.error is None
        assert [c[0] for c in m.calls] == ["stamp", "stamp", "refit", "stamp"]  # (the first stamp is the brush preview)
        assert m.calls[2] == ("refit", dict(tag=1.0), 0.5) and q.batch_sizes == [1, 1]  # the refit ended the batch gather
        assert len(got) == 2 and got[0] != got[1]
        with pytest.raises(RuntimeError, match="no such file"):
            q.refit("broken")
        assert m.tag == 0.5  # a failed refit leaves the model as it was
    finally:
        q.close()


def test_server_refit_reaches_every_replica():
    ms = [_FakeModel(), _FakeModel()]
    srv = S.StampServer(ms)
    try:
        srv.refit(dict(tag=2.0), 1.0)
        assert [m.tag for m in ms] == [2.0, 2.0]
        with pytest.raises(RuntimeError, match="replica 0.*replica 1"):
            srv.refit("broken")
    finally:
        srv.close()
