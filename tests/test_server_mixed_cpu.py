"""StampServer(mixed_settings=True) on CPU with fake models: stamps whose guidance settings differ share one call, each with its
own settings; what must not be overtaken still ends the batch; the option off (or a model without `per_stamp`) groups as before."""
import time

import numpy as np
import torch

from diffusiontexturepainting_amd import server as S, server_io as sio
from diffusiontexturepainting_amd.model_base import ConditionalInpainterBase

R = 16
WINDOW = 0.3  # generous gather window: every request submitted back to back is pending while a batch is gathered


class PlainModel(ConditionalInpainterBase):
    """raw output = the slot's brush colour * cfg_weight / 10, one cfg for the whole call (no per-stamp settings)."""

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

    def _raw(self, slots, each):
        return torch.cat([self.brushes[s] * float(st["cfg_weight"]) / 10.0 for s, st in zip(slots, each)])

    def generate(self, canvas, slots=None, **settings):
        slots = slots or [0] * canvas.shape[0]
        self.calls.append(dict(slots=tuple(slots), per_stamp=None, settings=dict(settings)))
        raw = self._raw(slots, [settings] * len(slots))
        a = canvas[:, 3:]
        return canvas[:, :3] * a + raw * (1 - a)


class MixedModel(PlainModel):
    """... and with per-stamp settings: stamp b's output uses per_stamp[b]['cfg_weight']."""

    def generate(self, canvas, slots=None, per_stamp=None, **settings):
        slots = slots or [0] * canvas.shape[0]
        self.calls.append(dict(slots=tuple(slots), per_stamp=per_stamp, settings=dict(settings)))
        each = [{**settings, **p} for p in per_stamp] if per_stamp is not None else [settings] * len(slots)
        raw = self._raw(slots, each)
        a = canvas[:, 3:]
        return canvas[:, :3] * a + raw * (1 - a)


def _hdr(steps=3, cfg=2.0, tg=1.0, tg_steps=3, pad=5):
    return sio.encode_inference_settings(steps=steps, width=R, context_pad=pad, cfg_weight=cfg, tg_weight=tg, tg_steps=tg_steps)


def _brush(colour):
    img = np.zeros((R, R, 4), np.uint8)
    img[..., :3] = colour
    return sio.encode_request_type(sio.RequestType.NEW_BRUSH_IMAGE) + _hdr() + sio.encode_new_brush_image_request(img)


def _stamp(**kw):
    canvas = np.zeros((R, R, 4), np.uint8)
    return sio.encode_request_type(sio.RequestType.NEW_STAMP) + _hdr(**kw) + sio.image_to_binary(canvas)


COLOURS = {"a": (200, 0, 0), "b": (0, 200, 0), "c": (0, 0, 200), "d": (100, 100, 100)}


def _server(model, mixed=True):
    srv = S.StampServer([model], max_batch=8, gather_window_s=WINDOW, mixed_settings=mixed)
    out = {k: [] for k in COLOURS}
    for k, col in COLOURS.items():
        srv.on_message(k, _brush(col), out[k].append, wait=True)
    model.calls.clear()
    return srv, out


def _pixel(frame):
    return sio.decode_response(frame)["image"][3, 3].astype(int)


def test_different_sliders_share_one_call_with_their_own_settings():
    m = MixedModel()
    srv, out = _server(m)
    sliders = {"a": dict(cfg=10.0, tg=0.0, tg_steps=0), "b": dict(cfg=5.0, tg=4.0, tg_steps=20),
               "c": dict(cfg=2.5, tg=1.5, tg_steps=7, pad=40), "d": dict(cfg=7.5, tg=2.0, tg_steps=3)}
    jobs = [srv.on_message(k, _stamp(**sliders[k]), out[k].append) for k in COLOURS]
    assert all(j.done.wait(10) for j in jobs)
    assert srv.queues[0].batch_sizes[-1] == 4 and len(m.calls) == 1
    call = m.calls[0]
    q = srv.queues[0]
    assert call["slots"] == tuple(q.clients[k] for k in COLOURS)
    for k, p in zip(COLOURS, call["per_stamp"]):
        assert float(p["cfg_weight"]) == sliders[k]["cfg"] and float(p["tg_weight"]) == sliders[k]["tg"]
        assert int(p["tg_steps"]) == sliders[k]["tg_steps"] and int(p["context_pad"]) == sliders[k].get("pad", 5)
        want = [int(v * sliders[k]["cfg"] / 10.0) for v in COLOURS[k]]  # each reply rendered with ITS client's cfg
        assert all(abs(g - w) <= 1 for g, w in zip(_pixel(out[k][1]), want)), (k, _pixel(out[k][1]), want)
    srv.close()


def test_what_must_not_be_overtaken_still_ends_the_batch():
    m = MixedModel()
    srv, out = _server(m)
    # other steps ends the batch; a brush change ends the next one; a client's second stamp is never batched with its first
    seq = [("a", _stamp(cfg=3.0)), ("b", _stamp(cfg=4.0)), ("c", _stamp(steps=4)), ("d", _stamp(steps=4, cfg=6.0)),
           ("a", _brush((10, 10, 10))), ("b", _stamp(cfg=5.0)), ("c", _stamp(cfg=6.0)), ("b", _stamp(cfg=7.0)), ("d", _stamp(cfg=8.0))]
    order = []
    jobs = [srv.on_message(k, msg, lambda f, k=k: order.append((k, sio.decode_response(f)["type"]))) for k, msg in seq]
    assert all(j.done.wait(10) for j in jobs)
    q = srv.queues[0]
    sl = {k: q.clients[k] for k in COLOURS}
    stamp_calls = [c["slots"] for c in m.calls]
    assert stamp_calls == [(sl["a"], sl["b"]), (sl["c"], sl["d"]), (sl["a"],), (sl["b"], sl["c"]), (sl["b"], sl["d"])], stamp_calls
    assert [c["settings"]["steps"] for c in m.calls] == [3, 4, 3, 3, 3]
    stamp, preview = sio.RequestType.RETURN_STAMP.value, sio.RequestType.RETURN_PREVIEW.value
    assert order == [("a", stamp), ("b", stamp), ("c", stamp), ("d", stamp), ("a", preview), ("b", stamp), ("c", stamp),
                     ("b", stamp), ("d", stamp)]  # arrival order
    srv.close()


def test_option_off_groups_by_equal_settings_as_before():
    m = MixedModel()
    srv, out = _server(m, mixed=False)
    assert not srv.queues[0].mixed
    jobs = [srv.on_message(k, _stamp(cfg=c), out[k].append) for k, c in (("a", 10.0), ("b", 10.0), ("c", 5.0), ("d", 5.0))]
    assert all(j.done.wait(10) for j in jobs)
    q = srv.queues[0]
    assert [c["slots"] for c in m.calls] == [(q.clients["a"], q.clients["b"]), (q.clients["c"], q.clients["d"])]
    assert all(c["per_stamp"] is None for c in m.calls)
    srv.close()


def test_a_model_without_per_stamp_never_gets_mixed_batches():
    m = PlainModel()
    srv, out = _server(m, mixed=True)
    assert not srv.queues[0].mixed
    jobs = [srv.on_message(k, _stamp(cfg=c), out[k].append) for k, c in (("a", 10.0), ("b", 5.0), ("c", 5.0))]
    assert all(j.done.wait(10) for j in jobs)
    q = srv.queues[0]
    assert [c["slots"] for c in m.calls] == [(q.clients["a"],), (q.clients["b"], q.clients["c"])]
    for k, cfg in (("a", 10.0), ("b", 5.0), ("c", 5.0)):
        want = [int(v * cfg / 10.0) for v in COLOURS[k]]
        assert all(abs(g - w) <= 1 for g, w in zip(_pixel(out[k][1]), want))
    srv.close()


def test_equal_settings_under_the_option_do_not_pass_per_stamp():
    m = MixedModel()
    srv, out = _server(m)
    t0 = time.perf_counter()
    jobs = [srv.on_message(k, _stamp(cfg=4.0), out[k].append) for k in ("a", "b")]
    assert all(j.done.wait(10) for j in jobs) and time.perf_counter() - t0 < 10
    assert len(m.calls) == 1 and m.calls[0]["per_stamp"] is None
    srv.close()
