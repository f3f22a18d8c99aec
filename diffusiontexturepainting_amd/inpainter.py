"""`MI355ConditionalInpainter` -- drop-in for the reference's `TRTConditionalInpainter`
(trt_inference/trt_model.py:22-121) on top of libdtp.so.

Same constructor shape (`resolution, device=0`), same methods and `.image` attribute, same
`settings` keys (numpy scalars from server_io are cast on entry), so `handler.py` / `run.py`
work unchanged with `model = MI355ConditionalInpainter(256)`.  torch only owns the I/O tensors,
the stream and the noise generator; all arithmetic runs in the HIP library, and a missing
library or a failing call raises (there is no fallback path).
"""
import ctypes as C
import operator
import os

import torch

from . import _lib, journal as _journal, mesh as _mesh, weights as W
from ._lib import Settings, check, ptr
from .model_base import ConditionalInpainterBase

DEFAULT_SETTINGS = dict(steps=20, context_pad=150, tg_steps=20, cfg_weight=2.0, tg_weight=1.0)  # Kit defaults, manager.py:104-110


def check_strength_args(strength, init_eps, B, h):
    """The `strength` / `init_eps` arguments of the generate calls: strength in (0, 1] (ValueError otherwise, NaN included); below 1,
    init_eps None, False or one [B,4,h,h] draw per stamp (at 1 it is ignored, as dtp_stamp_strength ignores it).  Returns strength as a
    float."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:  # (NaN fails too)
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    if strength < 1.0 and init_eps is not None and init_eps is not False and tuple(init_eps.shape) != (B, 4, h, h):
        raise ValueError(f"init_eps must be {B} x 4 x {h} x {h} (one draw per stamp), got {tuple(init_eps.shape)}")
    return strength


def check_seed_args(seeds, B, latents=None, vae_eps=None, init_eps=None, strength=1.0):
    """The `seeds` argument of the generate calls.  None: returns None (the unseeded path).  An int s: stamp b gets (s + b) mod 2^64; a
    sequence: B ints.  Every seed is an int in 0 .. 2^64 - 1 (ValueError otherwise).  The seeded call draws its own noise, so a
    `latents`, `vae_eps` or `init_eps` tensor next to `seeds` is a ValueError; vae_eps=False / init_eps=False (the distribution mean)
    stay valid, and below strength 1 the two must agree, since dtp_stamp_seeded has one switch for all VAE draws.
    Returns (list of B seeds, sample_vae)."""
    if seeds is None:
        return None
    for name, t in (("latents", latents), ("vae_eps", vae_eps), ("init_eps", init_eps)):
        if t is not None and t is not False:
            raise ValueError(f"seeds and {name} are exclusive: a seeded stamp draws its own noise (dtp_stamp_seeded)")
    if latents is False:
        raise ValueError("seeds with latents=False: the initial latents are always drawn")
    if float(strength) < 1.0 and (vae_eps is False) != (init_eps is False):
        raise ValueError("seeds below strength 1: pass vae_eps=False and init_eps=False together (one switch for all VAE draws)")
    try:
        if isinstance(seeds, (bool, str, bytes)):
            raise TypeError
        try:
            base = operator.index(seeds)  # an int (numpy integers included)
        except TypeError:
            if any(isinstance(v, bool) for v in seeds):
                raise
            out = [operator.index(v) for v in seeds]
        else:
            if not 0 <= base < 1 << 64:
                raise ValueError(f"seeds must be in 0 .. 2^64 - 1, got {base}")
            out = [(base + b) & ((1 << 64) - 1) for b in range(B)]
    except TypeError:
        raise ValueError(f"seeds must be an int or a sequence of {B} ints, got {seeds!r}") from None
    if len(out) != B:
        raise ValueError(f"{len(out)} seeds for {B} stamps")
    for v in out:
        if not 0 <= v < 1 << 64:
            raise ValueError(f"seeds must be in 0 .. 2^64 - 1, got {v}")
    return out, vae_eps is not False


def _stroke_modes(modes, n, slots=None):
    """The DTP_STROKE_* ids of the n stamps of a stroke (modes: see _stroke_stamps), after the checks every stroke shares."""
    if n < 1:
        raise ValueError("a stroke needs at least one position")
    if modes is None or isinstance(modes, (str, int)):
        modes = [0 if modes is None else modes] * n
    if len(modes) != n:
        raise ValueError(f"{len(modes)} modes for {n} stamps")
    ids = []
    for m in modes:
        if isinstance(m, str):
            if m.lower() not in _lib.STROKE_MODES:
                raise ValueError(f"brush mode {m!r} is not one of {', '.join(_lib.STROKE_MODES)}")
            m = _lib.STROKE_MODES[m.lower()]
        ids.append(int(m))
    if slots is not None and len(slots) != n:
        raise ValueError(f"{len(slots)} slots for {n} stamps")
    return ids


def _stroke_stamps(positions, seeds=None, modes=None, slots=None):
    """The dtp_stroke_stamp array of a stroke.  positions: (x, y) per stamp; seeds: as check_seed_args (None: all 0, for planning);
    modes: None (Inpaint), one mode for all or one per stamp, each a name of _lib.STROKE_MODES or its int (an unknown int is passed
    on: the library refuses it, naming the stamp); slots: None (slot 0) or one per stamp."""
    n = len(positions)
    ids = _stroke_modes(modes, n, slots)
    seeds = [0] * n if seeds is None else check_seed_args(seeds, n)[0]
    arr = (_lib.StrokeStamp * n)()
    for i, (x, y) in enumerate(positions):
        arr[i] = _lib.StrokeStamp(int(x), int(y), ids[i], int(slots[i]) if slots is not None else 0, seeds[i])
    return arr


def _extend_args(how, rings):
    """(how, rings as an int) of extend_selection; ValueError for a how that is not in the table or rings that is no integer (its range
    is the library's to refuse)."""
    if how not in _lib.EXTEND_HOWS:
        raise ValueError(f"how {how!r}: choose one of {', '.join(_lib.EXTEND_HOWS)}")
    if isinstance(rings, bool) or not isinstance(rings, int):
        raise ValueError(f"rings = {rings!r}: an integer in 1..64")
    return how, int(rings)


def _tint_args(color, opacity):
    """(the 3 bytes of a tint as a ctypes array, the opacity as an int); ValueError outside 0..255."""
    if len(color) != 3 or not all(0 <= int(v) <= 255 for v in color) or isinstance(opacity, bool) or not 0 <= int(opacity) <= 255:
        raise ValueError(f"a tint is 3 bytes in 0..255 and an opacity in 0..255, got {color!r} and {opacity!r}")
    return (C.c_uint8 * 3)(*[int(v) for v in color]), int(opacity)


def plan_stroke(positions, H, W, R, modes=None, wrap=False, max_group=1):
    """The groups dtp_stroke makes of a stroke on an H x W texture with R x R windows (dtp_stroke_plan, host only: needs no GPU): the
    list group_of, one non-decreasing group id per stamp.  Stamp i joins the current group iff the group has fewer than max_group
    members, no Erase stamp is involved and its window is disjoint from every window of the group; the order never changes."""
    arr = _stroke_stamps(positions, modes=modes)
    n = len(arr)
    group_of, ng = (C.c_int * n)(), C.c_int()
    check(_lib.load().dtp_stroke_plan(int(H), int(W), int(R), int(bool(wrap)), arr, n, int(max_group), group_of, C.byref(ng)), "dtp_stroke_plan")
    return list(group_of)


class MI355ConditionalInpainter(ConditionalInpainterBase):
    def __init__(self, resolution, device=0, weights="synthetic", max_batch=1, seed=42, use_graph=True, fp8_attention=None, fp8_linear=None,
                 fp8_operands=None, scheduler="DDIM"):
        """weights: "synthetic" (seeded random tensors with the real shapes -- no checkpoints can be
        downloaded in this environment) or a dict {unet, vae, [lora], [clip], [penc]} of
        {diffusers key: tensor} state dicts (see weights.load_checkpoint_file).
        scheduler: the sampler of every stamp, by the reference pipeline's names (stable_diffusion_pipeline.py:115-127):
        "DDIM" (default), "DPM" (DPM-Solver++ 2M) or "LMSD"; see set_scheduler."""
        super().__init__()
        sched_id = _lib.scheduler_id(scheduler)  # ValueError for EulerA / PNDM / unknown names, before any device work
        if not torch.cuda.is_available():
            raise _lib.DtpError("MI355ConditionalInpainter needs a ROCm GPU (torch.cuda.is_available() is False)")
        # GEMM (tile, split-K) choices are timed once per shape at build time and persisted in a per-user cache; the table
        # measured on the build's own MI355X ships with the package as a read-only seed (entries are validated on use)
        cache_dir = os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"),
                                 "diffusiontexturepainting_amd")
        try:
            os.makedirs(cache_dir, mode=0o700, exist_ok=True)
            os.environ.setdefault("DTP_TUNE_CACHE", os.path.join(cache_dir, "tune_cache.txt"))
        except OSError:
            pass  # no writable cache directory: tune in memory only
        seed_file = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tune_seed.txt")
        if os.path.exists(seed_file):
            os.environ.setdefault("DTP_TUNE_SEED", seed_file)
        self._lib = _lib.load()
        self._resolution = int(resolution)
        self._index = device if isinstance(device, int) else torch.device(device).index or 0
        self._device = torch.device("cuda", self._index)
        self.max_batch = int(max_batch)
        handle = C.c_void_p()
        check(self._lib.dtp_create(self._index, self._resolution, self.max_batch, C.byref(handle)), "dtp_create")
        self._h = handle
        if weights == "synthetic":
            weights = dict(unet=W.synthetic_unet(), lora=W.synthetic_lora(), vae=W.synthetic_vae(),
                           clip=W.synthetic_clip(), penc=W.synthetic_patch_encoder())
        self._load(weights)
        if not use_graph or os.environ.get("DTP_NO_GRAPH", "0") not in ("", "0"):  # eager launches instead of hipGraph replay (A/B, debugging)
            check(self._lib.dtp_set_option(self._h, b"use_graph", 0), "dtp_set_option(use_graph)")
        if fp8_attention is None:
            fp8_attention = os.environ.get("DTP_FP8", "0") not in ("", "0")
        self.fp8_attention = bool(fp8_attention)
        if self.fp8_attention:  # BASELINE configs[4]: UNet self-attention on the fp8 MX MFMA (before any program is built)
            check(self._lib.dtp_set_option(self._h, b"fp8_attention", 1), "dtp_set_option(fp8_attention)")
        if fp8_linear is None:
            fp8_linear = os.environ.get("DTP_FP8", "0") not in ("", "0")
        self.fp8_linear = bool(fp8_linear)
        if self.fp8_linear:  # ... and its transformer Linears / 1x1 convs
            check(self._lib.dtp_set_option(self._h, b"fp8_linear", 1), "dtp_set_option(fp8_linear)")
        if fp8_operands is None:
            fp8_operands = os.environ.get("DTP_FP8_OPERANDS", "0") not in ("", "0")
        self.fp8_operands = bool(fp8_operands)
        if self.fp8_operands:  # PARITY-ONLY: transformer Linears with K >= 1280 on e4m3 activations in memory (before any program is built)
            check(self._lib.dtp_set_option(self._h, b"fp8_operands", 1), "dtp_set_option(fp8_operands)")
        self.scheduler = scheduler
        if sched_id != _lib.SCHEDULERS["DDIM"]:
            check(self._lib.dtp_set_option(self._h, b"scheduler", sched_id), "dtp_set_option(scheduler)")
        # noise: seeded once, never reseeded (trt_model.py:54, stable_diffusion_pipeline.py:154-156)
        self.generator = torch.Generator(device=self._device).manual_seed(seed)
        self.stream = torch.cuda.Stream(device=self._device)
        self.pick_stream = torch.cuda.Stream(device=self._device)  # pick() alone runs here, beside whatever self.stream has queued
        self._view_stream = None  # render_view() alone runs there: made at the first view (see view_stream)
        self._view_mips = {}      # (TH, TW) -> the pyramid render_view(filter="trilinear") builds when it is given none
        self.conditioning = None
        self.image = None
        self._slots = {}  # conditioning slot -> (image [1,3,R,R], (cond, uncond))
        self.last_times_ms = None
        self._check_finite = False
        self.lora_scale = 1.0  # of the LoRA the handle holds (set_lora)
        self._stroke_seed = (int(seed) & 0xFFFFFFFF) << 32  # paint_stroke(seeds=None) counts up from here

    # ------------------------------------------------------------------ weights
    def _load(self, nets):
        W.check_against_spec(nets["unet"], W.unet_spec(), "unet")
        W.check_against_spec(nets["vae"], W.vae_spec(), "vae")
        for net, sd in nets.items():
            if sd is None:
                continue
            for key, t in sd.items():
                if net == "penc" and key.startswith("clip."):
                    continue  # frozen tower copy inside image_encoder.pth (dropped by strict=False, trt_model.py:59)
                t = t.detach().to(torch.float32).contiguous()
                shape = (C.c_int64 * t.dim())(*t.shape)
                check(self._lib.dtp_load_tensor(self._h, f"{net}.{key}".encode(), ptr(t), int(t.is_cuda), shape, t.dim()),
                      f"dtp_load_tensor({net}.{key})")
        check(self._lib.dtp_finalize_weights(self._h), "dtp_finalize_weights")

    def set_lora(self, lora, scale=1.0):
        """Replace the LoRA of the live handle (the reference's Engine.refit, utilities.py:88-189, with the lora_scale of
        models.py:1034,1083): every attention projection becomes base + scale * up @ down.  `lora`: a state dict in the key scheme of
        pytorch_lora_weights.bin, a path for weights.load_checkpoint_file, or None for the base model.  A partial dict is allowed (the
        modules it leaves out go back to the base model) and its rank may differ from the one the handle was built with; keys and shapes
        are checked against weights.lora_spec first (ValueError naming the tensor).  Programs, captured graphs, conditioning slots and
        settings survive; the call blocks until the handle's queued work and the refit have finished (dtp_refit_lora).  Sets
        `.lora_scale`.  Returns refit_info()."""
        if isinstance(lora, (str, os.PathLike)):
            lora = W.load_checkpoint_file(os.fspath(lora))
        lora = dict(lora) if lora is not None else {}
        scale = float(scale)
        W.check_lora_for_refit(lora)
        self.stream.synchronize()
        try:
            for key, t in lora.items():
                t = t.detach().to(torch.float32).contiguous()
                shape = (C.c_int64 * t.dim())(*t.shape)
                check(self._lib.dtp_refit_stage(self._h, f"lora.{key}".encode(), ptr(t), int(t.is_cuda), shape, t.dim()),
                      f"dtp_refit_stage(lora.{key})")
        except Exception:
            self._lib.dtp_refit_lora(self._h, C.c_float(float("nan")))  # drops what was staged; writes nothing
            raise
        check(self._lib.dtp_refit_lora(self._h, C.c_float(scale)), "dtp_refit_lora")
        self.lora_scale = scale
        return self.refit_info()

    def refit_info(self):
        """Of the last set_lora: matrices rewritten, kernel launches enqueued, device milliseconds (dtp_last_refit_info)."""
        m, n, ms = C.c_int(), C.c_int(), C.c_float()
        check(self._lib.dtp_last_refit_info(self._h, C.byref(m), C.byref(n), C.byref(ms)), "dtp_last_refit_info")
        return dict(matrices=m.value, launches=n.value, ms=ms.value)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.dtp_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ operator API
    def device(self):
        return self._device

    def resolution(self):
        return self._resolution

    def _s(self):
        return C.c_void_p(self.stream.cuda_stream)

    def set_brush(self, image, slot=0):
        """image: 3 x H x W float32 0..1 (trt_model.py:79-88).  Sets `.image` [1,3,R,R] on the device.
        `slot` (0..15) selects a conditioning slot: the multi-client server keeps one brush per client and batches their stamps
        (`generate(..., slots=[...])`); slot 0 is the reference's single brush."""
        img = image.detach().to(self._device, torch.float32).contiguous()
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError(f"set_brush expects a 3 x H x W image, got {tuple(img.shape)}")
        out = torch.empty(1, 3, self._resolution, self._resolution, dtype=torch.float32, device=self._device)
        self.stream.wait_stream(torch.cuda.current_stream(self._device))
        with torch.cuda.stream(self.stream):
            check(self._lib.dtp_set_brush_slot(self._h, int(slot), ptr(img), img.shape[1], img.shape[2], ptr(out), self._s()), "dtp_set_brush")
            cond = torch.empty(2, 1, 14, 768, dtype=torch.float32, device=self._device)
            check(self._lib.dtp_get_conditioning_slot(self._h, int(slot), ptr(cond[0]), ptr(cond[1]), self._s()), "dtp_get_conditioning")
        self.stream.synchronize()
        self._slots[int(slot)] = (out, (cond[0], cond[1]))
        if slot == 0:
            self.image = out
            self.conditioning = (cond[0], cond[1])

    def slot_image(self, slot):
        """The resized brush image [1,3,R,R] of a conditioning slot (what `.image` is for slot 0)."""
        return self._slots[int(slot)][0]

    def set_conditioning(self, image_embeds, negative_embeds, image, slot=0):
        """Install precomputed conditioning ([1,14,768] each) and the R x R brush image [1,3,R,R]."""
        ce = image_embeds.detach().to(self._device, torch.float32).reshape(14, 768).contiguous()
        ue = negative_embeds.detach().to(self._device, torch.float32).reshape(14, 768).contiguous()
        img = image.detach().to(self._device, torch.float32).reshape(3, self._resolution, self._resolution).contiguous()
        torch.cuda.current_stream(self._device).synchronize()
        check(self._lib.dtp_set_conditioning_slot(self._h, int(slot), ptr(ce), ptr(ue), ptr(img), self._s()), "dtp_set_conditioning")
        self.stream.synchronize()
        self._slots[int(slot)] = (img.unsqueeze(0), (ce.unsqueeze(0), ue.unsqueeze(0)))
        if slot == 0:
            self.image = img.unsqueeze(0)
            self.conditioning = (ce.unsqueeze(0), ue.unsqueeze(0))

    def _stamp(self, canvas, settings, composite, latents=None, vae_eps=None, output_u8=False, slots=None, per_stamp=None, strength=1.0,
               init_eps=None, seeds=None):
        if not self._slots:
            raise _lib.DtpError("no brush set: call set_brush() first")
        R, h = self._resolution, self._resolution // 8
        canvas = canvas.detach().to(self._device, torch.float32).contiguous()
        B = canvas.shape[0]
        if canvas.shape != (B, 4, R, R):
            raise ValueError(f"canvas must be B x 4 x {R} x {R}, got {tuple(canvas.shape)}")
        strength = check_strength_args(strength, init_eps, B, h)
        seeded = check_seed_args(seeds, B, latents, vae_eps, init_eps, strength)
        s = {**DEFAULT_SETTINGS, **{k: v for k, v in settings.items() if k in DEFAULT_SETTINGS}}

        def setting(e):  # numpy scalars are cast here (server_io.py:104-119)
            return Settings(int(e["steps"]), int(e["context_pad"]), int(e["tg_steps"]), float(e["cfg_weight"]), float(e["tg_weight"]),
                            int(composite), int(output_u8))

        st = setting(s)  # what dtp_stamp / dtp_stamp_slots take; the other entry points take `each`, one per stamp
        if per_stamp is not None:
            if len(per_stamp) != B:
                raise ValueError(f"{len(per_stamp)} per_stamp entries for {B} stamps")
            each = (Settings * B)(*[setting({**s, **{k: v for k, v in d.items() if k in DEFAULT_SETTINGS}}) for d in per_stamp])
        else:
            each = (Settings * B)(*([st] * B))
        if seeded is not None:  # the library draws: self.generator is not touched
            latents, vae_eps, init_eps = None, False, False
        if latents is None and seeded is None:
            latents = torch.randn((B, 4, h, h), device=self._device, dtype=torch.float32, generator=self.generator)
        if vae_eps is None:
            vae_eps = torch.randn((2, B, 4, h, h), device=self._device, dtype=torch.float32, generator=self.generator)
        if strength < 1.0 and init_eps is None:  # the third draw, after the two of today's path
            init_eps = torch.randn((B, 4, h, h), device=self._device, dtype=torch.float32, generator=self.generator)
        latents = latents.to(self._device, torch.float32).contiguous() if latents is not None else None
        vae_eps = vae_eps.to(self._device, torch.float32).contiguous() if vae_eps is not False else None
        init_eps = init_eps.to(self._device, torch.float32).contiguous() if strength < 1.0 and init_eps is not False else None
        out = (torch.empty(B, R, R, 3, dtype=torch.uint8, device=self._device) if output_u8
               else torch.empty(B, 3, R, R, dtype=torch.float32, device=self._device))
        self.stream.wait_stream(torch.cuda.current_stream(self._device))
        if slots is not None and len(slots) != B:
            raise ValueError(f"{len(slots)} slots for {B} stamps")
        arr = (C.c_int * B)(*[int(v) for v in slots]) if slots is not None else None
        if seeded is not None:  # dtp_stamp_seeded is dtp_stamp_strength with the library's own draws
            check(self._lib.dtp_stamp_seeded(self._h, ptr(canvas), each, (C.c_uint64 * B)(*seeded[0]), int(seeded[1]), C.c_double(strength),
                                             ptr(out), B, arr, self._s()), "dtp_stamp_seeded")
        elif strength < 1.0:  # strength is per call
            check(self._lib.dtp_stamp_strength(self._h, ptr(canvas), each, ptr(latents), ptr(vae_eps), ptr(init_eps), C.c_double(strength),
                                               ptr(out), B, arr, self._s()), "dtp_stamp_strength")
        elif per_stamp is not None:
            check(self._lib.dtp_stamp_mixed(self._h, ptr(canvas), each, ptr(latents), ptr(vae_eps), ptr(out), B, arr, self._s()),
                  "dtp_stamp_mixed")
        elif slots is None:
            check(self._lib.dtp_stamp(self._h, ptr(canvas), C.byref(st), ptr(latents), ptr(vae_eps), ptr(out), B, self._s()), "dtp_stamp")
        else:
            check(self._lib.dtp_stamp_slots(self._h, ptr(canvas), C.byref(st), ptr(latents), ptr(vae_eps), ptr(out), B, arr, self._s()),
                  "dtp_stamp_slots")
        torch.cuda.current_stream(self._device).wait_stream(self.stream)
        # keep the inputs alive until the stream has consumed them
        for t in (canvas, latents, vae_eps, init_eps, out):
            if t is not None:
                t.record_stream(self.stream)
        if self._check_finite and not self.last_stamp_finite():  # debug option: one sync per stamp, like the reference's assert
            raise _lib.DtpError("stamp produced NaN/inf (check_finite): latents or decoded image are not finite")
        return out

    def generate_raw(self, canvas, latents=None, vae_eps=None, slots=None, per_stamp=None, strength=1.0, init_eps=None, seeds=None,
                     **settings):
        """canvas B x 4 x R x R 0..1 -> B x 3 x R x R 0..1 (trt_model.py:90-121).  `latents`
        ([B,4,h,w]) / `vae_eps` ([2,B,4,h,w]; False = use the latent mean) override the internal
        generator -- the parity tests feed CPU-generated noise through them.  `per_stamp`: one dict of setting overrides per stamp
        (context_pad, tg_steps, cfg_weight, tg_weight), merged over `settings` and the defaults; `steps` must agree across the batch.
        `strength` in (0, 1] (the whole call; inpaint_pipeline.py:63): below 1 the stamp starts from the canvas's own latents noised to
        the sampler's t_start and runs only the last evaluations of the schedule (dtp_stamp_strength); 1 is today's
        stamp from pure noise.  `init_eps` ([B,4,h,w]; False = the latent mean; drawn after `vae_eps` when None): the normal draw of the
        canvas's VAE encode, used only below strength 1.
        `seeds` (an int s: stamp b gets s + b; or B ints, each 0 .. 2^64 - 1): the stamp's noise is drawn on the device from its own
        seed (dtp_stamp_seeded), the same numbers in any batch, slot order or replica; exclusive with `latents` / `vae_eps` / `init_eps`
        tensors (vae_eps=False and init_eps=False still select the means), and the internal generator is left alone."""
        return self._stamp(canvas, settings, composite=False, latents=latents, vae_eps=vae_eps, slots=slots, per_stamp=per_stamp,
                           strength=strength, init_eps=init_eps, seeds=seeds)

    def generate(self, canvas, latents=None, vae_eps=None, slots=None, per_stamp=None, strength=1.0, init_eps=None, seeds=None,
                 **settings):
        """generate_raw + alpha composite (model_base.py:51-58), fused into the final kernel.  `slots`: one conditioning slot per
        stamp of the batch (stamps of different clients / brushes in one call); None = slot 0 for all.  `per_stamp`, `strength`,
        `init_eps`, `seeds`: see generate_raw."""
        return self._stamp(canvas, settings, composite=True, latents=latents, vae_eps=vae_eps, slots=slots, per_stamp=per_stamp,
                           strength=strength, init_eps=init_eps, seeds=seeds)

    def generate_u8(self, canvas, composite=True, slots=None, per_stamp=None, strength=1.0, init_eps=None, seeds=None, **settings):
        """Same as generate() but returns the handler's wire image: uint8 HWC, truncated (handler.py:55-56)."""
        return self._stamp(canvas, settings, composite=composite, output_u8=True, slots=slots, per_stamp=per_stamp, strength=strength,
                           init_eps=init_eps, seeds=seeds)

    def plan_stroke(self, positions, H, W, modes=None, wrap=False, max_group=1):
        """The groups paint_stroke makes of these stamps on an H x W texture: plan_stroke at this model's resolution, with max_group
        bounded by max_batch as dtp_stroke bounds it."""
        return plan_stroke(positions, H, W, self._resolution, modes=modes, wrap=wrap, max_group=min(int(max_group), self.max_batch))

    def paint_stroke(self, texture, positions, seeds=None, modes=None, slots=None, wrap=False, margin=0, overpaint_margins=(10, 25),
                     mask=None, max_group=1, sample_vae=True, strength=1.0, **settings):
        """Paint a stroke into `texture` (uint8 [H,W,4] RGBA on the model's device, contiguous; painted in place and returned) without a
        host round trip per stamp: the Kit app's loop (manager.py:229-271) as one dtp_stroke call.  positions: (x, y) per stamp, the
        top-left texel (column x, row y) of its R x R window; any ints.  seeds: an int s (stamp i gets s + i), one per stamp, or None
        (an internal counter).  modes: "inpaint" | "erase" | "overpaint" (or 0 | 1 | 2), one for all or one per stamp (manager.py:70).
        slots: one conditioning slot per stamp.  wrap: window coordinates modulo H and W (a tileable texture stays tileable); otherwise
        texels outside the texture are unknown to the stamp and never written.  margin: the default paste mask is 1 on
        [margin, R - margin)^2 (make_stamp_mask); mask: an [R,R] tensor instead, applied where > 0.  overpaint_margins: (rows, columns)
        of overpaint_canvas.  max_group: up to this many (and max_batch) consecutive stamps with disjoint windows share one batched
        stamp (plan_stroke); 1 = strictly serial, bit for bit the host loop over generate_u8(composite=False, seeds=[seed]).
        sample_vae, strength, settings: as generate_raw(seeds=...), for every stamp.  The call only enqueues (dtp_stroke)."""
        if not self._slots:
            raise _lib.DtpError("no brush set: call set_brush() first")
        R = self._resolution
        if not (isinstance(texture, torch.Tensor) and texture.dtype == torch.uint8 and texture.dim() == 3 and texture.shape[2] == 4
                and texture.device == self._device and texture.is_contiguous()):
            raise ValueError(f"texture must be a contiguous uint8 [H, W, 4] tensor on {self._device} (it is painted in place)")
        n = len(positions)
        if seeds is None:
            seeds = self._stroke_seed
            self._stroke_seed = (self._stroke_seed + n) & ((1 << 64) - 1)
        stamps = _stroke_stamps(positions, seeds, modes, slots)
        strength = check_strength_args(strength, False, n, R // 8)
        s = {**DEFAULT_SETTINGS, **{k: v for k, v in settings.items() if k in DEFAULT_SETTINGS}}
        st = Settings(int(s["steps"]), int(s["context_pad"]), int(s["tg_steps"]), float(s["cfg_weight"]), float(s["tg_weight"]), 0, 0)
        opts = _lib.StrokeOpts(int(bool(wrap)), int(margin), int(overpaint_margins[0]), int(overpaint_margins[1]), int(max_group),
                               int(bool(sample_vae)), strength)
        if mask is not None:
            if tuple(mask.shape) != (R, R):
                raise ValueError(f"mask must be {R} x {R}, got {tuple(mask.shape)}")
            mask = (mask.detach().to(self._device) > 0).to(torch.uint8).contiguous()
        self.stream.wait_stream(torch.cuda.current_stream(self._device))
        check(self._lib.dtp_stroke(self._h, ptr(texture), texture.shape[0], texture.shape[1], stamps, n, C.byref(st), C.byref(opts),
                                   ptr(mask), self._s()), "dtp_stroke")
        torch.cuda.current_stream(self._device).wait_stream(self.stream)
        for t in (texture, mask):  # keep them alive until the stream has consumed them
            if t is not None:
                t.record_stream(self.stream)
        if self._check_finite and not self.last_stamp_finite():
            raise _lib.DtpError("stamp produced NaN/inf (check_finite): latents or decoded image are not finite")
        return texture

    def load_mesh(self, vertices, faces, face_uvs):
        """A mesh on this model's device for paint_mesh_stroke (dtp_mesh_create): vertices [V, 3], faces [F, 3], face_uvs [F, 3, 2]
        (per face and corner, in 0..1, v up), copied from the host once.  Returns a mesh.Mesh; it lives as long as this model."""
        return _mesh.Mesh(self._h, vertices, faces, face_uvs, keep=self)

    def paint_mesh_stroke(self, mesh, texture, positions, normals, prev_positions, fov, seeds=None, modes=None, slots=None,
                          flip_normals=False, margin=1, overpaint_margins=(10, 25), mask=None, sample_vae=True, strength=1.0, bleed=0,
                          face_mask=None, occlude=None, **settings):
        """Paint a stroke on a textured mesh without a host round trip per stamp: TexturePainterManager.stamp (manager.py:199-271) as one
        dtp_mesh_stroke call.  Per stamp, in order: an orthographic look-at camera from positions[i] + normals[i] at positions[i] with
        up = prev_positions[i] - positions[i] (mesh_camera), the render of `mesh` with `texture` (uint8 [H,W,4] on the model's device,
        contiguous; painted in place and returned) into the R x R window, the stamp, and the backprojection of the painted stamp into the
        texture through the faces the window shows.  fov: half the window's width in world units, one float or one per stamp (the Kit
        app's fov_distance * fov_scale).  seeds, modes, slots, mask, overpaint_margins, sample_vae, strength, settings: as paint_stroke;
        margin=1 is the Kit app's stamp mask; an "erase" stamp without `mask` uses the analytic disc.  flip_normals: a left-handed mesh.
        Strictly serial: stamp i + 1 renders what stamp i painted.  The call only enqueues.  bleed: a radius 1..16 in texels; after
        every stamp the texels no face of the mesh covers (the gutter between UV charts) take the nearest covered texel within that
        radius, inside the stamp's texel bounding box grown by the radius, so that the next stamp's render and any filtered view of the
        texture see no unpainted line along the seams (dtp_mesh_stroke_bleed; the first use with a texture size builds the mesh's
        coverage mask and waits for it once).  0: no pass, dtp_mesh_stroke exactly.
        face_mask: a face set (mesh.faceset_from_bool, select_faces): int32 [(F + 31) // 32] on the model's device,
        contiguous.  A face whose bit is 0 is never backprojected, so the stroke paints the texels of the selected faces alone; the
        render still shows the whole mesh and the stamp is the stamp it would have been (dtp_mesh_stroke_masked).  The set is read on
        the device when the stroke runs: the stroke's stream first waits for self.view_stream, so select-then-paint needs no
        synchronisation, and the tensor must stay unchanged until the stroke has run.  None: the call without the keyword.
        occlude: the per-texel occlusion test of the backprojection (dtp_mesh_stroke_occluded).  Without it a face the
        window shows is backprojected whole, the part of it that lies behind another face included, and those texels receive the
        pixels of the face in front.  With it a tap of the stamp image that shows a face more than `occlude` stamp pixels of depth in
        front of the texel's own face is left out, and a texel all of whose taps are is not written.  True: 1.0, which the bumps of a
        smooth surface pass untouched; a float >= 0: that tolerance; None or False: off, the call without the keyword.  It composes
        with bleed, face_mask and an open journal record."""
        occlude = _mesh.occlude_arg(occlude)
        if not self._slots:
            raise _lib.DtpError("no brush set: call set_brush() first")
        R = self._resolution
        if not isinstance(mesh, _mesh.Mesh):
            raise ValueError("mesh must come from load_mesh()")
        if not (isinstance(texture, torch.Tensor) and texture.dtype == torch.uint8 and texture.dim() == 3 and texture.shape[2] == 4
                and texture.device == self._device and texture.is_contiguous()):
            raise ValueError(f"texture must be a contiguous uint8 [H, W, 4] tensor on {self._device} (it is painted in place)")
        n = len(positions)
        ids = _stroke_modes(modes, n, slots)
        if seeds is None:
            seeds = self._stroke_seed
            self._stroke_seed = (self._stroke_seed + n) & ((1 << 64) - 1)
        stamps = _mesh.mesh_stamps(positions, normals, prev_positions, fov, check_seed_args(seeds, n)[0], ids, slots)
        strength = check_strength_args(strength, False, n, R // 8)
        s = {**DEFAULT_SETTINGS, **{k: v for k, v in settings.items() if k in DEFAULT_SETTINGS}}
        st = Settings(int(s["steps"]), int(s["context_pad"]), int(s["tg_steps"]), float(s["cfg_weight"]), float(s["tg_weight"]), 0, 0)
        opts = _lib.MeshStrokeOpts(int(bool(flip_normals)), int(margin), int(overpaint_margins[0]), int(overpaint_margins[1]),
                                   int(bool(sample_vae)), strength)
        if mask is not None:
            if tuple(mask.shape) != (R, R):
                raise ValueError(f"mask must be {R} x {R}, got {tuple(mask.shape)}")
            mask = (mask.detach().to(self._device) > 0).to(torch.uint8).contiguous()
        if face_mask is not None:
            _mesh.faceset_check(face_mask, mesh.num_faces, self._device)
        self.stream.wait_stream(torch.cuda.current_stream(self._device))
        if face_mask is not None and self._view_stream is not None:
            self.stream.wait_stream(self._view_stream)  # a select_faces that is still writing the set
        if occlude is not None:
            check(self._lib.dtp_mesh_stroke_occluded(self._h, mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], stamps, n,
                                                     C.byref(st), C.byref(opts), ptr(mask), int(bleed), ptr(face_mask),
                                                     0 if face_mask is None else face_mask.shape[0], C.c_float(occlude), self._s()),
                  "dtp_mesh_stroke_occluded")
        elif face_mask is not None:
            check(self._lib.dtp_mesh_stroke_masked(self._h, mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], stamps, n,
                                                   C.byref(st), C.byref(opts), ptr(mask), int(bleed), ptr(face_mask), face_mask.shape[0],
                                                   self._s()), "dtp_mesh_stroke_masked")
        elif int(bleed) == 0:
            check(self._lib.dtp_mesh_stroke(self._h, mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], stamps, n, C.byref(st),
                                            C.byref(opts), ptr(mask), self._s()), "dtp_mesh_stroke")
        else:
            check(self._lib.dtp_mesh_stroke_bleed(self._h, mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], stamps, n,
                                                  C.byref(st), C.byref(opts), ptr(mask), int(bleed), self._s()), "dtp_mesh_stroke_bleed")
        torch.cuda.current_stream(self._device).wait_stream(self.stream)
        for t in (texture, mask, face_mask):  # keep them alive until the stream has consumed them
            if t is not None:
                t.record_stream(self.stream)
        if self._check_finite and not self.last_stamp_finite():
            raise _lib.DtpError("stamp produced NaN/inf (check_finite): latents or decoded image are not finite")
        return texture

    def pick(self, mesh, origins, directions):
        """The closest hit of n rays on `mesh` (dtp_mesh_pick; what the Kit app asks MeshRaycast.raycast_closest for, ui/brush.py:154-156):
        origins, directions [n, 3] (or [3]), n in 1..4096; directions need not be unit vectors.  -> a dict of CPU tensors: face i32 [n]
        (-1: no hit, and zeros in every other field), w f32 [n, 3] the barycentric weights, pos [n, 3], normal [n, 3] the face's unit
        normal turned towards the ray's origin, uv [n, 2], t [n] the distance along the normalised direction.  The rule is the render's
        visibility at one sample per ray, exact and order-free; both sides of a face can be hit.  It runs on self.pick_stream and waits
        for that stream only: it takes no part in the hand-shake of self.stream, so it answers while a queued stroke is still painting.
        It reads the mesh's vertices, faces and UVs alone.  One pick of a mesh at a time."""
        if not isinstance(mesh, _mesh.Mesh):
            raise ValueError("mesh must come from load_mesh()")
        rays, n = _mesh.rays(origins, directions)
        rec = torch.zeros(n, _mesh.HIT_WORDS, dtype=torch.int32)
        check(self._lib.dtp_mesh_pick(mesh.handle, C.cast(rays.data_ptr(), C.POINTER(_lib.Ray)), n, ptr(rec),
                                      C.c_void_p(self.pick_stream.cuda_stream)), "dtp_mesh_pick")
        return _mesh.hits_dict(rec)

    def paint_mesh_path(self, mesh, texture, origins, directions, radius, stamps_per_radius=1, fov=None, state=None, **stroke_kwargs):
        """From the pointer's rays to paint (the Kit app's BrushTool.handle_mouse_move, ui/brush.py:139-198): pick(mesh, origins,
        directions) -> mesh.plan_path(hits, radius / stamps_per_radius, state) -> paint_mesh_stroke with the planned stamps.  radius:
        the brush radius in world units; fov defaults to it.  state: None for a new path, or what the last call returned, so that a
        path can be painted as the pointer events arrive.  Every other keyword is paint_mesh_stroke's (seeds, modes -- one mode for the
        whole path --, bleed, mask, face_mask, occlude, settings ...); a stamp whose camera is refused is refused by the stroke as always.  A path that
        plans no stamp (all rays miss, or the pointer has not moved far enough) paints nothing.  -> (texture, state, stamps painted)."""
        hits = self.pick(mesh, origins, directions)
        positions, normals, prevs, state = _mesh.plan_path(hits, float(radius) / float(stamps_per_radius), state)
        n = positions.shape[0]
        if n == 0:
            return texture, state, 0
        self.paint_mesh_stroke(mesh, texture, positions, normals, prevs, float(radius if fov is None else fov), **stroke_kwargs)
        return texture, state, n

    @property
    def view_stream(self):
        """The stream of render_view: not the pick's, not the stroke's.  Made at the first view, so that a model that never looks
        creates the streams it always did, and with high priority: the runtime keeps the queues of a priority apart, so a short frame
        never lands in the hardware queue in which a stroke -- or the caller's stream waiting for one -- is lined up."""
        if self._view_stream is None:
            self._view_stream = torch.cuda.Stream(device=self._device, priority=-1)
        return self._view_stream

    def render_view(self, mesh, texture, camera, size=None, cull=False, flip_normals=False, shade=True, ambient=0.25, unpainted=(128, 128, 128),
                    background=(0, 0, 0, 0), out=None, want_face_idx=False, want_depth=False, live=False, filter="bilinear", mips=None,
                    want_lod=False, clip_near=False, samples=1, want_coverage=False, anisotropy=1, want_taps=False, selection=None,
                    selection_color=(255, 160, 0), selection_opacity=128):
        """A perspective view of the whole painted mesh (dtp_mesh_view; in the Kit app the viewport is Omniverse RTX):
        `mesh` from load_mesh, `texture` uint8 [TH, TW, 4] on the model's device, `camera` from mesh.view_camera, size = (H, W) (default
        the camera's; each side 1..4096).  -> the frame, uint8 [H, W, 4] on the device (RGB the texture under its alpha over `unpainted`,
        shaded by ambient + (1 - ambient) |n_z| unless shade is off; alpha 255; `background` where no face is), and with want_face_idx /
        want_depth also int32 [H, W] (-1: no face) and float32 [H, W] (the distance along the view direction; 0: no face), as a tuple in
        that order.  cull: front faces only; flip_normals: a left-handed mesh.  A face with any vertex nearer than the camera's near
        plane is dropped whole, not clipped (unless clip_near, below); one sample per pixel, no mips: a preview that aliases under minification.  out: a frame to
        write into.  The call only enqueues, on self.view_stream.  live=False: that stream first waits for everything queued on the
        stroke's stream, so the frame shows all that was painted so far and is exact.  live=True: it waits for nothing and answers while
        a queued stroke is still painting; each texel is then either old or new, and the frame may catch a stamp halfway.  The
        caller's current stream waits for the frame (on the device; the host does not block).  One view of a mesh at a time.
        filter="trilinear" (dtp_mesh_view_mips): the sample is blended from two levels of the texture's mip pyramid,
        picked per pixel from the pixel's footprint in the texture, so a minified mesh shows its colour instead of single texels; a
        magnified frame is the bilinear one byte for byte.  mips: the pyramid from build_mips(texture) (complete before a live=True
        call, which waits for nothing); None: built here on the view's stream, after the same waits the frame makes, into a buffer the
        model keeps per texture shape -- so a live pyramid may catch a stamp halfway, as the frame may.  want_lod: also the level
        each pixel took, float32 [H, W] (0 where no face is), last in the tuple.
        clip_near=True (dtp_mesh_view_clip): a face ACROSS the near plane is drawn down to the plane instead of dropped
        -- the floor under the camera, the walls of a room painted from inside -- with either filter; no pixel then has a depth below
        the camera's near, and the face a frame shows at a pixel is the face mesh.view_rays' ray of that pixel hits.  Faces wholly in
        front keep their exact coverage, and a frame without a crossing face is the same bytes as without the keyword.
        samples=2 or 4 (dtp_mesh_view_aa): anti-aliasing, samples x samples centres per pixel on an ordered grid, in one
        pass.  The samples of pixel (i, j) are the pixels (samples i + a, samples j + b) of the frame the same call would draw at
        samples x the size (which is never stored), and the pixel is the rounded average of their bytes, per channel, the background's
        bytes included: with the default transparent background a silhouette pixel carries its colour premultiplied by its coverage,
        and the coverage in alpha.  face_idx, depth and lod are those of the sample just below and right of the pixel's centre; lod
        comes out about log2(samples) lower, because a sample covers that much less of the texture.  samples x each side <= 4096, so
        1080p takes samples=2.  want_coverage: also uint8 [H, W], how many of the pixel's samples a face covers (0 .. samples^2), last
        in the tuple.  samples=1 without want_coverage is the call it always was, launch for launch.
        anisotropy=2..16 with filter="trilinear" (dtp_mesh_view_aniso): the trilinear filter takes one level from the
        LONGER axis of the pixel's footprint, so a floor running away from the eye -- every surface of a room seen from inside -- is
        sampled several levels too coarse and turns grey.  With this the level comes from the shorter axis (never finer than a texel,
        never more than `anisotropy` times finer than the longer axis) and up to `anisotropy` trilinear taps spread along the longer
        axis are averaged: stripes across the line of sight stay stripes.  Works with clip_near, samples, mips, out, live, want_lod and
        want_coverage as before; a magnified frame is still the bilinear one byte for byte, and visibility, face_idx and depth do not
        change.  want_taps: also uint8 [H, W], the number of taps the pixel took (0 where no face is), after lod and before coverage.
        anisotropy=1 is the call without the keyword.
        selection: a face set; the pixels that show one of its faces are tinted after the raster, as
        tint_selection(frame, face_idx, selection, selection_color, selection_opacity) does.  None: no pass."""
        if selection is not None:
            if not isinstance(mesh, _mesh.Mesh):
                raise ValueError("mesh must come from load_mesh()")
            _mesh.faceset_check(selection, mesh.num_faces, self._device, what="selection")
            color, opacity = _tint_args(selection_color, selection_opacity)
        if filter not in ("bilinear", "trilinear"):
            raise ValueError(f"filter {filter!r}: choose 'bilinear' or 'trilinear'")
        anisotropy = _lib.view_anisotropy_check(anisotropy, filter, want_taps, least=2)
        trilinear = filter == "trilinear"
        if not trilinear and (mips is not None or want_lod):
            raise ValueError("mips and want_lod need filter='trilinear'")
        if not isinstance(mesh, _mesh.Mesh):
            raise ValueError("mesh must come from load_mesh()")
        if not isinstance(camera, _mesh.ViewCamera):
            raise ValueError("camera must come from mesh.view_camera()")
        H, W = (int(v) for v in (camera.size if size is None else size))
        if not (1 <= H <= _lib.VIEW_MAX and 1 <= W <= _lib.VIEW_MAX):
            raise ValueError(f"size = ({H}, {W}): each side 1..{_lib.VIEW_MAX}")
        samples = _lib.view_samples_check(samples, H, W)
        aa = samples > 1 or bool(want_coverage)
        if not (isinstance(texture, torch.Tensor) and texture.dtype == torch.uint8 and texture.dim() == 3 and texture.shape[2] == 4
                and texture.device == self._device and texture.is_contiguous()):
            raise ValueError(f"texture must be a contiguous uint8 [TH, TW, 4] tensor on {self._device}")
        if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 4) and out.device == self._device
                  and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 [{H}, {W}, 4] tensor on {self._device}")
        opts = _mesh.view_opts(cull, flip_normals, shade, ambient, unpainted, background)
        cam = camera.struct()
        cur = torch.cuda.current_stream(self._device)
        given = out
        build = trilinear and mips is None
        if trilinear:
            need = self._mip_bytes(texture)
            if mips is not None and not (isinstance(mips, torch.Tensor) and mips.dtype == torch.uint8 and mips.dim() == 1 and mips.numel() >= need
                                         and mips.device == self._device and mips.is_contiguous()):
                raise ValueError(f"mips must be a contiguous uint8 tensor of at least {need} bytes on {self._device} (build_mips)")
        with torch.cuda.stream(self.view_stream):  # the outputs belong to the view's stream: a live view waits for no other
            if out is None:
                out = torch.empty(H, W, 4, dtype=torch.uint8, device=self._device)
            face_idx = torch.empty(H, W, dtype=torch.int32, device=self._device) if want_face_idx or selection is not None else None
            depth = torch.empty(H, W, dtype=torch.float32, device=self._device) if want_depth else None
            lod = torch.empty(H, W, dtype=torch.float32, device=self._device) if want_lod else None
            coverage = torch.empty(H, W, dtype=torch.uint8, device=self._device) if want_coverage else None
            taps = torch.empty(H, W, dtype=torch.uint8, device=self._device) if want_taps else None
            if build:
                key = (texture.shape[0], texture.shape[1])
                if key not in self._view_mips:
                    self._view_mips[key] = torch.empty(need, dtype=torch.uint8, device=self._device)
                mips = self._view_mips[key]
        if not live:
            done = torch.cuda.Event()
            done.record(self.stream)
            self.view_stream.wait_event(done)
            self.view_stream.wait_stream(cur)
        vs = C.c_void_p(self.view_stream.cuda_stream)
        if trilinear and build:
            check(self._lib.dtp_texture_mips(ptr(texture), texture.shape[0], texture.shape[1], ptr(mips), need, vs), "dtp_texture_mips")
        if anisotropy > 1:
            check(self._lib.dtp_mesh_view_aniso(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], ptr(mips), C.byref(cam), H, W,
                                                C.byref(opts), int(bool(clip_near)), samples, anisotropy, ptr(out), ptr(face_idx), ptr(depth),
                                                ptr(lod), ptr(taps), ptr(coverage), vs), "dtp_mesh_view_aniso")
        elif aa:
            check(self._lib.dtp_mesh_view_aa(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], ptr(mips) if trilinear else None,
                                             C.byref(cam), H, W, C.byref(opts), int(trilinear), int(bool(clip_near)), samples, ptr(out),
                                             ptr(face_idx), ptr(depth), ptr(lod), ptr(coverage), vs), "dtp_mesh_view_aa")
        elif clip_near:
            check(self._lib.dtp_mesh_view_clip(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], ptr(mips) if trilinear else None,
                                               C.byref(cam), H, W, C.byref(opts), int(trilinear), ptr(out), ptr(face_idx), ptr(depth), ptr(lod), vs),
                  "dtp_mesh_view_clip")
        elif trilinear:
            check(self._lib.dtp_mesh_view_mips(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], ptr(mips), C.byref(cam), H, W,
                                               C.byref(opts), ptr(out), ptr(face_idx), ptr(depth), ptr(lod), vs), "dtp_mesh_view_mips")
        else:
            check(self._lib.dtp_mesh_view(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], C.byref(cam), H, W, C.byref(opts), ptr(out),
                                          ptr(face_idx), ptr(depth), vs), "dtp_mesh_view")
        if selection is not None:
            check(self._lib.dtp_view_tint(self._h, ptr(out), ptr(face_idx), H, W, ptr(selection), selection.shape[0], mesh.num_faces,
                                          C.byref(color), opacity, vs), "dtp_view_tint")
        cur.wait_stream(self.view_stream)
        for t in (texture, given, None if build else mips, selection):
            if t is not None:
                t.record_stream(self.view_stream)
        for t in (None if given is not None else out, face_idx, depth, lod, taps, coverage):
            if t is not None:
                t.record_stream(cur)
        extra = tuple(t for t in (face_idx if want_face_idx else None, depth, lod, taps, coverage) if t is not None)
        return (out,) + extra if extra else out

    def select_faces(self, mesh, face_idx, polygon, op="replace", out=None, extend=None, rings=1):
        """Lasso selection (dtp_mesh_select): the faces of `mesh` that a frame shows inside a polygon, as a face set --
        int32 [(F + 31) // 32] on the model's device, bit f % 32 of word f // 32 = face f (mesh.faceset_to_bool unpacks it; |, & and ~
        are union, intersection and complement).  face_idx: int32 [H, W] on the device, as render_view(want_face_idx=True) returns it
        (-1: no face; with samples > 1 the centre sample's face).  polygon: float [n, 2] as (x, y) in the frame's pixel coordinates,
        mesh.view_rays' convention (the centre of pixel (i, j) is (j + 0.5, i + 0.5)), 3 <= n <= 1024 and finite, else DtpError; a
        rectangle is four vertices.  A pixel is inside when its centre is, by the even-odd rule in exact integers on vertices snapped
        to 1 / 256 pixel, so a self-intersecting lasso follows even-odd; a face is selected when it is face_idx at one or more inside
        pixels: what the user sees, not hidden, back-facing or sub-pixel faces.  op: "replace" (out is zeroed first), "add" or
        "subtract" (out is the set to edit).  out: default a fresh zeroed set.  The call only enqueues, on self.view_stream, behind
        the frame it reads and behind the caller's current stream, which then waits for the set (on the device).  One select of a
        mesh at a time.  extend: None, or a `how` of extend_selection ("rings", "shrink", "linked", "charts") with its `rings`: the
        set the call leaves in `out` -- after the op, so with "add" the edited set -- is grown in place on the same stream
        (DESIGN.md 3.33)."""
        if not isinstance(mesh, _mesh.Mesh):
            raise ValueError("mesh must come from load_mesh()")
        if op not in _lib.SELECT_OPS:
            raise ValueError(f"op {op!r}: choose one of {', '.join(_lib.SELECT_OPS)}")
        if extend is not None:
            extend, rings = _extend_args(extend, rings)
        if not (isinstance(face_idx, torch.Tensor) and face_idx.dtype == torch.int32 and face_idx.dim() == 2 and face_idx.device == self._device
                and face_idx.is_contiguous()):
            raise ValueError(f"face_idx must be a contiguous int32 [H, W] tensor on {self._device}")
        poly, n = _mesh.lasso_polygon(polygon)
        if out is not None:
            _mesh.faceset_check(out, mesh.num_faces, self._device, what="out")
        cur = torch.cuda.current_stream(self._device)
        given = out
        with torch.cuda.stream(self.view_stream):
            if out is None:
                out = _mesh.faceset_empty(mesh.num_faces, self._device)
        self.view_stream.wait_stream(cur)
        src = poly if n else torch.zeros(1, 2, dtype=torch.float32)  # (an empty tensor has no address; n = 0 is the library's to refuse)
        check(self._lib.dtp_mesh_select(mesh.handle, ptr(face_idx), face_idx.shape[0], face_idx.shape[1], ptr(src), n,
                                        _lib.SELECT_OPS[op], ptr(out), out.shape[0], C.c_void_p(self.view_stream.cuda_stream)), "dtp_mesh_select")
        try:
            if extend is not None:
                check(self._lib.dtp_mesh_select_extend(mesh.handle, ptr(out), ptr(out), out.shape[0], _lib.EXTEND_HOWS[extend], rings,
                                                       C.c_void_p(self.view_stream.cuda_stream)), "dtp_mesh_select_extend")
        finally:
            cur.wait_stream(self.view_stream)  # (also when the growth is refused: the lasso is enqueued by then)
        for t in (face_idx, given):
            if t is not None:
                t.record_stream(self.view_stream)
        if given is None:
            out.record_stream(cur)
        return out

    def extend_selection(self, mesh, sel, how="rings", rings=1, out=None):
        """Grow a face set on the device (dtp_mesh_select_extend; Blender's select more / less, linked, UV island).  how:
        "rings": `rings` times, add every face that shares a point with a face of the set; "shrink": `rings` times, drop every face of the
        set that shares a point with a face outside it (an open border is no outside face: the full set stays full); "linked": every face
        of every part the set touches (the fixed point of "rings"); "charts": every face of every UV chart it touches.  A point is a
        position: vertices with the same coordinates are one, so a mesh whose vertices are split along UV seams is still linked across
        them (Mesh.topology() has the labels).  rings: 1..64, ignored by "linked" and "charts".  sel: a face set of `mesh` on the model's
        device; its bits at positions >= F are ignored and those of the result are 0.  out: default a fresh set; out=sel works in place.
        The call only enqueues, on self.view_stream with the waits select_faces makes, so lasso -> extend -> paint_mesh_stroke(face_mask=)
        needs no synchronise; only the mesh's first use waits for that stream (it builds the topology).  One extend of a mesh at a
        time."""
        if not isinstance(mesh, _mesh.Mesh):
            raise ValueError("mesh must come from load_mesh()")
        how, rings = _extend_args(how, rings)
        _mesh.faceset_check(sel, mesh.num_faces, self._device, what="sel")
        if out is not None:
            _mesh.faceset_check(out, mesh.num_faces, self._device, what="out")
        cur = torch.cuda.current_stream(self._device)
        given = out
        with torch.cuda.stream(self.view_stream):
            if out is None:
                out = torch.empty_like(sel)
        self.view_stream.wait_stream(cur)
        check(self._lib.dtp_mesh_select_extend(mesh.handle, ptr(sel), ptr(out), sel.shape[0], _lib.EXTEND_HOWS[how], rings,
                                               C.c_void_p(self.view_stream.cuda_stream)), "dtp_mesh_select_extend")
        cur.wait_stream(self.view_stream)
        for t in (sel, given):
            if t is not None:
                t.record_stream(self.view_stream)
        if given is None:
            out.record_stream(cur)
        return out

    def tint_selection(self, frame, face_idx, sel, color=(255, 160, 0), opacity=128, num_faces=None):
        """Show a face set on a finished frame, in place (dtp_view_tint): frame uint8 [H, W, 4] and face_idx int32
        [H, W] of one render_view call, on the model's device.  Where face_idx is a face of `sel`, each of R, G, B becomes
        (c * (255 - opacity) + color * opacity + 127) // 255; alpha and every other pixel are untouched.  num_faces: the mesh's F, so
        that stray bits of ~sel beyond it are ignored even against a hand-made face_idx (default: 32 per word, which a frame of the
        mesh never reaches).  The call only enqueues, on self.view_stream, as select_faces does.  -> frame."""
        color, opacity = _tint_args(color, opacity)
        if not (isinstance(frame, torch.Tensor) and frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 4
                and frame.device == self._device and frame.is_contiguous()):
            raise ValueError(f"frame must be a contiguous uint8 [H, W, 4] tensor on {self._device} (it is tinted in place)")
        H, W = frame.shape[0], frame.shape[1]
        if not (isinstance(face_idx, torch.Tensor) and face_idx.dtype == torch.int32 and tuple(face_idx.shape) == (H, W)
                and face_idx.device == self._device and face_idx.is_contiguous()):
            raise ValueError(f"face_idx must be a contiguous int32 [{H}, {W}] tensor on {self._device}")
        if num_faces is None and isinstance(sel, torch.Tensor) and sel.dim() == 1:
            num_faces = 32 * sel.shape[0]
        _mesh.faceset_check(sel, num_faces or 0, self._device, what="sel")
        cur = torch.cuda.current_stream(self._device)
        self.view_stream.wait_stream(cur)
        check(self._lib.dtp_view_tint(self._h, ptr(frame), ptr(face_idx), H, W, ptr(sel), sel.shape[0], int(num_faces), C.byref(color), opacity,
                                      C.c_void_p(self.view_stream.cuda_stream)), "dtp_view_tint")
        cur.wait_stream(self.view_stream)
        for t in (frame, face_idx, sel):
            t.record_stream(self.view_stream)
        return frame

    def _mip_bytes(self, texture):
        lay = _lib.MipLevels()
        check(self._lib.dtp_mip_layout(texture.shape[0], texture.shape[1], C.byref(lay)), "dtp_mip_layout")
        return int(lay.bytes)

    def build_mips(self, texture, out=None):
        """The mip pyramid of a painted texture (dtp_texture_mips): texture uint8 [TH, TW, 4] on the model's device ->
        uint8 [bytes], levels 1 .. levels - 1 one after the other as ops.mip_layout(TH, TW) says (level 0 is the texture itself; a
        1 x 1 texture has 0 bytes).  Alpha-weighted in exact integers: an unpainted texel (0, 0, 0, 0) adds no colour, so chart borders
        do not darken.  out: a buffer of at least that many bytes to write into.  For render_view(filter="trilinear", mips=...) and for
        an exporter that hands the levels to a renderer's sampler.  The call only enqueues, on the current stream."""
        if not (isinstance(texture, torch.Tensor) and texture.dtype == torch.uint8 and texture.dim() == 3 and texture.shape[2] == 4
                and texture.device == self._device and texture.is_contiguous()):
            raise ValueError(f"texture must be a contiguous uint8 [TH, TW, 4] tensor on {self._device}")
        need = self._mip_bytes(texture)
        if out is None:
            out = torch.empty(need, dtype=torch.uint8, device=self._device)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.dim() == 1 and out.numel() >= need and out.device == self._device
                  and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 tensor of at least {need} bytes on {self._device}")
        check(self._lib.dtp_texture_mips(ptr(texture), texture.shape[0], texture.shape[1], ptr(out), out.numel(),
                                         C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)), "dtp_texture_mips")
        return out

    def bleed_texture(self, mesh, texture, bleed, rect=None):
        """The bleed pass of paint_mesh_stroke on its own (dtp_mesh_bleed), for a texture that was loaded from a file or painted without
        it, or before an export: every texel of `texture` (uint8 [H,W,4] on the model's device, contiguous; changed in place and
        returned) that no face of `mesh` covers takes the four bytes of the nearest covered texel within `bleed` texels (1..16; ties go
        to the smaller row offset, then the smaller column offset; no wrap-around).  rect: (x0, y0, x1, y1) inclusive texel bounds of
        the pass, clipped to the texture; None = the whole texture.  Covered texels are only read.  The call only enqueues."""
        if not isinstance(mesh, _mesh.Mesh):
            raise ValueError("mesh must come from load_mesh()")
        if not (isinstance(texture, torch.Tensor) and texture.dtype == torch.uint8 and texture.dim() == 3 and texture.shape[2] == 4
                and texture.device == self._device and texture.is_contiguous()):
            raise ValueError(f"texture must be a contiguous uint8 [H, W, 4] tensor on {self._device} (it is changed in place)")
        r = None
        if rect is not None:
            if len(rect) != 4:
                raise ValueError(f"rect must be (x0, y0, x1, y1), got {rect!r}")
            r = C.byref((C.c_int * 4)(*[int(v) for v in rect]))
        self.stream.wait_stream(torch.cuda.current_stream(self._device))
        check(self._lib.dtp_mesh_bleed(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], int(bleed), r, self._s()),
              "dtp_mesh_bleed")
        torch.cuda.current_stream(self._device).wait_stream(self.stream)
        texture.record_stream(self.stream)
        return texture

    def journal(self, texture, capacity_tiles=None, depth=10):
        """An undo / redo journal of `texture` (uint8 [H,W,4] on the model's device, contiguous; dtp_journal_create):
        -> journal.Journal.  Between its begin() and end() -- or inside `with j.stroke():` -- paint_stroke, paint_mesh_stroke and
        paint_mesh_path on this texture first save the 16 x 16-texel tiles they are about to write, on the device and in stream order;
        undo() and redo() swap them back byte for byte.  What the Kit app does with a host copy of the whole texture per stroke
        (ui/brush.py:52-77,131-137), without the copy, and with redo.  depth: the most strokes kept (the Kit app's 10).
        capacity_tiles: the slots of the ring, 1 KiB each; a stroke that saves more tiles than that, or whose slots later strokes have
        overwritten, can no longer be undone (undo() raises, painting is never held up).  Default: 4 x the texture's tile count, i.e.
        room for four whole-texture copies.  Memory, all allocated here: capacity_tiles KiB of slots + 4 bytes per slot + 4 bytes per
        tile; for a 2048^2 texture at the default 64 MiB + 256 KiB + 64 KiB (the texture itself is 16 MiB; the Kit app's ten host
        copies are 160 MiB before encoding).  One record open per model at a time."""
        if capacity_tiles is None:
            capacity_tiles = 4 * _journal.tile_count(texture.shape[0], texture.shape[1])
        return _journal.Journal(self, texture, capacity_tiles, depth)

    def delta_tracker(self, shape_or_image, capacity_tiles=None):
        """A changed-tile tracker (dtp_delta_create) for images of one shape -- (H, W), or an image uint8 [H,W,4] to take
        the shape from: -> delta.DeltaTracker.  Its pull(image) finds, on the device, the 16 x 16-texel tiles of a painted texture or of a
        render_view frame whose bytes differ from what the tracker emitted last, and reads back those alone; frame(image) packs them for a
        client that keeps a mirror with delta.apply_frame.  What the Kit app does by pushing the whole texture to the viewport after
        every stamp (manager.py:349-354), for a client in another process.  capacity_tiles: the most tiles one pull emits (the rest follow
        with the next pulls); default the image's tile count, which never caps.  Memory, all allocated here: a shadow image of H W 4
        bytes, capacity_tiles KiB of payload on the device and the same pinned on the host, 2 bytes per tile; for a 2048^2 texture at
        the default 16 + 16 + 16 MiB."""
        from . import delta as _delta
        if isinstance(shape_or_image, torch.Tensor):
            if shape_or_image.dim() != 3 or shape_or_image.shape[2] != 4:
                raise ValueError("an image to take the shape from must be [H, W, 4]")
            H, W = int(shape_or_image.shape[0]), int(shape_or_image.shape[1])
        else:
            H, W = (int(v) for v in shape_or_image)
        if capacity_tiles is None:
            capacity_tiles = _journal.tile_count(H, W)
        return _delta.DeltaTracker(self, H, W, capacity_tiles)

    def stroke_info(self):
        """Of the last paint_stroke: its stamps, its groups and the UNet evaluations of all groups (dtp_last_stroke_info)."""
        a, b, e = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.dtp_last_stroke_info(self._h, C.byref(a), C.byref(b), C.byref(e)), "dtp_last_stroke_info")
        return dict(stamps=a.value, groups=b.value, unet_evals=e.value)

    def stage_times_ms(self):
        """[vae_encoder x2 + pre, denoise loop, vae + post] GPU ms of the last stamp (print_summary, sdp:486-503)."""
        arr = (C.c_float * 3)()
        check(self._lib.dtp_last_stamp_times(self._h, C.byref(arr)), "dtp_last_stamp_times")
        return list(arr)

    def stamp_info(self):
        a, b = C.c_int(), C.c_int()
        check(self._lib.dtp_last_stamp_info(self._h, C.byref(a), C.byref(b)), "dtp_last_stamp_info")
        return dict(unet_evals=a.value, graph_nodes=b.value)

    def stamp_unet_rows(self):
        """UNet rows the last stamp evaluated, summed over its evaluations (2B per evaluation + one per stamp still texture-guided)."""
        n = C.c_int()
        check(self._lib.dtp_last_stamp_unet_rows(self._h, C.byref(n)), "dtp_last_stamp_unet_rows")
        return n.value

    def profile(self, enable):
        """Bracket every kernel launch with HIP events (graph replay off) / switch back."""
        check(self._lib.dtp_profile(self._h, int(enable)), "dtp_profile")

    def profile_rows(self):
        rows = (_lib.ProfRow * 64)()
        n = C.c_int()
        check(self._lib.dtp_profile_rows(self._h, rows, 64, C.byref(n)), "dtp_profile_rows")
        return [dict(kernel=_lib.PROF_KINDS[r.kind], launches=r.launches, ms=r.ms, flops=r.flops, bytes=r.bytes)
                for r in rows[: n.value]]

    def profile_dump(self, path):
        check(self._lib.dtp_profile_dump(self._h, str(path).encode()), "dtp_profile_dump")

    def set_scheduler(self, name):
        """Switch the sampler ("DDIM" | "DPM" | "LMSD") from the next stamp on; that stamp rebuilds the schedule tables once (a host
        wait, like a change of steps).  DDIM runs steps - 1 UNet evaluations per stamp, DPM and LMSD run steps."""
        sid = _lib.scheduler_id(name)
        check(self._lib.dtp_set_option(self._h, b"scheduler", sid), "dtp_set_option(scheduler)")
        self.scheduler = name

    def set_option(self, name, value):
        check(self._lib.dtp_set_option(self._h, name.encode(), int(value)), "dtp_set_option")
        if name == "check_finite":
            self._check_finite = bool(value)

    def last_stamp_finite(self):
        """Verdict of the post-loop finiteness check of the last stamp (option "check_finite"); blocks on that stamp."""
        ok = C.c_int()
        check(self._lib.dtp_last_stamp_finite(self._h, C.byref(ok)), "dtp_last_stamp_finite")
        return bool(ok.value)

    # ------------------------------------------------------------------ engine-level access (inner boundary)
    def unet(self, sample, timestep, encoder_hidden_states):
        """Engine contract of models.py:1097-1129: sample f32 [N,9,h,w], timestep scalar, ehs f16 [N,14,768]."""
        sample = sample.to(self._device, torch.float32).contiguous()
        ehs = encoder_hidden_states.to(self._device, torch.float16).contiguous()
        n = sample.shape[0]
        out = torch.empty(n, 4, sample.shape[2], sample.shape[3], dtype=torch.float32, device=self._device)
        torch.cuda.current_stream(self._device).synchronize()
        check(self._lib.dtp_unet(self._h, ptr(sample), float(timestep), ptr(ehs), ptr(out), n, self._s()), "dtp_unet")
        self.stream.synchronize()
        return out

    def vae_encode(self, images, eps=None):
        images = images.to(self._device, torch.float32).contiguous()
        b, h = images.shape[0], self._resolution // 8
        out = torch.empty(b, 4, h, h, dtype=torch.float32, device=self._device)
        eps = eps.to(self._device, torch.float32).contiguous() if eps is not None else None
        torch.cuda.current_stream(self._device).synchronize()
        check(self._lib.dtp_vae_encode(self._h, ptr(images), ptr(eps), ptr(out), b, self._s()), "dtp_vae_encode")
        self.stream.synchronize()
        return out

    def vae_decode(self, latents):
        latents = latents.to(self._device, torch.float32).contiguous()
        b = latents.shape[0]
        out = torch.empty(b, 3, self._resolution, self._resolution, dtype=torch.float32, device=self._device)
        torch.cuda.current_stream(self._device).synchronize()
        check(self._lib.dtp_vae_decode(self._h, ptr(latents), ptr(out), b, self._s()), "dtp_vae_decode")
        self.stream.synchronize()
        return out
