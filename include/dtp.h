/* libdtp -- C ABI of the MI355X-native stamp-inpainting engine.
 *
 * Drop-in boundary for the hot path of nv-tlabs/DiffusionTexturePainting's trt_inference/
 * server.  Plain C: opaque handle, raw device pointers, sizes and int
 * error codes; no exceptions and no torch/TensorRT types cross this line.  One handle = one
 * GPU + one stream at a time; a handle is NOT thread-safe (the reference is single-threaded:
 * one tornado IOLoop, one stamp in flight -- trt_inference/handler.py:78-110).
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * trt_inference/).  Tensors are dense, row-major, in the reference's own layouts (NCHW fp32
 * images / latents, [N,14,768] conditioning); the NHWC fp16 working layout is internal.
 * Every function returns DTP_OK (0) or an error code; dtp_last_error() gives the message.
 */
#ifndef DTP_H
#define DTP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 3: the seeded entry points below (dtp_stamp_seeded, dtp_op_stamp_noise, dtp_philox4x32), the LoRA refit (dtp_refit_stage,
 * dtp_refit_lora, dtp_last_refit_info, dtp_op_lora_refit) and the strokes (dtp_stroke, dtp_stroke_plan, dtp_last_stroke_info,
 * dtp_op_stroke_gather, dtp_op_stroke_paste) and the mesh strokes (dtp_mesh_create, dtp_mesh_destroy, dtp_mesh_camera, dtp_mesh_stroke,
 * dtp_op_mesh_render, dtp_op_mesh_backproject) and their bleed pass (dtp_mesh_stroke_bleed, dtp_mesh_bleed, dtp_mesh_bleed_offsets,
 * dtp_op_mesh_coverage) and picking (dtp_mesh_pick, dtp_mesh_ray_frame, dtp_mesh_path_plan, dtp_op_mesh_pick) and the undo / redo journal
 * (dtp_journal_*, dtp_op_journal_tiles) and the view of a mesh (dtp_view_camera, dtp_view_rays, dtp_mesh_view, dtp_op_mesh_view) and the
 * mip pyramid with its filtered view (dtp_mip_layout, dtp_texture_mips, dtp_mesh_view_mips) and the changed tiles of an image (dtp_delta_*, dtp_op_delta_state)
 * and the view clipped at the near plane (dtp_mesh_view_clip, dtp_op_mesh_view_clip) and the anti-aliased view (dtp_mesh_view_aa,
 * dtp_op_mesh_view_aa) and the anisotropic view (dtp_mesh_view_aniso, dtp_op_mesh_view_aniso) and the occlusion test of the
 * backprojection (dtp_mesh_stroke_occluded, dtp_op_mesh_backproject_occluded) and the growth of a face set (dtp_topology_build,
 * dtp_mesh_topology, dtp_mesh_topology_labels, dtp_mesh_select_extend) are additions; nothing that existed at
 * version 3 changed its signature or behaviour, so a caller built against the earlier header keeps working. */
#define DTP_ABI_VERSION 3

/* error codes (every entry point returns one; dtp_last_error() has the text) */
enum { DTP_OK = 0, DTP_ERR_ARG = 1, DTP_ERR_HIP = 2, DTP_ERR_STATE = 3, DTP_ERR_MISSING = 4 };

typedef struct dtp_ctx dtp_ctx;
typedef void* dtp_stream; /* hipStream_t; NULL = the null stream */

int dtp_abi_version(void);
const char* dtp_last_error(void);

/* ---------------------------------------------------------------- lifecycle
 * replaces: TRTConditionalInpainter.__init__ (trt_model.py:28-71) -> InpaintPipeline(...)
 * + loadEngines + loadResources (stable_diffusion_pipeline.py:138-162,189-334).
 * `resolution` is fixed per handle like the reference's (run.py:30): any multiple of 8 from 64 up (the reference's check_dims rule);
 * at a multiple of 8 that is not one of 64 the UNet levels are ceil halvings of R / 8 and the parity-only fp8 options
 * are refused (DTP_ERR_STATE).  max_batch = stamps per call. */
int dtp_create(int device, int resolution, int max_batch, dtp_ctx** out);
void dtp_destroy(dtp_ctx* ctx);

/* ---------------------------------------------------------------- weights
 * replaces: UNet2DConditionModel / AutoencoderKL.from_pretrained + load_attn_procs
 * (models.py:1038-1042,1241,1332), torch.load(image_encoder.pth) (trt_model.py:57-59).
 * `name` is "<net>.<diffusers key>" with net in {unet, lora, vae, clip, penc}; data is fp32,
 * host or device memory.  dtp_finalize_weights merges LoRA (W += up @ down, models.py:1083),
 * packs everything to the fp16 kernel layouts and builds the launch programs. */
int dtp_load_tensor(dtp_ctx* ctx, const char* name, const float* data, int is_device, const int64_t* shape, int ndim);
int dtp_finalize_weights(dtp_ctx* ctx);

/* ---------------------------------------------------------------- LoRA refit of a finalized handle
 * replaces: Engine.refit (utilities.py:88-189, enable_refit / onnx_refit_dir of stable_diffusion_pipeline.py:203-206,312-327) for the
 * one set of weights a server swaps at run time, and the lora_scale of the reference's merge, W + lora_scale * up @ down
 * (models.py:1034,1083).  dtp_load_tensor keeps answering DTP_ERR_STATE after finalize; these two calls are the way in afterwards.
 *
 * dtp_refit_stage: stage one tensor of the LoRA to refit with; name = "lora.<module>.processor.<proj>_lora.{down,up}.weight" as for
 *   dtp_load_tensor; fp32, host or device; only on a finalized handle.  Staging changes nothing a stamp can see.
 * dtp_refit_lora: replace the handle's LoRA by the staged set at `scale`: every target matrix (q / k / v / out of attn1 and attn2 in the
 *   16 transformer blocks, 128 matrices) becomes base + scale * up @ down; a target without staged tensors becomes its base; an empty
 *   staged set = no LoRA.  Clears the staging area, whether the call succeeds or fails.
 *
 * Result.  After dtp_refit_lora the handle computes bit for bit what a handle created from (the same base weights, that LoRA with `up`
 *   pre-multiplied by `scale`) computes, given the same tile choices on both -- through every entry point: stamps of every kind, dtp_unet,
 *   the fp16 paths at every level.  (Exact when scale * up is: a power of two always is.  Both paths run the same device functions.)
 * What survives.  Launch programs, tune entries, captured graphs, conditioning slots, schedule tables and options.  The packed buffers are
 *   overwritten in place, so the pointers inside captured graphs stay valid; the call runs no tuner, builds no program and captures
 *   nothing.  The per-stamp cross-attention matrices (cached per batch layout, slots and slot versions) are invalidated: the next stamp
 *   rebuilds them without the caller touching its slots.
 * Blocking.  The call waits for the work already enqueued on the handle (on any stream), enqueues the refit and waits for it: it is
 *   host-blocking, like a change of `steps`.
 * Validation.  Everything is checked before anything is written; a failed call leaves the handle exactly as it was and keeps nothing
 *   staged.  DTP_ERR_MISSING, naming the tensor, for an `up` without its `down` or a `down` without its `up`; DTP_ERR_ARG, naming the
 *   tensor, for a name that is no LoRA tensor's, a target that does not exist or a shape that does not fit its target (down [rank, K],
 *   up [N, rank] for a target [N, K]); DTP_ERR_ARG for a non-finite scale.  The rank may differ from the original LoRA's and from matrix
 *   to matrix.
 * State.  DTP_ERR_STATE before dtp_finalize_weights; under any fp8 option (parity-only, calibrated per program: the precedent of
 *   dtp_stamp_strength); and while the opt-in DTP_GEMMWS fragment-order packing of the Linears is active (that copy is not rebuilt). */
int dtp_refit_stage(dtp_ctx* ctx, const char* name, const float* data, int is_device, const int64_t* shape, int ndim);
int dtp_refit_lora(dtp_ctx* ctx, float scale);
/* of the last successful refit: matrices rewritten, kernel launches it enqueued, device milliseconds (the refit has finished when
 * dtp_refit_lora returns).  DTP_ERR_STATE when no refit has run on the handle.  Any pointer may be NULL. */
int dtp_last_refit_info(dtp_ctx* ctx, int* matrices, int* launches, float* ms);

/* ---------------------------------------------------------------- engines (inner boundary)
 * replaces: Engine.infer(feed_dict, stream) for the three TensorRT engines (utilities.py:252-264,
 * runEngine stable_diffusion_pipeline.py:336-338) with the I/O contracts of models.py:1343-1377
 * (vae_encoder), :1097-1139 (unet), :1253-1284 (vae).  Pointers are device memory.
 *   vae_encoder: images f32 [B,3,R,R] -> latent f32 [B,4,h,w] = mean + exp(.5 logvar) * eps
 *                (eps f32 [B,4,h,w]; NULL = distribution mean).  Unscaled, like the engine.
 *   unet:        sample f32 [N,9,h,w], timestep f32 scalar, encoder_hidden_states f16 [N,14,768]
 *                -> f32 [N,4,h,w]
 *   vae:         latent f32 [B,4,h,w] -> images f32 [B,3,R,R] */
int dtp_vae_encode(dtp_ctx* ctx, const float* images, const float* eps, float* latent, int B, dtp_stream s);
int dtp_unet(dtp_ctx* ctx, const float* sample, float timestep, const void* ctx_f16, float* out, int N, dtp_stream s);
int dtp_vae_decode(dtp_ctx* ctx, const float* latent, float* images, int B, dtp_stream s);

/* ---------------------------------------------------------------- operator (primary boundary)
 * dtp_set_brush replaces TRTConditionalInpainter.set_brush (trt_model.py:79-88):
 *   crop_resize_square (handler.py:36-45) + ConditionPatchEncoder.encode_image
 *   (image_encoder.py:106-115).  image f32 [3,H,W] 0..1 (device); writes the resized brush
 *   f32 [1,3,R,R] to image_out (the `.image` attribute handler.py:97 reads).
 * dtp_set_conditioning installs precomputed conditioning instead (cond/uncond f32 [14,768],
 *   brush f32 [3,R,R]; device pointers). */
int dtp_set_brush(dtp_ctx* ctx, const float* image, int H, int W, float* image_out, dtp_stream s);
int dtp_set_conditioning(dtp_ctx* ctx, const float* cond, const float* uncond, const float* brush, dtp_stream s);
int dtp_get_conditioning(dtp_ctx* ctx, float* cond, float* uncond, dtp_stream s);

/* Conditioning slots (the multi-client server row): stamps of DIFFERENT clients -- each with its own brush --
 * can share one batched dtp_stamp_slots call.  Slot 0 is the brush the single-client entry points above use; the slot
 * variants take slot in [0, DTP_MAX_SLOTS). */
#define DTP_MAX_SLOTS 16
int dtp_set_brush_slot(dtp_ctx* ctx, int slot, const float* image, int H, int W, float* image_out, dtp_stream s);
int dtp_set_conditioning_slot(dtp_ctx* ctx, int slot, const float* cond, const float* uncond, const float* brush, dtp_stream s);
int dtp_get_conditioning_slot(dtp_ctx* ctx, int slot, float* cond, float* uncond, dtp_stream s);

typedef struct {
  int steps;        /* settings['steps']        (server_io.py:104) */
  int context_pad;  /* settings['context_pad']  */
  int tg_steps;     /* settings['tg_steps']     */
  float cfg_weight; /* settings['cfg_weight']   */
  float tg_weight;  /* settings['tg_weight']    */
  int composite;    /* 0 = generate_raw (trt_model.py:90-121); 1 = generate (model_base.py:51-58) */
  int output_u8;    /* 1: out is u8 HWC [B,R,R,3] = (img*255) truncated (handler.py:55-56) */
} dtp_settings;

/* replaces TRTConditionalInpainter.generate_raw / ConditionalInpainterBase.generate.
 *   canvas  f32 [B,4,R,R] 0..1, alpha 1 = known
 *   latents f32 [B,4,h,w]   initial N(0,1) draw (initialize_latents, sdp:340-346); required
 *   vae_eps f32 [2,B,4,h,w] normal draws of the two VAE encodes (models.py:1335); NULL = mean
 *   out     f32 [B,3,R,R] 0..1 (or u8, see output_u8)
 * Asynchronous on `s`: the call only enqueues (copies of the inputs, graph replays, kernels with the settings as kernel
 * arguments) and returns; back-to-back stamps overlap host enqueue with device work.  The caller keeps canvas / latents /
 * vae_eps / out alive until the stream has consumed them.  The one exception is a CHANGE of `steps` between two calls, or of the
 * "scheduler" option since the last stamp, which rebuilds the schedule tables (update_infer_settings, inpaint_pipeline.py:39-50)
 * and waits for the stream once.  The sampler is the handle's "scheduler" option (dtp_set_option; DDIM by default): it runs E
 * UNet evaluations, E = steps - 1 under DDIM and steps under DPM / LMSD (dtp_scheduler_tables). */
int dtp_stamp(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
              void* out, int B, dtp_stream s);
/* The same with one conditioning slot per stamp: slots = host int[B] (NULL = all slot 0).  Stamp b is conditioned on the brush
 * of slot slots[b] (its conditioning tokens and its hint image, trt_model.py:103-114); everything else is shared. */
int dtp_stamp_slots(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                    void* out, int B, const int* slots, dtp_stream s);
/* The same with one dtp_settings per stamp: st = host dtp_settings[B].  Stamp b gets exactly what dtp_stamp computes for it alone
 * with st[b]: its own context_pad (dilation window), cfg_weight, tg_weight and tg_steps.  steps, composite and output_u8 are per call:
 * DTP_ERR_ARG, naming the stamp, when they differ.  Every entry gets dtp_stamp's checks (steps 2..999, context_pad >= 1).
 * Stamp b evaluates the texture-guided branch for its first tg_evals_b = (tg_weight_b == 0 ? 0 : clamp(tg_steps_b, 0, E))
 * evaluations (E: see dtp_stamp); the UNet batch of evaluation i is 2B + #{b : tg_evals_b > i}, so a stamp whose guidance has ended costs two rows, not
 * three.  Programs are built per (B, tg rows) on first use, and the denoise loop is captured once per (B, steps, scheduler, sorted
 * tg_evals profile); the context keeps the 16 most recently used loop graphs.  Any cfg / tg values replay the same graph.  Under the fp8
 * options (fp8_attention, fp8_linear, fp8_operands), which calibrate one program per batch shape, the stamps of a batch must share
 * tg_evals: DTP_ERR_STATE otherwise.  dtp_stamp and dtp_stamp_slots are this call with st[0] applied to every stamp. */
int dtp_stamp_mixed(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                    void* out, int B, const int* slots, dtp_stream s);

/* Strength (inpaint_pipeline.py:63, the "repaint strength" of a stamp): dtp_stamp_mixed plus a start point other than pure noise.
 *   init_eps  f32 [B,4,h,w] normal draw of the init image's VAE encode; NULL = its distribution mean
 *   strength  in (0, 1] for the whole call.  The loop runs the reference's initialize_timesteps (stable_diffusion_pipeline.py:348-355):
 *             evaluations t_start .. steps - 1 of the full schedule (dtp_strength_schedule), from
 *             x = add_noise(z0, latents) = a z0 + b latents, z0 = 0.18215 sample(VAE_enc(canvas[:, :3] * 2 - 1)) of the FULL canvas
 *             (not the alpha-masked image).  The masked / context latents, masks, dilation and composite are dtp_stamp_mixed's.
 *             Texture guidance runs for clamp(tg_steps, 0, E) of the E evaluations; no sampler history carries over (DPM's first
 *             evaluation is first order).
 * strength == 1 is dtp_stamp_mixed exactly (init_eps ignored).  DTP_ERR_ARG for a strength outside (0, 1], NaN, or one that leaves no
 * evaluation; DTP_ERR_STATE under any fp8 option.  A change of strength between calls rebuilds no table and never waits for the
 * stream: the denoise loop is captured per start row, the pre-processing stage once with and once without the init image.  The first
 * strength < 1 call of a batch size builds its 3B-row VAE-encoder program and re-captures that batch size's stages once. */
int dtp_stamp_strength(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                       const float* init_eps, double strength, void* out, int B, const int* slots, dtp_stream s);

/* Seeded stamps: dtp_stamp_strength with its three noise pointers replaced by draws the library makes on the device, each a pure
 * function of (the stamp's seed, which draw, element) -- not of the batch index, the batch size, the slot order or the GPU it runs on,
 * so a stamp can be replayed alone, in any batch and on any replica with the same numbers.
 *   seeds       host uint64_t[B], one per stamp; read before the call returns
 *   sample_vae  1: the VAE encodes are sampled (draws 1, 2 and, below strength 1, 3); 0: their distribution means, i.e. vae_eps = NULL
 *               and init_eps = NULL, and only draw 0 is used
 *   strength    as dtp_stamp_strength; 1 is dtp_stamp_mixed
 * Generator (fixed: part of the ABI): Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (q & 0xffffffff, q >> 32,
 * draw, 0), q = e >> 2 for element e of ONE stamp's [4,h,w] tensor (NCHW), draw = 0 initial latents, 1 vae_eps of the masked image,
 * 2 vae_eps of the context image, 3 init_eps.  With u(w) = ((w >> 8) + 0.5) 2^-24, words (0,1) of a counter give elements 4q, 4q+1 =
 * r cos t, r sin t (r = sqrt(-2 ln u(w0)), t = 2 pi u(w1)) and words (2,3) give 4q+2, 4q+3; |z| <= 5.9.
 * Every check, error code and asynchrony guarantee of dtp_stamp_strength carries over: one kernel launch writes the draws into the
 * staging buffers in place of the three copies, outside the captured stages, so a change of seeds re-captures nothing and the host never
 * waits.  DTP_ERR_ARG naming "seeds" when seeds is NULL. */
int dtp_stamp_seeded(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const uint64_t* seeds, int sample_vae, double strength,
                     void* out, int B, const int* slots, dtp_stream s);
/* The n floats of draw `draw` (0..3) of a stamp seeded `seed`, through the same device function: out f32 [n] (device, 16-byte aligned),
 * n = 4 h w.  DTP_ERR_ARG unless n > 0, n % 4 == 0 and draw in 0..3. */
int dtp_op_stamp_noise(uint64_t seed, int draw, float* out, long long n, dtp_stream s);
/* Host-only: Philox4x32-10 of one (counter, key), compiled from the function the kernel runs (Random123's known answers hold). */
int dtp_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* ---------------------------------------------------------------- strokes on a device-resident texture
 * replaces: the loop the reference's Kit app runs on the host around every stamp (kit_app/.../python/manager.py:229-271, in 2D: the
 * window of a stamp is an axis-aligned R x R rectangle of the texture, not a render of a mesh): renderable_texture() = u8 / 255,
 * generate_raw, (painted.clip(max=1) * 255).to(uint8) written where the stamp mask is > 0, and its three brush modes (:37-45,70).
 *   texture     u8 [H][W][4] RGBA on the device, 4-byte aligned, H >= R and W >= R; painted in place
 *   stamps      host dtp_stroke_stamp[n], read before the call returns.  The window of a stamp is the R x R rectangle whose top-left texel
 *               is (row y, column x); x and y may be any int.  mode: DTP_STROKE_*; slot: the conditioning slot; seed: as dtp_stamp_seeded.
 *   st          ONE dtp_settings for every stamp of the stroke; composite and output_u8 must be 0
 *   o           wrap: 1 = coordinates are taken modulo H and W (painting across the border of a tileable texture keeps it tileable);
 *               0 = texels outside the texture read as 0 in all four channels (alpha 0: unknown, to be inpainted) and are never written.
 *               margin: the default paste mask is make_stamp_mask(R, margin) (manager.py:42-45), 1 on [margin, R - margin)^2, built once
 *               per handle and margin.  over_y, over_x: overpaint_canvas's margins (manager.py:37-39; the Kit app's are 10, 25).
 *               max_group: the largest number of stamps that may share one batched stamp (see dtp_stroke_plan; the handle's max_batch
 *               bounds it).  sample_vae, strength: as dtp_stamp_seeded, for every stamp.
 *   paste_mask  device u8 [R][R], applied where > 0; NULL = the default mask of o->margin
 * Per stamp: the canvas f32 [4][R][R] = window texel / 255 (a real fp32 division) goes straight into the stamp's staging buffer; in mode
 * OVERPAINT rows [over_y, R - over_y) x columns [over_x, R - over_x) of all four channels are then 0; the stamp runs as dtp_stamp_seeded
 * runs it; under the mask RGB = the u8 dtp_stamp writes with composite 0 and output_u8 1, (unsigned char)(clamp(v, 0, 1) * 255), and
 * A = 255.  Texels outside the mask are neither read nor written.  An ERASE stamp runs no stamp: the four channels under the mask become 0
 * (manager.py:270).
 * Grouping and order: the stamps are grouped by dtp_stroke_plan with min(o->max_group, max_batch); the call enqueues, group after group in
 * the caller's order, gather -> ONE stamp call of B = group size -> paste (an ERASE stamp: the paste only).  The stream keeps the groups
 * ordered, so stamp i + 1 sees what stamp i pasted; the windows of a group are disjoint, so its members neither see each other's result
 * nor race.  With max_group 1 the result is the host loop over single stamps, bit for bit; a group of k is the B = k stamp call.
 * Asynchronous like dtp_stamp: the whole stroke is enqueued and the call returns; a change of `steps` still waits once (and the first use
 * of a margin allocates its mask).  dtp_last_stamp_* and the check_finite verdict describe the last group that ran a stamp.
 * Validation: everything is checked before anything is enqueued, and a refused call does not touch the texture.  DTP_ERR_ARG, naming the
 * stamp where there is one: a NULL pointer, H < R or W < R, n < 1, an unknown mode, over_y / over_x outside [1, R/2) with an OVERPAINT
 * stamp present, margin outside [0, R/2), composite or output_u8 set, a slot outside 0..15, a window entirely outside a non-wrapping
 * texture.  What dtp_stamp_seeded refuses is refused with its code (an unset slot: DTP_ERR_STATE, naming the stamp; a bad strength;
 * strength < 1 under an fp8 option). */
enum { DTP_STROKE_INPAINT = 0, DTP_STROKE_ERASE = 1, DTP_STROKE_OVERPAINT = 2 };
typedef struct { int x, y, mode, slot; uint64_t seed; } dtp_stroke_stamp;
typedef struct { int wrap, margin, over_y, over_x, max_group, sample_vae; double strength; } dtp_stroke_opts;
int dtp_stroke(dtp_ctx* ctx, uint8_t* texture, int H, int W, const dtp_stroke_stamp* stamps, int n, const dtp_settings* st,
               const dtp_stroke_opts* o, const uint8_t* paste_mask, dtp_stream s);
/* Host-only: the groups of a stroke, and the contract its batching is held to.  Walking the stamps in order, stamp i joins the current
 * group in exactly one case: the group has fewer than max_group members, neither i nor the group is an ERASE stamp, and i's window is
 * disjoint from every window already in the group; otherwise i opens a new group.  The order is never changed.  Two windows are disjoint
 * iff they are disjoint on x or on y; on an axis, without wrap: |a_i - a_j| >= R; with wrap, on an axis of length L and with
 * d = (a_i - a_j) mod L: R <= d <= L - R.  group_of: int[n] (non-decreasing group ids from 0); n_groups may be NULL.  max_group <= 1 puts
 * every stamp in its own group.  DTP_ERR_ARG for a NULL stamps / group_of, n < 1, R < 1, H < R or W < R, an unknown mode (naming the stamp). */
int dtp_stroke_plan(int H, int W, int R, int wrap, const dtp_stroke_stamp* stamps, int n, int max_group, int* group_of, int* n_groups);
/* of the last dtp_stroke that was enqueued: its stamps, its groups, and the UNet evaluations summed over the groups that ran a stamp.
 * DTP_ERR_STATE when no stroke has run on the handle.  Any pointer may be NULL. */
int dtp_last_stroke_info(dtp_ctx* ctx, int* stamps, int* groups, int* unet_evals);

/* ---------------------------------------------------------------- strokes on a textured mesh
 * replaces: what the reference's Kit app does around every stamp when it paints on a mesh (kit_app/.../python/manager.py:199-271,
 * util/render.py:22-178): an orthographic look-at camera at the brush, a rasterisation of the mesh into the R x R stamp window with the
 * texture sampled through the interpolated UVs, generate_raw, and a rasterisation of the visible faces in UV space that carries the
 * painted stamp back into the texture.  Both rasterisations are kaolin's in the reference.  The contract below was written from kaolin
 * 0.15's documented conventions (the camera looks down -z, a larger camera z is nearer, NDC y is up, image row 0 is the top,
 * texture_mapping = bilinear grid_sample with align_corners=False, border padding, v flipped); it was not captured from a kaolin run.
 *
 * Camera (dtp_mesh_camera; host only, in double, rounded to fp32 once): eye = pos + normal, up = prev - pos, b = normalize(eye - pos),
 * r = normalize(cross(up, b)), u = cross(b, r); out = the rows (r, u, b), each followed by t = -row . eye: out[4 k .. 4 k + 2] the row,
 * out[4 k + 3] its t.  NDC x = cam.x / fov, y = cam.y / fov (OrthographicIntrinsics.from_frustum with width = height).  DTP_ERR_ARG for a
 * zero normal, an up that is zero or parallel to the normal (sine below 1e-9), a non-finite input, fov <= 0 or not finite, or a camera
 * that does not fit fp32.
 * Projection (per face, fp32, every operation rounded once, no contraction): cam_k = ((m0 x + m1 y) + m2 z) + t per row; the normal
 * cross(v1 - v0, v2 - v0) of the camera-space face, its z divided by its length (negated under flip_normals).  front: that z >= 0; steep:
 * that z < 0.5.  A face whose camera coordinates or unit normal are not finite (zero area: 0 / 0) is neither front nor rasterised.
 * Coverage (exact integers): every vertex is snapped to 1/256 pixel, X = rint((ndc_x + 1) * 128 R), Y = rint((1 - ndc_y) * 128 R), clamped
 * to +-2^26; pixel (row i, column j) has its centre at (256 j + 128, 256 i + 128); the edge functions are int64, both windings are taken
 * (multiplied by the sign of the area), and the top-left fill rule gives a centre on a shared edge to exactly one face.  kaolin's
 * coverage is floating point: a deliberate difference of at most 1/256 pixel, which makes coverage reproducible bit for bit.
 * Interpolation: w_k = (float)E_k / (float)A, an fp32 division; an attribute is (w0 a0 + w1 a1) + w2 a2.  Among the front faces that
 * cover a centre the winner is the largest (interpolated camera z, -face index): nearer wins, a tie goes to the lower index, whatever
 * the order of the faces.  face_idx i32 [R][R]: the winner, -1 for none.
 * Render: where face_idx != -1 the canvas f32 [4][R][R] is the bilinear sample of the texture (texel = byte / 255.0f) at x = u W - 0.5,
 * y = (1 - v) H - 0.5, clamped to [0, W - 1] x [0, H - 1]: ((t00 gx gy + t01 fx gy) + t10 gx fy) + t11 fx fy with fx = x - floor(x),
 * gx = 1 - fx.  Where face_idx == -1 it is 0 in all four channels (unknown; the reference samples the texel at uv = (0, 0) there, a quirk
 * that is not reproduced); an OVERPAINT window is 0 as well in rows [over_y, R - over_y) x columns [over_x, R - over_x).
 * Backprojection: a face is valid when it is front, not steep and the winner of at least one pixel.  The valid faces are rasterised in
 * texture space by the same integer rule: X = rint((u W) 256), Y = rint(((1 - v) H) 256), the same clamp, texel centres at
 * (256 j + 128, 256 i + 128); the lowest valid face index wins.  Its interpolated feature (p, q) = stamp NDC / 2 + 0.5 addresses the stamp
 * image at x = p R - 0.5, y = (1 - q) R - 0.5 (bilinear, border-clamped, the same expression), whose RGB is the decoder's value clamped
 * to 0..1 (dtp_stamp's with composite 0) and whose A is (mask[i][j] > 0) * (face_idx[i][j] != -1).  Where the sampled A is > 0, all four
 * bytes of the texel become (unsigned char)(min(v, 1) * 255.0f) -- alpha included, as manager.py:268 does, so texels at the silhouette get
 * a partial alpha.  An ERASE stamp runs no stamp and writes 0 to the four channels there.  Texels no valid face covers are neither read
 * nor written.
 *
 * dtp_mesh_create copies host arrays to the device of `ctx`: vertices f32 [V][3], faces i32 [F][3], face_uvs f32 [F][3][2] (UVs in 0..1,
 * v up), F <= 2^20; with them it allocates the per-face records of a stamp, so a stroke allocates nothing.  DTP_ERR_ARG, before any
 * device call, for a NULL pointer, V < 1, F outside 1..2^20, an index outside 0..V-1 or a non-finite UV (naming the face), a non-finite
 * vertex.  A mesh belongs to its handle: dtp_destroy frees the meshes still alive; dtp_mesh_destroy(NULL) is a no-op, and a handle that is
 * not a live mesh is DTP_ERR_ARG.
 *
 * dtp_mesh_stroke: per stamp, in the caller's order, on the one stream and without a host round trip: camera -> render (straight into the
 * stamp's staging buffer) -> the stamp as dtp_stamp_seeded runs it, B = 1 -> backproject.  Stamp i + 1 renders what stamp i pasted.
 *   texture     u8 [H][W][4] RGBA on the device, 4-byte aligned, 1 <= H, W <= 32768; painted in place
 *   stamps      host dtp_mesh_stamp[n]: pos, the brush position on the mesh; normal, the surface normal there (the camera sits at
 *               pos + normal); prev, the previous brush position (up = prev - pos); fov > 0, half the window's width in world units (the
 *               Kit app's fov_distance * fov_scale); mode DTP_STROKE_*; slot, seed as in dtp_stroke_stamp
 *   st          ONE dtp_settings for every stamp; composite and output_u8 must be 0
 *   o           flip_normals (a left-handed mesh, manager.py:197); margin: the default paste mask make_stamp_mask(R, margin) (the Kit
 *               app's is 1); over_y, over_x: overpaint_canvas's margins; sample_vae, strength: as dtp_stamp_seeded
 *   paste_mask  device u8 [R][R], applied where > 0, for every stamp; NULL = make_stamp_mask(R, o->margin), and for an ERASE stamp the
 *               analytic disc (2 i - (R - 1))^2 + (2 j - (R - 1))^2 <= (R - 4)^2 (the reference draws its circle_mask with PIL)
 * The call checks everything, then enqueues and returns: no wait (a change of `steps` still waits once, and the first use of a mask
 * allocates it), no allocation, no copy back.  DTP_ERR_ARG, naming the stamp where there is one: a NULL pointer, a mesh that is not alive
 * or belongs to another handle, H or W outside 1..32768, n < 1, an unknown mode, margin outside [0, R/2), over_y / over_x outside
 * [1, R/2) with an OVERPAINT stamp, a slot outside 0..15, a camera dtp_mesh_camera refuses.  What dtp_stamp_seeded refuses is refused with
 * its code (an unset slot: DTP_ERR_STATE).  A refused call leaves the texture untouched.  A window that the bounding box of the mesh
 * misses is skipped on the host; a window that meets the box and covers no face still runs its stamp, and pastes nothing.  Neither is an
 * error.  dtp_last_stroke_info answers for the call: stamps = groups = n, and the UNet evaluations of the stamps that ran. */
typedef struct dtp_mesh dtp_mesh;
typedef struct { float pos[3], normal[3], prev[3], fov; int mode, slot; uint64_t seed; } dtp_mesh_stamp;
typedef struct { int flip_normals, margin, over_y, over_x, sample_vae; double strength; } dtp_mesh_stroke_opts;
int dtp_mesh_create(dtp_ctx* ctx, const float* vertices, int V, const int* faces, int F, const float* face_uvs, dtp_mesh** out);
int dtp_mesh_destroy(dtp_mesh* mesh);
int dtp_mesh_camera(const float pos[3], const float normal[3], const float prev[3], float fov, float out[12]);
int dtp_mesh_stroke(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                    const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, dtp_stream s);

/* ---------------------------------------------------------------- bleeding painted texels across UV chart borders
 * The backprojection writes a texel only when its centre lies inside the UV triangle of a valid face, so the texels between the charts
 * of an atlas (the gutter) keep what they had, and every bilinear tap that straddles a chart border mixes a painted texel with an
 * unpainted one: the next stamp's render sees a line of partly unknown pixels along every seam, and so does any renderer that filters
 * the texture.  The bleed pass pads the charts (Blender's texture paint: "Bleed").  Everything below is exact integer arithmetic.
 *
 * Coverage of (mesh, H, W): texel (row i, column j) is covered when its centre (256 j + 128, 256 i + 128) is covered by at least one of
 * ALL F faces of the mesh in texture space, by the backprojection's rule: X = rint((u W) 256), Y = rint(((1 - v) H) 256), the +-2^26
 * clamp, int64 edge functions, both windings, the top-left fill rule (a centre on an edge two faces share belongs to one of them: no
 * hole), a face of zero area excluded.  It depends on no camera.
 * Source of a gutter texel at radius k, 1 <= k <= 16: for an uncovered texel g = (i, j), s(g) is the covered texel (i + di, j + dj) INSIDE
 * the texture (no wrap-around) with 0 < di^2 + dj^2 <= k^2 that minimises (di^2 + dj^2, di, dj) lexicographically; no candidate: no
 * source.
 * The pass over a texel rectangle: every uncovered texel of the rectangle that has a source receives all four bytes of texture[s(g)].
 * It reads only covered texels and writes only uncovered ones, so one launch needs no second buffer, its result does not depend on
 * scheduling, and applying it twice is applying it once.
 *
 * dtp_mesh_stroke_bleed is dtp_mesh_stroke with `bleed` = the radius: after the backprojection of every stamp that ran (INPAINT, OVERPAINT
 * and ERASE alike, which bleeds its zeros) the pass runs over that stamp's texel bounding box -- the union of the texel ranges of its
 * valid faces, kept on the device -- grown by `bleed` and clipped to the texture; no valid face, no pass; no host read.  Stamp i + 1
 * renders what stamp i bled.  Gutter texels outside those rectangles are NOT touched: a texture that was painted before, or loaded from
 * a file, is padded as a whole with dtp_mesh_bleed.  bleed == 0 is dtp_mesh_stroke exactly, the same launches and the same bytes; bleed
 * outside 0..16 is DTP_ERR_ARG naming "bleed", checked with everything else before anything is enqueued.  The first use of an (H, W)
 * with a mesh builds its coverage: one allocation (1 bit per texel) and its kernels, and the call waits for them once; later strokes
 * allocate nothing and never wait.  A mesh keeps ONE coverage mask: another size frees it and builds it again; it is freed with the mesh.
 * dtp_mesh_bleed: the pass on its own over rect = {x0, y0, x1, y1}, inclusive, clipped to the texture (NULL = the whole texture; nothing
 * of it inside the texture, or bleed == 0: nothing is done).  DTP_ERR_ARG for a NULL mesh or texture, bleed outside 0..16, H or W outside
 * 1..32768, x0 > x1 or y0 > y1, a mesh that is not alive.
 * dtp_op_mesh_coverage: the coverage as bytes 0 / 1, out u8 [H][W] on the device.
 * dtp_mesh_bleed_offsets (host only): *count = the number of candidates of `radius` (1..16) and, unless di_dj is NULL, di_dj[2 o],
 * di_dj[2 o + 1] = (di, dj) of candidate o in the order above (796 pairs at radius 16).  The table of radius k is the prefix with
 * di^2 + dj^2 <= k^2 of the table of radius 16.  DTP_ERR_ARG for a radius outside 1..16 or count NULL. */
int dtp_mesh_stroke_bleed(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                          const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, dtp_stream s);
int dtp_mesh_bleed(dtp_mesh* mesh, uint8_t* texture, int H, int W, int bleed, const int* rect, dtp_stream s);
int dtp_op_mesh_coverage(dtp_mesh* mesh, int H, int W, uint8_t* out, dtp_stream s);
int dtp_mesh_bleed_offsets(int radius, int* count, signed char* di_dj);

/* ---------------------------------------------------------------- picking on a mesh
 * replaces: what the Kit app's brush tool does with every pointer event (kit_app/.../python/ui/brush.py:139-198): a camera ray cast
 * against the mesh with MeshRaycast.raycast_closest (an Omniverse extension), and the chord from the previous hit to the new one cut
 * into stamps radius / stamps_per_radius apart.  Picking is the render's visibility rule applied to one sample per ray; nothing is
 * compared under a tolerance.  The spacing rule was written from the source of brush.py, not captured from a Kit run.
 *
 * The ray frame (dtp_mesh_ray_frame; host only, in double from the fp32 origin o and direction d, rounded to fp32 once):
 * b = -normalize(d), so the frame looks down -z as the stamp camera does; helper = the unit axis k of the smallest |d_k| (the lowest k
 * on a tie); r = normalize(cross(helper, b)), u = cross(b, r); out = the rows (r, u, b), each followed by t = -row . o, laid out as
 * dtp_mesh_camera's.  The ray is the frame's -z axis through x = y = 0.  DTP_ERR_ARG for a zero or non-finite direction, a non-finite
 * origin, a frame that does not fit fp32.
 * The grid: the eight corners of the vertices' bounding box go through the fp32 frame in double, x = ((m0 vx + m1 vy) + m2 vz) + t for
 * rows r and u; S = 2^e with e the largest integer such that S max(|x|, |y|) over the corners is <= 2^25, clamped to -64 <= e <= 64 (all
 * corners on the ray: 64).  S is a power of two: scaling by it is exact and no vertex of the mesh reaches the +-2^26 clamp of the snap.
 * Per face (fp32, every operation rounded once, no contraction): the camera-space x, y, z of the three vertices as the render computes
 * them, cam_k = ((m0 x + m1 y) + m2 z) + t; X = snap(x S), Y = snap(y S) with snap(v) = rint(v) clamped to +-2^26; the render's integer
 * coverage at the single centre (0, 0): int64 edge functions, both windings (multiplied by the sign of the area), the top-left fill
 * rule, so a ray through an edge or a vertex that faces of a closed surface share has exactly one of them, never none.  A face of zero
 * snapped area or with a non-finite camera coordinate is excluded.  w_k = (float)E_k / (float)A; z = (w0 z0 + w1 z1) + w2 z2, -0 taken
 * as +0.  A covered face with z <= 0 (not behind the origin) is a candidate.  Both sides of a face can be hit: there is no winding
 * option.
 * The hit is the candidate with the largest (z, -face index), the render's order: nearer wins, a tie goes to the lower index, whatever
 * the order of faces, workgroups or launches (a 64-bit atomic max over the order-preserving bits of z and ~face).
 * The record: face (-1: no hit, and every other field 0); w[3]; pos = (w0 p0 + w1 p1) + w2 p2 per component on the world vertices;
 * normal = the face's unit geometric normal, n = cross(p1 - p0, p2 - p0) with each component a product minus a product,
 * n / sqrt((nx nx + ny ny) + nz nz), negated when (nx dx + ny dy) + nz dz > 0 so that normal . d <= 0: it faces the ray's origin, which
 * is what the stamp camera needs; uv interpolated like pos; t = 0 - z, the distance along the ray in units of |d| = 1.
 *
 * dtp_mesh_pick: rays host dtp_ray[n], 1 <= n <= 4096; out_host host dtp_mesh_hit[n].  Every check comes before any device call:
 * DTP_ERR_ARG, naming the ray where there is one, for a NULL pointer, a mesh that is not alive, n outside 1..4096, a ray
 * dtp_mesh_ray_frame refuses; a refused call writes nothing.  The call enqueues on `s` (frames in, two kernels, records out), waits
 * for `s` ONLY, and fills out_host.  `s` should NOT be the stream of the strokes: a stroke only enqueues, and sixteen 512^2 stamps are
 * about 1.5 s of queued device work; a pick behind them on the same stream would answer after they finish, and the pointer would lag
 * the paint by the whole backlog.  The kernels read only what dtp_mesh_create copied (vertices, faces, face UVs); they neither read nor
 * write the per-face records, the window and valid lists, the coverage mask or anything else a stroke in flight writes, so a pick runs
 * beside a stroke of the same mesh.  Its own buffers (ray frames, one 64-bit slot per ray, the records, a pinned host copy) are
 * allocated at the first pick of a mesh, grow only when n exceeds what is held (in steps of 256 rays; growing frees, which waits for
 * the device), and are freed with the mesh; dtp_mesh_create allocates none of them.  Two picks of ONE mesh at the same time share these
 * buffers: they are the caller's to serialise.
 *
 * dtp_mesh_path_plan (host only): the stamps of a pointer path, brush.py:158-198 in double from the fp32 inputs, every result rounded
 * to fp32 once.  state = {has_prev, prev[3]} travels in and out, so a path can arrive in several calls; {0} starts one.  Per hit, in
 * order: a miss (face < 0) is skipped and leaves the state alone; the first hit sets prev = pos and gives no stamp; a later hit with
 * dist = |pos - prev| < stamp_distance changes nothing; otherwise num = (int)(dist / stamp_distance), step = dist / num,
 * dir = (pos - prev) / dist, and stamp k = 0 .. num - 1 sits at c_{k+1} = step dir + c_k with c_0 = prev (the chain stays in double;
 * the stamps lie on the chord, as in the reference), carries THIS hit's normal and prev_position = c_k; then prev = pos.  The arrays
 * pos, normal, prev hold 3 floats per stamp and `cap` stamps; *count = the stamps planned.  DTP_ERR_ARG for a NULL pointer, n < 0,
 * cap < 0, a stamp_distance that is <= 0 or not finite, a chord of more than 2^20 stamps, and for count > cap: then *count holds the
 * capacity needed, nothing usable is written and the state is unchanged. */
typedef struct { float origin[3], dir[3]; } dtp_ray;
typedef struct { int face; float w[3], pos[3], normal[3], uv[2], t; } dtp_mesh_hit;
typedef struct { int has_prev; float prev[3]; } dtp_path_state;
int dtp_mesh_pick(dtp_mesh* mesh, const dtp_ray* rays, int n, dtp_mesh_hit* out_host, dtp_stream s);
int dtp_mesh_ray_frame(const float origin[3], const float dir[3], float out[12]);
int dtp_mesh_path_plan(const dtp_mesh_hit* hits, int n, float stamp_distance, dtp_path_state* state, float* pos, float* normal, float* prev,
                       int cap, int* count);

/* ---------------------------------------------------------------- a view of a textured mesh
 * replaces: the viewport.  In the reference the painted mesh is seen through Omniverse RTX, which reads the texture through
 * update_material_texture (kit_app/.../python/manager.py:349-354).  dtp_mesh_view draws the whole mesh with a perspective camera into an
 * H x W RGBA frame on the device: a preview, so that a client without Omniverse sees what it painted, and the frame whose pixels
 * dtp_view_rays turns into the rays of dtp_mesh_pick.  The stamp camera of dtp_mesh_stroke stays orthographic, as the reference's is.
 * Every fp32 operation below is rounded once and in the order written (no contraction, correctly rounded division and square root);
 * nothing is compared under a tolerance.  The frame does not depend on the order in which faces are visited or on how they are binned.
 *
 * The camera (dtp_view_camera; host only, in double from the fp32 inputs, rounded to fp32 once): b = normalize(eye - at),
 * r = normalize(cross(up, b)), u = cross(b, r); m = the rows (r, u, b), each followed by t = -row . eye, laid out as dtp_mesh_camera's;
 * fy = 1 / tan((fov_y pi) / 360) with fov_y in degrees, fx = (fy H) / W; near as given.  DTP_ERR_ARG for anything non-finite, eye == at,
 * an up that is zero or parallel to the view direction, fov_y outside (0, 180), near <= 0, H or W outside 1..4096, a result that does
 * not fit fp32 (a non-finite value, fx or fy that round to 0, a near whose reciprocal is not finite).  A camera filled in by hand is held
 * to the same rule by the two calls that take one.
 * The rays (dtp_view_rays; host only, in double from the fp32 camera, rounded once): for pixel position (x, y), the centre of pixel
 * (i, j) being (j + 0.5, i + 0.5): ndc_x = (2 x) / W - 1, ndc_y = 1 - (2 y) / H; origin = the eye as the camera holds it,
 * -((r t_r + u t_u) + b t_b) per component; dir = (r (ndc_x / fx) + u (ndc_y / fy)) - b: a dtp_ray for dtp_mesh_pick.  pixels_xy host
 * float [n][2], n >= 1.
 *
 * Per face (fp32): the camera-space x_k, y_k, z_k of its three vertices exactly as a stamp's projection computes them,
 * ((m0 vx + m1 vy) + m2 vz) + t per row.  A face is drawn iff all nine values are finite and all three z_k <= -near.  A face with ANY
 * vertex nearer than the near plane (or behind the eye) is DROPPED WHOLE, NOT CLIPPED: that is the price of exact coverage, and a mesh
 * the camera stands inside loses the faces that cross the plane.  iw_k = 1.0f / (0.0f - z_k);
 * X_k = snap((((x_k fx) iw_k) + 1) (128 W)), Y_k = snap((1 - ((y_k fy) iw_k)) (128 H)) with snap(v) = rint(v) clamped to +-2^26 and
 * 128 W, 128 H exact.  A face of zero snapped area is not drawn.  Facing is the sign of the snapped integer area
 * A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0): A < 0 is FRONT (counter-clockwise on the screen with y up: the side a stamp's render
 * calls front), flip_normals swaps the two; cull = 0 draws both sides, cull = 1 front faces only.  nzu, for the shade, is the z of the
 * camera-space unit normal as a stamp's projection computes it: n = cross(c1 - c0, c2 - c0), each component a product minus a product,
 * nzu = nz / sqrt((nx nx + ny ny) + nz nz).
 * Per pixel (i, j), centre (256 j + 128, 256 i + 128): the coverage of the strokes unchanged (int64 edge functions, both windings, the
 * top-left fill rule) gives w_k = (float)E_k / (float)|A|; q_k = w_k iw_k; d = (q0 + q1) + q2, the inverse depth, which is linear on the
 * screen.  The winner is the covering face with the largest (d, -face index).  Perspective-correct UV: u = ((q0 u0 + q1 u1) + q2 u2) / d,
 * v likewise.
 * Colour: the texture (u8 [TH][TW][4]) is sampled as a stamp's render samples it: the four taps and weights of grid_sample
 * (align_corners False, border padding) at (u TW - 0.5, (1 - v) TH - 0.5), the blend ((v00 w00 + v01 w01) + v10 w10) + v11 w11 of
 * byte / 255 per channel: t_R, t_G, t_B, t_A.  s = 1 without shade; with it s = ambient + (1 - ambient) |nzu|.
 * c_ch = (t_ch t_A + (unpainted_ch / 255) (1 - t_A)) s for R, G, B; the byte is (unsigned char)(fminf(c_ch, 1) 255 + 0.5f) and the
 * alpha byte 255.  face_idx = the winner, depth = 1.0f / d (the distance from the eye along the view direction).  A pixel no face
 * covers gets the four bytes of background, face_idx -1, depth 0.  No colour management, no mip or anisotropic filtering, one sample
 * per pixel: the frame aliases under minification and along silhouettes (the sections below add each of them as an entry of its own).
 *
 * dtp_mesh_view: texture device u8 [TH][TW][4] (1..32768 a side), image device u8 [H][W][4], face_idx device i32 [H][W] or NULL,
 * depth device f32 [H][W] or NULL; all 4-byte aligned; 1 <= H, W <= 4096; ambient in 0..1; cull, flip_normals, shade 0 or 1.  Every
 * check comes before any device call, a mesh that is not alive is refused and not followed, and a refused call writes nothing.  The
 * call only ENQUEUES on `s` (a memset and four kernels) and returns.  The kernels read the vertices, faces and UVs of the mesh, the
 * texture, and the view's own buffers (a 64-byte record per face, 4 F + F list entries, the bin counters), allocated at the first view of
 * a mesh and freed with it; they touch nothing a stroke or a pick in flight uses, so a view on a stream of its own runs beside them.  A
 * view that runs WHILE a stroke writes the texture shows each texel either old or new (every writer stores whole 4-byte texels), and
 * may catch a stamp halfway; for a frame of everything painted so far, make `s` wait for the stroke's stream first.  Two views of ONE
 * mesh at the same time share the buffers: they are the caller's to serialise. */
typedef struct { float m[12]; float fx, fy, near; } dtp_view_cam;
typedef struct { int cull, flip_normals, shade; float ambient; uint8_t unpainted[3]; uint8_t background[4]; } dtp_view_opts;
int dtp_view_camera(const float eye[3], const float at[3], const float up[3], float fov_y_degrees, int H, int W, float near, dtp_view_cam* out);
int dtp_view_rays(const dtp_view_cam* cam, int H, int W, const float* pixels_xy, int n, dtp_ray* out);
int dtp_mesh_view(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const dtp_view_cam* cam, int H, int W, const dtp_view_opts* opts,
                  uint8_t* image, int* face_idx, float* depth, dtp_stream s);

/* ---------------------------------------------------------------- the mip pyramid of a texture and a trilinear-filtered view
 * A mesh seen whole is minified: many texels per pixel, and one bilinear sample of level 0 shows a nearly random one.
 * dtp_texture_mips builds the pyramid of a painted texture on the device in exact integers, alpha-weighted, because unpainted texels are
 * 0,0,0,0 and a plain box filter would drag black into every chart border; dtp_mesh_view_mips is dtp_mesh_view with a level chosen per
 * pixel from the footprint of the pixel in the texture.  An exporter feeds the same pyramid to a renderer's sampler.  Nothing is
 * compared under a tolerance.
 *
 * Layout (dtp_mip_layout; host only).  Level 0 is the texture itself and is never copied.  Level l + 1 has h' = (h + 1) / 2 rows and
 * w' = (w + 1) / 2 columns (integer division), down to 1 x 1; levels = the number of levels including level 0 (<= 16 for sides up to
 * 32768; a 1 x 1 texture has 1 level and 0 pyramid bytes).  Levels 1 .. levels - 1 lie one after the other in ONE buffer of 4-byte
 * texels, row-major: offset[l] is the byte offset of level l in it, offset[1] = 0, offset[l + 1] = offset[l] + 4 h[l] w[l]; bytes = their
 * sum.  h[0], w[0] = TH, TW; offset[0] and every entry from `levels` on are 0.  DTP_ERR_ARG for NULL and for sides outside 1..32768
 * (nothing written).  (The struct is dtp_mip_levels: C does not let a typedef and a function share a name.)
 *
 * Texel rule (integers only).  Texel (i, j) of level l + 1 reads four texels of level l (h x w): rows 2 i and min(2 i + 1, h - 1),
 * columns 2 j and min(2 j + 1, w - 1); a clamped index counts twice.  With the bytes c_k of a colour channel and a_k of alpha:
 * A = sum a_k; alpha = (A + 2) >> 2; colour = A ? (sum c_k a_k + (A >> 1)) / A : 0 (an unsigned 32-bit division; the largest numerator
 * is 4 x 255 x 255 + 510).  So a 2 x 2 block of one opaque red texel and three unpainted ones is 255,0,0,64, not a dark red.
 *
 * dtp_texture_mips: texture device u8 [TH][TW][4], mips device u8 [mips_bytes]; both 4-byte aligned; mips_bytes >= the layout's bytes.
 * With 1 level, mips may be NULL and nothing is launched.  Every check comes before any device call and a refused call writes nothing.
 * The call only ENQUEUES on `s`: one kernel per pass, a pass takes 64 x 64-texel tiles of its source level and writes that tile's part
 * of up to six levels; the passes start from levels 0, 6 and 12 (at most three launches; two for 2048 x 2048).  It reads the texture
 * and writes the pyramid alone; built while a stroke writes the texture it may catch a stamp halfway, as a view may.
 *
 * dtp_mesh_view_mips: dtp_mesh_view's arguments, checks, buffers and launches, plus mips (the pyramid of `texture` as dtp_texture_mips
 * lays it out; device, 4-byte aligned; may be NULL when the layout has 1 level) and lod (device f32 [H][W], 4-byte aligned, or NULL).
 * Visibility, face_idx and depth are dtp_mesh_view's.  Only the sample differs.  Per covered pixel, fp32, one rounded operation at a
 * time in the order written, with L = levels:
 *  1. (u, v) is the pixel's UV as dtp_mesh_view computes it.
 *  2. The WINNER FACE ALONE is evaluated at the neighbouring centres (px + 256, py) and (px, py + 256) with no inside test: E_k' the same
 *     sign-normalised int64 edge functions, w_k' = (float)E_k' / (float)|A|, q_k' = w_k' iw_k, d' = (q0' + q1') + q2',
 *     u' = ((q0' u0 + q1' u1) + q2' u2) / d', v' likewise.
 *  3. If either d' is not finite or not > 0 (the face's plane ends within a pixel: beyond the horizon), the level is L - 1 and f = 0.
 *  4. a = ((u'_x - u) TW)^2 + ((v'_x - v) TH)^2 with (float)TW, (float)TH of level 0 and each square a product; b the same from the y
 *     neighbour; rho2 = fmaxf(a, b).  A non-finite rho2 also takes level L - 1 with f = 0.
 *  5. l = the largest level in 0 .. L - 1 with 4^l <= rho2 (compared against exact powers of four; no logarithm), or 0 when rho2 < 1.
 *     f = 0 if l = L - 1 or rho2 <= 4^l, otherwise f = ((rho2 / 4^l) - 1) / 3: continuous and monotone, 0 at rho = 2^l and tending to 1
 *     at 2^(l + 1).  lod = (float)l + f; a pixel no face covers gets lod 0.
 *  6. t_l = the taps and blend of byte / 255 of dtp_mesh_view at level l with that level's h[l], w[l] in place of TH, TW.  If f > 0,
 *     t = t_l + (t_(l + 1) - t_l) f per channel (a difference, a product, a sum); otherwise t = t_l and level l + 1 is not read.
 *     The shade, the unpainted mix, the byte conversion and the background are dtp_mesh_view's.
 * A frame with rho2 <= 1 everywhere is dtp_mesh_view's frame byte for byte.  No anti-aliasing of silhouettes (dtp_mesh_view_aa), and ONE
 * level from the longer axis of the footprint: a surface at a grazing angle is sampled too coarse (dtp_mesh_view_aniso samples along it). */
typedef struct { int levels; int h[16], w[16]; uint64_t offset[16]; uint64_t bytes; } dtp_mip_levels;
int dtp_mip_layout(int TH, int TW, dtp_mip_levels* out);
int dtp_texture_mips(const uint8_t* texture, int TH, int TW, uint8_t* mips, uint64_t mips_bytes, dtp_stream s);
int dtp_mesh_view_mips(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                       const dtp_view_opts* opts, uint8_t* image, int* face_idx, float* depth, float* lod, dtp_stream s);

/* ---------------------------------------------------------------- a view clipped at the near plane
 * dtp_mesh_view drops a face whole as soon as one vertex is nearer than the near plane.  On a scan of sub-pixel faces that costs a rim;
 * on a floor under the camera, the walls of a room painted from inside, the long side of a box seen along its length it removes the
 * surface, and the frame shows background where dtp_mesh_pick of the pixel's ray hits.  dtp_mesh_view_clip is
 * dtp_mesh_view (filter 0) or dtp_mesh_view_mips (filter 1) that also draws the faces ACROSS the plane, down to the plane.  No geometry
 * is cut: a cut makes new vertices, whose snapped positions are no function of the mesh alone.  A crossing face is rasterised in
 * homogeneous form instead (Olano and Greer, "Triangle scan conversion using 2D homogeneous coordinates", 1997): per pixel the edge
 * functions of the camera-space triangle against the pixel's ray, which give the same q_k and d that the rest of the frame consumes.
 * fp32, one rounded operation at a time in the order written; nothing is compared under a tolerance.
 *
 * Classes of face, from the camera-space c_k = (x_k, y_k, z_k) exactly as dtp_mesh_view computes them:
 *   IN FRONT  all nine values finite and every z_k <= -near: dtp_mesh_view's face, bit for bit (snapped integers, int64 coverage).
 *   BEHIND    every z_k > -near, or any value not finite: not drawn.
 *   CROSSING  finite, at least one vertex on each side (a vertex with z_k == -near is in front): drawn as follows.
 * Per crossing face: n_0 = c_1 x c_2, n_1 = c_2 x c_0, n_2 = c_0 x c_1 with cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
 * a.x b.y - a.y b.x), each component a product minus a product; D = (c_0.x n_0.x + c_0.y n_0.y) + c_0.z n_0.z.  D == 0 or a D that is
 * not finite (the face's plane contains the eye): not drawn.  The face keeps m_k = n_k for D > 0, -n_k for D < 0 (a sign flip, exact)
 * and r = 1.0f / |D|, SEPARATELY: two faces that share an edge have n that are exact negations of each other, so the signs of their
 * edge functions at a pixel agree exactly and a centre on the shared edge is never refused by both.  Facing comes from the side of the
 * face's plane the eye is on: D < 0 is FRONT (the side dtp_mesh_view calls front: a face pushed back until it no longer crosses keeps
 * its facing), flip_normals swaps the two, cull = 1 draws front faces only.  nzu is computed as dtp_mesh_view computes it.
 * Per pixel (i, j): g_x = ((float)(2 j + 1) / (float)W - 1.0f) / fx, g_y = (1.0f - (float)(2 i + 1) / (float)H) / fy: the ray of the
 * centre as dtp_view_rays defines it, (g_x, g_y, -1) in camera space.  E_k = (m_k.x g_x + m_k.y g_y) - m_k.z.  The face covers the
 * centre iff every E_k >= 0 (edges are inclusive; the winner rule settles a double cover), and with q_k = E_k r, d = (q0 + q1) + q2:
 * d is finite and > 0 (the face's plane ends at its horizon), and 1.0f / d >= near.  That last test IS the clip: it generalises "every
 * z_k <= -near", and no pixel of a clipped frame has a depth below near.  From there on nothing is new: the winner is the covering face
 * with the largest (d, -face index) among faces of both kinds, u = ((q0 u0 + q1 u1) + q2 u2) / d, v likewise, the sample, the shade,
 * the byte, face_idx and depth = 1.0f / d are dtp_mesh_view's.  In real arithmetic q_k and d are the quantities the integer path computes.
 * filter 1: steps 2-3 of dtp_mesh_view_mips apply to a crossing winner with the same E_k, q_k', d' at the rays of the centres (i, j + 1)
 * and (i + 1, j), no inside test; a d' that is not finite or not > 0 gives level L - 1 with f = 0.
 * What is known and not hidden: crossing faces are watertight among themselves (the sign argument above), faces in front among
 * themselves (the integer rule).  Along an edge between a crossing face and a neighbour in front two rules meet, snapped integers and
 * fp32 homogeneous edge functions: a centre within the snap (1/256 pixel) of that edge may be claimed by both, and depth decides, or by
 * neither, and one pixel shows what lies behind.  It is a preview.  A scene without a crossing face gives dtp_mesh_view's (or
 * dtp_mesh_view_mips') frame byte for byte.
 *
 * dtp_mesh_view_clip: the arguments, checks, buffers and launches (a memset and four kernels) of dtp_mesh_view_mips, plus filter: 0 =
 * one bilinear sample of level 0 (mips and lod must be NULL), 1 = trilinear (mips may be NULL when the layout has 1 level; lod or NULL).
 * A filter that is neither is DTP_ERR_ARG.  Every check comes before any device call and a refused call writes nothing.  A crossing
 * face is streamed by every tile its pixel range meets; the range is the box of the projected polygon cut at z = -near, grown, and
 * holds every centre the face covers. */
int dtp_mesh_view_clip(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                       const dtp_view_opts* opts, int filter, uint8_t* image, int* face_idx, float* depth, float* lod, dtp_stream s);

/* ---------------------------------------------------------------- an anti-aliased view
 * The views above take one sample per pixel, at its centre: silhouettes, UV-chart borders and creases are staircases that crawl from
 * frame to frame, and a face about a pixel wide is there or not by chance.  The trilinear filter decides what is sampled INSIDE a face;
 * nothing above decides which face is sampled.  dtp_mesh_view_aa takes samples x samples centres per pixel on an ordered grid and stores
 * their average, in one pass.  No new arithmetic: the camera holds nothing that depends on the frame's size, so "the
 * same camera at s H x s W" is a frame the sections above define, and the samples of pixel (i, j) are its pixels.
 *
 * samples = s in {1, 2, 4}: 1, 4 or 16 samples per pixel.  filter and clip: 0 or 1 each.  The FINE frame is what dtp_mesh_view (filter 0,
 * clip 0), dtp_mesh_view_mips (filter 1, clip 0) or dtp_mesh_view_clip (clip 1, with that filter) writes for the same mesh, texture,
 * pyramid, camera and options at size (s H) x (s W): every rule of those sections with s H, s W in place of H, W -- the snap by 128 s W
 * and 128 s H, the centres 256 b + 128 of fine pixel b, the rays of clip, the footprint of filter 1 measured between the centres of
 * neighbouring FINE pixels.  So lod comes out about log2(s) lower than at samples 1: each sample covers that much less of the texture.
 *   image[i][j][ch]  = (sum of fine[s i + a][s j + b][ch] over a, b in 0 .. s - 1  +  s s / 2) >> log2(s s), per channel R, G, B, A: the
 *                      rounded box average of the BYTES of the fine frame, each sample rounded to its byte before it is summed, the
 *                      background's bytes where no face is.  With the default background 0,0,0,0 a silhouette pixel therefore
 *                      carries its colour premultiplied by its coverage, and the coverage in alpha.
 *   face_idx, depth, lod [i][j] (each or NULL; lod needs filter 1) = those of fine pixel (s i + s / 2, s j + s / 2): the sample just below
 *                      and right of the pixel's centre; for s = 1 the pixel itself.
 *   coverage[i][j]   device u8 [H][W] or NULL: how many of the pixel's samples a face covers, 0 .. s s.
 * samples 1 writes the bytes of the call it stands for.  The fine frame exists nowhere: the samples are resolved on the chip (registers and LDS), and the
 * view's per-mesh buffers are those of dtp_mesh_view whatever s is.  The checks are dtp_mesh_view_clip's (mips and lod must be NULL
 * with filter 0), plus clip in {0, 1}, samples in {1, 2, 4} and s H, s W <= 4096 (the pixel ranges of a face are packed in 16 bits and
 * there are 4096 bin counters, of the fine frame); every check comes before any device call and a refused call writes nothing.  The call
 * only enqueues on `s`: a memset and four kernels.  Not here: a rotated or jittered pattern; anisotropic filtering is dtp_mesh_view_aniso, below,
 * with the same samples. */
int dtp_mesh_view_aa(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                     const dtp_view_opts* opts, int filter, int clip, int samples, uint8_t* image, int* face_idx, float* depth, float* lod,
                     uint8_t* coverage, dtp_stream s);

/* ---------------------------------------------------------------- an anisotropic view
 * The trilinear filter picks ONE level from the LONGER of the two footprint axes.  A surface seen at a grazing angle -- the floor under
 * the camera, the walls of a room painted from inside: the poses clip exists for -- has a footprint many times longer than wide, is
 * sampled several levels too coarse, and what was painted across the line of sight turns grey a few metres out.
 * dtp_mesh_view_aniso takes the level from the SHORTER axis instead and averages up to max_aniso trilinear taps spread along the longer
 * one.  It is an addition to the dtp_mesh_view_mips contract: fp32, one rounded operation at a time in the order written, no
 * contraction; nothing is compared under a tolerance.  M = max_aniso, an integer in 1..16.  Per covered pixel:
 *  1. (u, v), the two neighbour evaluations of the winner face and the two footprint vectors in level-0 texels are those of steps 1-3
 *     of dtp_mesh_view_mips (the integer path, or the ray path of a face across the near plane: see dtp_mesh_view_clip, filter 1):
 *     du_a = u'_x - u, dv_a = v'_x - v, a = (du_a TW, dv_a TH); du_b, dv_b, b likewise from the y neighbour; la2 = a.x a.x + a.y a.y,
 *     lb2 = b.x b.x + b.y b.y.
 *  2. If a neighbour's d' is not finite or not > 0, or la2 or lb2 is not finite: the level is L - 1, f = 0, N = 1, one tap at (u, v) --
 *     the beyond-the-horizon branch of dtp_mesh_view_mips.  (That rule takes fmaxf of the two, which ignores a NaN on one axis alone;
 *     here such a pixel takes this branch.  It needs UVs whose products overflow fp32.)
 *  3. Otherwise pmax2 = fmaxf(la2, lb2), pmin2 = fminf(la2, lb2); the major axis is a if la2 >= lb2, else b, and (du, dv) is the major
 *     axis's UV difference BEFORE the scale by TW, TH.
 *  4. rho2 = fminf(pmax2, fmaxf(fmaxf(pmin2, 1.0f), pmax2 / (float)(M M))): the level comes from the minor axis, is never finer than a
 *     texel, never more than M times finer than the major axis asks for, and never coarser than the trilinear one.
 *  5. N = the smallest n in 1..M with pmax2 <= (float)(n n) rho2 (the product rounded once); M if there is none.
 *  6. l and f from rho2 by step 5 of dtp_mesh_view_mips, unchanged; lod = (float)l + f.
 *  7. For i = 0 .. N - 1: o_i = (float)(2 i + 1) / (float)(2 N) - 0.5f; u_i = u + du o_i, v_i = v + dv o_i (a product, a sum);
 *     t_i = step 6 of dtp_mesh_view_mips at (u_i, v_i) with this l and f for every tap: level l + 1 is not read when f = 0, and the
 *     taps clamp at the level's border as they do there.
 *  8. t = (((t_0 + t_1) + t_2) + ... + t_(N-1)) / (float)N per channel, all four channels, plain: the same non-weighted rule as the bilinear
 *     blend and the level blend, so a tap on an unpainted texel pulls colour and alpha towards 0 as a bilinear tap does.
 *  9. The shade, the unpainted mix, the byte conversion and the background are dtp_mesh_view's.
 * What follows from the rule: M = 1 gives rho2 = pmax2, N = 1 and o_0 = 0, so image, lod, face_idx and depth are dtp_mesh_view_mips'
 * byte for byte; where pmax2 <= 1 (magnified) N = 1, l = 0, f = 0 and the pixel is dtp_mesh_view's; where la2 == lb2 >= 1 the pixel is
 * the trilinear one; visibility, face_idx and depth never depend on the filter.  Not here: elliptical (EWA) weights, the true axes of a
 * sheared footprint (the longer of the two screen-axis vectors is the major axis), an alpha-weighted tap average.
 *
 * dtp_mesh_view_aniso: the arguments, checks, buffers and launches (a memset and four kernels) of dtp_mesh_view_aa with the filter
 * implied: mips is required (it may be NULL only when the layout has 1 level), clip in {0, 1}, samples in {1, 2, 4} with the fine
 * frame's rules (the footprint is measured between neighbouring FINE pixels), plus max_aniso in 1..16 (DTP_ERR_ARG outside, naming the
 * range) and taps: device u8 [H][W] or NULL, the N of the pixel (of the sample that stores face_idx, depth and lod), 0 where no face
 * is.  Every check comes before any device call and a refused call writes nothing.  max_aniso 1 is legal and runs this entry's own
 * kernels. */
int dtp_mesh_view_aniso(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                        const dtp_view_opts* opts, int clip, int samples, int max_aniso, uint8_t* image, int* face_idx, float* depth,
                        float* lod, uint8_t* taps, uint8_t* coverage, dtp_stream s);

/* ---------------------------------------------------------------- face sets: a lasso, masked strokes, a tint
 * Protecting part of a mesh from a stroke (Blender's "face selection masking").  A stamp writes every texel of every
 * visible face in its window; the [R][R] paste mask lives in stamp space and knows no face.
 *
 * A FACE SET of a mesh of F faces is (F + 31) / 32 32-bit words on the mesh's device, 4-byte aligned: bit f % 32 of word f / 32 is face
 * f.  It is the caller's memory and no object of this library.  Every kernel here ignores the bits at positions >= F of the last word,
 * so the complement of a set, word by word, is a set; union and intersection are OR and AND of the words.
 *
 * dtp_mesh_select: the faces a frame shows inside a polygon.  face_idx: device i32 [H][W] as a view writes it (-1: no face; with samples
 * > 1 the face of the sample that stores it), 1 <= H, W <= 4096.  polygon: host float [n][2], (x, y) in the frame's pixel coordinates, the
 * convention of dtp_view_rays: the centre of pixel (row i, column j) is (j + 0.5, i + 0.5); 3 <= n <= 1024 and every coordinate finite.
 * A rectangle is a polygon of four vertices.  The rule, in integers past the first step:
 *  1. Each vertex is snapped on the host by the raster's snap: X = snap(256.0f * x), Y = snap(256.0f * y) in fp32, snap = rintf clamped
 *     to +-2^26.  The centre of pixel (i, j) is P = (256 j + 128, 256 i + 128).
 *  2. P is inside by the even-odd rule over the n edges (a, b) = (vertex k, vertex (k + 1) mod n), in int64: an edge counts iff
 *     (a.y > P.y) != (b.y > P.y) and P lies strictly left of the edge's crossing of P's row, i.e.
 *     D = (P.x - a.x)(b.y - a.y) - (P.y - a.y)(b.x - a.x) is not zero and D < 0 exactly when b.y - a.y > 0.  P is inside iff an odd
 *     number of edges count.  (Every difference is below 2^27 + 2^20 and every product below 2^55.)  A horizontal edge never counts, a
 *     centre ON an edge or a vertex is decided by the strict comparisons, and a self-intersecting polygon follows even-odd.
 *  3. Face f is hit iff 0 <= f < F and f == face_idx[i][j] at one or more inside pixels.  A face_idx value outside -1 .. F - 1 is
 *     skipped, never used as an index.
 * op: DTP_SELECT_REPLACE: `out` is zeroed on the stream, then the bits of the hit faces are set; DTP_SELECT_ADD: they are set;
 * DTP_SELECT_SUBTRACT: they are cleared; out: the set to write or edit, `words` = (F + 31) / 32.  The result is an OR / AND-NOT of single
 * bits and does not depend on the order of the atomics.  This selects what the user SEES: a hidden, back-facing or sub-pixel face that
 * won no pixel is not hit.  The call only enqueues on `s`: the memset of REPLACE, at most three launches that carry the snapped polygon
 * to the mesh's 8 KB buffer in their arguments, and one workgroup per 16 x 16 pixels of the polygon's pixel bounding box clipped to the
 * frame (no other tile is launched; a box without a centre launches nothing).  One select of a mesh at a time, or all on one stream.
 * Refusals, DTP_ERR_ARG before anything is enqueued: n outside 3..1024, an unknown op, a side outside 1..4096, a vertex that is not finite
 * (these four before the mesh is looked at), a NULL pointer, a mesh that is not alive, words != (F + 31) / 32, a misaligned pointer.
 *
 * dtp_mesh_stroke_masked: dtp_mesh_stroke_bleed (bleed 0: dtp_mesh_stroke) with a face set.  A face whose bit is 0 never enters the
 * backprojection's valid list: valid = front, not steep, the winner of a pixel, AND selected.  Nothing else changes: the render shows
 * the whole mesh, the stamp is the stamp it would have been, and the paste writes the texels whose centre a selected valid face covers
 * (among several the lowest index wins); an Erase stamp follows the same rule.  The texel bounding box is that of the selected valid
 * faces, so an open journal record saves less and the bleed pass runs over less; an empty list pastes nothing and is no error.  The set
 * is read on the device in stream order, once per stamp: it must stay unchanged until the stroke has run.  face_mask NULL: the call
 * dtp_mesh_stroke_bleed makes, launch for launch and byte for byte (mask_words is then ignored).  Refusals beyond that call's:
 * mask_words != (F + 31) / 32 or a misaligned face_mask, DTP_ERR_ARG before anything is enqueued.
 *
 * dtp_view_tint: shows a set on a finished frame, in place.  frame: device u8 [H][W][4]; face_idx: that frame's; set, words, F as above
 * (F is given because the call takes no mesh).  Where face_idx[i][j] is a face of the set, each of R, G, B becomes
 * (c (255 - opacity) + color[ch] opacity + 127) / 255 in integers, 0 <= opacity <= 255; alpha is untouched, and every other pixel is
 * neither read nor written.  One thread per pixel, one launch on `s`.  A pass of its own, so that no raster kernel changes.
 *
 * Not here: selecting through the mesh (hidden faces), texel-space stencils and the 2D dtp_stroke, an outline instead of a tint, a wire
 * message.  (Growing a set to whole UV charts or by connectivity: the next section.) */
#define DTP_SELECT_REPLACE 0
#define DTP_SELECT_ADD 1
#define DTP_SELECT_SUBTRACT 2
int dtp_mesh_select(dtp_mesh* mesh, const int* face_idx, int H, int W, const float* polygon, int n, int op, uint32_t* out, int words,
                    dtp_stream s);
int dtp_mesh_stroke_masked(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n,
                           const dtp_settings* st, const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed,
                           const uint32_t* face_mask, int mask_words, dtp_stream s);
int dtp_view_tint(dtp_ctx* ctx, uint8_t* frame, const int* face_idx, int H, int W, const uint32_t* set, int words, int F,
                  const uint8_t color[3], int opacity, dtp_stream s);

/* ---------------------------------------------------------------- growing a face set
 * The lasso selects what a frame shows; what a painter means is "this chart", "this piece" or "what I circled plus a border" (DESIGN.md
 * 3.33; Blender's select more / less, select linked, select UV island).  The growth runs on the device, in stream order, so that lasso ->
 * extend -> masked stroke needs no synchronise.
 *
 * THE TOPOLOGY of a mesh is exact; no step uses a tolerance.
 *  - Points.  The key of a vertex is the bit pattern of its three fp32 coordinates with -0.0 taken as +0.0; vertices with equal keys are
 *    one point, named by the LOWEST vertex index that carries the key.  point[f][k] is the point of faces[f][k], a value in 0 .. V - 1.
 *    (This welds meshes whose vertices are split along UV seams.)
 *  - Parts.  Two faces are neighbours when they share a point; a part is a class of the transitive closure, and part[f] is the LOWEST
 *    face index of the class of f.
 *  - Charts.  Two faces are chart-neighbours when they share an edge -- the same unordered pair of two DIFFERENT points -- and at both
 *    points of it the UV each face carries there is equal (fp32, component-wise, -0.0 == +0.0).  An edge shared by more than two faces
 *    unites every pair whose UVs agree; a side of zero length is no edge.  chart[f] is the lowest face index of the class of f.  A chart
 *    never spans two parts.
 * dtp_topology_build (host only, like dtp_mesh_path_plan: no device, no handle): point i32 [F][3], part i32 [F], chart i32 [F];
 * counts = {distinct points the faces use, parts, charts}.  The argument checks are dtp_mesh_create's (DTP_ERR_ARG: a NULL pointer,
 * V < 1, F outside 1..2^20, a vertex or UV that is not finite, an index outside 0 .. V - 1).
 * dtp_mesh_topology: the first call for a mesh copies its vertices, faces and UVs back on `s`, runs dtp_topology_build, allocates, uploads
 * the three label arrays and allocates the scratch of dtp_mesh_select_extend (a mark bitset of (max(V, F) + 31) / 32 words and two face
 * sets); it waits for `s` only, never for the null stream, so it does not sit behind a stroke queued elsewhere.  Later calls only return
 * the counts (counts may be NULL).  The buffers are freed with the mesh.
 * dtp_mesh_topology_labels: builds the topology if need be, copies the labels to the host on `s` and waits for `s` (for a UI's "select
 * chart k" and for tests); a NULL array is skipped.
 *
 * dtp_mesh_select_extend: out = `in` grown by `how`, both face sets of the mesh on its device.
 *  - DTP_EXTEND_RINGS, `rings` times: add every face that shares a point with a face of the set.
 *  - DTP_EXTEND_SHRINK, `rings` times: drop every face of the set that shares a point with a face (< F) outside it.  An open border is
 *    no outside face: the full set stays full.
 *  - DTP_EXTEND_LINKED: every face of every part the set touches (the fixed point of RINGS).
 *  - DTP_EXTEND_CHARTS: every face of every chart the set touches.
 * Bits of `in` at positions >= F are ignored and bits of `out` there are written as 0; the empty set stays empty in every mode.
 * in == out is allowed, otherwise the two must not overlap.  rings is 1..64 for RINGS and SHRINK and ignored for the others.  One step
 * is three launches on `s` -- clear the mesh's mark bitset, mark (one thread per face: a face of the source, for SHRINK a face outside
 * it, ORs the bits of its three points, its part or its chart), gather (one thread per face tests its labels' marks; the 64 bits of a
 * wave leave as two word stores, each thread having read the source word of its own face before) -- so a call enqueues at most 3 x 64
 * launches, the steps before the last writing the mesh's two scratch sets in turn.  The result is an OR of single bits and does not
 * depend on the order of the atomics.  The call checks everything and then only enqueues: no host round trip and no allocation, except
 * at the mesh's first use, which builds the topology as dtp_mesh_topology does.  It reads only the topology and the two sets, so it runs
 * beside a stroke, a pick, a view or a lasso of the same mesh; one extend of a mesh at a time, because the scratch is the mesh's.
 * Refusals, DTP_ERR_ARG before anything is enqueued: an unknown how, rings outside 1..64 with RINGS or SHRINK (these two before the mesh
 * is looked at), a NULL pointer, a mesh that is not alive, words != (F + 31) / 32, a pointer that is not 4-byte aligned, `in` and `out`
 * that overlap without being equal.
 *
 * Not here: a flood by dihedral angle ("select flat": a loop whose length the host cannot know), rings by edge adjacency, selecting
 * through the mesh, an outline, a wire message. */
#define DTP_EXTEND_RINGS 0
#define DTP_EXTEND_SHRINK 1
#define DTP_EXTEND_LINKED 2
#define DTP_EXTEND_CHARTS 3
int dtp_topology_build(const float* vertices, int V, const int* faces, int F, const float* face_uvs, int* point, int* part, int* chart,
                       int counts[3]);
int dtp_mesh_topology(dtp_mesh* mesh, int counts[3], dtp_stream s);
int dtp_mesh_topology_labels(dtp_mesh* mesh, int* point, int* part, int* chart, dtp_stream s);
int dtp_mesh_select_extend(dtp_mesh* mesh, const uint32_t* in, uint32_t* out, int words, int how, int rings, dtp_stream s);

/* ---------------------------------------------------------------- occlusion in the backprojection
 * The render of a stamp decides visibility per pixel, the backprojection per face: a valid face (front, not steep, the winner of at
 * least one pixel) is backprojected whole, so a large face that is only partly visible -- a floor under a table, a wall behind a pillar
 * -- receives the stamp on the texels that lie behind the other face as well, and the pixels it samples there show the occluder
 * (DESIGN.md 3.32).  dtp_mesh_stroke_occluded tests every tap of every texel.  No depth buffer: the per-face records of the stamp's
 * projection and its face_idx are on the device already.  fp32, one rounded operation at a time in the order written, no contraction;
 * nothing is compared under a tolerance but the one the caller gives.
 *
 * occlude: a tolerance in stamp pixels, finite and >= 0.  On the host tol = ((occlude 2) fov) / R in double from the fp32 occlude and
 * fov, rounded to fp32 once: the depth, in camera units, of `occlude` pixel widths of a window that spans 2 fov camera units over R pixels.
 * Per texel the winner face f and the four taps of the stamp image are the backprojection's, unchanged.  For tap i at pixel (x_i, y_i) of
 * the window, g = face_idx[y_i][x_i].  If g is a face of the mesh (0 <= g < F; -1 and any other value are skipped, never used as an
 * index) and g != f: both faces' planes are evaluated at the tap's pixel centre c_i = (256 x_i + 128, 256 y_i + 128) with NO inside test --
 * w_k = (float)E_k / (float)|A| from the same sign-normalised int64 edge functions of the face's snapped window triangle as the
 * coverage's, z = (w0 z0 + w1 z1) + w2 z2 of the vertices' camera z -- giving z_g and z_f.  The tap is REJECTED iff (z_g - z_f) > tol: one
 * fp32 subtraction, one comparison; a NaN compares false and does not reject.  Larger camera z is nearer: a rejected tap shows a face in
 * front of f's plane by more than the tolerance.  (g won a pixel and f is valid, so it won one too: neither triangle has a zero
 * area; a record that has one, at op level, does not reject.)  The tap's mask byte plays no part in the test.
 * A texel none of whose taps is rejected is computed by the backprojection's arithmetic, operation for operation.  Otherwise the weight
 * of every rejected tap becomes 0; S = ((w00' + w01') + w10') + w11'; if !(S > 0) the texel is not written; a = blend'(alpha_i) / S with
 * alpha_i = (mask != 0 && face_idx != -1) as always and blend' the same expression over the weights left, and if !(a > 0) the texel is not
 * written; each colour is blend'(d_i) / S, an fp32 division; the bytes are then formed as always, (unsigned char)(min(v, 1) * 255.0f).
 * An ERASE stamp follows the same written / not written rule.  The weights are renormalised because a rejected tap has to leave the
 * colour as well as the alpha; and the tolerance cannot be 0, because two faces that share an edge differ at a centre near that edge by
 * the distance to the edge times the difference of their slopes: 1 pixel absorbs a slope difference of about 0.7 between neighbours.
 *
 * dtp_mesh_stroke_occluded: dtp_mesh_stroke_masked (face_mask NULL: dtp_mesh_stroke_bleed; bleed 0: dtp_mesh_stroke) whose every stamp,
 * ERASE stamps included, runs the occluded instantiation of the backprojection kernel with the tol of that stamp's fov.  The render, the
 * stamp, the valid list, the texel bounding box, the journal and the bleed pass are unchanged; a texel the test leaves unwritten inside
 * the box is saved by an open journal record and restored like any other.  Refusals beyond that call's, DTP_ERR_ARG before anything is
 * enqueued and with the texture untouched: an occlude that is negative or not finite (checked with `bleed`, before the handles are looked at, naming "occlude"), a stamp whose tol
 * does not fit fp32 (naming the stamp).  The entry points above never run the test: their launches and bytes are what they were.
 * Not here: a configurable steepness threshold or an angle falloff (the per-face record has no room for the normal), occluders that
 * belong to another mesh, a count of rejected texels in dtp_last_stroke_info, any change to what the stamp itself sees. */
int dtp_mesh_stroke_occluded(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n,
                             const dtp_settings* st, const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed,
                             const uint32_t* face_mask, int mask_words, float occlude, dtp_stream s);

/* ---------------------------------------------------------------- undo / redo journal of a texture
 * Taking a stroke back without the host.  The reference copies the whole texture to the host before every stroke, keeps
 * the last 10 copies and uploads one on Ctrl+Z (kit_app/.../python/ui/brush.py:52-77,131-137; redo is a TODO there).  A journal keeps, on
 * the device, the old bytes of the 16 x 16-texel tiles a stroke is about to write, and swaps them back: undo and redo, exact bytes.
 *
 * Tiles.  Tile t = (i / 16) * ceil(W / 16) + (j / 16) holds the texels of rows 16 (i / 16) .. + 15 and columns 16 (j / 16) .. + 15 that
 * lie inside the texture; a slot is 1 KiB = 256 RGBA texels.  An edge tile of an H or W that is no multiple of 16 saves and restores
 * only its texels inside the texture.
 *
 * dtp_journal_create: texture is the device pointer the journal guards, u8 [H][W][4], 4-byte aligned, 1 <= H, W <= 32768; capacity_tiles
 * >= 1 slots; depth in 1..64 the most records kept (the reference's is 10).  It allocates all the journal will ever need -- the slots,
 * one i32 per tile, one i32 per slot, the counters (capacity_tiles KiB + 4 bytes per tile and per slot) -- and belongs to its handle:
 * dtp_destroy frees the journals still alive; dtp_journal_destroy(NULL) is a no-op.  A pointer that is not a live journal is
 * DTP_ERR_ARG in every call here: refused, not followed.
 *
 * Records.  dtp_journal_begin opens a record and dtp_journal_end closes it; a stroke may arrive in several calls in between.  While a
 * record is open, every dtp_stroke, dtp_mesh_stroke and dtp_mesh_stroke_bleed call on that handle whose texture, H and W are the
 * journal's saves the tiles it may write before it writes them, on the stroke's stream, which must be the stream of begin:
 *   2D stroke, per group   every tile that meets a window of the group clipped to the texture, or with `wrap` a wrapped piece of it (the
 *                          paste mask is not consulted);
 *   mesh stamp             every tile that meets the texel bounding box of the stamp's valid faces, as the device has it after the valid
 *                          pass, grown by `bleed` and clipped; saved between the valid pass and the backprojection; an empty box saves
 *                          nothing; the host reads nothing.
 * A tile is saved once per record, however many stamps, groups, windows or wrapped pieces meet it.  A call on another texture, H or W is
 * not journalled and is no error.  With no record open the three calls enqueue exactly the launches they always did.  A journalled
 * stroke writes the bytes an unjournalled one writes.  dtp_journal_touch saves the tiles of n rectangles, host int[n][4] inclusive
 * {x0, y0, x1, y1} clipped to the texture, into the open record: for a client that writes the texture itself (dtp_mesh_bleed, a fill,
 * an upload).  begin, end, touch and the saves of the stroke calls never wait and never allocate.
 *
 * Storage.  The slots form a ring: a 64-bit device counter `head` only grows, and the k-th slot ever taken is slot k mod
 * capacity_tiles.  begin stamps start = head into the record and end stamps end = head, on the device.  A record is restorable iff
 * head - start <= capacity_tiles: nothing has landed on its first slot.  So a record larger than the capacity is not restorable, and a
 * small ring forgets its oldest records first; painting is never blocked or refused because the journal is full.
 *
 * Undo / redo.  The records form a list, oldest first, with a cursor: records [0, cursor) are applied, [cursor, records) undone.
 * dtp_journal_undo takes the newest applied record and SWAPS each of its slots with its tile: the texture's texels are then what they
 * were at that record's begin, and the slots hold the painted state.  dtp_journal_redo swaps the oldest undone record back: the texture
 * is then, byte for byte, what it was at that record's end.  begin drops all undone records (their redo is gone); head is NOT rewound, so
 * their slots stay taken until the ring comes round to them.  When `depth` records exist, begin drops the oldest.  undo, redo,
 * dtp_journal_info with a non-NULL head, dtp_journal_record_info and dtp_op_journal_tiles wait for the stream (info: the stream the
 * journal was used on last) and read a few words back; they run at a user's Ctrl+Z, not inside a stroke.
 *
 * Refusals, all before anything is enqueued; a refused call leaves the texture and the journal untouched.  DTP_ERR_ARG: a NULL pointer;
 * H or W outside 1..32768; a misaligned texture; capacity_tiles < 1; depth outside 1..64; a journal that is not alive; in touch n < 1 or
 * a rectangle with x0 > x1 or y0 > y1, naming it.  DTP_ERR_STATE: begin with a record open on this journal or on another journal of the
 * handle; end or touch with none open; undo or redo with a record open, with nothing to undo / redo ("nothing to undo", "nothing to
 * redo"), or of a record that is no longer restorable: the message says it was overwritten and gives the record's tiles and the
 * capacity, and that record and every older one are dropped.
 *
 * dtp_journal_info: the number of records, the cursor, whether a record is open, and head; any pointer may be NULL.
 * dtp_journal_record_info: start, end (of an open record: head) and restorable of record 0 <= record < records.
 * dtp_op_journal_tiles: the tile indices a restorable record saved, in slot order, into host tiles[max]; *n = their number (more than
 * max: DTP_ERR_ARG, nothing written).  dtp_journal_window_tiles (host only, no device): the ascending tile list of ONE 2D stroke window
 * at (x, y) by the rule above, 1 <= R <= min(H, W); *n = its length (more than max: DTP_ERR_ARG, nothing written; tiles may be NULL
 * with max = 0). */
typedef struct dtp_journal dtp_journal;
int dtp_journal_create(dtp_ctx* ctx, uint8_t* texture, int H, int W, int capacity_tiles, int depth, dtp_journal** out);
int dtp_journal_destroy(dtp_journal* j);
int dtp_journal_begin(dtp_journal* j, dtp_stream s);
int dtp_journal_end(dtp_journal* j, dtp_stream s);
int dtp_journal_touch(dtp_journal* j, const int* rects, int n, dtp_stream s);
int dtp_journal_undo(dtp_journal* j, dtp_stream s);
int dtp_journal_redo(dtp_journal* j, dtp_stream s);
int dtp_journal_info(dtp_journal* j, int* records, int* cursor, int* open, uint64_t* head);
int dtp_journal_record_info(dtp_journal* j, int record, uint64_t* start, uint64_t* end, int* restorable);
int dtp_op_journal_tiles(dtp_journal* j, int record, int* tiles_host, int max, int* n);
int dtp_journal_window_tiles(int H, int W, int R, int wrap, int x, int y, int* tiles, int max, int* n);

/* ---------------------------------------------------------------- changed tiles of an image
 * What a client in another process needs to keep a mirror of a painted texture or of a rendered frame current.  The
 * reference pushes the whole texture to the viewport after every stamp (kit_app/.../python/manager.py:349-354); here the device finds the
 * 16 x 16-texel tiles whose bytes changed since the client last got them, by comparison against a shadow copy the tracker owns, and
 * only those tiles cross to the host.  Comparison catches every writer -- strokes, the bleed pass, undo and redo, a torch write, a
 * re-rendered frame -- without any of them knowing, and a change that was changed back costs nothing.  Exact bytes; no tolerance.
 *
 * Image.  Any contiguous u8 [H][W][4] image on the handle's device, 1 <= H, W <= 16384, 4-byte aligned (no more is assumed).  The tracker
 * is made for a shape, not for a pointer: every scan names its image.
 *
 * Tiles.  The journal's tiles and numbers: tile t = (i / 16) * ceil(W / 16) + (j / 16); a payload is 1 KiB = 256 RGBA texels, row-major,
 * 64 bytes per row.
 *
 * dtp_delta_create makes a tracker for (ctx, H, W, capacity_tiles >= 1) and allocates all it will ever need, as dtp_delta_layout lists
 * it: a shadow image (H W 4 bytes), one stale mark per tile, one flag per tile and a count and a base per group of 64 tiles, the device
 * outputs ids i32 [capacity], tiles u8 [capacity][1024] and counts i32 [2], and one pinned host block (16 bytes that receive counts,
 * then ids, then tiles, at host_ids_offset and host_tiles_offset; dtp_delta_host gives the two addresses).  A tracker belongs to its
 * handle: dtp_destroy frees the trackers still alive; dtp_delta_destroy(NULL) is a no-op.  A pointer that is not a live tracker is
 * DTP_ERR_ARG in every call here: refused, not followed.
 *
 * State.  A new tracker has every tile stale.  dtp_delta_reset marks every tile stale again with one memset in stream order: for a
 * client that reconnected with an empty mirror.
 *
 * dtp_delta_scan(ctx, tracker, image, H, W, s).  A tile is CHANGED iff it is stale or any byte of it inside the image differs from the
 * shadow.  With total = the number of changed tiles and emitted = min(total, capacity), the scan writes the first `emitted` changed tiles
 * in ascending tile order: ids[k] = the tile, tiles[k] = its 1 KiB with the texels outside the image zero, counts = {emitted, total -
 * emitted}.  Slots from `emitted` on keep what they held.  For the emitted tiles, and only for those, the shadow takes the image's
 * bytes and the stale mark is cleared: a capped scan loses nothing and the next one goes on with the next tiles in order; a key frame is
 * the same call on a fresh (or reset) tracker.  The output does not depend on scheduling: a slot is the tile's rank in ascending order,
 * never claimed with an atomic counter.  It only ENQUEUES on `s`, three launches (flag the tiles and count per group of 64; one
 * workgroup scans the group counts and writes counts; gather), none of which waits for another workgroup.  Texels of an edge tile that
 * lie outside the image are neither read nor compared.  Scans of one tracker must be ordered with each other (one stream, or events).
 *
 * dtp_delta_device gives the device addresses of ids, tiles and counts, valid for the tracker's life, holding what the last scan wrote
 * once that scan has run.  dtp_delta_host gives the addresses of ids and tiles inside the pinned block.
 *
 * dtp_delta_pull is the scan and the read-back: it enqueues the scan, copies the 8 bytes of counts into the pinned block and waits for
 * `s`, then copies ids[:count] into host_ids and tiles[:count] into host_tiles (host memory with room for max_tiles tiles; the pinned
 * block's addresses are the fast choice) and waits again; *count = emitted, *remaining = total - emitted.  Nothing is copied when count
 * is 0.  max_tiles below the tracker's capacity is refused before any device work.
 *
 * Refusals, every one before the first device call and with every output left alone, DTP_ERR_ARG: a NULL pointer; H or W outside
 * 1..16384; capacity_tiles < 1; a tracker that is not alive, or that belongs to another handle; an image whose H, W are not the
 * tracker's, or that is not 4-byte aligned; max_tiles below the capacity.
 *
 * dtp_delta_layout (host only): the tiles in x and y, their number, the groups of 64, and the byte size of every buffer above. */
typedef struct dtp_delta dtp_delta;
typedef struct {
  int tiles_x, tiles_y, n_tiles, n_groups, capacity;
  uint64_t shadow_bytes, stale_bytes, flag_bytes, group_bytes, ids_bytes, tiles_bytes, counts_bytes;
  uint64_t host_ids_offset, host_tiles_offset, host_bytes;
} dtp_delta_sizes;
int dtp_delta_layout(int H, int W, int capacity_tiles, dtp_delta_sizes* out);
int dtp_delta_create(dtp_ctx* ctx, int H, int W, int capacity_tiles, dtp_delta** out);
int dtp_delta_destroy(dtp_delta* d);
int dtp_delta_reset(dtp_delta* d, dtp_stream s);
int dtp_delta_scan(dtp_ctx* ctx, dtp_delta* d, const uint8_t* image, int H, int W, dtp_stream s);
int dtp_delta_device(dtp_delta* d, int** ids, uint8_t** tiles, int** counts);
int dtp_delta_host(dtp_delta* d, int** ids, uint8_t** tiles);
int dtp_delta_pull(dtp_ctx* ctx, dtp_delta* d, const uint8_t* image, int H, int W, dtp_stream s, int* host_ids, uint8_t* host_tiles,
                   int max_tiles, int* count, int* remaining);
/* the tracker's shadow and stale marks copied to host memory (u8 [H][W][4] and u8 [n_tiles]; either may be NULL), for the kernel
 * tests: waits for `s` */
int dtp_op_delta_state(dtp_delta* d, uint8_t* shadow_host, uint8_t* stale_host, dtp_stream s);

/* Host-only: the DDIM tables dtp_stamp uses for `steps` inference steps -- timesteps[steps] (descending,
 * +1 offset), alphas_cumprod gathered at those timesteps, and final_alpha_cumprod
 * (DDIMScheduler.set_timesteps/configure, utilities.py:408-439).  Any pointer may be NULL. */
int dtp_ddim_tables(int steps, int64_t* timesteps, float* alphas, float* final_alpha);

/* Samplers of the stamp loop (dtp_set_option "scheduler"), the reference's names (stable_diffusion_pipeline.py:115-127):
 *   DTP_SCHED_DDIM  DDIMScheduler, eta 0, steps_offset 1 (utilities.py:370-529): E = steps - 1 evaluations
 *   DTP_SCHED_DPM   DPMScheduler: DPM-Solver++ multistep, order 2, midpoint, first order at the last evaluation when steps < 15
 *                   (utilities.py:649-1008): E = steps
 *   DTP_SCHED_LMSD  LMSDiscreteScheduler: linear multistep in sigma space (utilities.py:267-367): E = steps */
#define DTP_SCHED_DDIM 0
#define DTP_SCHED_DPM 1
#define DTP_SCHED_LMSD 2
#define DTP_SCHED_ROW 8 /* floats per evaluation in the coefficient table */
/* Host-only: everything a stamp needs for (scheduler, steps), steps 2..999.  Outputs (any pointer may be NULL):
 *   evals        E, the number of UNet evaluations
 *   init_sigma   init_noise_sigma (the initial latents are latents * init_sigma): 1 for DDIM / DPM, sigma_max for LMSD
 *   timesteps    f32 [E] the UNet's timestep input per evaluation (LMSD's are not integers)
 *   in_scale     f32 [E + 1] scale_model_input of the latent channels before evaluation i (entry E = 1: no evaluation follows)
 *   coefs        f32 [E][DTP_SCHED_ROW], unused entries 0:
 *     DDIM  sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev)                     x0 = (x - [0] e) / [1]; x' = [2] x0 + [3] e
 *     DPM   alpha_s, sigma_s, order (1 | 2), sigma_t / sigma_s, alpha_t (exp(-h) - 1), 0.5 alpha_t (exp(-h) - 1), 1 / r0
 *           m0 = (x - sigma_s e) / alpha_s;  x' = [3] x - [4] m0 (order 1)  or  [3] x - [4] m0 - [5] [6] (m0 - m_prev) (order 2)
 *     LMSD  sigma_i, order (1..4), c_0 .. c_3 (c_j = exact integral over [sigma_i, sigma_i+1] of the Lagrange basis polynomial of
 *           sigma_{i-j} on sigma_i .. sigma_{i-order+1})          d_i = (x - x0) / sigma_i, x0 = x - sigma_i e;  x' = x + sum c_j d_{i-j}
 * The DDIM rows are the values dtp_stamp has always used (from dtp_ddim_tables).  DTP_ERR_ARG for an unknown scheduler or steps. */
int dtp_scheduler_tables(int scheduler, int steps, int* evals, float* init_sigma, float* timesteps, float* in_scale, float* coefs);

/* Host-only: initialize_timesteps of (scheduler, steps) at `strength`, in double as Python computes it:
 *   init = min(int(steps * strength) + offset, steps), t_start = max(steps - init + offset, 0), evals = steps - t_start
 * (offset = steps_offset: 1 for DDIM, 0 for DPM / LMSD); noise_coefs[2] = (a, b) of the start point x = a z0 + b latents: the sampler's
 * add_noise at t_start (DDIM: sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod) at timesteps[t_start]; DPM: the same; LMSD: 1, sigma[t_start]),
 * and (0, init_sigma) at strength 1.  Evaluation i of the stamp uses row t_start - offset + i of dtp_scheduler_tables.  DTP_ERR_ARG
 * (naming "strength") for a strength outside (0, 1], NaN, or evals == 0; the dtp_scheduler_tables errors otherwise.  Any output may be NULL. */
int dtp_strength_schedule(int scheduler, int steps, double strength, int* t_start, int* evals, float* noise_coefs);

/* per-stage GPU time of the last dtp_stamp on this handle, ms (print_summary,
 * stable_diffusion_pipeline.py:486-503): [0]=pre+vae_encoder x2, [1]=denoise loop, [2]=vae decode+post.
 * Blocks until the stamp has finished. */
int dtp_last_stamp_times(dtp_ctx* ctx, float ms[3]);
/* number of UNet evaluations / kernel launches captured for the last stamp */
int dtp_last_stamp_info(dtp_ctx* ctx, int* unet_evals, int* graph_nodes);
/* UNet rows (samples) the last stamp evaluated, summed over its evaluations: sum_i (2B + tg rows of evaluation i) */
int dtp_last_stamp_unet_rows(dtp_ctx* ctx, int* rows);

/* ---------------------------------------------------------------- measurement
 * dtp_profile(ctx, 1): from now on every kernel launch of the engines is bracketed by HIP events on
 * the stream it runs on (graph replay is bypassed); dtp_profile_rows() aggregates them per kernel
 * class: kind 0-11 = gemm_kernel<BM,BN,NS> (the implicit-GEMM kernel; id = shape + 4*(NS-2), shape 0..3 =
 * 128x128 / 128x64 / 64x64 / 64x128), 12 = attention_kernel / attn_dma_kernel (self-attention), 13 = GroupNorm (stats+apply or fused),
 * 14 = layernorm, 15 = concat/elementwise, 16 = softmax_rows, 17-20 = conv_halo_kernel<8,16,64> / <8,16,128> / <8,8,64> /
 * <8,8,128> (halo-tiled 3x3 conv), 21-24 = gemm_kernel<256,128,2> / <256,128,3> / <128,256,2> / <128,256,3>,
 * 25-26 = gemm_wide_kernel<256,256> / <256,320> (8-wave wide tiles), 27 = gemm_fp8_kernel (all tiles),
 * 28-35 = gemm_kernel<BM,BN,NS,2> (the 8-wave twins of shapes 0..3 at 2 / 3 stages), 36-43 = gemm_kernel<BM,BN,3,1,LW> (4 / 8 loader
 * waves), 44 = xattn_kernel (fused cross-attention GEMM pair), 45-46 = conv_halo_kernel<8,8,64|128> with three images per workgroup,
 * 47 = lnlin_kernel (activation-stationary LayerNorm-folded Linear / GEGLU), 48-51 = convws_kernel (weight-streaming 3x3 conv:
 * three 8x8 images / one 16x16 image / an 8x16 pixel tile x 64 channels per workgroup / the same for two workgroups per CU),
 * 52 = gemmws_kernel (weight-streaming dense GEMM; DTP_EXPERIMENTAL=1 builds only), 53 = gemm_f8f8_kernel (two-operand e4m3 GEMM, option
 * "fp8_operands"; labels "f8f8 M=.. N=.. K=.."), 54 = quant8_kernel (its e4m3 quantise pass; labels "quant8 M=.. K=..").  flops/bytes are ALGORITHMIC (unpadded 2*M*N*K; each operand once in fp16).
 * dtp_profile(ctx, 0) switches back to graph replay.  The nvtx/cudaEvent hooks of
 * stable_diffusion_pipeline.py:146-149,486-503 are the reference counterpart. */
typedef struct { int kind; int launches; double ms; double flops; double bytes; } dtp_prof_row;
int dtp_profile(dtp_ctx* ctx, int enable);
int dtp_profile_rows(dtp_ctx* ctx, dtp_prof_row* rows, int max_rows, int* n_rows);
/* one CSV line per recorded launch: kind,us,tflops,algo_GBps,label */
int dtp_profile_dump(dtp_ctx* ctx, const char* path);
/* options: "scheduler" (default DTP_SCHED_DDIM): the sampler of the stamp loop, DTP_SCHED_DDIM | DTP_SCHED_DPM | DTP_SCHED_LMSD (any
 * other value: DTP_ERR_ARG); may be set at any time and takes effect from the next stamp, which rebuilds the schedule tables once (a
 * host-blocking wait, like a change of steps).  No sampler history carries over between stamps (set_timesteps runs on every infer,
 * stable_diffusion_pipeline.py:349).  "use_graph" (default 1): replay captured hipGraphs; "autotune" (default 1): time tile x split-K candidates per
 * contraction shape when a launch program is built; "check_finite" (default 0): after every stamp ONE reduction over the
 * final latents and the decoded image looks for NaN/inf (the reference asserts `not isnan` after every step with a host
 * sync each, stable_diffusion_pipeline.py:415) -- read the verdict with dtp_last_stamp_finite; "fp8_attention" / "fp8_linear"
 * (default 0): the UNet's self-attention / its transformer Linears and 1x1 convs (proj_in, q/k/v, to_out, GEGLU FFN,
 * ff.net.2 + proj_out) run on the fp8 (e4m3) MX MFMA -- BASELINE configs[4]; choose before the first stamp.  A PARITY-ONLY option, not a
 * performance path: every fp8 operand carries a calibrated power-of-two scale (an amax pass over the first evaluation of a launch
 * program, before it is captured; weights per tensor at load time) and the 256^2 / 8-step stamp stays inside the 1e-2 pixel gate on
 * both synthetic weight sets, but in three rounds of measurements it was never faster than fp16 on this chip: the
 * activations arrive in fp16 and are converted on the way into LDS.  "fp8_operands" (default 0; choose before the first UNet program is
 * built, DTP_ERR_STATE after): q/k/v, attn1.to_out and the GEGLU ff.net.0 of the C = 1280 transformer blocks (every Linear with K >= 1280
 * except proj_in and the merged ff.net.2 / proj_out) contract two e4m3 operands on gemm_f8f8_kernel: the activation is written as e4m3 by
 * a quantise pass (LayerNorm'd first, fixed scale; to_out's input with a calibrated scale); takes precedence over "fp8_linear" there.
 * PARITY-ONLY as well: inside the 1e-2 pixel gate (6.4e-3 at 64^2 x 8), but 0.9 % SLOWER at batch 8 and 1.8 % at batch 1 than fp16
 * (profiles/fp8_operands_ab.txt).  "fuse_gn_conv" exists only in DTP_EXPERIMENTAL=1 builds. */
int dtp_set_option(dtp_ctx* ctx, const char* name, int value);
/* *finite = 1 if the last stamp (run with "check_finite" on) produced only finite values, 0 otherwise.  Blocks until that
 * stamp has finished; DTP_ERR_STATE if the option was off. */
int dtp_last_stamp_finite(dtp_ctx* ctx, int* finite);

/* ---------------------------------------------------------------- kernel-level entry points
 * The individual HIP kernels behind the engines, exposed so each can
 * be parity-tested and profiled on its own.  All pointers are device memory; fp16 activations
 * are NHWC ("tokens x channels", row stride ld in elements). */
typedef struct {
  const void* A;     /* f16 activations: [M][lda], or NHWC image when conv=1 */
  const void* W;     /* f16 packed weights [>=roundup(N,128)][ldw] (dtp_op_pack_*) */
  void* C;           /* f16 [M][ldc] (f32 when flags & DTP_GF_OUT_F32) */
  const float* bias; /* f32 or NULL */
  const void* R;     /* f16 residual [M][ldr] or NULL */
  int M, N, K;       /* conv: K = 9*Cin */
  int lda, ldw, ldc, ldr;
  int conv, Hi, Wi, Ho, Wo, Cin, stride, pad, upsample2x;
  int flags;         /* DTP_GF_* */
  int tile;          /* -1 = heuristic; gemm_kernel: shape + 4*(stages-2), shape 0:128x128 1:128x64 2:64x64 3:64x128 (MxN),
                        stages 2..4; 12..15 = conv_halo_kernel (8x16|8x8 pixel tile) x (64|128 channels), needs Wcb;
                        16..19 = gemm_kernel 256x128 (2|3 stages), 128x256 (2|3 stages);
                        20 / 21 = gemm_wide_kernel 256x256 / 256x320 (8 waves; unsplit, N % 8 == 0; 21: no GEGLU);
                        24..28 = gemm_fp8_kernel 128x128 / 128x64 / 64x64 / 64x128 / 256x256 (8 waves) (needs W8; dense, unsplit);
                        32..39 = gemm_kernel with EIGHT waves on shape (id & 3), 2 + (id - 32) / 4 stages: waves 4-7 multiply the
                        second half of every k-block and the halves are summed through LDS (same features as ids 0..11);
                        40..47 = gemm_kernel on shape (id & 3), 3 stages, with 4 (40..43) or 8 (44..47) extra DMA-only loader waves;
                        48 / 49 = conv_halo_kernel 8x8 x (64|128) with the same pixel tile of THREE consecutive images per
                        workgroup (image count % 3 == 0, needs Wcb);
                        50 = lnlin_kernel: DTP_GF_LNFOLD (+ BIAS, GEGLU) with K = 320 or 640, statistics computed in-kernel
                        (st_in ignored); `splits` = column ranges per 128-row block (default 4);
                        51 .. 54 = convws_kernel (weight-streaming 3x3 conv, needs Wfr): 51 = 8x8 images in groups of three (image
                        count % 3 == 0), 52 = 16x16 images, 53 = 8x16 pixel tiles of images with H % 8 == 0, W % 16 == 0 and two
                        n-tiles (64 output channels) per workgroup, 54 = 53 built for two co-resident workgroups per CU; stride 1, pad 1, Cin % 64 == 0 (Cin2 % 64 == 0); `splits` =
                        K-slices (ranges of whole 64-channel blocks);
                        56 / 57 = the phase build of 53 / 54 for upsample2x convs (needs Wfr4): four 2x2 convs over the stored map, one
                        per output parity -- Ho = 2 Hi, Wo = 2 Wi, Hi % 8 == 0, Wi % 16 == 0, no A2, unsplit (dtp_op_conv_ws_supported);
                        the phase weights are not in this struct: such a launch goes through dtp_op_conv_ups4 */
  int splits;        /* 0 = heuristic; >=1 = forced split-K factor (conv_halo_kernel: slices are whole 64-channel blocks) */
  const float* lns;  /* DTP_GF_LNFOLD: row sums of the packed weights (dtp_op_rowsum) */
  float ln_eps;
  const void* A2;    /* conv only: fused 1x1-shortcut tail, f16 [M][lda2] with Cin2 channels appended to K (W = [W3x3 | W1x1]) */
  int lda2, Cin2;
  const void* Wcb;   /* 3x3 conv: channel-block-major packing (dtp_op_pack_conv_cb); selects conv_halo_kernel when tile = 12..15 */
  int batch;         /* grouped dense problems (0/1 = one): problem b reads A + b*a_bs, W + b*w_bs, R + b*r_bs, bias + b*bias_bs,
                        lns + b*lns_bs and writes C + b*c_bs (strides in elements) */
  int64_t a_bs, w_bs, c_bs, r_bs;
  int bias_bs, lns_bs;
  int sm_valid;      /* DTP_GF_SOFTMAX16: softmax over the first sm_valid columns of every aligned group of 16; the rest -> 0 */
  float* st_out;     /* DTP_GF_ROWSTATS: per-row (sum, sum of squares) of the fp16 output, one partial per N tile: f32
                        [ceil(N / tile columns)][M][2] (room for ceil(N/64) partials is always enough) */
  const float* st_in;/* DTP_GF_LNFOLD: row statistics of A handed over by its producer ([st_parts][M][2]); NULL = computed in-kernel */
  int st_parts;
  int st_parts_out;  /* written by dtp_op_gemm: number of partials per row the chosen tile emitted into st_out */
  const void* W8;    /* tile 24..28 (gemm_fp8_kernel, BASELINE configs[4]): e4m3 copy of the packed weights from dtp_op_quantize_w8,
                        [rows][ldw8] bytes, K padded to 128; with DTP_GF_LNFOLD the LayerNorm is applied while A is staged */
  int ldw8;
  float a_scale, w_scale; /* A8 = e4m3(A / a_scale), W8 = e4m3(W / w_scale) (powers of two); the product is applied to the accumulators */
  int gn_cpg;        /* DTP_GF_GNSTATS (tiles 53 / 54, unsplit): channels per group of the GroupNorm that consumes the output; st_out then
                        receives f32 [images][2 * ceil(Ho/8) * ceil(Wo/16)][N / gn_cpg][2] partial (sum, sum of squares) of the rounded
                        outputs, the input of dtp_op_groupnorm_apply.  DTP_GF_RAGGED (tiles 53 / 54): any Ho x Wo (partial 8 x 16 tiles),
                        and with upsample2x also Ho = 2 Hi - 1 / Wo = 2 Wi - 1 (the upsample cropped by its last row / column) */
  const void* Wfr;   /* 3x3 conv, tiles 51 .. 54: the weights in MFMA fragment order (dtp_op_pack_conv_ws); dense, tile 55: dtp_op_pack_linear_ws */
  /* dtp_op_gemm_f8f8 only (both operands e4m3 in memory): */
  const void* A8;    /* e4m3 activations [M][lda8] bytes = e4m3(A / a_scale) (dtp_op_quant_e4m3) */
  int lda8;
  const void* A2_8;  /* or NULL: e4m3 [M][lda2_8] supplying the LAST Cin2 columns of the contraction (same a_scale) */
  int lda2_8;
  void* C8;          /* or NULL: e4m3 output [M][ldc8] = e4m3(out / c_scale), quantised from the fp16-rounded output; C may then be NULL */
  int ldc8;
  float c_scale;
  float a2_scale;    /* scale of A2_8 (0 = a_scale); a different power of two needs (K - Cin2) % 128 == 0 */
} dtp_gemm_desc;
enum { DTP_GF_BIAS = 1, DTP_GF_BIAS_M = 2, DTP_GF_RESID = 4, DTP_GF_GEGLU = 8, DTP_GF_GELU = 64, DTP_GF_QUICKGELU = 128,
       DTP_GF_OUT_F32 = 256, DTP_GF_SILU = 512, DTP_GF_LNFOLD = 1024, DTP_GF_ROWSTATS = 2048, DTP_GF_SOFTMAX16 = 4096,
       DTP_GF_GNSTATS = 1 << 24, DTP_GF_RAGGED = 1 << 25 };

int dtp_op_gemm(dtp_gemm_desc* d, dtp_stream s);
/* Two-operand e4m3 GEMM (gemm_f8f8_kernel; option "fp8_operands" runs it): C = epilogue(a_scale * w_scale * A8 . W8^T) with A8 / A2_8 / W8
 * (d->W8, d->ldw8, d->w_scale from dtp_op_quantize_w8) all e4m3 bytes moved by LDS-DMA, on the MX MFMA.  Epilogues (d->flags): DTP_GF_BIAS,
 * DTP_GF_RESID (f16 R), DTP_GF_GEGLU (N % 128 == 0), DTP_GF_ROWSTATS (st_out: ceil(N / 128) partials per row, d->st_parts_out), and the
 * e4m3 output C8.  M arbitrary, N % 64 == 0, K % 16 == 0 (Cin2 % 16 == 0), rows 16-byte aligned.  W8 must hold roundup(N, 128) rows and
 * ldw8 >= roundup(K, 128) columns, zero beyond N / K (dtp_op_quantize_w8 on dtp_op_pack_linear output is).  Every scale is a power of two
 * (other values: DTP_ERR_ARG).  d->tile: 0 = 128x128, 1 = 64x128, -1 = heuristic.  Values beyond +-448 * c_scale saturate; NaN stays NaN. */
int dtp_op_gemm_f8f8(dtp_gemm_desc* d, dtp_stream s);
/* The e4m3 quantise pass of option "fp8_operands" (gemm_f8f8_kernel's activation operand): y u8 [M][ldy] = e4m3(x / scale) of x f16 [M][ldx] (K columns, K % 8 == 0), with ln = 1
 * of the LayerNorm (x - mean) * rstd (no gamma / beta; mean / rstd from st_in f32 [st_parts][M][2] per-row (sum, sumsq) partials as a
 * DTP_GF_ROWSTATS producer writes them, or computed here when st_in is NULL; eps).  x2 (or NULL): a second job over the same M rows in
 * the same launch (e.g. the raw and the normalised copy of one tensor).  Saturating (+-448; NaN stays NaN), round to nearest even;
 * scales are powers of two. */
int dtp_op_quant_e4m3(const void* x, int ldx, void* y, int ldy, int K, float scale, int ln, const void* x2, int ldx2, void* y2, int ldy2,
                      int K2, float scale2, int ln2, int M, const float* st_in, int st_parts, float eps, dtp_stream s);
/* w f32 [N][K] -> out f16 [rows][ldw] (caller zero-fills out); geglu=1 applies the [a|gate] tile packing */
int dtp_op_pack_linear(const float* w, void* out, int N, int K, int ldw, int geglu, dtp_stream s);
/* one matrix through lora_refit_kernel (dtp_refit_lora's kernel): out f16 [>= roundup(row0 + N, 128)][ldw], rows row0 .. row0 + N - 1 =
 * f16((w0 + scale * up @ down) * gamma[k]) (gamma NULL = 1; rank 0 = no LoRA, up / down unused); w0 f32 [N][K], up f32 [N][rank], down
 * f32 [rank][K]; rows outside and columns >= K are not written.  K % 8 == 0, ldw % 8 == 0, ldw >= K; w0, down, gamma and out 16-byte
 * aligned.  Waits for the stream once (the launch reads a job record the next call reuses). */
int dtp_op_lora_refit(const float* w0, const float* up, const float* down, int rank, float scale, const float* gamma, void* out, int row0,
                      int N, int K, int ldw, dtp_stream s);
/* w f32 [Cout][Cin][3][3] (or 1x1) -> out f16 [rows][ldw], k = tap*Cin_pad + ci (caller zero-fills out) */
/* out[r] = sum_k w[r][k] over packed fp16 rows (the `lns` vector of a LayerNorm-folded GEMM) */
int dtp_op_rowsum(const void* w, int ld, int K, float* out, int rows, dtp_stream s);
/* packed f16 weights [rows][ldw] -> e4m3 [rows][ldw8] (ldw8 = K rounded up to 128) with one per-tensor power-of-two scale
 * (amax / scale <= 448), returned in *w_scale.  Synchronises the stream once (it reads the amax back). */
int dtp_op_quantize_w8(const void* w, int ldw, int K, int rows, void* out, int ldw8, float* w_scale, dtp_stream s);
int dtp_op_pack_conv(const float* w, void* out, int Cout, int Cin, int Cin_pad, int taps, int ldw, dtp_stream s);
/* w f32 [Cout][Cin][3][3] -> out f16 [rows][ldw], k' = ((ci/64)*9 + tap)*64 + ci%64 (Cin % 64 == 0; caller zero-fills out) */
int dtp_op_pack_conv_cb(const float* w, void* out, int Cout, int Cin, int ldw, dtp_stream s);
/* w f32 [Cout][Cin][3][3] (Cin % 64 == 0) -> out f16, dtp_op_pack_conv_ws_elems(Cout, Cin, Cin2) elements: 1 KB fragments in the order
 * ((n-tile of 32 output channels, 64-channel block, channel quarter, tap), lane, 8 channels) that convws_kernel's waves stream; w1 (NULL
 * or f32 [Cout][Cin2], Cin2 % 64 == 0) = the 1x1 weights of a fused shortcut (desc.A2), packed behind them */
int dtp_op_pack_conv_ws(const float* w, const float* w1, void* out, int Cout, int Cin, int Cin2, dtp_stream s);
long long dtp_op_pack_conv_ws_elems(int Cout, int Cin, int Cin2);
/* w f32 [Cout][Cin][3][3] (Cin % 64 == 0) -> out f16, dtp_op_pack_conv_ws_ups4_elems(Cout, Cin) elements (16/9 of the nine-tap packing):
 * the weights of the four 2x2 phase convs that equal the 3x3 conv over the nearest-2x upsample, phase = 2 py + px major.  Phase tap
 * (ry, rx) of parity (py, px) is the sum of the original taps ky in S(py, ry), kx in S(px, rx) with S(0, .) = {0}, {1, 2} and
 * S(1, .) = {0, 1}, {2}, added in fp32 (ky ascending, kx ascending inside) and rounded to f16 once.  1 KB fragments in the order
 * ((phase, n-tile of 32 output channels, 64-channel block, channel quarter, tap = 2 ry + rx), lane, 8 channels) */
int dtp_op_pack_conv_ws_ups4(const float* w, void* out, int Cout, int Cin, dtp_stream s);
long long dtp_op_pack_conv_ws_ups4_elems(int Cout, int Cin);
/* dtp_op_gemm for a 3x3 conv with upsample2x that also carries wfr4 = the phase sets of dtp_op_pack_conv_ws_ups4 (not NULL): d->tile
 * 56 / 57 runs the phase build, any other tile (or -1) runs as dtp_op_gemm would */
int dtp_op_conv_ups4(dtp_gemm_desc* d, const void* wfr4, dtp_stream s);
/* 1 when convws_kernel tile `tile` (51 .. 54, 56, 57) takes the conv problem *d (wfr4: its phase sets or NULL) with `splits` K-slices,
 * else 0 (also for other tiles) */
int dtp_op_conv_ws_supported(const dtp_gemm_desc* d, const void* wfr4, int tile, int splits);
/* w f16: the packed rows [>= N][ldw] of dtp_op_pack_linear (K % 64 == 0) -> out f16, dtp_op_pack_linear_ws_elems(N, K) elements: 1 KB
   fragments (32-column n-tile, 64-wide k-block, 16-wide k-step) in the order the weight-streaming GEMM (tile 55) loads them */
int dtp_op_pack_linear_ws(const void* w, int ldw, void* out, int N, int K, dtp_stream s);
long long dtp_op_pack_linear_ws_elems(int N, int K);
int dtp_op_groupnorm(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta, int B, int HW, int C,
                     int groups, float eps, int silu, dtp_stream s);
/* the apply pass of the two-launch GroupNorm on partial sums f32 [B][nchunk][groups][2] that a producer emitted (a convws_kernel launch
 * with DTP_GF_GNSTATS): y = GroupNorm(x) (+SiLU) without a statistics pass over x */
int dtp_op_groupnorm_apply(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta, const float* partial, int nchunk,
                           int B, int HW, int C, int groups, float eps, int silu, dtp_stream s);
/* the two halves as the engine runs them on a claimed reduce: the statistics pass sums the split-K slabs part f32 [splits][B*HW][C]
 * (+ bias[C], + resid f16 [B*HW][C]) and writes x f16 [B*HW][C] (part == NULL: plain statistics of x as it is), then the apply pass
 * normalises from its partial sums: y = GroupNorm(x) (+SiLU) */
int dtp_op_groupnorm_stats_apply(const float* part, int splits, const float* bias, const void* resid, void* x, void* y, const float* gamma,
                                 const float* beta, int B, int HW, int C, int groups, float eps, int silu, dtp_stream s);
/* measured ceilings of this GPU (bench.py roofline.peak_measured): dense fp16 MFMA TFLOP/s with random operands on every SIMD, and
 * the HBM GB/s (read + write) of a 512 MiB float4 copy; blocking, ~50 ms */
int dtp_op_measure_peaks(double* mfma_f16_tflops, double* hbm_copy_gbs);
/* split-K slabs part f32 [splits][B*HW][C] (+ bias[C], + resid f16 [B*HW][C]) -> conv_out f16 [B*HW][C] and y = GroupNorm(conv_out)
 * (+SiLU): the reduce of a split 3x3 conv folded into the GroupNorm that consumes it (models.py:250-302 GroupNorm+Swish plugin
 * behind a conv); one launch for HW <= 256, reduce-in-statistics + apply above */
int dtp_op_reduce_groupnorm(const float* part, int splits, const float* bias, const void* resid, void* conv_out, void* y, const float* gamma,
                            const float* beta, int B, int HW, int C, int groups, float eps, int silu, dtp_stream s);
/* the same launch over a zero-copy concatenation (engine Builder::claim_reduce): the slabs (bias, resid) hold the FIRST cx channels
 * ([splits][B*HW][cx]); channels [cx, C) are already in conv_out; the GroupNorm runs over all C.  cx == C is the call above. */
int dtp_op_reduce_groupnorm_cx(const float* part, int splits, const float* bias, const void* resid, void* conv_out, void* y, const float* gamma,
                               const float* beta, int B, int HW, int C, int groups, float eps, int silu, int cx, dtp_stream s);
/* the two grouped GEMMs of the algebraically fused cross-attention (attn2 of BasicTransformerBlock against 14 context tokens) as ONE
 * launch: Y = softmax_16(LN(X) W1^T + b1) W2^T + b2 + R per sample.  X / R / Y f16 [N*S][C]; W1 f16 [N][128][C] (LayerNorm gamma
 * folded in), b1 / lns1 f32 [N][128]; st_in f32 [st_parts][N*S][2] = per-row (sum, sumsq) partials of X; W2 f16 [N][roundup(C,128)][128];
 * st_out f32 [ceil(C/128)][N*S][2] (or null) = the same partials of Y for the next LayerNorm-folded GEMM */
int dtp_op_xattn(const void* X, const void* W1, const float* b1, const float* lns1, const float* st_in, int st_parts, const void* W2, const float* b2,
                 const void* R, void* Y, float* st_out, int S, int C, int N, int sm_valid, float ln_eps, dtp_stream s);
/* the same with an explicit number of 128-column tiles per workgroup (ct >= 1; ct < 1 = the launcher's rule, i.e. the call above) */
int dtp_op_xattn_ct(const void* X, const void* W1, const float* b1, const float* lns1, const float* st_in, int st_parts, const void* W2, const float* b2,
                    const void* R, void* Y, float* st_out, int S, int C, int N, int sm_valid, float ln_eps, int ct, dtp_stream s);
/* attn1.to_out.0 + residual, LayerNorm-2 and the fused cross-attention pair above as ONE register-chained launch (round 6, xchain.hip;
 * BasicTransformerBlock of diffusers 0.12 as run by the UNet engine, models.py:1097-1139):
 *   Y2 = A Wo^T + bo + Y;  Y3 = softmax_16(LN(Y2) W1^T + b1) W2^T + b2 + Y2   per sample -- Y2 and its row statistics never leave registers.
 * A / Y / Y3 f16 [N*S][C]; Wo f16 packed [>= C][ldwo] (dtp_op_pack_linear); W1 / b1 / lns1 / W2 / b2 as for dtp_op_xattn; st_out f32 [N*S][2]
 * (or null) = per-row (sum, sumsq) of Y3, ONE partial per row.  C == 320, S % 128 == 0 (UNet level 0). */
int dtp_op_xchain(const void* A, const void* Wo, int ldwo, const float* bo, const void* Y, const void* W1, const float* b1, const float* lns1,
                  const void* W2, const float* b2, void* Y3, float* st_out, int S, int C, int N, int sm_valid, float ln_eps, dtp_stream s);
/* the feed-forward of a transformer block as ONE register-chained launch (round 6, ffchain.hip): Out = [GEGLU(LN(X) W1^T + b1) | X] Wm^T +
 * bm + R with the [M][4 C] hidden tensor held in registers.  X / R / Out f16 [M][C]; W1 f16 packed [8 C][ldw1] in the GEGLU row packing
 * (dtp_op_pack_linear geglu = 1) with the LayerNorm gamma folded in, lns1 / b1 f32 indexed by packed row; Wm f16 packed [>= C][ldwm],
 * K = 4 C (hidden) + C (X): the merged ff.net.2 / proj_out weights.  C == 320.  Replaces ff.net.0 / ff.net.2 / proj_out of
 * BasicTransformerBlock + Transformer2DModel (diffusers 0.12; models.py:1097-1139), SURVEY K4. */
int dtp_op_ffchain(const void* X, const void* W1, int ldw1, const float* lns1, const float* b1, const void* Wm, int ldwm, const float* bm,
                   const void* R, void* Out, int M, int C, float ln_eps, dtp_stream s);
/* GroupNorm (no activation) folded into the Linear / 1x1 conv that consumes it (Transformer2DModel: norm -> proj_in): from x f16
 * [B][HW][C] and the packed weights W f16 [rows][ldw] (+ bias[Nout]) compute per-sample Wout f16 [B][rows][ldw] = W diag(gamma * rstd_b)
 * and bias_out f32 [B][rows] = bias + W (beta - mean_b * rstd_b * gamma), rows = roundup(Nout, 128): proj(GN(x_b)) == Wout_b x_b + bias_out_b */
int dtp_op_gn_fold_weights(const void* x, const void* W, int ldw, const float* bias, const float* gamma, const float* beta, int B, int HW, int C,
                           int Nout, int groups, float eps, void* Wout, float* bias_out, dtp_stream s);
/* the same pair WITHOUT the fold (round 6): y f16 [B*HW][Nout] = W GroupNorm(x_b) + bias with the normalisation applied to the resident
 * activation fragments of the activation-stationary Linear (lnlin_kernel, GNA build): statistics pass + ONE launch on the raw tensor and
 * the shared weights W f16 [rows][ldw] (dtp_op_pack_linear).  C in {320, 640}, HW % 128 == 0, 32 groups; col_ranges = workgroups per
 * 128-row block (>= 1).  st_out (or null): f32 [col_ranges][B*HW][2] per-row (sum, sumsq) partials of y for a LayerNorm-folded consumer.
 * Replaces models.py Transformer2DModel norm -> proj_in (diffusers 0.12) at UNet levels 0-1. */
int dtp_op_gn_linear(const void* x, const void* W, int ldw, const float* bias, const float* gamma, const float* beta, int B, int HW, int C,
                     int Nout, int groups, float eps, void* y, float* st_out, int col_ranges, dtp_stream s);
int dtp_op_layernorm(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta, int rows, int C,
                     float eps, dtp_stream s);
int dtp_op_attention(const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo, int B, int H,
                     int Sq, int Skv, int D, int64_t qbs, int64_t kbs, int64_t vbs, int64_t obs, float scale, dtp_stream s);
/* The same attention with both contractions on the fp8 (OCP e4m3) block-scaled MFMA (BASELINE configs[4]): q / k / v / o stay f16 in
 * memory, tiles are quantised on their way into LDS.  q_scale, v_scale: per-tensor scales (powers of two; Q is stored as
 * Q*q_scale and K as K/q_scale so the scores are unchanged, V as V/v_scale).  D %% 8 == 0, D %% 64 != 0, D <= 184. */
/* the self-attention launch forced onto attn_dma_kernel (K / V by LDS-DMA; the stamp's dispatcher uses it from 512 keys on), whatever the
 * sequence length; nw = waves per workgroup (0 = the launcher's rule, 4, 8: d = 40 has both builds).  DTP_ERR_ARG when the kernel does
 * not take the problem (d not in {40, 80}, Skv % 64, Skv < 128, alignment); with all four pointers null the call only answers that
 * question.  Inputs must be finite (see dtp_launch_attention_dma). */
int dtp_op_attention_dma(const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo, int B, int H,
                         int Sq, int Skv, int D, int64_t qbs, int64_t kbs, int64_t vbs, int64_t obs, float scale, int nw, dtp_stream s);
int dtp_op_attention_fp8(const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo, int B, int H,
                         int Sq, int Skv, int D, int64_t qbs, int64_t kbs, int64_t vbs, int64_t obs, float scale, float q_scale,
                         float v_scale, dtp_stream s);
int dtp_op_softmax_rows(const void* x, int ldx, void* y, int ldy, int rows, int cols, float scale, dtp_stream s);
/* The start point of a strength < 1 stamp as its pre-processing stage computes it (the same device function): x[i] = a z0[i] + b eps[i]
 * over n f32 values, both products rounded before the sum (dtp_strength_schedule gives a, b). */
int dtp_op_strength_init(const float* z0, const float* eps, float a, float b, float* x, long long n, dtp_stream s);
/* kornia.morphology.dilation(alpha, ones(pad,pad)) of add_extra_context (handler.py:28-29) as the stamp runs it: canvas f32
 * [B,4,R,R] (the alpha plane is read), tmp / out f32 [B,R,R]; window rows/cols [i - pad/2, i + pad - pad/2 - 1], clipped */
int dtp_op_dilate(const float* canvas, float* tmp, float* out, int B, int R, int pad, dtp_stream s);
/* the same with one pad per image (host int pads[B], B <= 64), as dtp_stamp_mixed runs it */
int dtp_op_dilate_pads(const float* canvas, float* tmp, float* out, int B, int R, const int* pads, dtp_stream s);
/* One sampler update exactly as the stamp's loop runs it after UNet evaluation `step_index` (the same kernel): the guidance combine
 * e_b = u + cfg[b] (c - u) [+ tg[b] (g - c) while rank[b] < k], then the `scheduler` update of x with coefficient row `row`.
 *   eps_out f32 [2B + k][h*w][4]  the UNet's outputs in the stamp's row order [uncond x B | cond x B | tg x k], NHWC
 *   x       f32 [B][h*w][4]       the running latent, updated in place
 *   hist    f32 [3][B][h*w][4]    the sampler history (DPM: previous x0 in slot 0; LMSD: derivatives d_{i-1..i-3} in slot i % 3)
 *   in16    f16 [2B + k][h*w][16] channels 0-3 of every row receive x' * next_scale[0] (the next evaluation's input)
 *   row     f32 [DTP_SCHED_ROW] (device) a row of dtp_scheduler_tables' coefs; next_scale f32 [1] (device)
 *   cfg, tg f32 [B], rank int [B] (device): stamp b's texture-guided row is 2B + rank[b] while rank[b] < k.  B <= 64, 0 <= k <= B.
 *   step_index  the evaluation's index within the stamp's loop: DPM runs first order at step_index 0 whatever the row's order says (a
 *               strength < 1 stamp starts mid-table without a previous x0); LMSD's history ring is indexed by it. */
int dtp_op_sched_step(int scheduler, const float* eps_out, float* x, float* hist, void* in16, const float* row, const float* next_scale,
                      const float* cfg, const float* tg, const int* rank, int step_index, int B, int hw, int k, dtp_stream s);

/* The two kernels of dtp_stroke on their own, B <= 64 windows per launch: xs, ys, modes host int[B] (modes NULL = all INPAINT), the
 * top-left texel and DTP_STROKE_* mode of window b; texture u8 [H][W][4] (device, 4-byte aligned), H >= R, W >= R; wrap, over_y, over_x as in
 * dtp_stroke_opts.  gather: canvas f32 [B][4][R][R] = window texel / 255, 0 outside a non-wrapping texture and in an OVERPAINT window's
 * inner rectangle.  paste: dec f32 [B][R][R][4] is the VAE decoder's output in its working layout (NHWC, values around -1..1, channel 3
 * unused; NULL when every window is an ERASE window); under mask u8 [R][R] > 0 the texel becomes (u8(clamp(dec / 2 + 0.5, 0, 1) * 255) x 3,
 * 255), or 0 x 4 for an ERASE window.  Overlapping windows in ONE paste launch race; dtp_stroke never issues them. */
int dtp_op_stroke_gather(const uint8_t* texture, int H, int W, float* canvas, int R, int B, const int* xs, const int* ys, const int* modes,
                         int wrap, int over_y, int over_x, dtp_stream s);
int dtp_op_stroke_paste(const float* dec, const uint8_t* mask, uint8_t* texture, int H, int W, int R, int B, const int* xs, const int* ys,
                        const int* modes, int wrap, dtp_stream s);

/* The two halves of a dtp_mesh_stroke stamp on their own (the contract: see dtp_mesh_stroke).  render: cam the 12 floats of
 * dtp_mesh_camera; projects the mesh, keeps the per-face records with it, and writes canvas f32 [4][R][R] and face_idx i32 [R][R]
 * (device), 1 <= R <= 4096.  backproject: uses the records of the LAST render of this mesh and that render's face_idx; dec f32 [R][R][4] is
 * the VAE decoder's output in its working layout (values around -1..1, channel 3 unused), NULL = erase; dec_finished 1: dec holds the
 * clamped 0..1 values already (what dtp_stamp returns with composite 0, in the same [R][R][4] layout) and is used as it is; mask u8 [R][R]. */
int dtp_op_mesh_render(dtp_mesh* mesh, const float cam[12], float fov, int flip_normals, const uint8_t* texture, int H, int W, int R, int mode,
                       int over_y, int over_x, float* canvas, int* face_idx, dtp_stream s);
int dtp_op_mesh_backproject(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R, uint8_t* texture, int H, int W,
                            dtp_stream s);
/* dtp_op_mesh_backproject with a face set (the contract: see "face sets"): face_mask device u32 [mask_words], mask_words = (F + 31) / 32;
 * a face whose bit is 0 is not valid.  face_mask NULL: dtp_op_mesh_backproject exactly. */
int dtp_op_mesh_backproject_masked(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R,
                                   uint8_t* texture, int H, int W, const uint32_t* face_mask, int mask_words, dtp_stream s);
/* dtp_op_mesh_backproject_masked with the occlusion test (the contract: see "occlusion in the backprojection"): fov the fov of the render
 * whose records and face_idx these are, occlude the tolerance in stamp pixels; tol = ((occlude 2) fov) / R.  DTP_ERR_ARG, before the mesh is
 * looked at: occlude negative or not finite, R outside 1..4096, fov not finite or not > 0, a tol that does not fit fp32. */
int dtp_op_mesh_backproject_occluded(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R,
                                     uint8_t* texture, int H, int W, const uint32_t* face_mask, int mask_words, float fov, float occlude,
                                     dtp_stream s);
/* dtp_mesh_pick with the records left on the device (the contract: see "picking on a mesh"): rays host dtp_ray[n], out device
 * dtp_mesh_hit[n] (52 bytes each).  The same checks; it enqueues on `s` and waits for `s`, because the frames travel through the mesh's
 * pinned buffer. */
int dtp_op_mesh_pick(dtp_mesh* mesh, const dtp_ray* rays, int n, dtp_mesh_hit* out, dtp_stream s);
/* dtp_mesh_view (the contract: see "a view of a textured mesh") with the binning switched: binned 1 is dtp_mesh_view exactly; binned 0
 * puts every drawn face on the list that every 16 x 16 tile streams, the arm a measurement compares the bins with.  The frame is the
 * same bytes either way. */
int dtp_op_mesh_view(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const dtp_view_cam* cam, int H, int W, const dtp_view_opts* opts,
                     uint8_t* image, int* face_idx, float* depth, int binned, dtp_stream s);
/* dtp_mesh_view_clip (the contract: see "a view clipped at the near plane") with the binning switched: binned 1 is dtp_mesh_view_clip
 * exactly; binned 0 puts every drawn face on the list that every tile streams AND gives every crossing face the whole frame as its pixel
 * range: the arm against which the ranges are tested.  The frame is the same bytes either way. */
int dtp_op_mesh_view_clip(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                          const dtp_view_opts* opts, int filter, uint8_t* image, int* face_idx, float* depth, float* lod, int binned, dtp_stream s);
/* dtp_mesh_view_aa (the contract: see "an anti-aliased view") with the binning switched, as dtp_op_mesh_view_clip switches it: binned 1
 * is dtp_mesh_view_aa exactly.  The frame is the same bytes either way. */
int dtp_op_mesh_view_aa(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                        const dtp_view_opts* opts, int filter, int clip, int samples, uint8_t* image, int* face_idx, float* depth, float* lod,
                        uint8_t* coverage, int binned, dtp_stream s);
/* dtp_mesh_view_aniso (the contract: see "an anisotropic view") with the binning switched, as dtp_op_mesh_view_aa switches it: binned 1
 * is dtp_mesh_view_aniso exactly.  The frame is the same bytes either way. */
int dtp_op_mesh_view_aniso(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                           const dtp_view_opts* opts, int clip, int samples, int max_aniso, uint8_t* image, int* face_idx, float* depth,
                           float* lod, uint8_t* taps, uint8_t* coverage, int binned, dtp_stream s);
#ifdef __cplusplus
}
#endif
#endif /* DTP_H */
