// The stamp: everything TRTConditionalInpainter.generate_raw / InpaintPipeline.infer do around the
// three networks, as fused HIP kernels + hipGraph replay.
// Reference: trt_inference/trt_model.py:90-121, handler.py:25-33,55-56, model_base.py:51-58,
// inpaint_pipeline.py:39-153, stable_diffusion_pipeline.py:340-355,407-484, utilities.py:370-529.
#include <math.h>
#include <algorithm>
#include <stdio.h>
#include <string.h>

#include "stamp.h"
#include <dlfcn.h>

// roctx ranges around the stages of a stamp (host side, like the reference's NVTX ranges: stable_diffusion_pipeline.py:358-366), so that
// a rocprofv3 --marker-trace carries the stage names.  Resolved at run time from the ROCm marker library: no link dependency, a no-op
// when the library is absent.
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      void* h = dlopen(lib, RTLD_LAZY | RTLD_GLOBAL);
      if (!h) continue;
      push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
      pop = (int (*)())dlsym(h, "roctxRangePop");
      if (push && pop) return;
      push = nullptr; pop = nullptr;
    }
  }
};
const Roctx& roctx() { static Roctx r; return r; }
struct RoctxRange {
  explicit RoctxRange(const char* name) { if (roctx().push) roctx().push(name); }
  ~RoctxRange() { if (roctx().pop) roctx().pop(); }
};
}  // namespace

#define VAE_SCALE 0.18215f

// ---------------------------------------------------------------- kernels
namespace {

// separable flat dilation (kornia.morphology.dilation with ones(pad,pad), geodesic border), each stamp with its own pad:
// out[i] = max over [i - lo[b], i + hi[b]] clipped to the image, lo = pad/2, hi = pad - pad/2 - 1 (PadArgs, stamp.h).
__global__ void dilate_row_kernel(const float* __restrict__ canvas, float* __restrict__ tmp, int B, int R, PadArgs pa) {
  const long long total = (long long)B * R * R;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % R);
    const long long by = i / R;
    const int y = (int)(by % R), b = (int)(by / R);
    const int lo = pa.lo[b], hi = pa.hi[b];
    const float* a = canvas + ((size_t)b * 4 + 3) * R * R + (size_t)y * R;
    float m = -1e4f;
    for (int xx = max(0, x - lo); xx <= min(R - 1, x + hi); ++xx) m = fmaxf(m, a[xx]);
    tmp[i] = m;
  }
}
__global__ void dilate_col_kernel(const float* __restrict__ tmp, float* __restrict__ out, int B, int R, PadArgs pa) {
  const long long total = (long long)B * R * R;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % R);
    const long long by = i / R;
    const int y = (int)(by % R), b = (int)(by / R);
    const int lo = pa.lo[b], hi = pa.hi[b];
    const float* a = tmp + (size_t)b * R * R + x;
    float m = -1e4f;
    for (int yy = max(0, y - lo); yy <= min(R - 1, y + hi); ++yy) m = fmaxf(m, a[(size_t)yy * R]);
    out[i] = m;
  }
}

// trt_model.py:103-109 + handler.py:25-33: canvas -> VAE-encoder inputs (NHWC f16, 8 channels,
// batch [masked x B | context x B]) and the two latent-resolution masks (nearest, 1 = paint).  `init` (strength < 1): a third slab
// [canvas x B] holds the unmasked canvas RGB * 2 - 1, the init image whose latents the stamp starts from.
__global__ void prep_kernel(const float* __restrict__ canvas, const float* __restrict__ brush_slots, const int* __restrict__ slot_map,
                            const float* __restrict__ dil, f16* __restrict__ enc_in, float* __restrict__ masks, int B, int R, int init) {
  const int HW = R * R, h = R / 8;
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / HW), pix = (int)(i - (long long)b * HW);
    const float* cb = canvas + (size_t)b * 4 * HW;
    const float* brush = brush_slots + (size_t)slot_map[b] * 3 * HW;  // this stamp's brush (hint image source)
    const float a = cb[3 * HW + pix];
    const float hint = 1.0f - dil[i];
    f16x8 m8, c8, i8;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float img = cb[ch * HW + pix] * 2.0f - 1.0f;
      const float masked = img * a;
      const float src = brush[ch * HW + pix] * 2.0f - 1.0f;
      m8[ch] = (f16)masked;
      c8[ch] = (f16)(masked + src * hint);
      i8[ch] = (f16)img;
    }
#pragma unroll
    for (int ch = 3; ch < 8; ++ch) m8[ch] = c8[ch] = i8[ch] = (f16)0.f;
    *(f16x8*)(enc_in + i * 8) = m8;
    *(f16x8*)(enc_in + ((size_t)B * HW + i) * 8) = c8;
    if (init) *(f16x8*)(enc_in + ((size_t)2 * B * HW + i) * 8) = i8;
    const int y = pix / R, x = pix - y * R;
    if ((y & 7) == 0 && (x & 7) == 0) {  // F.interpolate(size=(h,w)) default 'nearest': src = dst * 8
      const size_t o = (size_t)b * h * h + (size_t)(y >> 3) * h + (x >> 3);
      masks[o] = 1.0f - a;
      masks[(size_t)B * h * h + o] = 1.0f - fminf(fmaxf(a + hint, 0.f), 1.f);
    }
  }
}

// scheduler.add_noise(z0, eps, t_start, timesteps[t_start]) of every sampler as x = a z0 + b eps (utilities.py:363-366, :524-529,
// :1000-1008): both products rounded to fp32 before the sum, as torch evaluates them
__device__ __forceinline__ float strength_init_value(float a, float b, float z0, float e) {
  float p = a * z0, q = b * e;
  asm volatile("" : "+v"(p));
  asm volatile("" : "+v"(q));
  return p + q;
}

// UNet input assembly (inpaint_pipeline.py:116,136; sdp:423-427): branch-major [uncond x B | cond x B | tg x k]; stamp b has the
// texture-guided row 2B + rank[b] while rank[b] < k (StampCoefs).  At stage 0 (lat_nchw set) the running latent starts as
// latents * init_noise_sigma (sdp:345), or, with the init-image latents z0 (strength < 1), as add_noise(z0, latents) with the pair
// and start row of params->strength; the latent channels of the input are scaled by scale_model_input of evaluation `eval_index`
// (with z0: of the start row; sdp:424; the mask and masked-latent channels are concatenated after scaling, :426-427).
__global__ void assemble_kernel(const float* __restrict__ lat_nchw, const float* __restrict__ z0, const float* __restrict__ masks,
                                const float* __restrict__ ml, const int* __restrict__ rank, f16* __restrict__ in16,
                                float* __restrict__ x32, const StampParams* __restrict__ params, int eval_index, int B, int HWl, int k) {
  const long long total = (long long)B * HWl;
  const float sig0 = params->init_sigma, scale = params->in_scale[z0 ? params->strength.row : eval_index];
  const float na = params->strength.a, nb = params->strength.b;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / HWl), p = (int)(i - (long long)b * HWl);
    float x[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (lat_nchw) {
        const size_t o = ((size_t)b * 4 + ch) * HWl + p;
        x[ch] = z0 ? strength_init_value(na, nb, z0[o], lat_nchw[o]) : lat_nchw[o] * sig0;
        x32[i * 4 + ch] = x[ch];
      } else {
        x[ch] = x32[i * 4 + ch];  // mid-loop switch to a program with fewer tg rows: keep the running latent
      }
      x[ch] *= scale;
      asm volatile("" : "+v"(x[ch]));  // round the scaled latent to fp32 before fp16, as the reference does
    }
    const int r = rank[b];
    const int NB = r < k ? 3 : 2;
    for (int br = 0; br < NB; ++br) {
      const int src = (br < 2) ? b : B + b;  // branches 0,1: masked image; branch 2: context image
      const int row = (br < 2) ? br * B + b : 2 * B + r;
      f16x8 lo, hi;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) lo[ch] = (f16)x[ch];
      lo[4] = (f16)masks[(size_t)src * HWl + p];
      lo[5] = (f16)ml[((size_t)src * 4 + 0) * HWl + p];
      lo[6] = (f16)ml[((size_t)src * 4 + 1) * HWl + p];
      lo[7] = (f16)ml[((size_t)src * 4 + 2) * HWl + p];
      hi[0] = (f16)ml[((size_t)src * 4 + 3) * HWl + p];
#pragma unroll
      for (int ch = 1; ch < 8; ++ch) hi[ch] = (f16)0.f;
      f16* o = in16 + ((size_t)row * HWl + p) * 16;
      *(f16x8*)o = lo;
      *(f16x8*)(o + 8) = hi;
    }
  }
}

// guidance combine + one sampler update + refresh of the latent channels of the UNet input (sdp:419-420,449-455).  Stamp b uses its
// own cfg / tg; its texture-guided branch is row 2B + rank[b] of a program with k tg rows, present while rank[b] < k, i.e. while
// step_index < its tg_evals (the stamps are ordered by descending tg_evals).  `kc`: this evaluation's coefficient row
// (dtp_scheduler_tables); `hist`: [3][B][HWl][4] sampler history; `step_index`: the evaluation's index within the stamp's loop (0 =
// its first evaluation).  One instantiation per sampler:
//   DDIM  eta = 0 step (utilities.py:463-503)
//   DPM   DPM-Solver++ first order / multistep second order, midpoint (utilities.py:838-852,873-880,888-931,953-994)
//   LMSD  linear multistep in sigma space (utilities.py:345-362)
template <int S>
__global__ void step_kernel(const float* __restrict__ eps_out, float* __restrict__ x32, f16* __restrict__ in16, float* __restrict__ hist,
                            const float* __restrict__ kc, const float* __restrict__ next_scale, const float* __restrict__ cfgs,
                            const float* __restrict__ tgs, const int* __restrict__ ranks, int step_index, int B, int HWl, int k) {
  const long long total = (long long)B * HWl * 4;
  const size_t bs = (size_t)B * HWl * 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / ((long long)HWl * 4));
    const long long j = i - (long long)b * HWl * 4;  // element within the stamp
    const int r = ranks[b];
    const float cfg = cfgs[b];
    const float u = eps_out[i], c = eps_out[bs + i];
    float e = u + cfg * (c - u);
    if (r < k) e += tgs[b] * (eps_out[(2 * (size_t)B + r) * HWl * 4 + j] - c);
    const float x = x32[i];
    float xn;
    if constexpr (S == DTP_SCHED_DDIM) {
      const float sqrt_beta_t = kc[0], sqrt_alpha_t = kc[1], sqrt_alpha_prev = kc[2], sqrt_beta_prev = kc[3];
      // the contractions spelled out: which product of the update the compiler folds into the fma otherwise depends on the
      // surrounding code, and these are the ones DDIM stamps have always been computed with
      const float x0 = fmaf(-sqrt_beta_t, e, x) / sqrt_alpha_t;
      xn = fmaf(sqrt_beta_prev, e, sqrt_alpha_prev * x0);
    } else if constexpr (S == DTP_SCHED_DPM) {
      const float m0 = (x - kc[1] * e) / kc[0];  // convert_model_output: the data prediction x0
      xn = kc[3] * x - kc[4] * m0;
      // second order: D1 = (1 / r0) (m0 - m_prev).  The first evaluation of a stamp is first order whatever its row says: a stamp
      // that starts at row t_start > 0 (strength < 1) has no previous x0 (lower_order_nums restarts at 0, utilities.py:805,979)
      if (kc[2] > 1.5f && step_index > 0) xn = xn - kc[5] * (kc[6] * (m0 - hist[i]));
      hist[i] = m0;
    } else {
      const float sigma = kc[0];
      const float x0 = x - sigma * e;
      const float d = (x - x0) / sigma;  // the ODE derivative, computed as the reference does
      const int order = min(max((int)kc[1], 1), 4);
      float acc = kc[2] * d;
      for (int m = 1; m < order; ++m) acc += kc[2 + m] * hist[(size_t)((step_index - m + 3) % 3) * bs + i];
      xn = x + acc;
      hist[(size_t)(step_index % 3) * bs + i] = d;
    }
    x32[i] = xn;
    // the fp16 copies are the rounded fp32 latent: keep the compiler from fusing the last fma into the conversion (v_fma_mix*_f16
    // rounds the exact product once, i.e. differently)
    asm volatile("" : "+v"(xn));
    if constexpr (S == DTP_SCHED_LMSD) {  // scale_model_input of the next evaluation (DDIM, DPM: 1)
      xn *= next_scale[0];
      asm volatile("" : "+v"(xn));
    }
    const long long pix = i >> 2, p = j >> 2;
    const int ch = (int)(i & 3);
    in16[((size_t)pix) * 16 + ch] = (f16)xn;
    in16[((size_t)B * HWl + pix) * 16 + ch] = (f16)xn;
    if (r < k) in16[((2 * (size_t)B + r) * HWl + p) * 16 + ch] = (f16)xn;
  }
}

// inpaint_pipeline.py:148 clamp, optional alpha composite (model_base.py:56-58) and the truncating
// u8 conversion (handler.py:55-56); finish_value / finish_u8: stamp.h, shared with the stroke's paste.
__global__ void finish_kernel(const float* __restrict__ dec, const float* __restrict__ canvas, void* __restrict__ out, int B,
                              int HW, int composite, int u8) {
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / HW), pix = (int)(i - (long long)b * HW);
    const float a = composite ? canvas[((size_t)b * 4 + 3) * HW + pix] : 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v = finish_value(dec[i * 4 + ch]);
      if (composite) v = canvas[((size_t)b * 4 + ch) * HW + pix] * a + v * (1.0f - a);
      if (u8) ((unsigned char*)out)[i * 3 + ch] = finish_u8(v);
      else ((float*)out)[((size_t)b * 3 + ch) * HW + pix] = v;
    }
  }
}

// ctx16[n][14][768]: rows [0, B) <- uncond, [B, 2B) <- cond, the tg rows 2B + j <- cond of stamp order[j] (inpaint_pipeline.py:140),
// each from the stamp's own slot
__global__ void build_ctx_kernel(const float* __restrict__ cond_slots, const int* __restrict__ slot_map, const int* __restrict__ order,
                                 f16* __restrict__ ctx16, int B, int N) {
  const int per = 14 * 768;
  const long long total = (long long)N * per;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int n = (int)(i / per), j = (int)(i - (long long)n * per);
    const int b = n < 2 * B ? n % B : order[n - 2 * B];
    ctx16[i] = (f16)cond_slots[(size_t)slot_map[b] * 2 * per + (n < B ? per : 0) + j];
  }
}

// the per-stamp slot ids travel as a kernel argument (SlotArgs, stamp.h)
__global__ void set_slots_kernel(int* __restrict__ dst, SlotArgs a, int B) {
  if ((int)threadIdx.x < B) dst[threadIdx.x] = a.s[threadIdx.x];
}

// the per-stamp cfg / tg and the tg row map travel as kernel ARGUMENTS into the device parameter block the captured kernels read:
// no host staging buffer, so dtp_stamp never has to wait for the stream
__global__ void set_header_kernel(StampCoefs* __restrict__ dst, StampCoefs a) {
  constexpr int words = (int)(sizeof(StampCoefs) / 4);
  for (int t = threadIdx.x; t < words; t += blockDim.x) ((int*)dst)[t] = ((const int*)&a)[t];
}

// the strength < 1 start point (add_noise pair, start row) into the parameter block, as set_header_kernel writes the header
__global__ void set_strength_kernel(StampStrength* __restrict__ dst, StampStrength a) {
  if (threadIdx.x == 0) *dst = a;
}

// dtp_op_strength_init: the stage-0 combine of assemble_kernel on its own, elementwise over n values
__global__ void strength_init_kernel(const float* __restrict__ z0, const float* __restrict__ eps, float a, float b, float* __restrict__ x,
                                     long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    x[i] = strength_init_value(a, b, z0[i], eps[i]);
}

// post-loop finiteness guard (the reference asserts `not isnan` after every step, stable_diffusion_pipeline.py:415, at the
// price of a host sync per step; here ONE pass over the final latents and the decoded image, debug option "check_finite")
__global__ void finite_check_kernel(const float* __restrict__ a, long long na, const float* __restrict__ b, long long nb,
                                    int* __restrict__ flag) {
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (long long)gridDim.x * 256) {
    const float v = i < na ? a[i] : b[i - na];
    bad |= !(fabsf(v) <= 3.0e38f);  // false for NaN and +-inf
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

inline int nblk(long long total) { return (int)std::min<long long>((total + 255) / 256, 4096); }

}  // namespace

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP)

static int get_bufs(Ctx* c, int B, StampBufs** out) {
  auto it = c->stamp_bufs.find(B);
  if (it == c->stamp_bufs.end()) {
    StampBufs sb;
    void* p;
    const size_t hw = (size_t)c->h * c->h;
    RC(ctx_persistent(c, 2 * B * hw * 4, &p, true)); sb.masks = (float*)p;
    RC(ctx_persistent(c, 2 * B * 4 * hw * 4, &p, true)); sb.ml = (float*)p;
    RC(ctx_persistent(c, B * 4 * hw * 4, &p, true)); sb.lat = (float*)p;
    RC(ctx_persistent(c, 2 * B * 4 * hw * 4, &p, true)); sb.eps = (float*)p;
    it = c->stamp_bufs.emplace(B, sb).first;
  }
  *out = &it->second;
  return DTP_OK;
}

// the first strength < 1 stamp of batch B: masked latents and VAE draws get a third slab (the init image).  The captured stages of B
// hold the two-slab buffers: they are dropped (a one-time wait, like building the 3B encoder program) and recaptured on the new ones,
// which every later stamp of B, strength 1 or not, uses.
static int grow_bufs_three(Ctx* c, int B, StampBufs* sb) {
  if (sb->three) return DTP_OK;
  HIP_CHECK(hipDeviceSynchronize());  // a captured stage may still be replaying on the old buffers
  graphs_drop(c, [B](const StageKey& k) { return k.B == B; });
  void* p;
  const size_t hw = (size_t)c->h * c->h;
  RC(ctx_persistent(c, 3 * B * 4 * hw * 4, &p, true)); sb->ml = (float*)p;
  RC(ctx_persistent(c, 3 * B * 4 * hw * 4, &p, true)); sb->eps = (float*)p;
  sb->three = true;
  return DTP_OK;
}

static PadArgs pad_args(const int* pads, int B) {
  PadArgs pa = {};
  for (int b = 0; b < B; ++b) { pa.lo[b] = pads[b] / 2; pa.hi[b] = pads[b] - pads[b] / 2 - 1; }
  return pa;
}

extern "C" {

// kernel-level entry points: the separable flat dilation of add_extra_context (handler.py:28-29) on the alpha plane of a canvas,
// with one pad for all B images / one pad per image
int dtp_op_dilate_pads(const float* canvas, float* tmp, float* out, int B, int R, const int* pads, dtp_stream s_) {
  if (!canvas || !tmp || !out || !pads || B < 1 || B > DTP_STAMP_MAXB || R < 1) { dtp_set_error("dtp_op_dilate: bad argument (B=%d, max %d)", B, DTP_STAMP_MAXB); return DTP_ERR_ARG; }
  for (int b = 0; b < B; ++b)
    if (pads[b] < 1) { dtp_set_error("dtp_op_dilate: pad %d of image %d must be >= 1", pads[b], b); return DTP_ERR_ARG; }
  hipStream_t s = (hipStream_t)s_;
  const PadArgs pa = pad_args(pads, B);
  hipLaunchKernelGGL(dilate_row_kernel, dim3(nblk((long long)B * R * R)), dim3(256), 0, s, canvas, tmp, B, R, pa);
  hipLaunchKernelGGL(dilate_col_kernel, dim3(nblk((long long)B * R * R)), dim3(256), 0, s, tmp, out, B, R, pa);
  return LAUNCH_OK();
}

static int launch_step(int scheduler, const float* eps_out, float* x, f16* in16, float* hist, const float* row, const float* next_scale,
                       const float* cfg, const float* tg, const int* rank, int step_index, int B, int HWl, int k, hipStream_t s) {
  const dim3 grid(nblk((long long)B * HWl * 4)), block(256);
  if (scheduler == DTP_SCHED_DDIM)
    hipLaunchKernelGGL(step_kernel<DTP_SCHED_DDIM>, grid, block, 0, s, eps_out, x, in16, hist, row, next_scale, cfg, tg, rank, step_index, B, HWl, k);
  else if (scheduler == DTP_SCHED_DPM)
    hipLaunchKernelGGL(step_kernel<DTP_SCHED_DPM>, grid, block, 0, s, eps_out, x, in16, hist, row, next_scale, cfg, tg, rank, step_index, B, HWl, k);
  else
    hipLaunchKernelGGL(step_kernel<DTP_SCHED_LMSD>, grid, block, 0, s, eps_out, x, in16, hist, row, next_scale, cfg, tg, rank, step_index, B, HWl, k);
  return LAUNCH_OK();
}

int dtp_op_sched_step(int scheduler, const float* eps_out, float* x, float* hist, void* in16, const float* row, const float* next_scale,
                      const float* cfg, const float* tg, const int* rank, int step_index, int B, int hw, int k, dtp_stream s) {
  if (scheduler != DTP_SCHED_DDIM && scheduler != DTP_SCHED_DPM && scheduler != DTP_SCHED_LMSD) {
    dtp_set_error("dtp_op_sched_step: unknown scheduler %d (DDIM = 0, DPM = 1, LMSD = 2)", scheduler);
    return DTP_ERR_ARG;
  }
  if (!eps_out || !x || !hist || !in16 || !row || !next_scale || !cfg || !tg || !rank || B < 1 || B > DTP_STAMP_MAXB || hw < 1 || k < 0 ||
      k > B || step_index < 0) {
    dtp_set_error("dtp_op_sched_step: bad argument (B=%d, max %d, k=%d, hw=%d, step_index=%d)", B, DTP_STAMP_MAXB, k, hw, step_index);
    return DTP_ERR_ARG;
  }
  return launch_step(scheduler, eps_out, x, (f16*)in16, hist, row, next_scale, cfg, tg, rank, step_index, B, hw, k, (hipStream_t)s);
}

int dtp_op_strength_init(const float* z0, const float* eps, float a, float b, float* x, long long n, dtp_stream s) {
  if (!z0 || !eps || !x || n < 1) { dtp_set_error("dtp_op_strength_init: bad argument (n=%lld)", n); return DTP_ERR_ARG; }
  hipLaunchKernelGGL(strength_init_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)s, z0, eps, a, b, x, n);
  return LAUNCH_OK();
}

int dtp_op_dilate(const float* canvas, float* tmp, float* out, int B, int R, int pad, dtp_stream s) {
  if (!canvas || !tmp || !out || B < 1 || R < 1 || pad < 1) { dtp_set_error("dtp_op_dilate: bad argument"); return DTP_ERR_ARG; }
  const std::vector<int> pads(DTP_STAMP_MAXB, pad);
  const size_t RR = (size_t)R * R;
  for (int b0 = 0; b0 < B; b0 += DTP_STAMP_MAXB)
    RC(dtp_op_dilate_pads(canvas + b0 * 4 * RR, tmp + b0 * RR, out + b0 * RR, std::min(B - b0, DTP_STAMP_MAXB), R, pads.data(), s));
  return DTP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- one plan per stamp call (StampPlan: stamp.h)
int stamp_plan(Ctx* c, StampPlan& p) {
  const dtp_settings* st = p.st;
  const int B = p.B;
  if (p.seeded && !p.seeds) { dtp_set_error("dtp_stamp_seeded: seeds is NULL (one uint64 per stamp, host memory)"); return DTP_ERR_ARG; }
  if (!(p.strength > 0.0 && p.strength <= 1.0)) { dtp_set_error("dtp_stamp_strength: strength %g outside (0, 1]", p.strength); return DTP_ERR_ARG; }
  p.init = p.strength < 1.0;  // strength 1 is dtp_stamp_mixed, init_eps unused
  if (!c || !c->finalized) { dtp_set_error("dtp_stamp: weights not finalized"); return DTP_ERR_STATE; }
  if (p.init) {  // (these come before the checks of the other arguments, and the schedule's refusals under the stamp's own names)
    if (!st || B < 1 || B > c->maxB) { dtp_set_error("dtp_stamp: bad argument (B=%d, max %d)", B, c->maxB); return DTP_ERR_ARG; }
    if (c->fp8_linear || c->fp8_attention || c->fp8_operands) {
      dtp_set_error("dtp_stamp_strength: strength < 1 is not offered under the fp8 options (parity-only, calibrated per program)");
      return DTP_ERR_STATE;
    }
    if (st[0].steps < 2 || st[0].steps > 999) { dtp_set_error("dtp_stamp: steps=%d of stamp 0 outside 2..999", st[0].steps); return DTP_ERR_ARG; }
    int t_start;
    float ab[2];
    const int rc = dtp_strength_schedule(c->scheduler, st[0].steps, p.strength, &t_start, &p.E, ab);
    if (rc) { dtp_set_error("dtp_stamp_strength: strength %g leaves no evaluation at %d steps", p.strength, st[0].steps); return rc; }
    p.row0 = t_start - (c->scheduler == DTP_SCHED_DDIM ? 1 : 0);
    p.a = ab[0]; p.b = ab[1];
  }
  if ((!p.canvas && !p.canvas_staged) || !st || (!p.latents && !p.seeded) || (!p.out && !p.paste) || B < 1 || B > c->maxB) { dtp_set_error("dtp_stamp: bad argument (B=%d, max %d)", B, c->maxB); return DTP_ERR_ARG; }
  for (int b = 0; b < B; ++b) {
    const int sl = p.slot_ids ? p.slot_ids[b] : 0;
    if (sl < 0 || sl >= DTP_MAX_SLOTS) { dtp_set_error("dtp_stamp: slot %d of stamp %d outside 0..%d", sl, b, DTP_MAX_SLOTS - 1); return DTP_ERR_ARG; }
    if (!c->slot_set[sl]) { dtp_set_error("dtp_stamp: no brush set in slot %d (call dtp_set_brush / dtp_set_conditioning)", sl); return DTP_ERR_STATE; }
    p.slots.s[b] = sl;
  }
  int pads[DTP_STAMP_MAXB];
  for (int b = 0; b < B; ++b) {
    if (st[b].steps < 2 || st[b].steps > 999) { dtp_set_error("dtp_stamp: steps=%d of stamp %d outside 2..999", st[b].steps, b); return DTP_ERR_ARG; }
    if (st[b].context_pad < 1) { dtp_set_error("dtp_stamp: context_pad=%d of stamp %d must be >= 1", st[b].context_pad, b); return DTP_ERR_ARG; }
    if (st[b].steps != st[0].steps || st[b].composite != st[0].composite || st[b].output_u8 != st[0].output_u8) {
      dtp_set_error("dtp_stamp: stamp %d has steps=%d composite=%d output_u8=%d, stamp 0 has %d/%d/%d (these are per call)", b, st[b].steps,
                    st[b].composite, st[b].output_u8, st[0].steps, st[0].composite, st[0].output_u8);
      return DTP_ERR_ARG;
    }
    pads[b] = st[b].context_pad;
  }
  p.pads = pad_args(pads, B);
  p.steps = st[0].steps; p.composite = st[0].composite; p.output_u8 = st[0].output_u8;
  if (p.paste && (p.composite || p.output_u8)) {
    dtp_set_error("dtp_stroke: composite=%d output_u8=%d: both must be 0 (the stamps are pasted into the texture)", p.composite, p.output_u8);
    return DTP_ERR_ARG;
  }
  p.sched = c->scheduler;
  p.E_full = sched_evals(p.sched, p.steps);
  if (!p.init) p.E = p.E_full;
  const int E = p.E;
  // Per stamp: the third (texture-guided) branch contributes nothing once its coefficient is 0: skip it (bit-identical).  The stamps are
  // ordered by descending tg_evals (a stable order: a uniform batch keeps the identity), and evaluation i runs the UNet on
  // [uncond x B | cond x B | tg x k_i] with k_i = #{b : tg_evals_b > i}: finished stamps leave the batch.
  StampCoefs& coef = p.coef;
  for (int b = 0; b < B; ++b) {
    p.tg_evals[b] = (st[b].tg_weight == 0.0f) ? 0 : std::max(0, std::min(E, st[b].tg_steps));
    coef.cfg[b] = st[b].cfg_weight;
    coef.tg[b] = st[b].tg_weight;
    coef.order[b] = b;
  }
  std::stable_sort(coef.order, coef.order + B, [&](int x, int y) { return p.tg_evals[x] > p.tg_evals[y]; });
  for (int j = 0; j < B; ++j) coef.rank[coef.order[j]] = j;
  p.ks.resize(E);
  for (int i = 0; i < E; ++i) {
    int k = 0;
    while (k < B && p.tg_evals[coef.order[k]] > i) ++k;
    p.ks[i] = k;
  }
  const int tg_max = p.tg_evals[coef.order[0]], tg_min = p.tg_evals[coef.order[B - 1]];
  if ((c->fp8_linear || c->fp8_attention || c->fp8_operands) && tg_max != tg_min) {
    // the fp8 options calibrate each program once, for a batch whose stamps all take the same branches
    dtp_set_error("dtp_stamp: stamps with different texture-guidance evaluations (tg_evals %lld..%lld) cannot share a batch under the fp8 options",
                  (long long)tg_min, (long long)tg_max);
    return DTP_ERR_STATE;
  }
  p.use_eps = p.seeded ? p.sample_vae : p.vae_eps != nullptr;
  p.use_init = p.init && (p.seeded ? p.sample_vae : p.init_eps != nullptr);
  return DTP_OK;
}

// ---------------------------------------------------------------- the steps of a stamp, in stream order
struct StampRes {
  UNetProg* prog[DTP_STAMP_MAXB + 1] = {};  // by k
  VaeEncProg* enc = nullptr;
  VaeDecProg* dec = nullptr;
  StampBufs* sb = nullptr;
};

static int stamp_acquire(Ctx* c, const StampPlan& p, StampRes& r) {
  const int B = p.B;
  // branches 0 (uncond) and 1 (cond) see identical samples: the programs evaluate the UNet prefix once for both (unet.hip, struct Dup)
  for (int k : p.ks)
    if (!r.prog[k]) RC(get_unet_prog(c, 2 * B + k, B, &r.prog[k]));
  RC(get_enc_prog(c, (p.init ? 3 : 2) * B, &r.enc));  // strength < 1: the init image's rows join the one batched encode
  RC(get_dec_prog(c, B, &r.dec));
  RC(get_bufs(c, B, &r.sb));
  if (p.init) RC(grow_bufs_three(c, B, r.sb));
  return DTP_OK;
}

// schedule tables (update_infer_settings, inpaint_pipeline.py:39-50): rebuilt when the step count or the scheduler changes
static int stamp_refresh_schedule(Ctx* c, const StampPlan& p, hipStream_t s) {
  if (c->sched_steps == p.steps && c->sched_kind == p.sched) return DTP_OK;
  HIP_CHECK(hipStreamSynchronize(s));  // rare (a settings change): the only host-blocking part of dtp_stamp
  std::vector<float> ts(p.E_full), sc(p.E_full + 1), k((size_t)DTP_SCHED_ROW * p.E_full);
  int ne;
  float sig0;
  RC(dtp_scheduler_tables(p.sched, p.steps, &ne, &sig0, ts.data(), sc.data(), k.data()));
  RC(ensure_temb(c, ts));
  HIP_CHECK(hipMemcpy(c->stamp_params->sched, k.data(), k.size() * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(c->stamp_params->in_scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(&c->stamp_params->init_sigma, &sig0, 4, hipMemcpyHostToDevice));
  c->sched_steps = p.steps;
  c->sched_kind = p.sched;
  return DTP_OK;
}

static void stamp_write_params(Ctx* c, const StampPlan& p, hipStream_t s) {
  hipLaunchKernelGGL(set_header_kernel, dim3(1), dim3(256), 0, s, &c->stamp_params->coef, p.coef);
  hipLaunchKernelGGL(set_slots_kernel, dim3(1), dim3(64), 0, s, c->slot_map, p.slots, p.B);
  if (p.init) hipLaunchKernelGGL(set_strength_kernel, dim3(1), dim3(64), 0, s, &c->stamp_params->strength, StampStrength{p.a, p.b, p.row0, 0});
}

// cross-attention K/V for the current brushes
static int stamp_refresh_kv(Ctx* c, const StampPlan& p, StampRes& r, hipStream_t s) {
  const int B = p.B;
  for (int k = 0; k <= B; ++k) {
    UNetProg* up = r.prog[k];
    if (!up) continue;
    // the cached per-stamp matrices are valid for exactly this (B, k) split, the slots of the cond rows and these slot versions
    std::vector<int> rows(p.slots.s, p.slots.s + B);
    for (int j = 0; j < k; ++j) rows.push_back(p.slots.s[p.coef.order[j]]);
    bool valid = up->kv_ver != 0 && up->kv_B == B && up->kv_k == k && up->kv_slots == rows;
    for (size_t n = 0; valid && n < rows.size(); ++n) valid = up->kv_slot_ver[n] == c->slot_version[rows[n]];
    if (!valid) {
      hipLaunchKernelGGL(build_ctx_kernel, dim3(nblk((long long)up->N * 14 * 768)), dim3(256), 0, s, c->cond32, c->slot_map,
                         c->stamp_params->coef.order, up->ctx16, B, up->N);
      RC(up->kv.run(s, 0));
      up->kv_ver = c->cond_version; up->kv_B = B; up->kv_k = k;
      up->kv_slot_ver.resize(rows.size());
      for (size_t n = 0; n < rows.size(); ++n) up->kv_slot_ver[n] = c->slot_version[rows[n]];
      up->kv_slots = std::move(rows);
    }
  }
  return DTP_OK;
}

// pre-processing + the VAE encodes (one batch-2B pass; 3B with the init image)
static int stamp_encode(Ctx* c, const StampPlan& p, const StampRes& r, hipStream_t s) {
  RoctxRange r0("dtp_stamp: pre-processing + vae_encoder x2");
  const int B = p.B, R = c->R, HW = R * R, HWl = c->h * c->h;
  StampBufs* sb = r.sb;
  VaeEncProg* enc = r.enc;
  float* eps3 = sb->eps + (size_t)2 * B * 4 * HWl;  // (third slab: only with init)
  if (p.seeded) {  // one launch draws what the copies below deliver: latents (draw 0), the two VAE draws (1, 2), the init image's (3)
    NoiseArgs na = {};
    for (int b = 0; b < B; ++b) na.seed[b] = p.seeds[b];
    int nd = 0;
    na.dst[nd] = sb->lat; na.draw[nd++] = 0;
    if (p.use_eps) {
      na.dst[nd] = sb->eps; na.draw[nd++] = 1;
      na.dst[nd] = sb->eps + (size_t)B * 4 * HWl; na.draw[nd++] = 2;
    }
    if (p.use_init) { na.dst[nd] = eps3; na.draw[nd++] = 3; }
    RC(dtp_launch_stamp_noise(na, nd, B, HWl, s));
  } else {
    HIP_CHECK(hipMemcpyAsync(sb->lat, p.latents, (size_t)B * 4 * HWl * 4, hipMemcpyDeviceToDevice, s));
    if (p.use_eps) HIP_CHECK(hipMemcpyAsync(sb->eps, p.vae_eps, (size_t)2 * B * 4 * HWl * 4, hipMemcpyDeviceToDevice, s));
    if (p.use_init) HIP_CHECK(hipMemcpyAsync(eps3, p.init_eps, (size_t)B * 4 * HWl * 4, hipMemcpyDeviceToDevice, s));
  }
  if (!p.canvas_staged) HIP_CHECK(hipMemcpyAsync(c->canvas32, p.canvas, (size_t)B * 4 * HW * 4, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(dilate_row_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, s, c->canvas32, c->alpha_tmp, B, R, p.pads);
  hipLaunchKernelGGL(dilate_col_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, s, c->alpha_tmp,
                     c->alpha_tmp + (size_t)c->maxB * HW, B, R, p.pads);
  const int k0 = p.ks[0];
  UNetProg* first = r.prog[k0];
  // keyed by "init image on/off" (and its draw), not by the strength: the add_noise pair and start row are read from the parameter block
  StageKey key;
  key.stage = 1; key.B = B; key.k0 = k0; key.vae_eps = p.use_eps; key.init_image = p.init; key.init_eps = p.use_init;
  return graph_run(c, key, s, [&](hipStream_t q) -> int {
    hipLaunchKernelGGL(prep_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, q, c->canvas32, c->brush32, c->slot_map,
                       c->alpha_tmp + (size_t)c->maxB * HW, enc->in8, sb->masks, B, R, p.init ? 1 : 0);
    RC(enc->main.run(q, 0));
    RC(launch_vae_sample(c, enc->moments, p.use_eps ? sb->eps : nullptr, sb->ml, (p.init ? 3 : 2) * B, VAE_SCALE, q,
                         p.use_init ? eps3 : nullptr, 2 * B));
    const float* z0 = p.init ? sb->ml + (size_t)2 * B * 4 * HWl : nullptr;  // 0.18215 * sample(VAE_enc(canvas)): the init-image latents
    hipLaunchKernelGGL(assemble_kernel, dim3(nblk((long long)B * HWl)), dim3(256), 0, q, sb->lat, z0, sb->masks, sb->ml,
                       c->stamp_params->coef.rank, first->in16, c->x32, c->stamp_params, 0, B, HWl, k0);
    return LAUNCH_OK();
  });
}

// fp8 (configs[4]): the first stamp of a program measures its activation ranges once, before the loop is captured.  (Under these
// options every stamp of the batch has the same tg_evals: the programs are the 3B one for the first evaluations, the 2B one after.)
static int stamp_calibrate_fp8(Ctx* c, const StampPlan& p, const StampRes& r, hipStream_t s) {
  if (!(c->fp8_linear || c->fp8_attention || c->fp8_operands)) return DTP_OK;
  const int B = p.B, HWl = c->h * c->h;
  UNetProg *u3 = r.prog[B], *u2 = r.prog[0];
  if (u3 && !u3->fp8_calibrated) RC(fp8_calibrate(c, u3, s, 0));
  if (u2 && !u2->fp8_calibrated) {
    if (p.ks[0] > 0)  // (u2 is not the first program:) its input is normally assembled where the loop switches programs: do it now, from the initial latents
      hipLaunchKernelGGL(assemble_kernel, dim3(nblk((long long)B * HWl)), dim3(256), 0, s, (const float*)nullptr, (const float*)nullptr,
                         r.sb->masks, r.sb->ml, c->stamp_params->coef.rank, u2->in16, c->x32, c->stamp_params, 0, B, HWl, 0);
    RC(fp8_calibrate(c, u2, s, 0));
  }
  return DTP_OK;
}

// the denoise loop
static int stamp_loop(Ctx* c, const StampPlan& p, const StampRes& r, hipStream_t s) {
  RoctxRange r1("dtp_stamp: denoise loop (unet)");
  const int B = p.B, HWl = c->h * c->h;
  StageKey key;
  key.stage = 2; key.B = B; key.sched = p.sched; key.steps = p.steps; key.row0 = p.row0;
  for (int j = 0; j < B; ++j) key.tg_profile.push_back(p.tg_evals[p.coef.order[j]]);
  return graph_run(c, key, s, [&](hipStream_t q) -> int {
    StampParams* pb = c->stamp_params;
    for (int i = 0; i < p.E; ++i) {
      UNetProg* up = r.prog[p.ks[i]];
      if (i > 0 && p.ks[i] != p.ks[i - 1]) {
        // switching to a program with fewer tg rows: its input needs mask/masked-latent channels + current x
        hipLaunchKernelGGL(assemble_kernel, dim3(nblk((long long)B * HWl)), dim3(256), 0, q, (const float*)nullptr, (const float*)nullptr,
                           r.sb->masks, r.sb->ml, pb->coef.rank, up->in16, c->x32, pb, p.row0 + i, B, HWl, p.ks[i]);
      }
      const int row = p.row0 + i;  // the table row (temb, in_scale, sched) of loop index i
      RC(up->main.run(q, row));
      RC(launch_step(p.sched, up->out32, c->x32, up->in16, c->hist32, pb->sched + DTP_SCHED_ROW * row, pb->in_scale + row + 1, pb->coef.cfg,
                     pb->coef.tg, pb->coef.rank, i, B, HWl, p.ks[i], q));
    }
    return LAUNCH_OK();
  });
}

// latents / 0.18215 -> VAE decode -> clamp (+ composite, u8), and the finiteness guard
static int stamp_decode(Ctx* c, const StampPlan& p, const StampRes& r, hipStream_t s) {
  const int B = p.B, HW = c->R * c->R, HWl = c->h * c->h;
  VaeDecProg* dec = r.dec;
  {
    RoctxRange r2("dtp_stamp: vae decode + post-processing");
    StageKey key;
    key.stage = 3; key.B = p.B;
    RC(graph_run(c, key, s, [&](hipStream_t q) -> int {
      RC(launch_post_quant(c, c->x32, 1, 1.0f / VAE_SCALE, dec->in8, B, q));
      return dec->main.run(q, 0);
    }));
    if (p.paste)  // a stroke group: straight into the texture, no [B,3,R,R] image in between
      RC(p.paste(dec->out32, c->R, B, s));
    else
      hipLaunchKernelGGL(finish_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, s, dec->out32, c->canvas32, p.out, B, HW, p.composite,
                         p.output_u8);
  }
  c->finite_pending = c->check_finite;
  if (c->check_finite) {
    HIP_CHECK(hipMemsetAsync(c->finite_flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(finite_check_kernel, dim3(nblk((long long)B * HW * 4)), dim3(256), 0, s, c->x32, (long long)B * HWl * 4, dec->out32,
                       (long long)B * HW * 4, c->finite_flag);
  }
  return DTP_OK;
}

int stamp_enqueue(Ctx* c, const StampPlan& p, hipStream_t s) {
  HIP_CHECK(hipSetDevice(c->device));
  StampRes r;
  RC(stamp_acquire(c, p, r));
  RC(stamp_refresh_schedule(c, p, s));
  stamp_write_params(c, p, s);
  RC(stamp_refresh_kv(c, p, r, s));
  c->last_nodes = 0; c->last_evals = p.E; c->last_unet_rows = 0;
  for (int k : p.ks) c->last_unet_rows += 2 * p.B + k;
  RoctxRange whole("dtp_stamp");
  HIP_CHECK(hipEventRecord(c->ev[0], s));
  RC(stamp_encode(c, p, r, s));
  HIP_CHECK(hipEventRecord(c->ev[1], s));
  RC(stamp_calibrate_fp8(c, p, r, s));
  RC(stamp_loop(c, p, r, s));
  HIP_CHECK(hipEventRecord(c->ev[2], s));
  RC(stamp_decode(c, p, r, s));
  HIP_CHECK(hipEventRecord(c->ev[3], s));
  return LAUNCH_OK();
}

static int stamp_run(dtp_ctx* ctx, StampPlan& p, dtp_stream s) {
  RC(stamp_plan((Ctx*)ctx, p));
  return stamp_enqueue((Ctx*)ctx, p, (hipStream_t)s);
}

// ---------------------------------------------------------------- C ABI: the stamp entry points
extern "C" {

int dtp_stamp(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
              void* out, int B, dtp_stream s) {
  return dtp_stamp_slots(ctx, canvas, st, latents, vae_eps, out, B, nullptr, s);
}

int dtp_stamp_slots(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                    void* out, int B, const int* slots, dtp_stream s) {
  if (!st || B < 1 || B > DTP_STAMP_MAXB) return dtp_stamp_mixed(ctx, canvas, st, latents, vae_eps, out, B, slots, s);  // (its checks)
  dtp_settings each[DTP_STAMP_MAXB];
  for (int b = 0; b < B; ++b) each[b] = *st;
  return dtp_stamp_mixed(ctx, canvas, each, latents, vae_eps, out, B, slots, s);
}

int dtp_stamp_mixed(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                    void* out, int B, const int* slots, dtp_stream s) {
  return dtp_stamp_strength(ctx, canvas, st, latents, vae_eps, nullptr, 1.0, out, B, slots, s);  // (strength 1 ignores init_eps)
}

int dtp_stamp_strength(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                       const float* init_eps, double strength, void* out, int B, const int* slots, dtp_stream s) {
  StampPlan p;
  p.canvas = canvas; p.st = st; p.out = out; p.B = B; p.slot_ids = slots; p.strength = strength;
  p.latents = latents; p.vae_eps = vae_eps; p.init_eps = init_eps;
  return stamp_run(ctx, p, s);
}

int dtp_stamp_seeded(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const uint64_t* seeds, int sample_vae, double strength,
                     void* out, int B, const int* slots, dtp_stream s) {
  StampPlan p;
  p.canvas = canvas; p.st = st; p.out = out; p.B = B; p.slot_ids = slots; p.strength = strength;
  p.seeded = true; p.seeds = seeds; p.sample_vae = sample_vae != 0;
  return stamp_run(ctx, p, s);
}

}  // extern "C"
