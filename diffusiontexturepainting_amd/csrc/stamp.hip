// The stamp: everything TRTConditionalInpainter.generate_raw / InpaintPipeline.infer do around the
// three networks, as fused HIP kernels + hipGraph replay.
// Reference: trt_inference/trt_model.py:90-121, handler.py:25-33,55-56, model_base.py:51-58,
// inpaint_pipeline.py:39-153, stable_diffusion_pipeline.py:340-355,407-484, utilities.py:370-529.
#include <math.h>
#include <algorithm>
#include <stdio.h>
#include <string.h>

#include "engine.h"
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

int get_unet_prog(Ctx* c, int N, int dupB, UNetProg** out);
int get_enc_prog(Ctx* c, int B, VaeEncProg** out);
int get_dec_prog(Ctx* c, int B, VaeDecProg** out);
int launch_vae_sample(Ctx* c, const float* mom, const float* eps, float* out, int B, float scale, hipStream_t s, const float* eps3, int n_eps);
int launch_post_quant(Ctx* c, const float* z, int nhwc, float in_scale, f16* out, int B, hipStream_t s);
int load_imgenc_weights(Ctx* c);
void dtp_gemm_init();
void dtp_conv_halo_init();
void dtp_gemm_wide_init();
void dtp_gemm_fp8_init();

#define VAE_SCALE 0.18215f

// ---------------------------------------------------------------- DDIM tables (host, fp32 like torch)
// alphas_cumprod of the scaled-linear beta schedule every sampler shares (utilities.py:383-388, :283-285, :684-688)
static const float* alphas_cumprod() {
  static float full[1000];
  static bool have = false;
  if (!have) {
    const int T = 1000;
    const float start = (float)sqrt(0.00085), end = (float)sqrt(0.012);
    const float step = (end - start) / (float)(T - 1);
    double acc = 1.0;  // torch's CPU cumprod accumulates float in double and rounds every output
    for (int i = 0; i < T; ++i) {
      const float l = (i < T / 2) ? start + step * (float)i : end - step * (float)(T - 1 - i);
      const float beta = l * l;
      acc *= (double)(1.0f - beta);
      full[i] = (float)acc;
    }
    have = true;
  }
  return full;
}

// utilities.py:432-439 (timesteps), :416 (gather), :397 (final alpha).
extern "C" int dtp_ddim_tables(int steps, int64_t* timesteps, float* alphas, float* final_alpha) {
  // the largest timestep is (steps-1)*(1000/steps) + 1: steps = 1000 would index alphas_cumprod[1000] (the reference raises
  // IndexError there, utilities.py:416)
  if (steps < 1 || steps > 999) { dtp_set_error("ddim: steps %d outside 1..999", steps); return DTP_ERR_ARG; }
  const int T = 1000;
  const float* full = alphas_cumprod();
  const int ratio = T / steps;
  for (int i = 0; i < steps; ++i) {
    const int64_t t = (int64_t)(steps - 1 - i) * ratio + 1;
    if (timesteps) timesteps[i] = t;
    if (alphas) alphas[i] = full[t];
  }
  if (final_alpha) *final_alpha = full[0];
  return DTP_OK;
}

// ---------------------------------------------------------------- schedule tables of every sampler (host)
static int sched_evals(int scheduler, int steps) { return scheduler == DTP_SCHED_DDIM ? steps - 1 : steps; }

// integral over [a, b] of prod_{m != j} (tau - s[m]) / (s[j] - s[m]) (m, j < n <= 4): the Lagrange basis polynomial is expanded
// into monomials and integrated exactly (the reference integrates it numerically, scipy quad with epsrel 1e-4: utilities.py:330-341)
static double lagrange_integral(const double* s, int n, int j, double a, double b) {
  double p[4] = {1.0, 0.0, 0.0, 0.0};  // p[d]: coefficient of tau^d
  int deg = 0;
  for (int m = 0; m < n; ++m) {
    if (m == j) continue;
    const double inv = 1.0 / (s[j] - s[m]);
    for (int d = deg + 1; d >= 0; --d) p[d] = ((d > 0 ? p[d - 1] : 0.0) - s[m] * p[d]) * inv;
    ++deg;
  }
  double r = 0.0;
  for (int d = 0; d <= deg; ++d) r += p[d] * (pow(b, d + 1) - pow(a, d + 1)) / (d + 1);
  return r;
}

extern "C" int dtp_scheduler_tables(int scheduler, int steps, int* evals, float* init_sigma, float* timesteps, float* in_scale,
                                    float* coefs) {
  if (scheduler != DTP_SCHED_DDIM && scheduler != DTP_SCHED_DPM && scheduler != DTP_SCHED_LMSD) {
    dtp_set_error("scheduler tables: unknown scheduler %d (DDIM = 0, DPM = 1, LMSD = 2)", scheduler);
    return DTP_ERR_ARG;
  }
  if (steps < 2 || steps > 999) { dtp_set_error("scheduler tables: steps %d outside 2..999", steps); return DTP_ERR_ARG; }
  const int E = sched_evals(scheduler, steps), W = DTP_SCHED_ROW;
  const float* full = alphas_cumprod();
  std::vector<float> ts(E), sc(E + 1, 1.0f), k((size_t)E * W, 0.0f);
  float sig0 = 1.0f;
  if (scheduler == DTP_SCHED_DDIM) {  // the N - 1 evaluations of timesteps[1:] (stable_diffusion_pipeline.py:348-355)
    std::vector<int64_t> t(steps);
    std::vector<float> al(steps);
    float fin;
    RC(dtp_ddim_tables(steps, t.data(), al.data(), &fin));
    for (int i = 0; i < E; ++i) {
      const int idx = 1 + i;
      const float a_t = al[idx], a_prev = (idx + 1 < steps) ? al[idx + 1] : fin;
      ts[i] = (float)t[idx];
      k[W * i + 0] = sqrtf(1.0f - a_t);
      k[W * i + 1] = sqrtf(a_t);
      k[W * i + 2] = sqrtf(a_prev);
      k[W * i + 3] = sqrtf(1.0f - a_prev);
    }
  } else if (scheduler == DTP_SCHED_DPM) {
    // set_timesteps: linspace(0, 999, N + 1).round()[::-1][:-1] -- numpy rounds half to even (utilities.py:797-805)
    std::vector<int> t(steps + 1);
    for (int i = 0; i < steps; ++i) t[i] = (int)nearbyint((double)(steps - i) * (999.0 / steps));
    t[0] = 999;
    t[steps] = 0;  // prev_timestep of the last evaluation (utilities.py:970)
    // alpha_t, sigma_t, lambda_t in fp32 like the reference's torch tables (utilities.py:692-694)
    auto alpha = [&](int i) { return sqrtf(full[i]); };
    auto sigma = [&](int i) { return sqrtf(1.0f - full[i]); };
    auto lambda = [&](int i) { return logf(alpha(i)) - logf(sigma(i)); };
    for (int i = 0; i < E; ++i) {
      const int s0 = t[i], tt = t[i + 1];
      const float h = lambda(tt) - lambda(s0);
      const float c2 = alpha(tt) * (expf(-h) - 1.0f);
      // first order at the first evaluation and, for schedules shorter than 15, at the last (lower_order_final, :971-985)
      const bool first = i == 0 || (i == E - 1 && steps < 15);
      float inv_r0 = 0.0f;
      if (i > 0) {
        const float h0 = lambda(s0) - lambda(t[i - 1]);
        inv_r0 = 1.0f / (h0 / h);  // D1 = (1 / r0) (m0 - m1), utilities.py:907-912
      }
      ts[i] = (float)s0;
      float* r = &k[W * i];
      r[0] = alpha(s0);
      r[1] = sigma(s0);
      r[2] = first ? 1.0f : 2.0f;
      r[3] = sigma(tt) / sigma(s0);
      r[4] = c2;
      r[5] = 0.5f * c2;
      r[6] = first ? 0.0f : inv_r0;
    }
  } else {  // LMSD
    // sigmas of the training schedule, fp32 like torch; init_noise_sigma is their maximum (utilities.py:286-292)
    float sfull[1000];
    for (int i = 0; i < 1000; ++i) sfull[i] = sqrtf((1.0f - full[i]) / full[i]);
    sig0 = *std::max_element(sfull, sfull + 1000);
    // set_timesteps: timesteps = linspace(0, 999, N)[::-1], sigmas = np.interp(timesteps, arange(1000), sfull) + [0] (:298-306)
    std::vector<float> sg(steps + 1, 0.0f);
    for (int i = 0; i < steps; ++i) {
      const double x = i == 0 ? 999.0 : (double)(steps - 1 - i) * (999.0 / (steps - 1));
      const int j = std::min((int)x, 998);
      const double v = x == (double)j ? (double)sfull[j]
                                      : ((double)sfull[j + 1] - (double)sfull[j]) * (x - (double)j) + (double)sfull[j];
      ts[i] = (float)x;
      sg[i] = (float)v;
    }
    for (int i = 0; i <= steps; ++i) sc[i] = 1.0f / sqrtf(sg[i] * sg[i] + 1.0f);  // latent_scales (:314)
    // configure() (:316-343) rebinds its local `order` to min(step_index + 1, order) on every pass, so after the first evaluation it
    // stays 1: every row of the reference is first order.  Reproduced; the row and the kernel carry orders up to 4.
    int order = 4;
    for (int i = 0; i < E; ++i) {
      order = std::min(i + 1, order);
      double s[4];
      for (int m = 0; m < order; ++m) s[m] = (double)sg[i - m];
      float* r = &k[W * i];
      r[0] = sg[i];
      r[1] = (float)order;
      for (int j = 0; j < order; ++j) r[2 + j] = (float)lagrange_integral(s, order, j, (double)sg[i], (double)sg[i + 1]);
    }
  }
  if (evals) *evals = E;
  if (init_sigma) *init_sigma = sig0;
  if (timesteps) memcpy(timesteps, ts.data(), (size_t)E * 4);
  if (in_scale) memcpy(in_scale, sc.data(), (size_t)(E + 1) * 4);
  if (coefs) memcpy(coefs, k.data(), k.size() * 4);
  return DTP_OK;
}

// initialize_timesteps (stable_diffusion_pipeline.py:348-355) in double, as Python evaluates it, and the add_noise pair of the sampler at
// t_start (utilities.py:363-366 LMSD, :524-529 DDIM on the gathered table, :1000-1008 DPM on the full table at timesteps[t_start]).
extern "C" int dtp_strength_schedule(int scheduler, int steps, double strength, int* t_start, int* evals, float* noise_coefs) {
  if (!(strength > 0.0 && strength <= 1.0)) {  // (NaN fails both)
    dtp_set_error("strength schedule: strength %g outside (0, 1]", strength);
    return DTP_ERR_ARG;
  }
  const int E_full = (scheduler == DTP_SCHED_DDIM || scheduler == DTP_SCHED_DPM || scheduler == DTP_SCHED_LMSD) ? sched_evals(scheduler, steps) : 0;
  std::vector<float> k((size_t)std::max(E_full, 1) * DTP_SCHED_ROW);
  int ne;
  float sig0;
  RC(dtp_scheduler_tables(scheduler, steps, &ne, &sig0, nullptr, nullptr, k.data()));  // (its checks: scheduler, steps)
  const int offset = scheduler == DTP_SCHED_DDIM ? 1 : 0;  // steps_offset (utilities.py:379, :274, :664)
  const int init = std::min((int)((double)steps * strength) + offset, steps);
  const int ts = std::max(steps - init + offset, 0);
  const int E = steps - ts;
  if (E < 1) {
    dtp_set_error("strength schedule: strength %g leaves no evaluation at %d steps (int(steps * strength) = 0)", strength, steps);
    return DTP_ERR_ARG;
  }
  float a = 0.0f, b = sig0;  // strength 1: latents * init_noise_sigma
  if (strength < 1.0) {
    const float* r = &k[(size_t)DTP_SCHED_ROW * (ts - offset)];
    if (scheduler == DTP_SCHED_DDIM) { a = r[1]; b = r[0]; }        // sqrt(a_t), sqrt(1 - a_t) of the gathered alphas_cumprod[t_start]
    else if (scheduler == DTP_SCHED_DPM) { a = r[0]; b = r[1]; }    // alpha_s, sigma_s at timesteps[t_start]
    else { a = 1.0f; b = r[0]; }                                     // z0 + sigma[t_start] eps
  }
  if (t_start) *t_start = ts;
  if (evals) *evals = E;
  if (noise_coefs) { noise_coefs[0] = a; noise_coefs[1] = b; }
  return DTP_OK;
}

// ---------------------------------------------------------------- kernels
namespace {

// separable flat dilation (kornia.morphology.dilation with ones(pad,pad), geodesic border), each stamp with its own pad:
// out[i] = max over [i - lo[b], i + hi[b]] clipped to the image, lo = pad/2, hi = pad - pad/2 - 1.
struct PadArgs { int lo[DTP_STAMP_MAXB], hi[DTP_STAMP_MAXB]; };
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
// u8 conversion (handler.py:55-56).
__global__ void finish_kernel(const float* __restrict__ dec, const float* __restrict__ canvas, void* __restrict__ out, int B,
                              int HW, int composite, int u8) {
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / HW), pix = (int)(i - (long long)b * HW);
    const float a = composite ? canvas[((size_t)b * 4 + 3) * HW + pix] : 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v = fminf(fmaxf(dec[i * 4 + ch] / 2.0f + 0.5f, 0.f), 1.f);
      if (composite) v = canvas[((size_t)b * 4 + ch) * HW + pix] * a + v * (1.0f - a);
      if (u8) ((unsigned char*)out)[i * 3 + ch] = (unsigned char)(v * 255.0f);
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

struct SlotArgs { int s[64]; };
// the per-stamp slot ids travel as a kernel argument (no host staging buffer to keep alive, no sync)
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

int stamp_init(Ctx* c) {
  void* p;
  const size_t hw = (size_t)c->h * c->h, RR = (size_t)c->R * c->R;
  RC(ctx_persistent(c, c->maxB * hw * 4 * 4, &p, true)); c->x32 = (float*)p;
  RC(ctx_persistent(c, 3 * c->maxB * hw * 4 * 4, &p, true)); c->hist32 = (float*)p;
  RC(ctx_persistent(c, c->maxB * 4 * RR * 4, &p, true)); c->canvas32 = (float*)p;
  RC(ctx_persistent(c, 2 * c->maxB * RR * 4, &p, true)); c->alpha_tmp = (float*)p;
  RC(ctx_persistent(c, sizeof(StampParams), &p, true)); c->stamp_params = (StampParams*)p;
  RC(ctx_persistent(c, (size_t)DTP_MAX_SLOTS * 2 * 14 * 768 * 4, &p, true)); c->cond32 = (float*)p;
  RC(ctx_persistent(c, (size_t)DTP_MAX_SLOTS * 3 * RR * 4, &p, true)); c->brush32 = (float*)p;
  RC(ctx_persistent(c, 64 * sizeof(int), &p, true)); c->slot_map = (int*)p;
  RC(ctx_persistent(c, 256, &p, true)); c->finite_flag = (int*)p;
  return DTP_OK;
}

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

static void destroy_graph(StampGraph& g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
}

// the first strength < 1 stamp of batch B: masked latents and VAE draws get a third slab (the init image).  The captured stages of B
// hold the two-slab buffers: they are dropped (a one-time wait, like building the 3B encoder program) and recaptured on the new ones,
// which every later stamp of B, strength 1 or not, uses.
static int grow_bufs_three(Ctx* c, int B, StampBufs* sb) {
  if (sb->three) return DTP_OK;
  HIP_CHECK(hipDeviceSynchronize());  // a captured stage may still be replaying on the old buffers
  for (auto g = c->graphs.begin(); g != c->graphs.end();) {
    if (((g->first[0] >> 32) & 0xff) == B) { destroy_graph(g->second); g = c->graphs.erase(g); }
    else ++g;
  }
  void* p;
  const size_t hw = (size_t)c->h * c->h;
  RC(ctx_persistent(c, 3 * B * 4 * hw * 4, &p, true)); sb->ml = (float*)p;
  RC(ctx_persistent(c, 3 * B * 4 * hw * 4, &p, true)); sb->eps = (float*)p;
  sb->three = true;
  return DTP_OK;
}

// run `body` on stream s, replaying a captured hipGraph when possible.  `loop`: a denoise-loop graph, of which the context keeps the
// DTP_LOOP_GRAPH_CAP most recently replayed
template <class F>
static int run_stage(Ctx* c, const std::vector<long long>& key, bool loop, hipStream_t s, F body) {
  if (!c->use_graph || c->profile || s == nullptr) return body(s);
  auto it = c->graphs.find(key);
  if (it == c->graphs.end()) {
    if (loop) {
      int n = 0;
      auto lru = c->graphs.end();
      for (auto g = c->graphs.begin(); g != c->graphs.end(); ++g) {
        if (g->first[0] >> 60 != 2) continue;
        ++n;
        if (lru == c->graphs.end() || g->second.used < lru->second.used) lru = g;
      }
      if (n >= DTP_LOOP_GRAPH_CAP) {  // (rare: a new profile; its capture costs far more than this wait)
        HIP_CHECK(hipDeviceSynchronize());  // the evicted graph may still be replaying
        destroy_graph(lru->second);
        c->graphs.erase(lru);
      }
    }
    StampGraph g;
    HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = body(s);
    hipError_t e = hipStreamEndCapture(s, &g.graph);
    if (rc != DTP_OK) { if (g.graph) (void)hipGraphDestroy(g.graph); return rc; }
    if (e != hipSuccess) { dtp_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return DTP_ERR_HIP; }
    size_t n = 0;
    (void)hipGraphGetNodes(g.graph, nullptr, &n);
    g.nodes = (int)n;
    HIP_CHECK(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    it = c->graphs.emplace(key, g).first;
  }
  it->second.used = ++c->graph_clock;
  c->last_nodes += it->second.nodes;
  HIP_CHECK(hipGraphLaunch(it->second.exec, s));
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

int dtp_finalize_weights(dtp_ctx* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { dtp_set_error("dtp_finalize_weights: null handle"); return DTP_ERR_ARG; }
  if (c->finalized) { dtp_set_error("dtp_finalize_weights: already finalized"); return DTP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(c->device));
  dtp_gemm_init();
  dtp_conv_halo_init();
  dtp_gemm_wide_init();
  dtp_gemm_fp8_init();
  dtp_gemm_f8f8_init();
  dtp_xattn_init();
  dtp_lnlin_init();
  dtp_xchain_init();
  dtp_ffchain_init();
  dtp_conv_ws_init();
  dtp_gemm_ws_init();
  RC(load_unet_weights(c));
  RC(load_vae_weights(c));
  bool has_clip = false;
  for (auto& kv : c->staged)
    if (kv.first.rfind("clip.", 0) == 0) { has_clip = true; break; }
  if (has_clip) RC(load_imgenc_weights(c));
  HIP_CHECK(hipDeviceSynchronize());
  for (auto& s : c->staged) (void)hipFree(s.second.d);
  c->staged.clear();
  RC(stamp_init(c));
  c->finalized = true;
  return DTP_OK;
}

int dtp_set_conditioning_slot(dtp_ctx* ctx, int slot, const float* cond, const float* uncond, const float* brush, dtp_stream s_) {
  Ctx* c = (Ctx*)ctx;
  hipStream_t s = (hipStream_t)s_;
  if (!c || !c->finalized || !cond || !uncond || !brush) { dtp_set_error("dtp_set_conditioning: bad state/argument"); return DTP_ERR_STATE; }
  if (slot < 0 || slot >= DTP_MAX_SLOTS) { dtp_set_error("dtp_set_conditioning: slot %d outside 0..%d", slot, DTP_MAX_SLOTS - 1); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(c->device));
  float* dst = c->cond32 + (size_t)slot * 2 * 14 * 768;
  HIP_CHECK(hipMemcpyAsync(dst, cond, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dst + 14 * 768, uncond, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(c->brush32 + (size_t)slot * 3 * c->R * c->R, brush, (size_t)3 * c->R * c->R * 4, hipMemcpyDeviceToDevice, s));
  c->slot_set[slot] = true;
  c->slot_version[slot] = ++c->cond_version;
  return DTP_OK;
}

int dtp_set_conditioning(dtp_ctx* ctx, const float* cond, const float* uncond, const float* brush, dtp_stream s) {
  return dtp_set_conditioning_slot(ctx, 0, cond, uncond, brush, s);
}

int dtp_get_conditioning_slot(dtp_ctx* ctx, int slot, float* cond, float* uncond, dtp_stream s_) {
  Ctx* c = (Ctx*)ctx;
  hipStream_t s = (hipStream_t)s_;
  if (!c || slot < 0 || slot >= DTP_MAX_SLOTS || !c->slot_set[slot]) { dtp_set_error("dtp_get_conditioning: no brush set in slot %d", slot); return DTP_ERR_STATE; }
  const float* src = c->cond32 + (size_t)slot * 2 * 14 * 768;
  HIP_CHECK(hipMemcpyAsync(cond, src, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(uncond, src + 14 * 768, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  return DTP_OK;
}

int dtp_get_conditioning(dtp_ctx* ctx, float* cond, float* uncond, dtp_stream s) { return dtp_get_conditioning_slot(ctx, 0, cond, uncond, s); }

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

// a strength < 1 stamp (dtp_stamp_strength): its loop runs rows [row, row + evals) of the (scheduler, steps) tables from the init image
struct StrengthPlan {
  int row, evals;
  float a, b;
  const float* init_eps;
};

// a seeded stamp (dtp_stamp_seeded): the call's draws are generated into the staging buffers (noise.hip) instead of copied from the caller
struct SeedPlan {
  const uint64_t* seeds;  // host, [B]
  bool sample_vae;        // draws 1, 2 (and 3 below strength 1) are used; false = the distribution means
};

static int stamp_run(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                     void* out, int B, const int* slots, dtp_stream s_, const StrengthPlan* sp, const SeedPlan* seeded = nullptr);

int dtp_stamp_mixed(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                    void* out, int B, const int* slots, dtp_stream s) {
  return stamp_run(ctx, canvas, st, latents, vae_eps, out, B, slots, s, nullptr);
}

// dtp_stamp_strength, and dtp_stamp_seeded with `seeded` in place of the three noise pointers
static int stamp_strength(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                          const float* init_eps, double strength, void* out, int B, const int* slots, dtp_stream s, const SeedPlan* seeded) {
  Ctx* c = (Ctx*)ctx;
  if (!(strength > 0.0 && strength <= 1.0)) { dtp_set_error("dtp_stamp_strength: strength %g outside (0, 1]", strength); return DTP_ERR_ARG; }
  if (strength == 1.0) return stamp_run(ctx, canvas, st, latents, vae_eps, out, B, slots, s, nullptr, seeded);  // dtp_stamp_mixed, init_eps unused
  if (!c || !c->finalized) { dtp_set_error("dtp_stamp: weights not finalized"); return DTP_ERR_STATE; }
  if (!st || B < 1 || B > c->maxB) { dtp_set_error("dtp_stamp: bad argument (B=%d, max %d)", B, c->maxB); return DTP_ERR_ARG; }
  if (c->fp8_linear || c->fp8_attention || c->fp8_operands) {
    dtp_set_error("dtp_stamp_strength: strength < 1 is not offered under the fp8 options (parity-only, calibrated per program)");
    return DTP_ERR_STATE;
  }
  const int sched = c->scheduler;
  StrengthPlan sp;
  int t_start;
  float ab[2];
  if (st[0].steps < 2 || st[0].steps > 999) { dtp_set_error("dtp_stamp: steps=%d of stamp 0 outside 2..999", st[0].steps); return DTP_ERR_ARG; }
  const int rc = dtp_strength_schedule(sched, st[0].steps, strength, &t_start, &sp.evals, ab);
  if (rc) { dtp_set_error("dtp_stamp_strength: strength %g leaves no evaluation at %d steps", strength, st[0].steps); return rc; }
  sp.row = t_start - (sched == DTP_SCHED_DDIM ? 1 : 0);
  sp.a = ab[0];
  sp.b = ab[1];
  sp.init_eps = init_eps;
  return stamp_run(ctx, canvas, st, latents, vae_eps, out, B, slots, s, &sp, seeded);
}

int dtp_stamp_strength(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                       const float* init_eps, double strength, void* out, int B, const int* slots, dtp_stream s) {
  return stamp_strength(ctx, canvas, st, latents, vae_eps, init_eps, strength, out, B, slots, s, nullptr);
}

int dtp_stamp_seeded(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const uint64_t* seeds, int sample_vae, double strength,
                     void* out, int B, const int* slots, dtp_stream s) {
  if (!seeds) { dtp_set_error("dtp_stamp_seeded: seeds is NULL (one uint64 per stamp, host memory)"); return DTP_ERR_ARG; }
  const SeedPlan seeded = {seeds, sample_vae != 0};
  return stamp_strength(ctx, canvas, st, nullptr, nullptr, nullptr, strength, out, B, slots, s, &seeded);
}

static int stamp_run(dtp_ctx* ctx, const float* canvas, const dtp_settings* st, const float* latents, const float* vae_eps,
                     void* out, int B, const int* slots, dtp_stream s_, const StrengthPlan* sp, const SeedPlan* seeded) {
  Ctx* c = (Ctx*)ctx;
  hipStream_t s = (hipStream_t)s_;
  if (!c || !c->finalized) { dtp_set_error("dtp_stamp: weights not finalized"); return DTP_ERR_STATE; }
  if (!canvas || !st || (!latents && !seeded) || !out || B < 1 || B > c->maxB) { dtp_set_error("dtp_stamp: bad argument (B=%d, max %d)", B, c->maxB); return DTP_ERR_ARG; }
  SlotArgs sa = {};
  for (int b = 0; b < B; ++b) {
    const int sl = slots ? slots[b] : 0;
    if (sl < 0 || sl >= DTP_MAX_SLOTS) { dtp_set_error("dtp_stamp: slot %d of stamp %d outside 0..%d", sl, b, DTP_MAX_SLOTS - 1); return DTP_ERR_ARG; }
    if (!c->slot_set[sl]) { dtp_set_error("dtp_stamp: no brush set in slot %d (call dtp_set_brush / dtp_set_conditioning)", sl); return DTP_ERR_STATE; }
    sa.s[b] = sl;
  }
  for (int b = 0; b < B; ++b) {
    if (st[b].steps < 2 || st[b].steps > 999) { dtp_set_error("dtp_stamp: steps=%d of stamp %d outside 2..999", st[b].steps, b); return DTP_ERR_ARG; }
    if (st[b].context_pad < 1) { dtp_set_error("dtp_stamp: context_pad=%d of stamp %d must be >= 1", st[b].context_pad, b); return DTP_ERR_ARG; }
    if (st[b].steps != st[0].steps || st[b].composite != st[0].composite || st[b].output_u8 != st[0].output_u8) {
      dtp_set_error("dtp_stamp: stamp %d has steps=%d composite=%d output_u8=%d, stamp 0 has %d/%d/%d (these are per call)", b, st[b].steps,
                    st[b].composite, st[b].output_u8, st[0].steps, st[0].composite, st[0].output_u8);
      return DTP_ERR_ARG;
    }
  }
  const int R = c->R, h = c->h, HW = R * R, HWl = h * h;
  const int steps = st[0].steps, sched = c->scheduler, E_full = sched_evals(sched, steps);
  // strength < 1: the loop runs rows [row0, row0 + E) of the tables (the reference index t_start + i, minus steps_offset)
  const int row0 = sp ? sp->row : 0, E = sp ? sp->evals : E_full;
  // Per stamp: the third (texture-guided) branch contributes nothing once its coefficient is 0: skip it (bit-identical).  The stamps are
  // ordered by descending tg_evals (a stable order: a uniform batch keeps the identity), and evaluation i runs the UNet on
  // [uncond x B | cond x B | tg x k_i] with k_i = #{b : tg_evals_b > i}: finished stamps leave the batch.
  int tg_evals[DTP_STAMP_MAXB];
  StampCoefs coef = {};
  for (int b = 0; b < B; ++b) {
    tg_evals[b] = (st[b].tg_weight == 0.0f) ? 0 : std::max(0, std::min(E, st[b].tg_steps));
    coef.cfg[b] = st[b].cfg_weight;
    coef.tg[b] = st[b].tg_weight;
    coef.order[b] = b;
  }
  std::stable_sort(coef.order, coef.order + B, [&](int x, int y) { return tg_evals[x] > tg_evals[y]; });
  std::vector<long long> loop_key = {((long long)B << 32) | ((long long)sched << 40) | ((long long)steps << 12) | ((long long)row0 << 44) |
                                     (2LL << 60)};
  for (int j = 0; j < B; ++j) { coef.rank[coef.order[j]] = j; loop_key.push_back(tg_evals[coef.order[j]]); }
  std::vector<int> ks(E);  // k_i
  for (int i = 0; i < E; ++i) {
    int k = 0;
    while (k < B && tg_evals[coef.order[k]] > i) ++k;
    ks[i] = k;
  }
  if ((c->fp8_linear || c->fp8_attention || c->fp8_operands) && loop_key[1] != loop_key[B]) {
    // the fp8 options calibrate each program once, for a batch whose stamps all take the same branches
    dtp_set_error("dtp_stamp: stamps with different texture-guidance evaluations (tg_evals %lld..%lld) cannot share a batch under the fp8 options",
                  loop_key[B], loop_key[1]);
    return DTP_ERR_STATE;
  }
  HIP_CHECK(hipSetDevice(c->device));

  UNetProg* prog[DTP_STAMP_MAXB + 1] = {};  // by k
  VaeEncProg* enc;
  VaeDecProg* dec;
  StampBufs* sb;
  // branches 0 (uncond) and 1 (cond) see identical samples: the programs evaluate the UNet prefix once for both (unet.hip, struct Dup)
  for (int i = 0; i < E; ++i)
    if (!prog[ks[i]]) RC(get_unet_prog(c, 2 * B + ks[i], B, &prog[ks[i]]));
  RC(get_enc_prog(c, (sp ? 3 : 2) * B, &enc));  // strength < 1: the init image's rows join the one batched encode
  RC(get_dec_prog(c, B, &dec));
  RC(get_bufs(c, B, &sb));
  if (sp) RC(grow_bufs_three(c, B, sb));

  // ---- schedule tables (update_infer_settings, inpaint_pipeline.py:39-50): rebuilt when the step count or the scheduler changes
  if (c->sched_steps != steps || c->sched_kind != sched) {  // rare (a settings change): the only host-blocking part of dtp_stamp
    HIP_CHECK(hipStreamSynchronize(s));
    std::vector<float> ts(E_full), sc(E_full + 1), k((size_t)DTP_SCHED_ROW * E_full);
    int ne;
    float sig0;
    RC(dtp_scheduler_tables(sched, steps, &ne, &sig0, ts.data(), sc.data(), k.data()));
    RC(ensure_temb(c, ts));
    HIP_CHECK(hipMemcpy(c->stamp_params->sched, k.data(), k.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(c->stamp_params->in_scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(&c->stamp_params->init_sigma, &sig0, 4, hipMemcpyHostToDevice));
    c->sched_steps = steps;
    c->sched_kind = sched;
  }
  hipLaunchKernelGGL(set_header_kernel, dim3(1), dim3(256), 0, s, &c->stamp_params->coef, coef);
  hipLaunchKernelGGL(set_slots_kernel, dim3(1), dim3(64), 0, s, c->slot_map, sa, B);
  if (sp) hipLaunchKernelGGL(set_strength_kernel, dim3(1), dim3(64), 0, s, &c->stamp_params->strength, StampStrength{sp->a, sp->b, row0, 0});

  // ---- cross-attention K/V for the current brushes
  for (int k = 0; k <= B; ++k) {
    UNetProg* up = prog[k];
    if (!up) continue;
    // the cached per-stamp matrices are valid for exactly this (B, k) split, the slots of the cond rows and these slot versions
    std::vector<int> rows(sa.s, sa.s + B);
    for (int j = 0; j < k; ++j) rows.push_back(sa.s[coef.order[j]]);
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

  c->last_nodes = 0;
  c->last_evals = E;
  c->last_unet_rows = 0;
  for (int i = 0; i < E; ++i) c->last_unet_rows += 2 * B + ks[i];
  const int* rank = c->stamp_params->coef.rank;
  RoctxRange whole("dtp_stamp");
  HIP_CHECK(hipEventRecord(c->ev[0], s));
  // ---- stage 0: pre-processing + both VAE encodes (one batch-2B pass)
  {
  RoctxRange r0("dtp_stamp: pre-processing + vae_encoder x2");
  float* eps3 = sb->eps + (size_t)2 * B * 4 * HWl;  // (third slab: only with sp)
  // which VAE draws the stage consumes: the caller's pointers, or the seeded call's one switch
  const bool use_eps = seeded ? seeded->sample_vae : vae_eps != nullptr;
  const bool use_init = sp && (seeded ? seeded->sample_vae : sp->init_eps != nullptr);
  if (seeded) {  // one launch draws what the copies below deliver: latents (draw 0), the two VAE draws (1, 2), the init image's (3)
    NoiseArgs na = {};
    for (int b = 0; b < B; ++b) na.seed[b] = seeded->seeds[b];
    int nd = 0;
    na.dst[nd] = sb->lat; na.draw[nd++] = 0;
    if (use_eps) {
      na.dst[nd] = sb->eps; na.draw[nd++] = 1;
      na.dst[nd] = sb->eps + (size_t)B * 4 * HWl; na.draw[nd++] = 2;
    }
    if (use_init) { na.dst[nd] = eps3; na.draw[nd++] = 3; }
    RC(dtp_launch_stamp_noise(na, nd, B, HWl, s));
  } else {
    HIP_CHECK(hipMemcpyAsync(sb->lat, latents, (size_t)B * 4 * HWl * 4, hipMemcpyDeviceToDevice, s));
    if (use_eps) HIP_CHECK(hipMemcpyAsync(sb->eps, vae_eps, (size_t)2 * B * 4 * HWl * 4, hipMemcpyDeviceToDevice, s));
    if (use_init) HIP_CHECK(hipMemcpyAsync(eps3, sp->init_eps, (size_t)B * 4 * HWl * 4, hipMemcpyDeviceToDevice, s));
  }
  HIP_CHECK(hipMemcpyAsync(c->canvas32, canvas, (size_t)B * 4 * HW * 4, hipMemcpyDeviceToDevice, s));
  int pads[DTP_STAMP_MAXB];
  for (int b = 0; b < B; ++b) pads[b] = st[b].context_pad;
  const PadArgs pa = pad_args(pads, B);
  hipLaunchKernelGGL(dilate_row_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, s, c->canvas32, c->alpha_tmp, B, R, pa);
  hipLaunchKernelGGL(dilate_col_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, s, c->alpha_tmp,
                     c->alpha_tmp + (size_t)c->maxB * HW, B, R, pa);
  const int k0 = ks[0];
  UNetProg* first = prog[k0];
  // keyed by "init image on/off" (and its draw), not by the strength: the add_noise pair and start row are read from the parameter block
  const long long init_bits = sp ? ((1LL << 20) | (use_init ? 1LL << 21 : 0)) : 0;
  RC(run_stage(c, {((long long)B << 32) | ((long long)k0 << 4) | (use_eps ? 2 : 0) | (k0 > 0 ? 1 : 0) | init_bits | (1LL << 60)}, false, s,
               [&](hipStream_t q) -> int {
    hipLaunchKernelGGL(prep_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, q, c->canvas32, c->brush32, c->slot_map,
                       c->alpha_tmp + (size_t)c->maxB * HW, enc->in8, sb->masks, B, R, sp ? 1 : 0);
    RC(enc->main.run(q, 0));
    RC(launch_vae_sample(c, enc->moments, use_eps ? sb->eps : nullptr, sb->ml, (sp ? 3 : 2) * B, VAE_SCALE, q, use_init ? eps3 : nullptr,
                         2 * B));
    const float* z0 = sp ? sb->ml + (size_t)2 * B * 4 * HWl : nullptr;  // 0.18215 * sample(VAE_enc(canvas)): the init-image latents
    hipLaunchKernelGGL(assemble_kernel, dim3(nblk((long long)B * HWl)), dim3(256), 0, q, sb->lat, z0, sb->masks, sb->ml, rank, first->in16,
                       c->x32, c->stamp_params, 0, B, HWl, k0);
    return LAUNCH_OK();
  }));
  }
  HIP_CHECK(hipEventRecord(c->ev[1], s));
  // fp8 (configs[4]): the first stamp of a program measures its activation ranges once, before the loop is captured.  (Under these
  // options every stamp of the batch has the same tg_evals: the programs are the 3B one for the first evaluations, the 2B one after.)
  if ((c->fp8_linear || c->fp8_attention || c->fp8_operands)) {
    UNetProg *u3 = prog[B], *u2 = prog[0];
    if (u3 && !u3->fp8_calibrated) RC(fp8_calibrate(c, u3, s, 0));
    if (u2 && !u2->fp8_calibrated) {
      if (ks[0] > 0)  // (u2 is not the first program:) its input is normally assembled where the loop switches programs: do it now, from the initial latents
        hipLaunchKernelGGL(assemble_kernel, dim3(nblk((long long)B * HWl)), dim3(256), 0, s, (const float*)nullptr, (const float*)nullptr,
                           sb->masks, sb->ml, rank, u2->in16, c->x32, c->stamp_params, 0, B, HWl, 0);
      RC(fp8_calibrate(c, u2, s, 0));
    }
  }
  // ---- stage 1: the denoise loop
  {
  RoctxRange r1("dtp_stamp: denoise loop (unet)");
  RC(run_stage(c, loop_key, true, s, [&](hipStream_t q) -> int {
    for (int i = 0; i < E; ++i) {
      UNetProg* up = prog[ks[i]];
      if (i > 0 && ks[i] != ks[i - 1]) {
        // switching to a program with fewer tg rows: its input needs mask/masked-latent channels + current x
        hipLaunchKernelGGL(assemble_kernel, dim3(nblk((long long)B * HWl)), dim3(256), 0, q, (const float*)nullptr, (const float*)nullptr,
                           sb->masks, sb->ml, rank, up->in16, c->x32, c->stamp_params, row0 + i, B, HWl, ks[i]);
      }
      const int r = row0 + i;  // the table row (temb, in_scale, sched) of loop index i
      RC(up->main.run(q, r));
      StampParams* pb = c->stamp_params;
      RC(launch_step(sched, up->out32, c->x32, up->in16, c->hist32, pb->sched + DTP_SCHED_ROW * r, pb->in_scale + r + 1, pb->coef.cfg,
                     pb->coef.tg, pb->coef.rank, i, B, HWl, ks[i], q));
    }
    return LAUNCH_OK();
  }));
  }
  HIP_CHECK(hipEventRecord(c->ev[2], s));
  // ---- stage 2: latents / 0.18215 -> VAE decode -> clamp (+ composite, u8)
  {
  RoctxRange r2("dtp_stamp: vae decode + post-processing");
  RC(run_stage(c, {((long long)B << 32) | (3LL << 60)}, false, s, [&](hipStream_t q) -> int {
    RC(launch_post_quant(c, c->x32, 1, 1.0f / VAE_SCALE, dec->in8, B, q));
    return dec->main.run(q, 0);
  }));
  hipLaunchKernelGGL(finish_kernel, dim3(nblk((long long)B * HW)), dim3(256), 0, s, dec->out32, c->canvas32, out, B, HW,
                     st[0].composite, st[0].output_u8);
  }
  c->finite_pending = c->check_finite;
  if (c->check_finite) {
    HIP_CHECK(hipMemsetAsync(c->finite_flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(finite_check_kernel, dim3(nblk((long long)B * HW * 4)), dim3(256), 0, s, c->x32, (long long)B * HWl * 4, dec->out32,
                       (long long)B * HW * 4, c->finite_flag);
  }
  HIP_CHECK(hipEventRecord(c->ev[3], s));
  return LAUNCH_OK();
}

int dtp_last_stamp_finite(dtp_ctx* ctx, int* finite) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !finite) return DTP_ERR_ARG;
  if (!c->finite_pending) { dtp_set_error("dtp_last_stamp_finite: the last stamp ran without the \"check_finite\" option"); return DTP_ERR_STATE; }
  HIP_CHECK(hipEventSynchronize(c->ev[3]));
  int flag = 0;
  HIP_CHECK(hipMemcpy(&flag, c->finite_flag, sizeof(int), hipMemcpyDeviceToHost));
  *finite = flag ? 0 : 1;
  return DTP_OK;
}

int dtp_last_stamp_times(dtp_ctx* ctx, float ms[3]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !ms) return DTP_ERR_ARG;
  HIP_CHECK(hipEventSynchronize(c->ev[3]));
  for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
  return DTP_OK;
}

int dtp_profile(dtp_ctx* ctx, int enable) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return DTP_ERR_ARG;
  HIP_CHECK(hipDeviceSynchronize());
  for (ProfRec& r : c->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  c->prof.clear();
  c->profile = enable != 0;
  return DTP_OK;
}

int dtp_profile_rows(dtp_ctx* ctx, dtp_prof_row* rows, int max_rows, int* n_rows) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !rows || !n_rows) return DTP_ERR_ARG;
  HIP_CHECK(hipDeviceSynchronize());
  dtp_prof_row acc[PK_COUNT] = {};  // PK_COUNT kinds, see include/dtp.h
  for (int k = 0; k < PK_COUNT; ++k) acc[k].kind = k;
  for (const ProfRec& r : c->prof) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
    dtp_prof_row& a = acc[r.kind];
    a.launches += 1; a.ms += ms; a.flops += r.flops; a.bytes += r.bytes;
  }
  int n = 0;
  for (int k = 0; k < PK_COUNT && n < max_rows; ++k)
    if (acc[k].launches) rows[n++] = acc[k];
  *n_rows = n;
  return DTP_OK;
}

int dtp_profile_dump(dtp_ctx* ctx, const char* path) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !path) return DTP_ERR_ARG;
  HIP_CHECK(hipDeviceSynchronize());
  FILE* f = fopen(path, "w");
  if (!f) { dtp_set_error("dtp_profile_dump: cannot open %s", path); return DTP_ERR_ARG; }
  fprintf(f, "kind,us,tflops,algo_GBps,label\n");
  for (const ProfRec& r : c->prof) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    fprintf(f, "%d,%.2f,%.1f,%.1f,%s\n", r.kind, ms * 1e3, r.flops / (ms * 1e-3) / 1e12, r.bytes / (ms * 1e-3) / 1e9, r.label ? r.label : "");
  }
  fclose(f);
  return DTP_OK;
}

int dtp_set_option(dtp_ctx* ctx, const char* name, int value) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !name) return DTP_ERR_ARG;
  if (!strcmp(name, "scheduler")) {  // takes effect from the next stamp, which rebuilds the schedule tables
    if (value != DTP_SCHED_DDIM && value != DTP_SCHED_DPM && value != DTP_SCHED_LMSD) {
      dtp_set_error("dtp_set_option: scheduler %d is not one of DDIM = 0, DPM = 1, LMSD = 2", value);
      return DTP_ERR_ARG;
    }
    c->scheduler = value;
    return DTP_OK;
  }
  if (!strcmp(name, "use_graph")) { c->use_graph = value != 0; return DTP_OK; }
  if (!strcmp(name, "autotune")) { c->autotune = value != 0; return DTP_OK; }
  if (!strcmp(name, "check_finite")) { c->check_finite = value != 0; return DTP_OK; }
  if (!strcmp(name, "fuse_gn_conv")) {
#ifndef DTP_EXPERIMENTAL
    if (value) { dtp_set_error("dtp_set_option: fuse_gn_conv is an experiment (slower: DESIGN.md 3.6) -- build with DTP_EXPERIMENTAL=1"); return DTP_ERR_ARG; }
#endif
    if (!c->unet_progs.empty() || !c->enc_progs.empty() || !c->dec_progs.empty()) {
      dtp_set_error("dtp_set_option: fuse_gn_conv must be chosen before the first launch program is built");
      return DTP_ERR_STATE;
    }
    c->fuse_gn_conv = value != 0;
    return DTP_OK;
  }
  if (!strcmp(name, "dedupe_prefix")) {  // programs are keyed by it: switching only affects which (cached) program a stamp uses
    c->dedupe_prefix = value != 0;
    for (auto& g : c->graphs) destroy_graph(g.second);  // captured stages hold the old program's launches
    c->graphs.clear();
    return DTP_OK;
  }
  // the fp8 options are parity-only (inside the 1e-2 gate at multiples of 64) and were never measured at the ragged
  // maps of a resolution that is a multiple of 8 but not of 64: refused there
  if (value && c->R % 64 && (!strcmp(name, "fp8_linear") || !strcmp(name, "fp8_operands") || !strcmp(name, "fp8_attention"))) {
    dtp_set_error("dtp_set_option: %s is parity-only and not offered at resolution %d (a multiple of 8 that is not a multiple of 64)", name, c->R);
    return DTP_ERR_STATE;
  }
  if (!strcmp(name, "fp8_linear")) {
    if (!c->unet_progs.empty() && c->fp8_linear != (value != 0)) {
      dtp_set_error("dtp_set_option: fp8_linear must be chosen before the first UNet program is built");
      return DTP_ERR_STATE;
    }
    c->fp8_linear = value != 0;
    return DTP_OK;
  }
  if (!strcmp(name, "fp8_operands")) {
    if (!c->unet_progs.empty() && c->fp8_operands != (value != 0)) {
      dtp_set_error("dtp_set_option: fp8_operands must be chosen before the first UNet program is built");
      return DTP_ERR_STATE;
    }
    c->fp8_operands = value != 0;
    return DTP_OK;
  }
  if (!strcmp(name, "fp8_attention")) {
    if (!c->unet_progs.empty() && c->fp8_attention != (value != 0)) {
      dtp_set_error("dtp_set_option: fp8_attention must be chosen before the first UNet program is built");
      return DTP_ERR_STATE;
    }
    c->fp8_attention = value != 0;
    return DTP_OK;
  }
  dtp_set_error("dtp_set_option: unknown option '%s'", name);
  return DTP_ERR_ARG;
}

int dtp_last_stamp_info(dtp_ctx* ctx, int* unet_evals, int* graph_nodes) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return DTP_ERR_ARG;
  if (unet_evals) *unet_evals = c->last_evals;
  if (graph_nodes) *graph_nodes = c->last_nodes;
  return DTP_OK;
}

int dtp_last_stamp_unet_rows(dtp_ctx* ctx, int* rows) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !rows) return DTP_ERR_ARG;
  *rows = c->last_unet_rows;
  return DTP_OK;
}

}  // extern "C"
