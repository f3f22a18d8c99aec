// Host-only schedule math of the samplers: the tables a stamp uploads and the start point of a strength < 1 stamp.
// Reference: trt_inference/utilities.py (DDIM :370-529, LMSD :274-366, DPM-Solver++ :664-1008), stable_diffusion_pipeline.py:340-355.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "engine.h"

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
int sched_evals(int scheduler, int steps) { return scheduler == DTP_SCHED_DDIM ? steps - 1 : steps; }

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
