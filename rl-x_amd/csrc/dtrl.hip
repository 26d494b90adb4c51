// dtrl.hip -- PPO with differentiable trust-region layers (rl_x/algorithms/ppo_dtrl/flax_full_jit; Otto et al. 2021, arXiv
// 2101.09207): PPO whose Gaussian policy is projected into a KL trust region around the rollout policy before the surrogate is
// evaluated.  The nets, the optimiser (optax.chain(clip_by_global_norm, adam)), acting, next values and GAE are the full-jit
// PPO's (rlx_ppo_rollout_f32, rlx_ppo_next_values_f32, rlx_gae_f32); this file is the part between the policy head and the
// surrogate -- the projection layer, forward and backward -- and the update loop around it on net_pass.h and adam_body.h.
//
// Notation: head output m [mb, A], logstd ls [A] (a parameter), std = exp(ls); rollout policy mo [mb, A], so = exp(old ls).
//   k_dtrl_cov_proj  ONE wave, once per minibatch step (trust_region_layer.py:8-79, :198-213, :218-233; ppo_dtrl.py:188-195).  std and
//                    so are the same for every row, so the per-row vmap of kl_cov_proj solves one scalar problem mb times: it is
//                    solved once.  Component k on lane k, everything in double.  kl_cov = 0.5 sum(2 (log so - ls) + (std / so)^2 -
//                    1); above cov_bound: the eta > 0 with KL(so || s(eta)) = cov_bound, s(eta)^2 = (eta + 1) / max(eta / so^2 + 1
//                    / std^2, 1e-8).  The KL falls monotonically in eta: the root is bracketed by doubling and closed in by Newton
//                    steps that fall back to bisection when they leave the bracket (the reference runs 50 L-BFGS steps at 1e-9).
//                    Leaves the row kernel's per-component constants: projected std, the two vectors of the backward rule
//                    (appendix B.5), the logstd after the entropy projection (+ (beta - H) / A when H < beta = H(so) 0.5^(10
//                    global_step / total_timesteps)), and the row-independent metrics.
//   k_dtrl_adv_stats one workgroup: mean and 1 / (population std + 1e-8) of the minibatch's advantages, two passes in double.
//   k_dtrl_row_loss  one pass over the rows.  A row's A values sit on the lanes of a sub-group of W = next_pow2(A) lanes, 64 / W rows
//                    per wave; row sums are xor-shuffles inside the sub-group, no LDS.  Per row: the mean projection (maha = 0.5
//                    sum((mo - m) / so)^2 > mean_bound: pm = mo + (m - mo) sqrt(mean_bound / maha)), the trust-region regression
//                    loss against the detached projection, the log-prob of the stored action under (pm, fully projected std), the
//                    clipped surrogate with the minibatch-normalised advantage, the critic's squared error; and the backward of
//                    all of it: d m [mb, A] (through the scale factor of the mean projection), d v [mb], and the row's share of d
//                    ls through the entropy projection (I - 1 1^T / A), the covariance projection's hand-written rule and the
//                    regression loss.  The reference clamps d_cov_pred at 1e-20 from below PER ROW (trust_region_layer.py:132), so
//                    d ls is not linear in the row cotangents: the rule runs per row here, not once on a sum.
//   k_dtrl_finish    per-workgroup partials (doubles) of d ls and the row metrics, added in workgroup order: d ls into the policy
//                    gradient vector's logstd slot, the 12 metrics.
// Every reduction has a fixed order, no atomics: two identical calls give identical bits.  No matrix instruction fits this work
// (O(mb A), A <= 64); every GEMM of the update is net_pass.h's, on the exact-fp32 engine at every size.
// CPU twin: tests/dtrl_twin.py (float64 torch; the covariance projection an autograd.Function with the rule above).
#include "net_pass.h"
#include "adam_body.h"

namespace rlx {

constexpr int DT_METRICS = 12;
constexpr int DT_ROW_METRICS = 8;                      // the row sums: pg, critic, trust-region, approx_kl, clip_fraction, eta_mu, kl_mean, projected kl_mean
constexpr int DT_SLAB = 64 + DT_ROW_METRICS;           // doubles per workgroup: [d ls (64) | row metrics]
constexpr int DT_MAX_BLOCKS = 1024;
constexpr double DT_HALF_LOG_2PI = 0.9189385332046727;   // 0.5 log(2 pi)
constexpr double DT_HALF_LOG_2PIE = 1.4189385332046727;  // 0.5 log(2 pi e)
// cov[row][lane], floats: the covariance step's results
enum { DC_STD = 0, DC_IVO, DC_PS, DC_PLS2, DC_DQ, DC_DETA, DC_TRG, DC_SCAL, DC_ROWS };
// DC_SCAL: eta, eta + 1, covariance projection active, entropy projection active, kl_cov, projected kl_cov, entropy, regression
// loss's covariance part
enum { DS_ETA = 0, DS_EO, DS_COV_ON, DS_ENT_ON, DS_KL_COV, DS_POST_KL_COV, DS_ENTROPY, DS_TR_COV };

// ------------------------------------------------------------------------------------------------------------- kernels
__device__ __forceinline__ double dt_wave_sum(double v) {   // xor butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int W>
__device__ __forceinline__ float dt_sub_sum(float v) {
#pragma unroll
  for (int o = W >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int W>
__device__ __forceinline__ double dt_sub_sum(double v) {
#pragma unroll
  for (int o = W >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// KL(so || s) - bound and its derivative in eta at s^2 = (eta + 1) / max(eta io + ip, 1e-8), io = 1 / so^2, ip = 1 / std^2
__device__ __forceinline__ double dt_kl_at(double eta, double io, double ip, bool on, double bound, double* slope) {
  const double q = fmax(eta * io + ip, 1e-8);
  const double v = (eta + 1.0) / q;
  const double t = on ? -log(io * v) + v * io - 1.0 : 0.0;
  const double d = on ? (io - 1.0 / v) * ((ip - io) / (q * q)) : 0.0;
  *slope = 0.5 * dt_wave_sum(d);
  return 0.5 * dt_wave_sum(t) - bound;
}

__global__ __launch_bounds__(64) void k_dtrl_cov_proj(const float* __restrict__ logstd, const float* __restrict__ old_logstd, int A,
                                                      float cov_bound, float global_step, float total_timesteps,
                                                      float* __restrict__ cov) {
  const int k = threadIdx.x;
  const bool on = k < A;
  const double ls = on ? (double)logstd[k] : 0.0, lo = on ? (double)old_logstd[k] : 0.0;
  const double std_ = exp(ls), io = exp(-2.0 * lo), ip = exp(-2.0 * ls);
  const double bound = (double)cov_bound;
  const double kl_cov = 0.5 * dt_wave_sum(on ? 2.0 * (lo - ls) + std_ * std_ * io - 1.0 : 0.0);
  double eta = 0.0, ps = std_, pls = ls, post = kl_cov, dq = 0.0, deta = 0.0;
  const bool cov_on = kl_cov > bound;
  if (cov_on) {   // (wave-uniform)
    double slope, a = 0.0, b = 1.0;
    for (int i = 0; i < 1000 && dt_kl_at(b, io, ip, on, bound, &slope) > 0.0; ++i) { a = b; b *= 2.0; }
    double x = a;
    for (int i = 0; i < 200 && b - a > 1e-15 * b; ++i) {
      const double f = dt_kl_at(x, io, ip, on, bound, &slope);
      if (f > 0.0) a = x; else b = x;
      if (f == 0.0) break;
      const double xn = x - f / slope;   // slope < 0; a NaN or a step outside the bracket bisects
      const bool newton = xn > a && xn < b;
      const bool done = newton && fabs(xn - x) <= 1e-15 * fabs(xn);
      x = newton ? xn : 0.5 * (a + b);
      if (done) break;
    }
    eta = x;
    const double eo = eta + 1.0;
    const double pv = fmax(eo / fmax(eta * io + ip, 1e-8), 1e-16);
    ps = sqrt(pv);
    pls = 0.5 * log(pv);
    post = 0.5 * dt_wave_sum(on ? -log(io * pv) + pv * io - 1.0 : 0.0);
    // appendix B.5 (trust_region_layer.py:96-127)
    const double f2 = pv * (1.0 - io * pv);
    const double sum = dt_wave_sum(on ? f2 * ((io - ip) / eo) : 0.0);
    const double c = -1.0 / (fabs(sum) < 1e-8 ? (sum > 0.0 ? 1e-8 : (sum < 0.0 ? -1e-8 : 0.0)) : sum + 1e-12);
    deta = c * f2;
    dq = (io - ip) / (eo * eo);
  }
  // entropy projection (trust_region_layer.py:218-233) against beta = H(so) 0.5^(10 global_step / total_timesteps)
  const double H = dt_wave_sum(on ? pls + DT_HALF_LOG_2PIE : 0.0);
  const double beta = dt_wave_sum(on ? lo + DT_HALF_LOG_2PIE : 0.0) * pow(0.5, 10.0 * (double)global_step / (double)total_timesteps);
  const bool ent_on = H < beta;
  const double pls2 = ent_on ? pls + (beta - H) / (double)A : pls;
  const double entropy = dt_wave_sum(on ? pls2 + DT_HALF_LOG_2PIE : 0.0);
  const double r = std_ / ps;
  const double tr_cov = 0.5 * dt_wave_sum(on ? 2.0 * (log(ps) - ls) + r * r - 1.0 : 0.0);
  cov[DC_STD * 64 + k] = (float)std_;
  cov[DC_IVO * 64 + k] = on ? (float)io : 0.f;
  cov[DC_PS * 64 + k] = (float)ps;
  cov[DC_PLS2 * 64 + k] = (float)pls2;
  cov[DC_DQ * 64 + k] = (float)dq;
  cov[DC_DETA * 64 + k] = (float)deta;
  cov[DC_TRG * 64 + k] = on ? (float)(r * r - 1.0) : 0.f;
  const double sc[8] = {eta, eta + 1.0, cov_on ? 1.0 : 0.0, ent_on ? 1.0 : 0.0, kl_cov, post, entropy, tr_cov};
  if (k < 8) cov[DC_SCAL * 64 + k] = (float)sc[k];
}

// stats[0] = mean(adv), stats[1] = 1 / (population std + 1e-8) (ppo_dtrl.py:272-273)
__global__ __launch_bounds__(1024) void k_dtrl_adv_stats(const float* __restrict__ adv, int mb, float* __restrict__ stats) {
  __shared__ double s_w[16];
  double s = 0.0;
  for (int r = threadIdx.x; r < mb; r += 1024) s += (double)adv[r];
  s = dt_wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  double mean = 0.0;
  for (int i = 0; i < 16; ++i) mean += s_w[i];
  mean /= (double)mb;
  __syncthreads();
  double q = 0.0;
  for (int r = threadIdx.x; r < mb; r += 1024) q += ((double)adv[r] - mean) * ((double)adv[r] - mean);
  q = dt_wave_sum(q);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    double var = 0.0;
    for (int i = 0; i < 16; ++i) var += s_w[i];
    stats[0] = (float)mean;
    stats[1] = (float)(1.0 / (sqrt(var / (double)mb) + 1e-8));
  }
}

struct DtRows { float *xp, *xc, *act, *mo, *lp, *adv, *ret; int ldp, ldc; };   // the minibatch's row buffers ([mb, .]); ldc 0: xc is xp

// The minibatch of one step: row r <- rollout row rows[r] (clamped into [0, B)): policy / critic observations (row stride a multiple
// of four, zero padded), actions, rollout means, old log-probs, advantages, returns
__global__ __launch_bounds__(256) void k_dtrl_gather(const float* __restrict__ states, int Op, const float* __restrict__ cstates, int Oc,
                                                     const float* __restrict__ actions, const float* __restrict__ old_means, int A,
                                                     const float* __restrict__ log_probs, const float* __restrict__ advantages,
                                                     const float* __restrict__ returns, const int32_t* __restrict__ rows, int64_t B, int mb,
                                                     DtRows o) {
  const int W = o.ldp + o.ldc + 2 * A + 3;
  const int64_t n = (int64_t)mb * W;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int r = (int)(e / W);
    int c = (int)(e - (int64_t)r * W);
    int64_t row = rows ? rows[r] : r;
    row = row < 0 ? 0 : (row >= B ? B - 1 : row);
    if (c < o.ldp) { o.xp[(int64_t)r * o.ldp + c] = c < Op ? states[row * Op + c] : 0.f; continue; }
    c -= o.ldp;
    if (c < o.ldc) { o.xc[(int64_t)r * o.ldc + c] = c < Oc ? cstates[row * Oc + c] : 0.f; continue; }
    c -= o.ldc;
    if (c < A) o.act[(int64_t)r * A + c] = actions[row * A + c];
    else if (c < 2 * A) o.mo[(int64_t)r * A + c - A] = old_means[row * A + c - A];
    else if (c == 2 * A) o.lp[r] = log_probs[row];
    else if (c == 2 * A + 1) o.adv[r] = advantages[row];
    else o.ret[r] = returns[row];
  }
}

struct DtLoss { float clip_range, entropy_coef, critic_coef, mean_bound, tr_coef; };

// loss_fn (ppo_dtrl.py:184-245) meaned over the minibatch, and its backward, for the rows (blockIdx.x 256 + threadIdx.x) / W + i
// gridDim.x 256 / W; lane k of a sub-group owns action component k.  slab: [gridDim.x][DT_SLAB] doubles.
template <int W>
__global__ __launch_bounds__(256) void k_dtrl_row_loss(const float* __restrict__ mean, const float* __restrict__ old_mean,
                                                       const float* __restrict__ act, const float* __restrict__ old_lp,
                                                       const float* __restrict__ adv, const float* __restrict__ adv_stats,
                                                       const float* __restrict__ value, const float* __restrict__ ret,
                                                       const float* __restrict__ cov, int mb, int A, DtLoss hp, float* __restrict__ dmean, float* __restrict__ dvalue,
                                                       double* __restrict__ slab) {
  __shared__ double s_red[DT_ROW_METRICS + 1][256];
  const int t = threadIdx.x, k = t & (W - 1);
  const bool on = k < A;
  const float sd = cov[DC_STD * 64 + k], ivo = on ? cov[DC_IVO * 64 + k] : 0.f, ps = cov[DC_PS * 64 + k], pls2 = cov[DC_PLS2 * 64 + k];
  const float dq = cov[DC_DQ * 64 + k], deta = cov[DC_DETA * 64 + k], trg = cov[DC_TRG * 64 + k];
  const float eo = cov[DC_SCAL * 64 + DS_EO], tr_cov = cov[DC_SCAL * 64 + DS_TR_COV];
  const bool cov_on = cov[DC_SCAL * 64 + DS_COV_ON] != 0.f, ent_on = cov[DC_SCAL * 64 + DS_ENT_ON] != 0.f;
  const float iv2 = expf(-2.0f * pls2);                  // 1 / (fully projected std)^2
  const float ivp = 1.0f / (ps * ps), pv = ps * ps;      // the KL-projected covariance and its inverse
  const float ip = 1.0f / (sd * sd);
  const float a_mean = adv_stats[0], a_inv = adv_stats[1];
  const float inv_mb = 1.0f / (float)mb, inv_A = 1.0f / (float)A;
  double acc[DT_ROW_METRICS] = {0, 0, 0, 0, 0, 0, 0, 0}, acc_ls = 0.0;
  const int rows_per_pass = gridDim.x * (256 / W);
  for (int r = (blockIdx.x * 256 + t) / W; r < mb; r += rows_per_pass) {   // (a sub-group's lanes share r: the shuffles stay inside it)
    const int64_t i = (int64_t)r * A + k;
    const float m = on ? mean[i] : 0.f, mo = on ? old_mean[i] : 0.f, a = on ? act[i] : 0.f;
    // ---- mean projection (trust_region_layer.py:164-195)
    const float d = m - mo;
    const float maha = 0.5f * dt_sub_sum<W>(d * d * ivo);
    const bool m_on = maha > hp.mean_bound;
    const float s = m_on ? sqrtf(hp.mean_bound / maha) : 1.0f;
    const float pm = m_on ? mo + d * s : m;
    const float post_mean = m_on ? 0.5f * dt_sub_sum<W>((mo - pm) * (mo - pm) * ivo) : maha;
    // ---- regression loss against the detached projection (ppo_dtrl.py:197-201)
    const float e = pm - m;
    const float tr = 0.5f * dt_sub_sum<W>(on ? e * e * ivp : 0.f) + tr_cov;
    // ---- surrogate (ppo_dtrl.py:207-218); the row's log-prob and its difference to the old one in double, as espo.hip forms them
    const float z = a - pm;
    const double lp = dt_sub_sum<W>(on ? -0.5 * (double)(z * z * iv2) - DT_HALF_LOG_2PI - (double)pls2 : 0.0);
    const float lr = (float)(lp - (double)old_lp[r]);
    const float ratio = expf(lr);
    const float an = (adv[r] - a_mean) * a_inv;
    const float pg1 = -an * ratio, pg2 = -an * fminf(fmaxf(ratio, 1.0f - hp.clip_range), 1.0f + hp.clip_range);
    const bool inside = ratio >= 1.0f - hp.clip_range && ratio <= 1.0f + hp.clip_range;
    const float w = ((inside || pg1 > pg2) ? -an : 0.f) * ratio * inv_mb;                    // d loss / d log-prob
    // ---- backward: d pm, d (projected logstd) -> entropy projection -> covariance projection -> d ls
    const float g_pm = on ? w * z * iv2 : 0.f;
    float g = on ? w * (z * z * iv2 - 1.0f) - hp.entropy_coef * inv_mb : 0.f;
    const float g_sum = dt_sub_sum<W>(g);
    if (ent_on && on) g -= g_sum * inv_A;
    if (cov_on) {   // kl_cov_proj_backward (trust_region_layer.py:82-135) on this row's cotangent of the projected covariance
      const float d_Q = -pv * (g / (2.0f * pv)) * pv;
      const float d_eta = dt_sub_sum<W>(on ? d_Q * dq : 0.f);
      float dcp = -ip * (d_eta * deta + d_Q / eo) * ip;
      dcp = dcp != dcp ? 0.f : fminf(dcp, 3.4028234664e38f);                                 // nan_to_num
      dcp = fmaxf(dcp, 1e-20f);
      g = on ? 2.0f * sd * dcp * sd : 0.f;
    }
    acc_ls += (double)(g + hp.tr_coef * inv_mb * trg);
    // ---- d m: through the mean projection's scale factor, plus the regression loss
    float g_m = g_pm;
    if (m_on) g_m = s * g_pm - (0.5f * s / maha) * dt_sub_sum<W>(g_pm * d) * d * ivo;
    if (on) dmean[i] = g_m - hp.tr_coef * inv_mb * e * ivp;
    if (k == 0) {
      const float dv = value[r] - ret[r];
      dvalue[r] = hp.critic_coef * dv * inv_mb;
      acc[0] += (double)fmaxf(pg1, pg2);
      acc[1] += 0.5 * (double)dv * (double)dv;
      acc[2] += (double)tr;
      acc[3] += (double)((ratio - 1.0f) - lr);
      acc[4] += fabsf(ratio - 1.0f) > hp.clip_range ? 1.0 : 0.0;
      acc[5] += m_on ? (double)(sqrtf(maha / hp.mean_bound) - 1.0f) : 0.0;
      acc[6] += (double)maha;
      acc[7] += (double)post_mean;
    }
  }
#pragma unroll
  for (int j = 0; j < DT_ROW_METRICS; ++j) s_red[j][t] = acc[j];
  s_red[DT_ROW_METRICS][t] = acc_ls;
  __syncthreads();
  double* out = slab + (int64_t)blockIdx.x * DT_SLAB;
  if (t < 64) {            // component t of d ls: the threads t, t + W, ... in that order
    double sum = 0.0;
    if (t < A)
      for (int u = t; u < 256; u += W) sum += s_red[DT_ROW_METRICS][u];
    out[t] = sum;
  } else if (t < 64 + DT_ROW_METRICS) {
    double sum = 0.0;
    for (int u = 0; u < 256; u += W) sum += s_red[t - 64][u];
    out[t] = sum;
  }
}

// slabs added in workgroup order: d ls -> g_logstd [A]; metrics[12] = {pg_loss, critic_loss, entropy_loss, trust_region_loss,
// approx_kl, clip_fraction, eta_mu, eta_cov, unprojected / projected kl_mean, unprojected / projected kl_cov} (ppo_dtrl.py:230-243)
__global__ __launch_bounds__(128) void k_dtrl_finish(const double* __restrict__ slab, int n_slabs, const float* __restrict__ cov, int mb,
                                                     int A, float* __restrict__ g_logstd, float* __restrict__ metrics) {
  __shared__ double s_m[DT_ROW_METRICS];
  const int t = threadIdx.x;
  double sum = 0.0;
  if (t < DT_SLAB)
    for (int b = 0; b < n_slabs; ++b) sum += slab[(int64_t)b * DT_SLAB + t];
  if (t < A) g_logstd[t] = (float)sum;
  if (t >= 64 && t < DT_SLAB) s_m[t - 64] = sum / (double)mb;
  __syncthreads();
  if (t == 0) {
    const float* sc = cov + DC_SCAL * 64;
    const float m[DT_METRICS] = {(float)s_m[0], (float)s_m[1], sc[DS_ENTROPY], (float)s_m[2], (float)s_m[3], (float)s_m[4], (float)s_m[5],
                                 sc[DS_ETA], (float)s_m[6], (float)s_m[7], sc[DS_KL_COV], sc[DS_POST_KL_COV]};
    for (int j = 0; j < DT_METRICS; ++j) metrics[j] = m[j];
  }
}

// ------------------------------------------------------------------------------------------------------------- host
// 512 LayerNorm ELU, 256 ELU, 128 ELU, head (ppo_dtrl/flax_full_jit/policy.py, critic.py) and whatever else of rlx_mlp_desc
// net_pass.h's blocks take: 1..3 hidden layers, widths multiples of 64 up to 1024 (a LayerNorm layer: 768 with ELU, 512 with tanh)
static int dt_check_desc(const rlx_mlp_desc* d, bool policy, const std::string& f) {
  const std::string n = f + (policy ? ": pdesc" : ": cdesc");
  RLX_REQUIRE(d, RLX_EINVAL, n + " is NULL");
  RLX_REQUIRE(d->in_dim >= 1, RLX_EINVAL, n + "->in_dim >= 1");
  RLX_REQUIRE(d->n_hidden >= 1 && d->n_hidden <= 3 && (d->act == RLX_ACT_ELU || d->act == RLX_ACT_TANH), RLX_EUNSUP,
              n + ": 1..3 hidden layers, act ELU or TANH");
  for (int l = 0; l < d->n_hidden; ++l) {
    const int cap = (d->ln_first && l == 0) ? (d->act == RLX_ACT_TANH ? 512 : 768) : 1024;
    RLX_REQUIRE(d->hidden[l] >= 64 && d->hidden[l] % 64 == 0 && d->hidden[l] <= cap, RLX_EUNSUP,
                n + "->hidden: multiples of 64 up to 1024 (behind the LayerNorm: 768 with ELU, 512 with tanh)");
  }
  RLX_REQUIRE(d->has_logstd == (policy ? 1 : 0), RLX_EUNSUP, n + (policy ? "->has_logstd must be 1" : "->has_logstd must be 0"));
  if (policy) RLX_REQUIRE(d->out_dim >= 1 && d->out_dim <= 64, RLX_EUNSUP, n + "->out_dim (action dim) in 1..64: a row sits in one wave");
  else RLX_REQUIRE(d->out_dim == 1, RLX_EUNSUP, n + "->out_dim must be 1");
  return RLX_OK;
}
static int dt_check_hp(const rlx_dtrl_hparams* hp, const std::string& f) {
  RLX_REQUIRE(hp, RLX_EINVAL, f + ": hp is NULL");
  RLX_REQUIRE(hp->mean_bound > 0.f && hp->cov_bound > 0.f && hp->total_timesteps > 0.f, RLX_EINVAL,
              f + ": hp->mean_bound, cov_bound and total_timesteps must be positive");
  return RLX_OK;
}
static Chain dt_chain(const rlx_mlp_desc& d) {   // the flat layout of rlx_mlp_param_count (make_layout): a LayerNorm after the first Dense only
  Chain L{};
  L.n_hidden = d.n_hidden;
  int64_t off = 0;
  int in = d.in_dim;
  for (int l = 0; l < d.n_hidden; ++l) {
    L.layer[l] = make_block(off, in, d.hidden[l], d.ln_first && l == 0 ? NORM_LAYER : NORM_NONE, d.act, 1e-6f);
    in = d.hidden[l];
  }
  L.head = make_block(off, in, d.out_dim);
  L.n_params = off;
  return L;
}

struct DtNet {
  Chain L;
  const float* params;
  float* grads;
  int64_t n;                 // parameters (the chain's, plus the policy's logstd)
  ChainBufs b;
  float *out, *dout;
  const float* x;
  int ldx;
};
struct DtStep {              // the buffers of one minibatch step
  DtNet P, C;
  DtRows rows;
  float *cov, *adv_stats;
  double* slab;
  int mb, A, n_slabs;
};
static int dt_slabs(int mb, int W) {
  const int g = div_up((int64_t)mb * W, 256);
  return g > DT_MAX_BLOCKS ? DT_MAX_BLOCKS : g;
}
static int dt_width(int A) {
  int W = 1;
  while (W < A) W <<= 1;
  return W;
}
static void dt_carve(DtStep& S, Arena& a, bool shared_x, bool own_grads) {
  const int mb = S.mb, A = S.A;
  for (DtNet* N : {&S.P, &S.C}) {
    chain_carve(N->L, mb, a, &N->b);
    N->out = a.take((size_t)mb * N->L.head.out);
    N->dout = a.take((size_t)mb * N->L.head.out);
    if (own_grads) N->grads = a.take((size_t)N->n);
  }
  S.rows.xp = a.take((size_t)mb * S.rows.ldp);
  S.rows.xc = shared_x ? S.rows.xp : a.take((size_t)mb * S.rows.ldc);
  S.rows.act = a.take((size_t)mb * A);
  S.rows.mo = a.take((size_t)mb * A);
  S.rows.lp = a.take(mb);
  S.rows.adv = a.take(mb);
  S.rows.ret = a.take(mb);
  S.cov = a.take(DC_ROWS * 64);
  S.adv_stats = a.take(64);
  S.slab = reinterpret_cast<double*>(a.take(2 * (size_t)S.n_slabs * DT_SLAB));
}

template <int W>
static void dt_launch_rows(const DtStep& S, const DtLoss& hp, hipStream_t st) {
  hipLaunchKernelGGL(k_dtrl_row_loss<W>, dim3(S.n_slabs), dim3(256), 0, st, (const float*)S.P.out, (const float*)S.rows.mo,
                     (const float*)S.rows.act, (const float*)S.rows.lp, (const float*)S.rows.adv, (const float*)S.adv_stats,
                     (const float*)S.C.out, (const float*)S.rows.ret, (const float*)S.cov, S.mb, S.A, hp, S.P.dout, S.C.dout, S.slab);
}

// one minibatch on the gathered rows: both forwards, the projection layer and the losses, both backwards; the gradients land in
// P.grads / C.grads and the 12 metrics in `metrics`
static int dt_loss_step(rlx_ctx* ctx, DtStep& S, const float* old_logstd, float global_step, const rlx_dtrl_hparams& hp, float* metrics,
                        hipStream_t st) {
  const int mb = S.mb, A = S.A;
  const float* logstd = S.P.params + S.P.L.n_params;
  int rc = chain_fwd(ctx, S.C.L, S.C.params, S.C.x, S.C.ldx, S.C.b, S.C.out, mb, st);
  if (!rc) rc = chain_fwd(ctx, S.P.L, S.P.params, S.P.x, S.P.ldx, S.P.b, S.P.out, mb, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_dtrl_cov_proj, dim3(1), dim3(64), 0, st, logstd, old_logstd, A, hp.cov_bound, global_step, hp.total_timesteps, S.cov);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_dtrl_adv_stats, dim3(1), dim3(1024), 0, st, (const float*)S.rows.adv, mb, S.adv_stats);
  RLX_LAUNCH_CHECK();
  const DtLoss lh{hp.clip_range, hp.entropy_coef, hp.critic_coef, hp.mean_bound, hp.trust_region_coef};
  switch (dt_width(A)) {
    case 1: dt_launch_rows<1>(S, lh, st); break;
    case 2: dt_launch_rows<2>(S, lh, st); break;
    case 4: dt_launch_rows<4>(S, lh, st); break;
    case 8: dt_launch_rows<8>(S, lh, st); break;
    case 16: dt_launch_rows<16>(S, lh, st); break;
    case 32: dt_launch_rows<32>(S, lh, st); break;
    default: dt_launch_rows<64>(S, lh, st); break;
  }
  RLX_LAUNCH_CHECK();
  for (DtNet* N : {&S.C, &S.P}) {
    FsDefer defer(ctx);
    rc = defer.begin(chain_stage_floats(ctx, N->L, mb, true));
    if (!rc) rc = chain_bwd(ctx, N->L, N->params, N->x, N->ldx, N->b, N->dout, N->grads, nullptr, 0, mb, st);
    if (!rc) rc = defer.finish(st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_dtrl_finish, dim3(1), dim3(128), 0, st, (const double*)S.slab, S.n_slabs, (const float*)S.cov, mb, A,
                     S.P.grads + S.P.L.n_params, metrics);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

static int dt_setup(DtStep& S, const rlx_mlp_desc* pdesc, const float* pparams, const rlx_mlp_desc* cdesc, const float* cparams, int mb,
                    const std::string& f) {
  int rc = dt_check_desc(pdesc, true, f);
  if (!rc) rc = dt_check_desc(cdesc, false, f);
  if (rc) return rc;
  RLX_REQUIRE(mb >= 2, RLX_EUNSUP, f + ": the minibatch needs at least two rows (one advantage has no spread to normalise by)");
  S.P.L = dt_chain(*pdesc);
  S.C.L = dt_chain(*cdesc);
  S.P.params = pparams;
  S.C.params = cparams;
  S.P.n = S.P.L.n_params + pdesc->out_dim;      // (+ policy_logstd)
  S.C.n = S.C.L.n_params;
  S.mb = mb;
  S.A = pdesc->out_dim;
  S.n_slabs = dt_slabs(mb, dt_width(S.A));
  S.rows.ldp = (pdesc->in_dim + 3) & ~3;
  S.rows.ldc = (cdesc->in_dim + 3) & ~3;
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_dtrl_loss_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, const float* pparams, float* pgrads, const rlx_mlp_desc* cdesc,
                      const float* cparams, float* cgrads, const float* states, const float* actions, const float* old_means,
                      const float* old_logstd, const float* log_probs, const float* returns, const float* advantages, int mb,
                      float global_step, const rlx_dtrl_hparams* hp, float* metrics, void* stream) {
  const std::string f("rlx_dtrl_loss_f32");
  RLX_REQUIRE(ctx && pparams && pgrads && cparams && cgrads && states && actions && old_means && old_logstd && log_probs && returns &&
                  advantages && metrics,
              RLX_EINVAL, f + ": NULL pointer");
  int rc = dt_check_hp(hp, f);
  if (rc) return rc;
  DtStep S{};
  rc = dt_setup(S, pdesc, pparams, cdesc, cparams, mb, f);
  if (rc) return rc;
  const bool shared_x = !hp->critic_states;
  RLX_REQUIRE(!shared_x || pdesc->in_dim == cdesc->in_dim, RLX_EINVAL, f + ": without hp->critic_states both nets read `states`");
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  ctx->bank = 0;
  if (shared_x) S.rows.ldc = 0;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) { dt_carve(S, a, shared_x, false); });
  if (rc) return rc;
  S.P.grads = pgrads;
  S.C.grads = cgrads;
  S.P.x = S.rows.xp; S.P.ldx = S.rows.ldp;
  S.C.x = S.rows.xc; S.C.ldx = shared_x ? S.rows.ldp : S.rows.ldc;
  hipLaunchKernelGGL(k_dtrl_gather, dim3(elem_grid((int64_t)mb * (S.rows.ldp + S.rows.ldc + 2 * S.A + 3))), dim3(256), 0, st, states,
                     pdesc->in_dim, hp->critic_states, cdesc->in_dim, actions, old_means, S.A, log_probs, advantages, returns,
                     (const int32_t*)nullptr, (int64_t)mb, mb, S.rows);
  RLX_LAUNCH_CHECK();
  ExactDwScope exact(ctx);
  return dt_loss_step(ctx, S, old_logstd, global_step, *hp, metrics, st);
}

int rlx_dtrl_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* cdesc,
                        float* cparams, float* cm, float* cv, const float* states, const float* actions, const float* old_means,
                        const float* log_probs, const float* returns, const float* advantages, int T, int N, int nr_epochs,
                        int minibatch_size, uint32_t key_io[2], int scheme, int64_t* opt_count_io, const float* lr_schedule,
                        float global_step, const rlx_dtrl_hparams* hp, float* metrics_out, void* stream) {
  const std::string f("rlx_dtrl_update_f32");
  RLX_REQUIRE(ctx && pparams && pm && pv && cparams && cm && cv && states && actions && log_probs && returns && advantages && key_io &&
                  opt_count_io && lr_schedule && metrics_out,
              RLX_EINVAL, f + ": NULL pointer");
  int rc = dt_check_hp(hp, f);
  if (rc) return rc;
  const int64_t B = (int64_t)T * N;
  RLX_REQUIRE(T > 0 && N > 0 && nr_epochs > 0, RLX_EINVAL, f + ": T, N and nr_epochs must be positive");
  RLX_REQUIRE(minibatch_size > 0 && B % minibatch_size == 0, RLX_EINVAL, f + ": batch (T*N) must be a positive multiple of minibatch_size");
  RLX_REQUIRE(B <= INT32_MAX, RLX_EINVAL, f + ": T*N must fit the permutation's int32 indices");
  RLX_REQUIRE(*opt_count_io >= 0, RLX_EINVAL, f + ": *opt_count_io >= 0");
  RLX_REQUIRE(ctx->world == 1, RLX_EUNSUP, f + ": no data-parallel form (the context's world size must be 1)");
  const int mb = minibatch_size, M = (int)(B / mb), n_upd = nr_epochs * M;
  DtStep S{};
  rc = dt_setup(S, pdesc, pparams, cdesc, cparams, mb, f);
  if (rc) return rc;
  const bool shared_x = !hp->critic_states;
  RLX_REQUIRE(!shared_x || pdesc->in_dim == cdesc->in_dim, RLX_EINVAL, f + ": without hp->critic_states both nets read `states`");
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  ctx->bank = 0;
  if (shared_x) S.rows.ldc = 0;
  const int A = S.A, Op = pdesc->in_dim;
  float *means = nullptr, *old_logstd = nullptr;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    dt_carve(S, a, shared_x, true);
    means = old_means ? nullptr : a.take((size_t)B * A);
    old_logstd = a.take(64);
  });
  float* psq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  float* csq = (float*)scratch(ctx, SL_NORM2, REDUCE_MAX_BLOCKS * sizeof(float));
  int32_t* perm = (int32_t*)scratch(ctx, SL_PERM, (size_t)nr_epochs * B * sizeof(int32_t));
  if (rc || !psq || !csq || !perm) return rc ? rc : RLX_ENOMEM;
  S.P.x = S.rows.xp; S.P.ldx = S.rows.ldp;
  S.C.x = S.rows.xc; S.C.ldx = shared_x ? S.rows.ldp : S.rows.ldc;
  // the permutation (ppo_dtrl.py:264-267, drawn as PPO's): a prefetched one for exactly this key is only waited for
  if (ctx->pf_valid && !ctx->pf_dist && ctx->pf_key_in[0] == key_io[0] && ctx->pf_key_in[1] == key_io[1] && ctx->pf_E == nr_epochs &&
      ctx->pf_B == B && ctx->pf_scheme == scheme) {
    RLX_HIP_TRY(hipStreamWaitEvent(st, ctx->pf_done, 0));
    key_io[0] = ctx->pf_key_out[0];
    key_io[1] = ctx->pf_key_out[1];
  } else {
    if (ctx->pf_valid && ctx->pf_done) RLX_HIP_TRY(hipStreamWaitEvent(st, ctx->pf_done, 0));
    rc = rlx_permutation_i32(ctx, key_io, perm, nr_epochs, B, scheme, stream);
    if (rc) return rc;
  }
  ctx->pf_valid = false;
  ExactDwScope exact(ctx);
  // the rollout policy: its logstd is the parameter at entry; its means are given, or computed here from the incoming parameters
  // (nothing has changed them since the rollout), one minibatch-sized pass at a time through the step's own buffers
  RLX_HIP_TRY(hipMemcpyAsync(old_logstd, pparams + S.P.L.n_params, (size_t)A * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (!old_means) {
    for (int c = 0; c < M && !rc; ++c) {
      rc = fs_concat(states + (int64_t)c * mb * Op, Op, nullptr, 0, S.rows.xp, S.rows.ldp, mb, st);
      if (!rc) rc = chain_fwd(ctx, S.P.L, pparams, S.rows.xp, S.rows.ldp, S.P.b, means + (int64_t)c * mb * A, mb, st);
    }
    if (rc) return rc;
    old_means = means;
  }
  for (int u = 0; u < n_upd; ++u) {
    float* met = metrics_out + (int64_t)u * (DT_METRICS + 2);
    hipLaunchKernelGGL(k_dtrl_gather, dim3(elem_grid((int64_t)mb * (S.rows.ldp + S.rows.ldc + 2 * A + 3))), dim3(256), 0, st, states, Op,
                       hp->critic_states, cdesc->in_dim, actions, old_means, A, log_probs, advantages, returns,
                       (const int32_t*)(perm + (int64_t)u * mb), B, mb, S.rows);
    RLX_LAUNCH_CHECK();
    rc = dt_loss_step(ctx, S, old_logstd, global_step, *hp, met, st);
    if (rc) return rc;
    // optax.chain(clip_by_global_norm, adam) (ppo_dtrl.py:97-108, :288-292): a non-finite norm skips the step on the device
    const int64_t step = *opt_count_io + u + 1;
    const int ncb = launch_sumsq_partials(S.C.grads, S.C.n, csq, st);
    RLX_LAUNCH_CHECK();
    rc = launch_clip_adam(cparams, S.C.grads, cm, cv, S.C.n, csq, ncb, step, lr_schedule[u], hp->max_grad_norm, hp->adam_b1, hp->adam_b2,
                          hp->adam_eps, met + DT_METRICS + 1, st);
    if (rc) return rc;
    const int npb = launch_sumsq_partials(S.P.grads, S.P.n, psq, st);
    RLX_LAUNCH_CHECK();
    rc = launch_clip_adam(pparams, S.P.grads, pm, pv, S.P.n, psq, npb, step, lr_schedule[u], hp->max_grad_norm, hp->adam_b1, hp->adam_b2,
                          hp->adam_eps, met + DT_METRICS, st);
    if (rc) return rc;
  }
  *opt_count_io += n_upd;
  if (!ctx->ev_perm_free) RLX_HIP_TRY(hipEventCreateWithFlags(&ctx->ev_perm_free, hipEventDisableTiming));
  RLX_HIP_TRY(hipEventRecord(ctx->ev_perm_free, st));   // the next permutation prefetch may overwrite the index buffer behind this
  ctx->perm_free_recorded = true;
  return RLX_OK;
}

}  // extern "C"
