// Fused V-trace loss head for the tanh-Gaussian policy of continuous (Box) action spaces, forward + backward: the
// counterpart of csrc/loss.hip for `normal_tanh_distribution` (common/parametric_distribution.py:124-202 of the
// reference; the loss itself, agents/vtrace/learner.py:82-157, does not depend on the distribution).  Plus the
// stand-alone log_prob / entropy, the sampler and the standard-normal fill the learner draws its entropy noise with.
//
// Same decomposition as loss.hip, deliberately plain: a workgroup owns CB adjacent batch columns for all T+1 steps;
//   * phase 1 (row-parallel): 8 lanes per (t, b) row, each lane walks the action dimensions d = sub, sub + 8, ... < D
//     with guarded scalar loads; log_prob under the learner and under the behaviour parameters (fp64 terms and sums:
//     normal_tanh_math.h says why) and the entropy estimate are summed over D by 3-step shuffles; the log importance
//     ratio is rounded to fp32 once and staged in LDS with reward / discount / value;
//   * phase 2: the shared V-trace recursion (loss_shared.h);
//   * phase 3 (row-parallel): the per-element maths again, now for the gradients wrt loc and s, written to
//     d_params[row, 0..2D-1]; loss partial sums reduced wave -> block in a fixed order (no atomics).
// The per-element maths is csrc/normal_tanh_math.h, which the host harness (tests/host/normal_tanh_emul.cpp) runs too.
// Algorithmic bytes per (t, b): 24 D + 9 read (learner and behaviour parameters 8 D each, action and noise 4 D each,
// baseline, reward, done), 8 D + 4 (+8 with vs / pg_adv emitted) written; the launch is latency-bound at learner sizes.
//
// Compiled with -ffp-contract=off like loss.hip.
#include "common.h"
#include "../../include/seedhip.h"
#include "normal_tanh_math.h"

namespace {

#include "loss_shared.h"

namespace nt = seedhip::nt;

constexpr int kMaxD = 64;

__device__ __forceinline__ double grp_sum_f64(double v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  return v;
}

struct NtLossParams {
  const float* tgt;          // [T+1,B,logits_ld] learner parameters [loc(D) | s(D)] per row
  const float* baseline;     // [T+1,B] (stride baseline_ld)
  const float* beh;          // [T+1,B,2D] behaviour parameters
  const float* actions;      // [T+1,B,D] in [-1, 1]
  const float* noise;        // [T,B,D] standard-normal draws of the entropy estimate
  const float* rewards;      // [T+1,B]
  const uint8_t* done;       // [T+1,B]
  int T, B, D;
  int logits_ld, baseline_ld;
  float entropy_cost, baseline_cost, kl_cost, discounting, lambda_, max_abs_reward;
  float clip_rho, clip_pg_rho;
  float inv_n;               // 1 / mean_denominator
  const float* ec_param;     // learnable entropy cost (see loss.hip); null = fixed
  float ec_mul;
  float* d_params;           // [T+1,B,logits_ld], columns 0..2D-1 written
  float* d_baseline;         // [T+1,B] (stride baseline_ld)
  float* vs;                 // [T,B] or null
  float* pg_adv;             // [T,B] or null
  float* partials;           // [nblocks, kNumPartials]
};

template <int CB>
__global__ void __launch_bounds__(kThreads)
normal_tanh_loss_kernel(NtLossParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int T = p.T, B = p.B, D = p.D;
  const int T1 = T + 1;
  // LDS carve: [T1][CB] arrays, the same budget as the categorical head (kRowArrays).  The shared V-trace phase takes
  // exp(a - b) of two arrays: here a = the log importance ratio (a difference of fp64 sums, rounded once) and b = 0.
  float* s_lrho = smem;                // target - behaviour log-prob
  float* s_zero = s_lrho + T1 * CB;    // 0
  float* s_tlp = s_zero + T1 * CB;     // target log-prob
  float* s_ent = s_tlp + T1 * CB;      // entropy estimate of the target policy
  float* s_rew = s_ent + T1 * CB;      // reward[t+1] (clipped)
  float* s_dis = s_rew + T1 * CB;      // discount[t]
  float* s_val = s_dis + T1 * CB;      // baseline[t]
  float* s_pg = s_val + T1 * CB;       // pg_adv[t]; after phase 2
  float* s_vs = s_pg + T1 * CB;        // vs[t]
  __shared__ float s_red[kThreads / 64][kNumPartials];

  const int tid = threadIdx.x;
  const int sub = tid & (kLPR - 1);
  const int grp = tid / kLPR;
  const int b0 = blockIdx.x * CB;
  const int nrows = T1 * CB;

  // ---------------- phase 1: per-row log-probs and entropy ----------------- //
  for (int r = grp; r < nrows; r += kGroups) {
    const int t = r / CB, c = r - t * CB;
    const int b = b0 + c;
    if (b >= B) continue;                           // uniform within the 8-lane group
    const long long tb = (long long)t * B + b;
    if (sub == 0) s_val[r] = p.baseline[tb * p.baseline_ld];
    if (t >= T) continue;                           // bootstrap row: value only
    const long long rowt = tb * p.logits_ld;        // learner parameters: strided
    const long long rowb = tb * (2LL * D);          // behaviour parameters: contiguous
    const long long rowa = tb * D;                  // actions / noise
    double lpt = 0., lpb = 0.;
    float ent = 0.f;
    for (int d = sub; d < D; d += kLPR) {
      const float a = p.actions[rowa + d];
      const float loc = p.tgt[rowt + d], s = p.tgt[rowt + D + d];
      lpt += nt::log_prob_term(a, loc, s).v;
      lpb += nt::log_prob_term(a, p.beh[rowb + d], p.beh[rowb + D + d]).v;
      ent += nt::entropy_term(loc, s, p.noise[rowa + d]).v;
    }
    lpt = grp_sum_f64(lpt); lpb = grp_sum_f64(lpb); ent = grp_sum(ent);
    if (sub == 0) {
      s_lrho[r] = (float)(lpt - lpb); s_zero[r] = 0.f; s_tlp[r] = (float)lpt; s_ent[r] = ent;
      const long long tb1 = tb + B;                 // env_outputs[1:], learner.py:87
      float rw = p.rewards[tb1];
      if (p.max_abs_reward != 0.f) rw = fminf(fmaxf(rw, -p.max_abs_reward), p.max_abs_reward);
      s_rew[r] = rw;
      s_dis[r] = (p.done[tb1] ? 0.f : 1.f) * p.discounting;   // learner.py:93
    }
  }
  __syncthreads();

  // ---------------- phase 2: V-trace recursion per column ------------------ //
  vtrace_columns<CB>(s_lrho, s_zero, s_rew, s_dis, s_val, s_pg, s_vs, T, B, b0, tid, p.clip_rho, p.clip_pg_rho, p.lambda_);
  __syncthreads();

  // ---------------- phase 3: gradients + loss partial sums ----------------- //
  const float ec = p.ec_param ? expf(p.ec_mul * p.ec_param[0]) : p.entropy_cost;   // a constant here (stop_gradient)
  float acc_pg = 0.f, acc_v2 = 0.f, acc_ent = 0.f, acc_kl = 0.f, acc_val = 0.f, acc_maxa = 0.f, acc_std = 0.f;
  for (int r = grp; r < nrows; r += kGroups) {
    const int t = r / CB, c = r - t * CB;
    const int b = b0 + c;
    if (b >= B) continue;
    const long long tb = (long long)t * B + b;
    const long long rowt = tb * p.logits_ld;
    if (t >= T) {                                   // bootstrap row: no gradient
      for (int d = sub; d < D; d += kLPR) { p.d_params[rowt + d] = 0.f; p.d_params[rowt + D + d] = 0.f; }
      if (sub == 0) p.d_baseline[tb * p.baseline_ld] = 0.f;
      continue;
    }
    const long long rowa = tb * D;
    const float pg = s_pg[r], vs = s_vs[r], v = s_val[r];
    const float coef = (pg + p.kl_cost) * p.inv_n;  // policy-gradient + KL terms both go through log_prob
    const float ecn = ec * p.inv_n;
    for (int d = sub; d < D; d += kLPR) {
      const float a = p.actions[rowa + d];
      const float loc = p.tgt[rowt + d], s = p.tgt[rowt + D + d];
      const nt::LpTerm lp = nt::log_prob_term(a, loc, s);
      const nt::Term en = nt::entropy_term(loc, s, p.noise[rowa + d]);
      p.d_params[rowt + d] = -(coef * lp.dloc) - ecn * en.dloc;
      p.d_params[rowt + D + d] = -(coef * lp.ds) - ecn * en.ds;
      acc_maxa = fmaxf(acc_maxa, fabsf(a));
      acc_std += nt::sigma_of(s);
    }
    if (sub == 0) {
      const float verr = vs - v;
      p.d_baseline[tb * p.baseline_ld] = p.baseline_cost * (v - vs) * p.inv_n;
      if (p.vs) p.vs[tb] = vs;
      if (p.pg_adv) p.pg_adv[tb] = pg;
      acc_pg += s_tlp[r] * pg; acc_v2 += verr * verr; acc_ent += s_ent[r];
      acc_kl += -s_lrho[r]; acc_val += v;
    }
  }
  // wave -> block reduction in a fixed order.
  acc_pg = seedhip::wave_sum(acc_pg); acc_v2 = seedhip::wave_sum(acc_v2);
  acc_ent = seedhip::wave_sum(acc_ent); acc_kl = seedhip::wave_sum(acc_kl);
  acc_val = seedhip::wave_sum(acc_val); acc_maxa = seedhip::wave_max(acc_maxa);
  acc_std = seedhip::wave_sum(acc_std);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    s_red[wave][0] = acc_pg; s_red[wave][1] = acc_v2; s_red[wave][2] = acc_ent;
    s_red[wave][3] = acc_kl; s_red[wave][4] = acc_val; s_red[wave][5] = acc_maxa; s_red[wave][6] = acc_std;
  }
  __syncthreads();
  if (tid == 0) {
    float o[kNumPartials] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w < kThreads / 64; ++w) {
      for (int k = 0; k < 5; ++k) o[k] += s_red[w][k];
      o[5] = fmaxf(o[5], s_red[w][5]);
      o[6] += s_red[w][6];
    }
    for (int k = 0; k < kNumPartials; ++k) p.partials[(long long)blockIdx.x * kNumPartials + k] = o[k];
  }
}

// The shared finalize plus policy/std (learner.py:151-152): mean sigma over rows and dimensions, as this replica's
// share of the global mean like every other scalar (std_scale = inv_n / D).
__global__ void normal_tanh_loss_finalize_kernel(const float* __restrict__ partials, int nblocks, float inv_n,
                                                 float entropy_cost, float baseline_cost, float kl_cost,
                                                 const float* __restrict__ ec_param, float ec_mul, int has_target,
                                                 float target_entropy_share, float* __restrict__ d_ec_param,
                                                 float std_scale, float* __restrict__ scalars) {
  const float std_sum = loss_finalize<true>(partials, nblocks, inv_n, entropy_cost, baseline_cost, kl_cost, ec_param,
                                            ec_mul, has_target, target_entropy_share, d_ec_param, scalars);
  if (threadIdx.x == 0) scalars[SEEDHIP_LOSS_POLICY_STD] = std_sum * std_scale;
}

template <int CB>
void launch_nt_loss(const NtLossParams& p, int nblocks, size_t lds, hipStream_t s) {
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)normal_tanh_loss_kernel<CB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((normal_tanh_loss_kernel<CB>), dim3(nblocks), dim3(kThreads), lds, s, p);
}

}  // namespace

extern "C" int seedhip_normal_tanh_loss_fwd_bwd(
    const float* learner_params, int logits_ld, const float* learner_baseline, int baseline_ld,
    const float* behaviour_params, const float* actions, const float* entropy_noise,
    const float* rewards, const uint8_t* done, int T, int B, int D,
    float entropy_cost, const float* entropy_cost_param, float entropy_cost_adjustment_speed, int has_target_entropy,
    float target_entropy, float* d_entropy_cost_param,
    float baseline_cost, float kl_cost, float discounting, float lambda_,
    float max_abs_reward, float clip_rho_threshold, float clip_pg_rho_threshold,
    float mean_denominator, float* d_params, float* d_baseline, float* vs, float* pg_advantages,
    float* scalars, void* workspace, size_t workspace_bytes, void* stream) {
  SEEDHIP_REQUIRE(T >= 1 && B >= 1, "normal_tanh_loss: need T>=1,B>=1 (got %d,%d)", T, B);
  SEEDHIP_REQUIRE(D >= 1 && D <= kMaxD, "normal_tanh_loss: D=%d outside 1..%d", D, kMaxD);
  SEEDHIP_REQUIRE(logits_ld >= 2 * D && baseline_ld >= 1, "normal_tanh_loss: bad row strides (logits_ld=%d < 2D=%d?)",
                  logits_ld, 2 * D);
  SEEDHIP_REQUIRE(learner_params && learner_baseline && behaviour_params && actions && entropy_noise && rewards &&
                  done && d_params && d_baseline && scalars && workspace, "normal_tanh_loss: null pointer");
  SEEDHIP_REQUIRE(!entropy_cost_param == !d_entropy_cost_param,
                  "normal_tanh_loss: entropy_cost_param and d_entropy_cost_param go together");
  SEEDHIP_REQUIRE(entropy_cost_param || !has_target_entropy,
                  "normal_tanh_loss: a target entropy needs the learnable entropy-cost parameter");
  SEEDHIP_REQUIRE(workspace_bytes >= seedhip_impala_loss_workspace_bytes(T, B), "normal_tanh_loss: workspace too small");
  SEEDHIP_REQUIRE(mean_denominator > 0.f, "normal_tanh_loss: mean_denominator must be > 0");
  const int cb = pick_cb(B);
  const size_t lds = loss_lds_bytes(T, cb);
  SEEDHIP_REQUIRE(lds <= kLossLdsMax, "normal_tanh_loss: T=%d too long for LDS staging", T);
  NtLossParams p;
  p.tgt = learner_params; p.baseline = learner_baseline; p.beh = behaviour_params; p.actions = actions;
  p.noise = entropy_noise; p.rewards = rewards; p.done = done;
  p.T = T; p.B = B; p.D = D; p.logits_ld = logits_ld; p.baseline_ld = baseline_ld;
  p.entropy_cost = entropy_cost_param ? 0.f : entropy_cost; p.baseline_cost = baseline_cost; p.kl_cost = kl_cost;
  p.discounting = discounting; p.lambda_ = lambda_; p.max_abs_reward = max_abs_reward;
  p.clip_rho = clip_rho_threshold; p.clip_pg_rho = clip_pg_rho_threshold;
  p.inv_n = 1.0f / mean_denominator;
  p.ec_param = entropy_cost_param; p.ec_mul = entropy_cost_adjustment_speed;
  p.d_params = d_params; p.d_baseline = d_baseline; p.vs = vs; p.pg_adv = pg_advantages;
  p.partials = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int nblocks = (B + cb - 1) / cb;
  if (cb == 8) launch_nt_loss<8>(p, nblocks, lds, s);
  else if (cb == 4) launch_nt_loss<4>(p, nblocks, lds, s);
  else launch_nt_loss<2>(p, nblocks, lds, s);
  int rc = seedhip::check_launch("normal_tanh_loss_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(normal_tanh_loss_finalize_kernel, dim3(1), dim3(64), 0, s, (const float*)workspace, nblocks,
                     p.inv_n, p.entropy_cost, baseline_cost, kl_cost, entropy_cost_param, entropy_cost_adjustment_speed,
                     has_target_entropy, target_entropy, d_entropy_cost_param, p.inv_n / (float)D, scalars);
  return seedhip::check_launch("normal_tanh_loss_finalize_kernel");
}

// ---- stand-alone log_prob / entropy (common/parametric_distribution.py:69-74 with the tanh-Gaussian) ---- //
namespace {
__global__ void __launch_bounds__(kThreads)
normal_tanh_kernel(const float* __restrict__ params, const float* __restrict__ actions,
                   const float* __restrict__ noise, long long rows, int D, float* __restrict__ log_prob,
                   float* __restrict__ entropy) {
  const int sub = threadIdx.x & (kLPR - 1);
  const long long r = ((long long)blockIdx.x * kThreads + threadIdx.x) / kLPR;
  if (r >= rows) return;                            // uniform within the 8-lane group
  const long long rowp = r * (2LL * D), rowa = r * D;
  double lp = 0.;
  float ent = 0.f;
  for (int d = sub; d < D; d += kLPR) {
    const float loc = params[rowp + d], s = params[rowp + D + d];
    if (actions) lp += nt::log_prob_term(actions[rowa + d], loc, s).v;
    if (noise) ent += nt::entropy_term(loc, s, noise[rowa + d]).v;
  }
  lp = grp_sum_f64(lp); ent = grp_sum(ent);
  if (sub == 0) { if (log_prob) log_prob[r] = (float)lp; if (entropy) entropy[r] = ent; }
}

// Four standard-normal draws from one Philox block by Box-Muller; u in (0, 1) exactly as in sample_categorical_row.
__device__ __forceinline__ void normal4(uint4 ctr, uint2 key, float out[4]) {
  const uint4 r = seedhip::philox4x32_10(ctr, key);
  const float k = 1.0f / 8388608.0f, two_pi = 6.2831853071795865f;
  const float u0 = ((float)(r.x >> 9) + 0.5f) * k, u1 = ((float)(r.y >> 9) + 0.5f) * k;
  const float u2 = ((float)(r.z >> 9) + 0.5f) * k, u3 = ((float)(r.w >> 9) + 0.5f) * k;
  const float ra = sqrtf(-2.f * logf(u0)), rb = sqrtf(-2.f * logf(u2));
  out[0] = ra * cosf(two_pi * u1); out[1] = ra * sinf(two_pi * u1);
  out[2] = rb * cosf(two_pi * u3); out[3] = rb * sinf(two_pi * u3);
}

// actions[r, d] = tanh(loc + sigma * eps), eps keyed by (seed, call, row, d): one lane per row.
__global__ void __launch_bounds__(256)
normal_tanh_sample_kernel(const float* __restrict__ params, int ld, long long rows, int D,
                          const unsigned long long* __restrict__ rng, float* __restrict__ actions) {
  const unsigned long long seed = rng[0], call = rng[1];
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
  const float* row = params + r * ld;
  for (int d0 = 0; d0 < D; d0 += 4) {
    float e[4];
    normal4(make_uint4((uint32_t)call, (uint32_t)(call >> 32), (uint32_t)r, (uint32_t)(d0 >> 2)), key, e);
    for (int j = 0; j < 4; ++j) {
      const int d = d0 + j;
      if (d < D) actions[r * D + d] = tanhf(row[d] + nt::sigma_of(row[D + d]) * e[j]);
    }
  }
}

// out[i] ~ N(0, 1), keyed by (seed, call, i / 4): one lane per four elements.
__global__ void __launch_bounds__(256)
normal_fill_kernel(float* __restrict__ out, long long n, const unsigned long long* __restrict__ rng) {
  const unsigned long long seed = rng[0], call = rng[1];
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q * 4 >= n) return;
  float e[4];
  normal4(make_uint4((uint32_t)call, (uint32_t)(call >> 32), (uint32_t)q, (uint32_t)((unsigned long long)q >> 32)),
          make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), e);
  for (int j = 0; j < 4; ++j) if (q * 4 + j < n) out[q * 4 + j] = e[j];
}

__global__ void nt_rng_advance_kernel(unsigned long long* rng) { rng[1] += 1; }
}  // namespace

extern "C" int seedhip_normal_tanh_log_prob_entropy(const float* params, const float* actions, const float* noise,
                                                    long long rows, int D, float* log_prob, float* entropy,
                                                    void* stream) {
  SEEDHIP_REQUIRE(rows >= 0 && D >= 1 && D <= kMaxD, "normal_tanh: bad rows=%lld D=%d", rows, D);
  if (rows == 0) return SEEDHIP_OK;
  SEEDHIP_REQUIRE(params && (log_prob || entropy), "normal_tanh: null pointer");
  SEEDHIP_REQUIRE(!log_prob || actions, "normal_tanh: log_prob needs actions");
  SEEDHIP_REQUIRE(!entropy || noise, "normal_tanh: the entropy estimate needs its noise");
  SEEDHIP_REQUIRE(rows <= (1LL << 32), "normal_tanh: rows=%lld too many for one launch", rows);
  const int nblocks = seedhip::cdiv(rows * kLPR, kThreads);
  hipLaunchKernelGGL(normal_tanh_kernel, dim3(nblocks), dim3(kThreads), 0, (hipStream_t)stream, params,
                     log_prob ? actions : nullptr, entropy ? noise : nullptr, rows, D, log_prob, entropy);
  return seedhip::check_launch("normal_tanh_kernel");
}

extern "C" int seedhip_normal_tanh_sample(const float* params, int ld, long long rows, int D,
                                          unsigned long long* rng_state, float* actions, void* stream) {
  SEEDHIP_REQUIRE(rows >= 0 && rows <= 0xFFFFFFFFLL && D >= 1 && D <= kMaxD && ld >= 2 * D,
                  "normal_tanh_sample: bad rows=%lld / D=%d / ld=%d", rows, D, ld);
  SEEDHIP_REQUIRE(rng_state, "normal_tanh_sample: null rng_state");
  hipStream_t s = (hipStream_t)stream;
  if (rows > 0) {
    SEEDHIP_REQUIRE(params && actions, "normal_tanh_sample: null pointer");
    hipLaunchKernelGGL(normal_tanh_sample_kernel, dim3(seedhip::cdiv(rows, 256)), dim3(256), 0, s, params, ld, rows, D,
                       rng_state, actions);
  }
  hipLaunchKernelGGL(nt_rng_advance_kernel, dim3(1), dim3(1), 0, s, rng_state);
  return seedhip::check_launch("normal_tanh_sample_kernel");
}

extern "C" int seedhip_normal_fill(float* out, long long n, unsigned long long* rng_state, void* stream) {
  SEEDHIP_REQUIRE(n >= 0 && n <= (1LL << 40), "normal_fill: bad n=%lld", n);
  SEEDHIP_REQUIRE(rng_state, "normal_fill: null rng_state");
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    SEEDHIP_REQUIRE(out, "normal_fill: null pointer");
    hipLaunchKernelGGL(normal_fill_kernel, dim3(seedhip::cdiv((n + 3) / 4, 256)), dim3(256), 0, s, out, n, rng_state);
  }
  hipLaunchKernelGGL(nt_rng_advance_kernel, dim3(1), dim3(1), 0, s, rng_state);
  return seedhip::check_launch("normal_fill_kernel");
}
