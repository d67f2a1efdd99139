// What the fused V-trace loss heads have in common (csrc/loss.hip: categorical policy; csrc/loss_normal_tanh.hip:
// tanh-Gaussian policy): the launch geometry, the column-serial V-trace phase that runs out of the per-row LDS scalars,
// and the one-block finalize that turns the per-workgroup partial sums into the logged scalars.  Each translation unit
// includes this header INSIDE its own unnamed namespace (after common.h and seedhip.h), so everything here keeps
// internal linkage in both.
#pragma once

constexpr int kLPR = 8;            // lanes per row
constexpr int kThreads = 256;
constexpr int kGroups = kThreads / kLPR;
constexpr int kNumPartials = 8;    // per-block partial sums
constexpr int kRowArrays = 9;      // [T+1][CB] LDS arrays of a loss head

__device__ __forceinline__ float grp_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
  return v;
}
__device__ __forceinline__ float grp_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  return v;
}

// V-trace recursion per column (common/vtrace.py:84-148): the first CB lanes of the workgroup each run the T-step
// recursion of one batch column out of LDS.  The caller brackets it with __syncthreads().
template <int CB>
__device__ __forceinline__ void vtrace_columns(const float* s_tlp, const float* s_blp, const float* s_rew,
                                               const float* s_dis, const float* s_val, float* s_pg, float* s_vs,
                                               int T, int B, int b0, int tid, float clip_rho, float clip_pg_rho,
                                               float lambda_) {
  if (tid < CB && b0 + tid < B) {
    const int c = tid;
    const bool has_rho = clip_rho >= 0.f, has_pg = clip_pg_rho >= 0.f;
    const float boot = s_val[T * CB + c];           // learner.py:82
    float acc = 0.f, vs_next = boot, v_next = boot;
    for (int t = T - 1; t >= 0; --t) {
      const int r = t * CB + c;
      const float rho = expf(s_tlp[r] - s_blp[r]);
      const float crho = has_rho ? fminf(clip_rho, rho) : rho;
      const float cs = fminf(1.0f, rho) * lambda_;
      const float d = s_dis[r], rw = s_rew[r], v = s_val[r];
      const float delta = crho * ((rw + d * v_next) - v);
      acc = delta + (d * cs) * acc;
      const float vs = acc + v;
      const float cpg = has_pg ? fminf(clip_pg_rho, rho) : rho;
      const float pg = cpg * ((rw + d * vs_next) - v);
      s_vs[r] = vs; s_pg[r] = pg;
      vs_next = vs; v_next = v;
    }
  }
}

// scalars[]: see SEEDHIP_LOSS_* indices in seedhip.h.
// Entropy-cost adjustment (learner.py:127-135, :225-234): with a learnable parameter theta the cost is
// c = exp(speed * theta); entropy_adjustment_loss = c * stop_gradient(mean(H) - target) when a target entropy is set
// (its only gradient: d/dtheta = speed * c * (mean(H) - target)), and 0 * c otherwise (gradient 0, never None).
// One wave.  Returns (on every lane) the sum of partial slot 6 when kExtra, which only the tanh-Gaussian head fills.
template <bool kExtra>
__device__ __forceinline__ float loss_finalize(const float* __restrict__ partials, int nblocks, float inv_n,
                                               float entropy_cost, float baseline_cost, float kl_cost,
                                               const float* __restrict__ ec_param, float ec_mul, int has_target,
                                               float target_entropy_share, float* __restrict__ d_ec_param,
                                               float* __restrict__ scalars) {
  // each lane sums a strided subset in fixed order, then a shuffle tree.
  float o[6] = {0, 0, 0, 0, 0, 0};
  float extra = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 64) {
    for (int k = 0; k < 5; ++k) o[k] += partials[(long long)i * kNumPartials + k];
    o[5] = fmaxf(o[5], partials[(long long)i * kNumPartials + 5]);
    if (kExtra) extra += partials[(long long)i * kNumPartials + 6];
  }
  for (int k = 0; k < 5; ++k) o[k] = seedhip::wave_sum(o[k]);
  o[5] = seedhip::wave_max(o[5]);
  if (kExtra) extra = seedhip::wave_sum(extra);
  if (threadIdx.x == 0) {
    if (ec_param) entropy_cost = expf(ec_mul * ec_param[0]);
    const float policy_loss = -(o[0] * inv_n);                        // learner.py:111-112
    const float mse = o[1] * inv_n;
    const float v_loss = baseline_cost * 0.5f * mse;                  // :115-116
    const float entropy = o[2] * inv_n;                               // :119-120
    const float entropy_loss = entropy_cost * -entropy;               // :121
    const float kl_mean = o[3] * inv_n;
    const float kl_loss = kl_cost * kl_mean;                          // :124-125
    float adjustment = 0.f;                                           // :128-132
    if (has_target) adjustment = entropy_cost * (entropy - target_entropy_share);
    if (d_ec_param) d_ec_param[0] = has_target ? ec_mul * entropy_cost * (entropy - target_entropy_share) : 0.f;
    scalars[SEEDHIP_LOSS_TOTAL] = policy_loss + v_loss + entropy_loss + kl_loss + adjustment;  // :134-135
    scalars[SEEDHIP_LOSS_POLICY] = policy_loss;
    scalars[SEEDHIP_LOSS_V] = v_loss;
    scalars[SEEDHIP_LOSS_ENTROPY] = entropy_loss;
    scalars[SEEDHIP_LOSS_KL] = kl_loss;
    scalars[SEEDHIP_LOSS_ENTROPY_MEAN] = entropy;
    scalars[SEEDHIP_LOSS_KL_MEAN] = kl_mean;
    scalars[SEEDHIP_LOSS_VALUE_MEAN] = o[4] * inv_n;                  // :138-140
    scalars[SEEDHIP_LOSS_V_L2_ERROR] = sqrtf(mse);                    // :141
    scalars[SEEDHIP_LOSS_MAX_ACTION_ABS] = o[5];                      // :152-153
    scalars[SEEDHIP_LOSS_ENTROPY_COST] = entropy_cost;                // :155
    scalars[SEEDHIP_LOSS_ENTROPY_ADJUSTMENT] = adjustment;
  }
  return extra;
}

// Columns per workgroup.  8 keeps whole 32-byte sectors of the [T+1, B] scalars per workgroup; at the learner's own
// sizes (B = 512 per GPU: 64 workgroups of which each spends its V-trace phase on 8 lanes) the launch is latency-bound
// and under-fills the 256 CUs, so narrower column groups are used until the grid reaches the CU count: B = 512 -> 2
// columns x 256 workgroups (r02: 31 -> ~15 us per launch).
inline int pick_cb(int B) { return B >= 8 * 256 ? 8 : (B >= 4 * 256 ? 4 : 2); }

inline size_t loss_lds_bytes(int T, int cb) { return (size_t)(T + 1) * cb * kRowArrays * sizeof(float); }
constexpr size_t kLossLdsMax = 150 * 1024;
