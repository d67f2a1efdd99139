// Host build of the tanh-Gaussian loss head: seed_rl_amd/csrc/normal_tanh_math.h (the very header the HIP kernel uses)
// compiled by g++ with AddressSanitizer + UBSan, plus a plain-loop version of the whole head in the kernel's own order
// of operations (per-row sums over D, V-trace recursion per column, gradients, scalars) for tests/test_normal_tanh_host.py.
// Built with -ffp-contract=off like the device code.  A program, not a library (a sanitized library cannot be loaded
// into an unsanitized Python): `normal_tanh_emul MODE IN OUT` reads raw little-endian arrays from IN and writes OUT;
// every array lives in a heap block of exactly its size, so an index that strays is an AddressSanitizer report.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../seed_rl_amd/csrc/normal_tanh_math.h"

namespace nt = seedhip::nt;

extern "C" {

// out[i] = {log_ndtr(z), dlog_ndtr(z)}
void nt_log_ndtr(const float* z, int n, float* out) {
  for (int i = 0; i < n; ++i) { out[2 * i] = (float)nt::log_ndtr((double)z[i]); out[2 * i + 1] = (float)nt::dlog_ndtr((double)z[i]); }
}

// per element: out[i] = {lp, dlp/dloc, dlp/ds, ent, dent/dloc, dent/ds}
void nt_terms(const float* a, const float* loc, const float* s, const float* eps, int n, float* out) {
  for (int i = 0; i < n; ++i) {
    const nt::LpTerm lp = nt::log_prob_term(a[i], loc[i], s[i]);
    const nt::Term en = nt::entropy_term(loc[i], s[i], eps[i]);
    float* o = out + 6 * i;
    o[0] = (float)lp.v; o[1] = lp.dloc; o[2] = lp.ds; o[3] = en.v; o[4] = en.dloc; o[5] = en.ds;
  }
}

// The whole head, argument for argument the C ABI of seedhip_normal_tanh_loss_fwd_bwd (no workspace / stream).
int nt_loss_host(const float* tgt, int logits_ld, const float* baseline, int baseline_ld, const float* beh,
                 const float* actions, const float* noise, const float* rewards, const uint8_t* done, int T, int B, int D,
                 float entropy_cost, const float* ec_param, float ec_mul, int has_target, float target_share,
                 float* d_ec_param, float baseline_cost, float kl_cost, float discounting, float lambda_,
                 float max_abs_reward, float clip_rho, float clip_pg_rho, float mean_denominator, float* d_params,
                 float* d_baseline, float* vs_out, float* pg_out, float* scalars) {
  if (T < 1 || B < 1 || D < 1 || D > 64 || logits_ld < 2 * D || baseline_ld < 1 || !(mean_denominator > 0.f)) return -1;
  const float inv_n = 1.0f / mean_denominator;
  const float ec = ec_param ? expf(ec_mul * ec_param[0]) : entropy_cost;
  std::vector<float> tlp((size_t)T * B), lrho((size_t)T * B), ent((size_t)T * B), vs((size_t)T * B), pg((size_t)T * B);
  for (int t = 0; t < T; ++t)
    for (int b = 0; b < B; ++b) {
      const long long tb = (long long)t * B + b;
      double lane_t[8] = {0}, lane_b[8] = {0};                     // the kernel's 8 lanes per row, then its xor tree
      float lane_e[8] = {0};
      for (int d = 0; d < D; ++d) {
        const float a = actions[tb * D + d];
        const float loc = tgt[tb * logits_ld + d], s = tgt[tb * logits_ld + D + d];
        lane_t[d & 7] += nt::log_prob_term(a, loc, s).v;
        lane_b[d & 7] += nt::log_prob_term(a, beh[tb * 2 * D + d], beh[tb * 2 * D + D + d]).v;
        lane_e[d & 7] += nt::entropy_term(loc, s, noise[tb * D + d]).v;
      }
      auto tree = [](auto* v) {
        for (int o = 1; o < 8; o <<= 1) { double w[8]; for (int i = 0; i < 8; ++i) w[i] = v[i] + v[i ^ o]; for (int i = 0; i < 8; ++i) v[i] = w[i]; }
        return v[0];
      };
      const double lt = tree(lane_t), lb = tree(lane_b);
      tlp[tb] = (float)lt; lrho[tb] = (float)(lt - lb); ent[tb] = tree(lane_e);
    }
  const bool has_rho = clip_rho >= 0.f, has_pg = clip_pg_rho >= 0.f;
  for (int b = 0; b < B; ++b) {
    const float boot = baseline[((long long)T * B + b) * baseline_ld];
    float acc = 0.f, vs_next = boot, v_next = boot;
    for (int t = T - 1; t >= 0; --t) {
      const long long tb = (long long)t * B + b;
      float rw = rewards[tb + B];
      if (max_abs_reward != 0.f) rw = fminf(fmaxf(rw, -max_abs_reward), max_abs_reward);
      const float dsc = (done[tb + B] ? 0.f : 1.f) * discounting;
      const float v = baseline[tb * baseline_ld];
      const float rho = expf(lrho[tb] - 0.f);
      const float crho = has_rho ? fminf(clip_rho, rho) : rho;
      const float cs = fminf(1.0f, rho) * lambda_;
      const float delta = crho * ((rw + dsc * v_next) - v);
      acc = delta + (dsc * cs) * acc;
      const float vv = acc + v;
      const float cpg = has_pg ? fminf(clip_pg_rho, rho) : rho;
      pg[tb] = cpg * ((rw + dsc * vs_next) - v);
      vs[tb] = vv;
      vs_next = vv; v_next = v;
    }
  }
  double s_pg = 0, s_v2 = 0, s_ent = 0, s_kl = 0, s_val = 0, s_std = 0;   // the scalars: summed wide (order-free)
  float maxa = 0.f;
  for (int t = 0; t <= T; ++t)
    for (int b = 0; b < B; ++b) {
      const long long tb = (long long)t * B + b;
      float* dp = d_params + tb * logits_ld;
      if (t == T) {
        for (int d = 0; d < 2 * D; ++d) dp[d] = 0.f;
        d_baseline[tb * baseline_ld] = 0.f;
        continue;
      }
      const float v = baseline[tb * baseline_ld];
      const float coef = (pg[tb] + kl_cost) * inv_n, ecn = ec * inv_n;
      for (int d = 0; d < D; ++d) {
        const float a = actions[tb * D + d];
        const float loc = tgt[tb * logits_ld + d], s = tgt[tb * logits_ld + D + d];
        const nt::LpTerm lp = nt::log_prob_term(a, loc, s);
        const nt::Term en = nt::entropy_term(loc, s, noise[tb * D + d]);
        dp[d] = -(coef * lp.dloc) - ecn * en.dloc;
        dp[D + d] = -(coef * lp.ds) - ecn * en.ds;
        maxa = fmaxf(maxa, fabsf(a));
        s_std += nt::sigma_of(s);
      }
      d_baseline[tb * baseline_ld] = baseline_cost * (v - vs[tb]) * inv_n;
      if (vs_out) vs_out[tb] = vs[tb];
      if (pg_out) pg_out[tb] = pg[tb];
      const float verr = vs[tb] - v;
      s_pg += tlp[tb] * pg[tb]; s_v2 += verr * verr; s_ent += ent[tb]; s_kl += -lrho[tb]; s_val += v;
    }
  const float policy_loss = -((float)s_pg * inv_n), mse = (float)s_v2 * inv_n;
  const float v_loss = baseline_cost * 0.5f * mse, entropy = (float)s_ent * inv_n;
  const float entropy_loss = ec * -entropy, kl_mean = (float)s_kl * inv_n, kl_loss = kl_cost * kl_mean;
  float adjustment = 0.f;
  if (has_target) adjustment = ec * (entropy - target_share);
  if (d_ec_param) d_ec_param[0] = has_target ? ec_mul * ec * (entropy - target_share) : 0.f;
  for (int k = 0; k < 16; ++k) scalars[k] = 0.f;
  scalars[0] = policy_loss + v_loss + entropy_loss + kl_loss + adjustment;
  scalars[1] = policy_loss; scalars[2] = v_loss; scalars[3] = entropy_loss; scalars[4] = kl_loss;
  scalars[5] = entropy; scalars[6] = kl_mean; scalars[7] = (float)s_val * inv_n; scalars[8] = sqrtf(mse);
  scalars[9] = maxa; scalars[10] = ec; scalars[11] = adjustment; scalars[12] = (float)s_std * (inv_n / (float)D);
  return 0;
}

}  // extern "C"

namespace {
struct Reader {
  FILE* f;
  template <class V> std::vector<V> take(size_t n) {
    std::vector<V> v(n);
    if (n && fread(v.data(), sizeof(V), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
  }
};
template <class V> void put(FILE* f, const std::vector<V>& v) { if (!v.empty()) fwrite(v.data(), sizeof(V), v.size(), f); }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s ndtr|terms|loss IN OUT\n", argv[0]); return 2; }
  const std::string mode = argv[1];
  Reader in{fopen(argv[2], "rb")};
  FILE* out = fopen(argv[3], "wb");
  if (!in.f || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  int rc = 0;
  if (mode == "ndtr") {
    const int n = in.take<int32_t>(1)[0];
    const auto z = in.take<float>(n);
    std::vector<float> o(2 * (size_t)n);
    nt_log_ndtr(z.data(), n, o.data());
    put(out, o);
  } else if (mode == "terms") {
    const int n = in.take<int32_t>(1)[0];
    const auto a = in.take<float>(n), loc = in.take<float>(n), s = in.take<float>(n), eps = in.take<float>(n);
    std::vector<float> o(6 * (size_t)n);
    nt_terms(a.data(), loc.data(), s.data(), eps.data(), n, o.data());
    put(out, o);
  } else if (mode == "loss") {
    // ints: T B D ld has_param has_target; floats: entropy_cost ec_param ec_mul target_share baseline_cost kl_cost
    // discounting lambda max_abs_reward clip_rho clip_pg_rho mean_denominator; then head [T+1,B,ld] (baseline in column
    // 2 D), beh, actions, noise, rewards, done
    const auto h = in.take<int32_t>(6);
    const auto c = in.take<float>(12);
    const int T = h[0], B = h[1], D = h[2], ld = h[3];
    if (T < 1 || B < 1 || D < 1 || ld < 2 * D + 1) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t N1 = (size_t)(T + 1) * B, N = (size_t)T * B;
    const auto head = in.take<float>(N1 * ld), beh = in.take<float>(N1 * 2 * D), act = in.take<float>(N1 * D);
    const auto noise = in.take<float>(N * D), rew = in.take<float>(N1);
    const auto done = in.take<uint8_t>(N1);
    std::vector<float> d_head(N1 * ld, 7.0f), vs(N), pg(N), scalars(16), d_ec(1, 7.0f);
    const float ecp = c[1];
    rc = nt_loss_host(head.data(), ld, head.data() + 2 * D, ld, beh.data(), act.data(), noise.data(), rew.data(),
                      done.data(), T, B, D, c[0], h[4] ? &ecp : nullptr, c[2], h[5], c[3], h[4] ? d_ec.data() : nullptr,
                      c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], d_head.data(), d_head.data() + 2 * D, vs.data(),
                      pg.data(), scalars.data());
    put(out, d_head); put(out, vs); put(out, pg); put(out, scalars); put(out, d_ec);
  } else {
    fprintf(stderr, "unknown mode\n");
    rc = 2;
  }
  fclose(in.f); fclose(out);
  return rc;
}
