// Per-element maths of the tanh-Gaussian policy head (csrc/loss_normal_tanh.hip), as plain fp32 inline functions that
// compile for the device AND for the host: tests/host/normal_tanh_emul.cpp includes this file under g++ with
// AddressSanitizer / UBSan and runs the same arithmetic against the fp64 oracle before anything is launched.
//
// Distribution (common/parametric_distribution.py:124-202 of the reference): per action dimension
//   sigma = softplus(s) + 1e-3,   x ~ N(loc, sigma),   a = tanh(x),
// log_prob(a) with the action clipped to +-thr (thr = 0.999):
//   |a| <  thr:  log N(atanh a; loc, sigma) - fldj(atanh a),   fldj(x) = 2 (log 2 - x - softplus(-2 x)) = log(1 - tanh^2 x)
//   a  <= -thr:  log Phi((-atanh thr - loc) / sigma) - log(1 - thr)          (mass left of the clip, averaged over it)
//   a  >=  thr:  log Phi((loc - atanh thr) / sigma)  - log(1 - thr)          (log survival function)
// entropy: the single-sample estimate 0.5 log(2 pi e sigma^2) + fldj(loc + sigma eps), eps ~ N(0, 1) given by the caller.
//
// Derivatives (DESIGN.md "tanh-Gaussian loss head"), z = (x - loc) / sigma:
// (the functions below return d / d s = d / d sigma * sigmoid(s) directly)
//   interior:  d lp / d loc = z / sigma,        d lp / d sigma = (z^2 - 1) / sigma            (no gradient wrt the action)
//   left:      z = (-x0 - loc) / sigma, r = phi(z) / Phi(z):   d lp / d loc = -r / sigma,  d lp / d sigma = -r z / sigma
//   right:     z = (loc - x0) / sigma:                         d lp / d loc = +r / sigma,  d lp / d sigma = -r z / sigma
//   entropy:   u = loc + sigma eps:  d H / d loc = -2 tanh u,  d H / d sigma = 1 / sigma - 2 eps tanh u
//   d sigma / d s = sigmoid(s).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SEEDHIP_NT_HD __host__ __device__ inline
#else
#define SEEDHIP_NT_HD inline
#endif

namespace seedhip {
namespace nt {

constexpr float kThreshold = 0.999f;                 // TanhTransformedDistribution(threshold=.999)
constexpr float kMinStd = 1e-3f;                     // softplus_default_std_fn
constexpr float kLn2 = 0.69314718055994531f;
constexpr float kHalfLog2Pi = 0.91893853320467274f;  // 0.5 log(2 pi)
constexpr double kLogEps = -6.9077552789821359;     // log(1. - .999) in Python floats, as the reference takes it
constexpr float kErfcxSeries = 4.0f;                 // from here on erfcx comes from its continued fraction

SEEDHIP_NT_HD float softplus(float x) {              // log(1 + e^x) without overflow
  return x > 0.f ? x + log1pf(expf(-x)) : log1pf(expf(x));
}
SEEDHIP_NT_HD float sigmoid(float x) {
  if (x >= 0.f) return 1.f / (1.f + expf(-x));
  const float e = expf(x);
  return e / (1.f + e);
}
SEEDHIP_NT_HD float sigma_of(float s) { return softplus(s) + kMinStd; }

// forward log-det-Jacobian of tanh at x (tfp.bijectors.Tanh); d fldj / dx = -2 tanh x
SEEDHIP_NT_HD float fldj(float x) { return 2.f * ((kLn2 - x) - softplus(-2.f * x)); }

// ---- log_prob: evaluated in fp64 ------------------------------------------------------------------------------------ //
// The V-trace importance ratio is exp(sum_d (lp_target - lp_behaviour)): a difference of two sums of up to 64 terms of
// magnitude up to a few hundred each, and every term is ill-conditioned in its own inputs (d log Phi / dz ~ |z|, the
// interior term carries z^2): in fp32 the rounding of sigma, of atanh(a) and of z alone moves a term by several 1e-6 and
// the sum by 1e-5 .. 1e-4.  The head is latency-bound, so the terms and their sum over D are simply taken in fp64 and
// rounded once (the entropy estimate and everything downstream stay fp32).

SEEDHIP_NT_HD double softplus_d(double x) { return x > 0. ? x + log1p(exp(-x)) : log1p(exp(x)); }

// erfcx(x) = exp(x^2) erfc(x) for x >= kErfcxSeries, by the continued fraction
//   sqrt(pi) erfcx(x) = 1 / (x + (1/2) / (x + (2/2) / (x + (3/2) / (x + ...)))),
// evaluated bottom-up at a fixed depth (16 levels: below 1e-13 relative from x = 4 on).
SEEDHIP_NT_HD double erfcx_large(double x) {
  double t = x;
  for (int k = 16; k >= 1; --k) t = x + (0.5 * (double)k) / t;
  return 0.56418958354775629 / t;
}

// log Phi(z), a true log_ndtr: no -inf for very negative z (z = -20 gives about -203.9).
//   z >= -1:               log1p(-erfc(z / sqrt 2) / 2)
//   z <  -1, x = -z/sqrt2: log(erfcx(x) / 2) - z^2 / 2; below kErfcxSeries erfc(x) itself is far from underflow
//                          (erfc(4) = 1.5e-8), so exp(x^2) cancels exactly and log(erfc(x) / 2) is the same thing
SEEDHIP_NT_HD double log_ndtr(double z) {
  if (z >= -1.) return log1p(-0.5 * erfc(z * 0.70710678118654752));
  const double x = -z * 0.70710678118654752;
  if (x < (double)kErfcxSeries) return log(0.5 * erfc(x));
  return log(0.5 * erfcx_large(x)) - 0.5 * z * z;
}

// d log Phi(z) / dz = phi(z) / Phi(z) = exp(log phi(z) - log Phi(z)); written without the cancellation of the two logs:
// phi / (erfc(x) / 2) while erfc(x) is far from underflow, sqrt(2 / pi) / erfcx(x) beyond.
SEEDHIP_NT_HD double dlog_ndtr(double z) {
  const double x = -z * 0.70710678118654752;
  if (x < (double)kErfcxSeries) return (0.39894228040143268 * exp(-0.5 * z * z)) / (0.5 * erfc(x));
  return 0.79788456080286536 / erfcx_large(x);
}

struct LpTerm { double v; float dloc, ds; };         // log_prob term (fp64) and its derivatives wrt loc and s
struct Term { float v, dloc, ds; };                  // entropy term and its derivatives wrt loc and s

// One action dimension of log_prob(a) for the parameters (loc, s); x0 = atanh(thr) with thr the fp32 0.999.
SEEDHIP_NT_HD LpTerm log_prob_term(float a, float loc_, float s) {
  const double x0 = atanh((double)kThreshold), loc = (double)loc_;
  const double sigma = softplus_d((double)s) + 1e-3;
  const double dsig = (double)sigmoid(s);            // d sigma / d s
  LpTerm o;
  if (a <= -kThreshold || a >= kThreshold) {
    const double sgn = a > 0.f ? 1. : -1.;           // right: Phi((loc - x0) / sigma); left: Phi((-x0 - loc) / sigma)
    const double z = (sgn * loc - x0) / sigma;
    const double r = dlog_ndtr(z);
    o.v = log_ndtr(z) - (double)kLogEps;
    o.dloc = (float)(sgn * r / sigma);
    o.ds = (float)(-(r * z) / sigma * dsig);
    return o;
  }
  const double x = atanh((double)a);
  const double z = (x - loc) / sigma;
  const double j = 2. * ((0.69314718055994531 - x) - softplus_d(-2. * x));     // fldj(x)
  o.v = ((-0.5 * z * z - log(sigma)) - 0.91893853320467274) - j;
  o.dloc = (float)(z / sigma);
  o.ds = (float)((z * z - 1.) / sigma * dsig);
  return o;
}

// One action dimension of the single-sample entropy estimate.
SEEDHIP_NT_HD Term entropy_term(float loc, float s, float eps) {
  const float sigma = sigma_of(s);
  const float u = loc + sigma * eps;
  const float th = tanhf(u);
  Term o;
  o.v = ((0.5f + kHalfLog2Pi) + logf(sigma)) + fldj(u);
  o.dloc = -2.f * th;
  o.ds = (1.f / sigma - 2.f * (eps * th)) * sigmoid(s);
  return o;
}

}  // namespace nt
}  // namespace seedhip
