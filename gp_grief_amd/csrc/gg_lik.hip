// Non-Gaussian likelihoods for the Laplace approximation on a grid (Poisson
// with a log link, binomial with a logit link): the streaming passes between
// the Kronecker matvec f = K a and the weighted masked CG (gg_cgm.hip) of a
// Newton step.
//
// gg_lik_newton: one fused grid-stride pass over (y, aux, f, a, mask) that
// writes the Newton step's noise 1 / w and right-hand side select(mask, f + g /
// w, 0) and reduces the five sums the host steers the iteration by.  Launches:
// the pass (vec_blocks(n) workgroups, five partials each) and a one-block
// finishing kernel; no atomics, so the sums are deterministic for a given n
// and lane width.  Lanes: 16 bytes where every stream of the call is 16-byte
// aligned, else 8 bytes for the whole pass (the rule of gg_cgm_set_noise).
// The element arithmetic is one function (lik_point) whatever the lanes, so
// the element outputs do not depend on the alignment.
//
// Transcendentals per observed point: one exp (Poisson; a second where |f| >
// 700, for the rate at the unclamped f), one exp and two log1p (binomial; one
// log1p where |f| > 700; the write form besides a two-term exp(f) for f >= 0,
// about 60 multiply-adds and no division), one log of aux only when aux is
// given (sum log w); divisions: one (Poisson, write form), two (binomial, one
// in the read-only form).  lgamma is not here: the normaliser of log p does
// not depend on f and stays on the host (include/gp_grief_amd.h).
//
// gg_lik_response_accumulate: r = exp(f + w) or sigmoid(f + w) folded into
// Welford's moments, the contract of gg_sample_accumulate.
#include "gg_internal.h"

// every fused multiply-add of this file is written out: the element outputs
// and the sums are then the same IEEE operations in every instantiation (lane
// width, write / read-only form)
#pragma clang fp contract(off)

namespace gg {

constexpr int kLikSums = 5;
// |f| beyond this is clamped where the curvature w is formed (never for log p
// or g): exp(-700) ~ 1e-304 keeps 1 / w finite
constexpr double kLikClamp = 700.0;

// exp(x) for 0 <= x <= 700 as an unevaluated sum hi + lo, to about 2^-66 of
// its value: x = k ln 2 + r with ln 2 in three parts (k L1 is exact), exp(r / 8)
// as 1 + q + q^2 / 2 in two-term arithmetic plus the Taylor tail from q^3 on in
// plain double (|q| <= 0.044: the tail is below 2^-16 of the sum), squared
// three times, scaled by 2^k.
__device__ __forceinline__ void exp_dd(double x, double& hi, double& lo) {
  const double k = rint(x * 0x1.71547652b82fep+0);
  const double r1 = fma(-k, 0x1.62e42fee00000p-1, x);           // exact
  const double p = k * 0x1.a39ef35793c76p-33;
  const double pe = fma(k, 0x1.a39ef35793c76p-33, -p);          // k L2 = p + pe
  double rh = r1 - p;                                           // two-sum
  double bb = rh - r1;
  double rl = ((r1 - (rh - bb)) - (p + bb)) - fma(k, 0x1.cc01f97b57a08p-87, pe);
  const double qh = 0.125 * (rh + rl);
  const double ql = 0.125 * ((rh - 8.0 * qh) + rl);
  double t = 1.0 / 39916800.0;
  t = fma(t, qh, 1.0 / 3628800.0);
  t = fma(t, qh, 1.0 / 362880.0);
  t = fma(t, qh, 1.0 / 40320.0);
  t = fma(t, qh, 1.0 / 5040.0);
  t = fma(t, qh, 1.0 / 720.0);
  t = fma(t, qh, 1.0 / 120.0);
  t = fma(t, qh, 1.0 / 24.0);
  t = fma(t, qh, 1.0 / 6.0);
  const double q2 = qh * qh;
  const double q2e = fma(qh, qh, -q2);                          // qh^2 = q2 + q2e
  const double tail = t * q2 * qh;
  const double s1 = 1.0 + qh;                                   // fast two-sum, 1 > |qh|
  const double e1 = qh - (s1 - 1.0);
  const double h2 = 0.5 * q2;
  const double s2 = s1 + h2;                                    // fast two-sum, s1 > h2
  const double e2 = h2 - (s2 - s1);
  double l = (e1 + e2) + (fma(qh, ql, 0.5 * q2e) + ql) + fma(ql, h2, tail);
  double h = s2 + l;
  l = l - (h - s2);
#pragma unroll
  for (int i = 0; i < 3; ++i) {                                 // (h + l)^2
    const double ph = h * h;
    const double pl = fma(h, h, -ph) + 2.0 * (h * l);
    h = ph + pl;
    l = pl - (h - ph);
  }
  const int ik = (int)k;
  hi = ldexp(h, ik);
  lo = ldexp(l, ik);
}

// what one observed point contributes
struct LikPoint {
  double logp;   // log p without its f-independent normaliser
  double g;      // d log p / d f
  double logw;   // log of w = -d^2 log p / d f^2 (f clamped)
  double noise;  // 1 / w                       (WRITE only)
  double b;      // f + g / w                   (WRITE only)
};

// KIND 0: Poisson, rate e exp(f).  KIND 1: binomial, y of e trials, logit link.
// b = f + g / w is formed from y / w and the closed form of the rest (-1, or
// -1 / sigmoid(-f)), not from the quotient of two rounded values.  Binomial, f
// >= 0: 1 / sigmoid(-f) = 1 + exp(f) dwarfs f, and where y = 0 it is all of b,
// with 1e-14 (f + 1) as its error budget -- less than half the spacing of the
// doubles at b from f = 36 on, so b has to be the correctly rounded value
// there.  It is taken as 1 + (r + r_lo), r + r_lo = exp(f) to 2^-64 (exp_dd: a
// reciprocal of the rounded exp(-f) would carry that exp's ulp, a whole
// spacing of b), and joined to the rest by an exact two-term sum, so b carries
// one rounding.
template <int KIND, bool WRITE>
__device__ __forceinline__ LikPoint lik_point(double y, double e, bool has_aux, double f) {
  LikPoint o;
  o.noise = o.b = 0.0;
  const double fc = fmin(fmax(f, -kLikClamp), kLikClamp);
  if (KIND == 0) {
    const double ec = exp(fc);
    // the rate at the unclamped f: one exp serves both within the clamp; beyond
    // it exp(f) itself (finite up to f = 709.78, then inf; denormal, then 0)
    const double ex = fabs(f) > kLikClamp ? exp(f) : ec;
    const double rate = e * ex;
    o.g = y - rate;
    o.logp = fma(y, f, -rate);
    o.logw = has_aux ? fc + log(e) : fc;
    if (WRITE) {
      o.noise = 1.0 / (e * ec);
      o.b = f + fma(y, o.noise, -1.0);
    }
  } else {
    const double af = fabs(f);
    const double afc = fabs(fc);
    const double t = exp(-afc);   // never exp of a positive argument
    // exp(-|f|) at the unclamped f: 0 beyond the clamp, as exp gives there
    const double tu = af > kLikClamp ? 0.0 : t;
    const double rdu = 1.0 / (1.0 + tu);
    const double sig = f >= 0.0 ? rdu : tu * rdu;   // sigmoid(f)
    o.g = fma(-e, sig, y);
    o.logp = fma(y, f, -e * (fmax(f, 0.0) + log1p(tu)));
    const double lw = -afc - 2.0 * log1p(t);
    o.logw = has_aux ? lw + log(e) : lw;
    if (WRITE) {
      const double den = 1.0 + t;
      o.noise = (den * den) / (e * t);              // 1 / (e sigmoid(f) sigmoid(-f))
      // b = (y / w + f - 1) - r - r_lo, r + r_lo = exp(|fc|) (f >= 0) or t
      double r = t, r_lo = 0.0;
      if (f >= 0.0) exp_dd(afc, r, r_lo);
      const double s = fma(y, o.noise, f - 1.0);
      const double hi = s - r;                       // two-sum: hi + lo = s - r
      const double bb = hi - s;
      const double lo = (s - (hi - bb)) - (r + bb);
      o.b = hi + (lo - r_lo);
    }
  }
  return o;
}

struct LikAcc {
  double s[kLikSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
};

// one point: the element outputs (write form) and the five sums, everything
// at a missing point selected away (y, aux and f's terms may be NaN there)
template <int KIND, bool WRITE>
__device__ __forceinline__ void lik_elem(uint8_t m, double y, double e, bool has_aux, double f,
                                         double a, LikAcc& acc, double& noise, double& b) {
  if (!m) {
    noise = 1.0;
    b = 0.0;
    return;
  }
  const LikPoint p = lik_point<KIND, WRITE>(y, e, has_aux, f);
  noise = p.noise;
  b = p.b;
  const double d = p.g - a;
  acc.s[0] += p.logp;
  acc.s[1] = fma(a, f, acc.s[1]);
  acc.s[2] += p.logw;
  acc.s[3] = fma(d, d, acc.s[3]);
  acc.s[4] = fma(p.g, p.g, acc.s[4]);
}

// V2: 16-byte lanes (every stream 16-byte aligned).  WRITE false: the
// read-only objective evaluation -- the same sums by the same operations
// (contraction is off in this file: every fma is written out), no store.
// partials: kLikSums rows of kVecBlocks.
template <int KIND, bool V2, bool WRITE>
__global__ __launch_bounds__(kVecThreads) void lik_newton_kernel(
    const double* __restrict__ y, const double* __restrict__ aux, const double* __restrict__ f,
    const double* __restrict__ a, const uint8_t* __restrict__ mask, double* __restrict__ noise,
    double* __restrict__ b, int64_t n, double* __restrict__ partials) {
  LikAcc acc;
  const bool has_aux = aux != nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (V2) {
    const int64_t n2 = n / 2;
    const double2* y2 = reinterpret_cast<const double2*>(y);
    const double2* e2 = reinterpret_cast<const double2*>(aux);
    const double2* f2 = reinterpret_cast<const double2*>(f);
    const double2* a2 = reinterpret_cast<const double2*>(a);
    double2* d2 = reinterpret_cast<double2*>(noise);
    double2* b2 = reinterpret_cast<double2*>(b);
    for (int64_t i = tid; i < n2; i += stride) {
      const uint8_t m0 = mask ? mask[2 * i] : 1, m1 = mask ? mask[2 * i + 1] : 1;
      const double2 yv = y2[i], fv = f2[i], av = a2[i];
      const double2 ev = has_aux ? e2[i] : make_double2(1.0, 1.0);
      double2 dv, bv;
      lik_elem<KIND, WRITE>(m0, yv.x, ev.x, has_aux, fv.x, av.x, acc, dv.x, bv.x);
      lik_elem<KIND, WRITE>(m1, yv.y, ev.y, has_aux, fv.y, av.y, acc, dv.y, bv.y);
      if (WRITE) {
        d2[i] = dv;
        b2[i] = bv;
      }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const int64_t i = n - 1;
      double dv, bv;
      lik_elem<KIND, WRITE>(mask ? mask[i] : 1, y[i], has_aux ? aux[i] : 1.0, has_aux, f[i],
                            a[i], acc, dv, bv);
      if (WRITE) {
        noise[i] = dv;
        b[i] = bv;
      }
    }
  } else {
    for (int64_t i = tid; i < n; i += stride) {
      double dv, bv;
      lik_elem<KIND, WRITE>(mask ? mask[i] : 1, y[i], has_aux ? aux[i] : 1.0, has_aux, f[i],
                            a[i], acc, dv, bv);
      if (WRITE) {
        noise[i] = dv;
        b[i] = bv;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kLikSums; ++k) {
    if (k) __syncthreads();   // block_sum's shared scratch is reused
    const double s = block_sum(acc.s[k]);
    if (threadIdx.x == 0) partials[(int64_t)k * kVecBlocks + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(1024) void lik_finish_kernel(const double* __restrict__ partials,
                                                          int64_t count,
                                                          double* __restrict__ sums) {
  for (int k = 0; k < kLikSums; ++k) {
    if (k) __syncthreads();
    const double s = sum_partials(partials + (int64_t)k * kVecBlocks, count);
    if (threadIdx.x == 0) sums[k] = s;
  }
}

template <int KIND>
__device__ __forceinline__ double lik_response(double x) {
  if (KIND == 0) return exp(x);
  const double t = exp(-fabs(x));
  const double inv = 1.0 / (1.0 + t);
  return x >= 0.0 ? inv : t * inv;
}

// the running moments of gg_sample_accumulate's Welford update (gg_sample.hip)
__device__ __forceinline__ void lik_welford(double x, int k, double inv_k, double& mean,
                                            double& m2) {
  if (k == 1) {
    mean = x;
    m2 = 0.0;
  } else {
    const double dlt = x - mean;
    mean += dlt * inv_k;
    m2 = fma(dlt, x - mean, m2);
  }
}

template <int KIND>
__global__ __launch_bounds__(kVecThreads) void lik_response_kernel(
    const double* __restrict__ f, const double* __restrict__ w, double* __restrict__ mean,
    double* __restrict__ m2, int k, int64_t n, int wide) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double inv_k = 1.0 / (double)k;
  if (wide) {
    const int64_t n2 = n / 2;
    const double2* f2 = reinterpret_cast<const double2*>(f);
    const double2* w2 = reinterpret_cast<const double2*>(w);
    double2* mean2 = reinterpret_cast<double2*>(mean);
    double2* m22 = reinterpret_cast<double2*>(m2);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += stride) {
      const double2 fv = f2[j], wv = w2[j];
      double2 mu = make_double2(0.0, 0.0), q = make_double2(0.0, 0.0);
      if (k != 1) {
        mu = mean2[j];
        q = m22[j];
      }
      lik_welford(lik_response<KIND>(fv.x + wv.x), k, inv_k, mu.x, q.x);
      lik_welford(lik_response<KIND>(fv.y + wv.y), k, inv_k, mu.y, q.y);
      mean2[j] = mu;
      m22[j] = q;
    }
    if (!(n & 1) || blockIdx.x != 0 || threadIdx.x != 0) return;
  }
  // 8-byte lanes: every element, or the odd tail of the wide path
  const int64_t first = wide ? n - 1 : (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = first; i < n; i += stride) {
    double mu = 0.0, q = 0.0;
    if (k != 1) {
      mu = mean[i];
      q = m2[i];
    }
    lik_welford(lik_response<KIND>(f[i] + w[i]), k, inv_k, mu, q);
    mean[i] = mu;
    m2[i] = q;
  }
}

static bool doubles(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

template <int KIND, bool V2>
static void launch_lik_newton2(int nb, hipStream_t s, const double* y, const double* aux,
                               const double* f, const double* a, const uint8_t* mask,
                               double* noise, double* b, int64_t n, double* partials) {
  if (noise != nullptr)
    hipLaunchKernelGGL((lik_newton_kernel<KIND, V2, true>), dim3(nb), dim3(kVecThreads), 0, s, y,
                       aux, f, a, mask, noise, b, n, partials);
  else
    hipLaunchKernelGGL((lik_newton_kernel<KIND, V2, false>), dim3(nb), dim3(kVecThreads), 0, s,
                       y, aux, f, a, mask, noise, b, n, partials);
}

template <int KIND>
static void launch_lik_newton(bool v2, int nb, hipStream_t s, const double* y, const double* aux,
                              const double* f, const double* a, const uint8_t* mask,
                              double* noise, double* b, int64_t n, double* partials) {
  if (v2)
    launch_lik_newton2<KIND, true>(nb, s, y, aux, f, a, mask, noise, b, n, partials);
  else
    launch_lik_newton2<KIND, false>(nb, s, y, aux, f, a, mask, noise, b, n, partials);
}

}  // namespace gg

int gg_lik_newton(int kind, const double* y_dev, const double* aux_dev, const double* f_dev,
                  const double* a_dev, const uint8_t* mask_dev, double* noise_out,
                  double* b_out, double* sums_dev, double* partials_dev, int64_t n,
                  gg_stream s) {
  return gg::guard([&] {
    GG_REQUIRE(kind == GG_LIK_POISSON || kind == GG_LIK_BINOMIAL, GG_ERR_VALUE,
               "unknown likelihood kind");
    GG_REQUIRE(y_dev && f_dev && a_dev && sums_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    GG_REQUIRE((noise_out == nullptr) == (b_out == nullptr), GG_ERR_VALUE,
               "noise_out and b_out are given together");
    GG_REQUIRE(partials_dev != nullptr || n == 0, GG_ERR_VALUE, "NULL partials");
    GG_REQUIRE(gg::doubles(y_dev) && gg::doubles(aux_dev) && gg::doubles(f_dev) &&
                   gg::doubles(a_dev) && gg::doubles(noise_out) && gg::doubles(b_out) &&
                   gg::doubles(sums_dev) && gg::doubles(partials_dev),
               GG_ERR_VALUE, "the vectors must hold doubles (8-byte aligned)");
    hipStream_t st = gg::as_stream(s);
    if (n == 0) {
      GG_HIP(hipMemsetAsync(sums_dev, 0, gg::kLikSums * sizeof(double), st));
      return;
    }
    const bool v2 = gg::aligned16(y_dev) && gg::aligned16(aux_dev) && gg::aligned16(f_dev) &&
                    gg::aligned16(a_dev) && gg::aligned16(noise_out) && gg::aligned16(b_out);
    const int nb = gg::vec_blocks(n);
    if (kind == GG_LIK_POISSON)
      gg::launch_lik_newton<0>(v2, nb, st, y_dev, aux_dev, f_dev, a_dev, mask_dev, noise_out,
                               b_out, n, partials_dev);
    else
      gg::launch_lik_newton<1>(v2, nb, st, y_dev, aux_dev, f_dev, a_dev, mask_dev, noise_out,
                               b_out, n, partials_dev);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gg::lik_finish_kernel, dim3(1), dim3(1024), 0, st, partials_dev,
                       (int64_t)nb, sums_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_lik_response_accumulate(int kind, const double* f_dev, const double* w_dev,
                               double* mean_dev, double* m2_dev, int k, int64_t n, gg_stream s) {
  return gg::guard([&] {
    GG_REQUIRE(kind == GG_LIK_POISSON || kind == GG_LIK_BINOMIAL, GG_ERR_VALUE,
               "unknown likelihood kind");
    GG_REQUIRE(f_dev && w_dev && mean_dev && m2_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    GG_REQUIRE(k >= 1, GG_ERR_VALUE, "draws are numbered from 1");
    GG_REQUIRE(gg::doubles(f_dev) && gg::doubles(w_dev) && gg::doubles(mean_dev) &&
                   gg::doubles(m2_dev),
               GG_ERR_VALUE, "the vectors must hold doubles (8-byte aligned)");
    if (n == 0) return;
    const int wide = gg::aligned16(f_dev) && gg::aligned16(w_dev) && gg::aligned16(mean_dev) &&
                             gg::aligned16(m2_dev)
                         ? 1
                         : 0;
    const dim3 grid(gg::vec_blocks(n)), block(gg::kVecThreads);
    if (kind == GG_LIK_POISSON)
      hipLaunchKernelGGL(gg::lik_response_kernel<0>, grid, block, 0, gg::as_stream(s), f_dev,
                         w_dev, mean_dev, m2_dev, k, n, wide);
    else
      hipLaunchKernelGGL(gg::lik_response_kernel<1>, grid, block, 0, gg::as_stream(s), f_dev,
                         w_dev, mean_dev, m2_dev, k, n, wide);
    GG_LAUNCH_CHECK();
  });
}
