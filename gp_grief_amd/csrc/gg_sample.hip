// Posterior sampling on the grid: a counter-based Gaussian stream and the
// streaming passes that turn one draw of normals into one posterior draw
// (DESIGN.md section 4.12).
//
// The stream: element i of (seed, stream) is a function of (seed, stream, i)
// alone -- splitmix64's finaliser on a counter (the hash of the Rademacher
// probes, another constant) and Box-Muller on a pair of hashes -- so a vector
// is the same whatever the launch shape and the fused kernels regenerate the
// normals they need instead of reading them.  A thread owns one pair
// (elements 2j, 2j + 1): one hash per element, one log, one sqrt and one
// sincospi per pair, one 16-byte store.
//
// No reference counterpart (the reference draws no posterior sample).
#include <cmath>

#include "gg_internal.h"

namespace gg {

static uint64_t normal_base(uint64_t seed, int stream) {
  return (((seed & 0xffffffffull) << 32) ^ (((uint64_t)stream & 0xffffull) << 16) ^
          0xD1B54A32D192ED03ull);
}

// z[2j] = r cos(2 pi u2), z[2j + 1] = r sin(2 pi u2), r = sqrt(-2 ln u1),
// u1 in (0, 1] and u2 in [0, 1) from the top 53 bits of h(2j), h(2j + 1).
// sincospi(2 u2): 2 u2 is exact, so the angle carries no rounding of 2 pi u2.
__device__ __forceinline__ void normal_pair(uint64_t base, int64_t j, double& zc, double& zs) {
  const uint64_t e = 2 * (uint64_t)j;
  const uint64_t h0 = probe_mix(base + e * 0x9E3779B97F4A7C15ull);
  const uint64_t h1 = probe_mix(base + (e + 1) * 0x9E3779B97F4A7C15ull);
  const double u1 = (double)((h0 >> 11) + 1) * 0x1p-53;
  const double u2 = (double)(h1 >> 11) * 0x1p-53;
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  zc = r * cs;
  zs = r * sn;
}

// store the pair (a, b) to elements 2j, 2j + 1 of v (n elements; the odd
// tail keeps a alone): one 16-byte store when wide
__device__ __forceinline__ void store_pair(double* v, int64_t j, int64_t n, int wide, double a,
                                           double b) {
  const int64_t i = 2 * j;
  if (i + 1 < n) {
    if (wide) {
      reinterpret_cast<double2*>(v)[j] = make_double2(a, b);
    } else {
      v[i] = a;
      v[i + 1] = b;
    }
  } else {
    v[i] = a;
  }
}

__global__ __launch_bounds__(kVecThreads) void normal_fill_kernel(uint64_t base,
                                                                  double* __restrict__ z,
                                                                  int64_t n, int wide) {
  const int64_t np = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < np; j += stride) {
    double a, b;
    normal_pair(base, j, a, b);
    store_pair(z, j, n, wide, a, b);
  }
}

// product of the head's eigenvalues (every factor but the last) at head index h
template <typename kIdx>
__device__ __forceinline__ double kron_head_at(const KronDiag& kd, const double* lam, kIdx h) {
  double t = 1.0;
  for (int k = kd.d - 2; k >= 0; --k) {
    const kIdx mk = (kIdx)kd.m[k];
    const kIdx nx = h / mk;
    t *= lam[kd.off[k] + (int64_t)(h - nx * mk)];
    h = nx;
  }
  return t;
}

// Kronecker eigenvalues of elements i (even) and i + 1: the head is decoded
// once for the pair unless the pair straddles two runs of the last factor
// (t1 = 0 past the end: the odd tail never uses it)
template <typename kIdx>
__device__ __forceinline__ void kron_eig_pair(const KronDiag& kd, const double* lam, kIdx i,
                                              kIdx n, double& t0, double& t1) {
  const kIdx ml = (kIdx)kd.m[kd.d - 1];
  const double* lastl = lam + kd.off[kd.d - 1];
  const kIdx h = i / ml;
  const kIdx l = i - h * ml;
  const double head = kron_head_at<kIdx>(kd, lam, h);
  t0 = head * lastl[l];
  if (i + 1 >= n)
    t1 = 0.0;
  else if (l + 1 < ml)
    t1 = head * lastl[l + 1];
  else
    t1 = kron_head_at<kIdx>(kd, lam, h + 1) * lastl[0];
}

__device__ __forceinline__ double post_coeff(double t, double s, double yt, double z) {
  const double den = t + s;
  return t / den * yt + sqrt(fmax(t, 0.0) * s / den) * z;
}

// c = t / (t + s) yt + sqrt(max(t, 0) s / (t + s)) z: one read, one write
template <typename kIdx>
__global__ __launch_bounds__(kVecThreads) void posterior_coeffs_kernel(
    KronDiag kd, const double* __restrict__ lam, double shift, const double* __restrict__ yt,
    uint64_t base, double* __restrict__ c, int64_t n, int wide) {
  const int64_t np = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < np; j += stride) {
    const int64_t i = 2 * j;
    double y0, y1 = 0.0;
    if (wide && i + 1 < n) {
      const double2 v = reinterpret_cast<const double2*>(yt)[j];
      y0 = v.x;
      y1 = v.y;
    } else {
      y0 = yt[i];
      if (i + 1 < n) y1 = yt[i + 1];
    }
    double t0, t1, z0, z1;
    kron_eig_pair<kIdx>(kd, lam, (kIdx)i, (kIdx)n, t0, t1);
    normal_pair(base, j, z0, z1);
    // t1 = 0 past the end: the unused second value stays finite (shift > 0)
    store_pair(c, j, n, wide, post_coeff(t0, shift, y0, z0), post_coeff(t1, shift, y1, z1));
  }
}

// c = sqrt(max(t, 0)) z: write only
template <typename kIdx>
__global__ __launch_bounds__(kVecThreads) void prior_coeffs_kernel(KronDiag kd,
                                                                   const double* __restrict__ lam,
                                                                   uint64_t base,
                                                                   double* __restrict__ c,
                                                                   int64_t n, int wide) {
  const int64_t np = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < np; j += stride) {
    double t0, t1, z0, z1;
    kron_eig_pair<kIdx>(kd, lam, (kIdx)(2 * j), (kIdx)n, t0, t1);
    normal_pair(base, j, z0, z1);
    store_pair(c, j, n, wide, sqrt(fmax(t0, 0.0)) * z0, sqrt(fmax(t1, 0.0)) * z1);
  }
}

// b = select(mask, y - f - noise_sd z, 0): the select keeps whatever y holds
// at a missing point (NaN included) out of b
__global__ __launch_bounds__(kVecThreads) void sample_residual_kernel(
    const double* __restrict__ y, const double* __restrict__ f,
    const uint8_t* __restrict__ mask, double noise_sd, uint64_t base, double* __restrict__ b,
    int64_t n, int wide) {
  const int64_t np = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < np; j += stride) {
    const int64_t i = 2 * j;
    const bool two = i + 1 < n;
    double y0, y1 = 0.0, f0, f1 = 0.0;
    if (wide && two) {
      const double2 yv = reinterpret_cast<const double2*>(y)[j];
      const double2 fv = reinterpret_cast<const double2*>(f)[j];
      y0 = yv.x;
      y1 = yv.y;
      f0 = fv.x;
      f1 = fv.y;
    } else {
      y0 = y[i];
      f0 = f[i];
      if (two) {
        y1 = y[i + 1];
        f1 = f[i + 1];
      }
    }
    const bool o0 = mask == nullptr || mask[i] != 0;
    const bool o1 = mask == nullptr || (two && mask[i + 1] != 0);
    double z0, z1;
    normal_pair(base, j, z0, z1);
    store_pair(b, j, n, wide, o0 ? y0 - f0 - noise_sd * z0 : 0.0,
               o1 ? y1 - f1 - noise_sd * z1 : 0.0);
  }
}

// per-point noise: b = select(mask, y - f - sqrt(noise) z, 0); noise at a
// missing point is selected away like y (NaN allowed); wide also needs noise
// 16-byte aligned
__global__ __launch_bounds__(kVecThreads) void sample_residual_noise_kernel(
    const double* __restrict__ y, const double* __restrict__ f,
    const double* __restrict__ noise, const uint8_t* __restrict__ mask, uint64_t base,
    double* __restrict__ b, int64_t n, int wide) {
  const int64_t np = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < np; j += stride) {
    const int64_t i = 2 * j;
    const bool two = i + 1 < n;
    double y0, y1 = 0.0, f0, f1 = 0.0, d0, d1 = 0.0;
    if (wide && two) {
      const double2 yv = reinterpret_cast<const double2*>(y)[j];
      const double2 fv = reinterpret_cast<const double2*>(f)[j];
      const double2 dv = reinterpret_cast<const double2*>(noise)[j];
      y0 = yv.x;
      y1 = yv.y;
      f0 = fv.x;
      f1 = fv.y;
      d0 = dv.x;
      d1 = dv.y;
    } else {
      y0 = y[i];
      f0 = f[i];
      d0 = noise[i];
      if (two) {
        y1 = y[i + 1];
        f1 = f[i + 1];
        d1 = noise[i + 1];
      }
    }
    const bool o0 = mask == nullptr || mask[i] != 0;
    const bool o1 = two && (mask == nullptr || mask[i + 1] != 0);
    double z0, z1;
    normal_pair(base, j, z0, z1);
    store_pair(b, j, n, wide, o0 ? y0 - f0 - sqrt(d0) * z0 : 0.0,
               o1 ? y1 - f1 - sqrt(d1) * z1 : 0.0);
  }
}

// draw number k of Welford's running moments
__device__ __forceinline__ void welford(double x, int k, double inv_k, double& mean, double& m2) {
  if (k == 1) {
    mean = x;
    m2 = 0.0;
  } else {
    const double dlt = x - mean;
    mean += dlt * inv_k;
    m2 = fma(dlt, x - mean, m2);
  }
}

// x = f + w, stored to out and / or folded into (mean, m2) as draw k.  out
// may be f or w themselves (element-wise), so none of the three is restrict.
__global__ __launch_bounds__(kVecThreads) void sample_accumulate_kernel(
    const double* f, const double* w, double* out, double* __restrict__ mean,
    double* __restrict__ m2, int k, int64_t n, int wide) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double inv_k = 1.0 / (double)(k > 0 ? k : 1);
  if (wide) {
    const int64_t n2 = n / 2;
    const double2* f2 = reinterpret_cast<const double2*>(f);
    const double2* w2 = reinterpret_cast<const double2*>(w);
    double2* o2 = reinterpret_cast<double2*>(out);
    double2* mean2 = reinterpret_cast<double2*>(mean);
    double2* m22 = reinterpret_cast<double2*>(m2);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += stride) {
      const double2 a = f2[j], b = w2[j];
      double2 x;
      x.x = a.x + b.x;
      x.y = a.y + b.y;
      if (out != nullptr) o2[j] = x;
      if (mean != nullptr) {
        double2 mu = make_double2(0.0, 0.0), q = make_double2(0.0, 0.0);
        if (k != 1) {
          mu = mean2[j];
          q = m22[j];
        }
        welford(x.x, k, inv_k, mu.x, q.x);
        welford(x.y, k, inv_k, mu.y, q.y);
        mean2[j] = mu;
        m22[j] = q;
      }
    }
    if (!(n & 1) || blockIdx.x != 0 || threadIdx.x != 0) return;
  }
  // 8-byte lanes: every element, or the odd tail of the wide path
  const int64_t first = wide ? n - 1 : (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = first; i < n; i += stride) {
    const double x = f[i] + w[i];
    if (out != nullptr) out[i] = x;
    if (mean != nullptr) {
      double mu = 0.0, q = 0.0;
      if (k != 1) {
        mu = mean[i];
        q = m2[i];
      }
      welford(x, k, inv_k, mu, q);
      mean[i] = mu;
      m2[i] = q;
    }
  }
}

// blocks of a grid-stride kernel over the (n + 1) / 2 pairs of n elements
static int pair_blocks(int64_t n) { return vec_blocks(n + 1); }

static void require_stream(int stream) {
  GG_REQUIRE(stream >= 0 && stream <= 65535, GG_ERR_VALUE, "stream must be in [0, 65535]");
}

}  // namespace gg

int gg_normal_fill(uint64_t seed, int stream, double* z_dev, int64_t n, gg_stream s) {
  return gg::guard([&] {
    GG_REQUIRE(z_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    gg::require_stream(stream);
    if (n == 0) return;
    hipLaunchKernelGGL(gg::normal_fill_kernel, dim3(gg::pair_blocks(n)), dim3(gg::kVecThreads),
                       0, gg::as_stream(s), gg::normal_base(seed, stream), z_dev, n,
                       gg::aligned16(z_dev) ? 1 : 0);
    GG_LAUNCH_CHECK();
  });
}

int gg_kron_posterior_coeffs(int d, const int64_t* m, const double* lam_dev, double shift,
                             const double* yt_dev, uint64_t seed, int stream, double* c_dev,
                             gg_stream s) {
  return gg::guard([&] {
    int64_t n = 0;
    gg::KronDiag kd = gg::make_diag(d, m, &n);
    GG_REQUIRE(lam_dev && yt_dev && c_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(shift > 0.0, GG_ERR_VALUE, "shift must be positive");
    gg::require_stream(stream);
    const int wide = gg::aligned16(yt_dev) && gg::aligned16(c_dev) ? 1 : 0;
    const dim3 grid(gg::pair_blocks(n)), block(gg::kVecThreads);
    const uint64_t base = gg::normal_base(seed, stream);
    if (n < (int64_t(1) << 31))
      hipLaunchKernelGGL(gg::posterior_coeffs_kernel<uint32_t>, grid, block, 0, gg::as_stream(s),
                         kd, lam_dev, shift, yt_dev, base, c_dev, n, wide);
    else
      hipLaunchKernelGGL(gg::posterior_coeffs_kernel<int64_t>, grid, block, 0, gg::as_stream(s),
                         kd, lam_dev, shift, yt_dev, base, c_dev, n, wide);
    GG_LAUNCH_CHECK();
  });
}

int gg_kron_prior_coeffs(int d, const int64_t* m, const double* lam_dev, uint64_t seed,
                         int stream, double* c_dev, gg_stream s) {
  return gg::guard([&] {
    int64_t n = 0;
    gg::KronDiag kd = gg::make_diag(d, m, &n);
    GG_REQUIRE(lam_dev && c_dev, GG_ERR_VALUE, "NULL argument");
    gg::require_stream(stream);
    const int wide = gg::aligned16(c_dev) ? 1 : 0;
    const dim3 grid(gg::pair_blocks(n)), block(gg::kVecThreads);
    const uint64_t base = gg::normal_base(seed, stream);
    if (n < (int64_t(1) << 31))
      hipLaunchKernelGGL(gg::prior_coeffs_kernel<uint32_t>, grid, block, 0, gg::as_stream(s), kd,
                         lam_dev, base, c_dev, n, wide);
    else
      hipLaunchKernelGGL(gg::prior_coeffs_kernel<int64_t>, grid, block, 0, gg::as_stream(s), kd,
                         lam_dev, base, c_dev, n, wide);
    GG_LAUNCH_CHECK();
  });
}

int gg_sample_residual(const double* y_dev, const double* f_dev, const uint8_t* mask_dev,
                       double noise_sd, uint64_t seed, int stream, double* b_dev, int64_t n,
                       gg_stream s) {
  return gg::guard([&] {
    GG_REQUIRE(y_dev && f_dev && b_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    gg::require_stream(stream);
    if (n == 0) return;
    const int wide = gg::aligned16(y_dev) && gg::aligned16(f_dev) && gg::aligned16(b_dev) ? 1 : 0;
    hipLaunchKernelGGL(gg::sample_residual_kernel, dim3(gg::pair_blocks(n)),
                       dim3(gg::kVecThreads), 0, gg::as_stream(s), y_dev, f_dev, mask_dev,
                       noise_sd, gg::normal_base(seed, stream), b_dev, n, wide);
    GG_LAUNCH_CHECK();
  });
}

int gg_sample_residual_noise(const double* y_dev, const double* f_dev, const double* noise_dev,
                             const uint8_t* mask_dev, uint64_t seed, int stream, double* b_dev,
                             int64_t n, gg_stream s) {
  return gg::guard([&] {
    GG_REQUIRE(y_dev && f_dev && noise_dev && b_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    gg::require_stream(stream);
    if (n == 0) return;
    const int wide = gg::aligned16(y_dev) && gg::aligned16(f_dev) && gg::aligned16(noise_dev) &&
                             gg::aligned16(b_dev)
                         ? 1
                         : 0;
    hipLaunchKernelGGL(gg::sample_residual_noise_kernel, dim3(gg::pair_blocks(n)),
                       dim3(gg::kVecThreads), 0, gg::as_stream(s), y_dev, f_dev, noise_dev,
                       mask_dev, gg::normal_base(seed, stream), b_dev, n, wide);
    GG_LAUNCH_CHECK();
  });
}

int gg_sample_accumulate(const double* f_dev, const double* w_dev, double* out_dev,
                         double* mean_dev, double* m2_dev, int k, int64_t n, gg_stream s) {
  return gg::guard([&] {
    GG_REQUIRE(f_dev && w_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    GG_REQUIRE((mean_dev == nullptr) == (m2_dev == nullptr), GG_ERR_VALUE,
               "mean and m2 are given together");
    GG_REQUIRE(mean_dev == nullptr || k >= 1, GG_ERR_VALUE, "draws are numbered from 1");
    if (n == 0 || (out_dev == nullptr && mean_dev == nullptr)) return;
    const int wide = gg::aligned16(f_dev) && gg::aligned16(w_dev) && gg::aligned16(out_dev) &&
                             gg::aligned16(mean_dev) && gg::aligned16(m2_dev)
                         ? 1
                         : 0;
    hipLaunchKernelGGL(gg::sample_accumulate_kernel, dim3(gg::vec_blocks(n)),
                       dim3(gg::kVecThreads), 0, gg::as_stream(s), f_dev, w_dev, out_dev,
                       mean_dev, m2_dev, k, n, wide);
    GG_LAUNCH_CHECK();
  });
}
