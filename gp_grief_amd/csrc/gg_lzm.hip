// Masked Lanczos on a Kronecker grid with missing observations
// (gg_lanczos_probe_masked):  A = W K W + s I,  W = diag(mask), from the
// Rademacher probe zeroed at the missing points.
// Every Lanczos vector is zero off the observed set, so restricted to it the
// recurrence is that of K_oo + s I, and u.(K u + s u) = u.A u: the
// shift-and-dot epilogue of the last mode product (gg::kron_apply, grid basis)
// is already alpha's dot -- the observation gg_cgm.hip makes for p.A p.  Only
// the update pass needs the mask.
//
// One step: the matvec's launches, then
//   update  w = select(mask, cy Y, 0) + cu u + cp u_prev in place of Y, with
//           |w|^2 partials            (3 reads + 1 write + the mask, N / 8 of one)
// and the one-thread scalar kernels of the grid-basis probe (lz_coef_kernel,
// lz_beta_kernel, gg_lanczos.hip).  The vectors stay unnormalised with device
// scales as there (v = sV u, v_prev = sP u_prev): no normalisation pass and no
// masking pass over Y; the start vector is select(mask, z, 0) with sV =
// 1 / sqrt(n_obs), n_obs counted on the device by the pass that zeroes z.
// The update mirrors lz_update_kernel (same grid, same lane order, same fma
// order), so with a mask of all ones the tridiagonal is the grid-basis
// probe's to rounding.  The select is a select, never a multiply.
#include <cmath>

#include "gg_internal.h"

namespace gg {

// u = select(mask, u, 0) in place (u holds the +-1 probe); partial observed
// counts (exact in a double: whole numbers below 2^53)
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void lzm_start_kernel(
    double* __restrict__ u, const uint8_t* __restrict__ mask, int64_t n,
    double* __restrict__ partials) {
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    double2* u2 = reinterpret_cast<double2*>(u);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const uint8_t m0 = mask[2 * i], m1 = mask[2 * i + 1];
      double2 uv = u2[i];
      uv.x = sel(m0, uv.x);
      uv.y = sel(m1, uv.y);
      u2[i] = uv;
      acc += (m0 ? 1.0 : 0.0) + (m1 ? 1.0 : 0.0);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const uint8_t m = mask[n - 1];
      u[n - 1] = sel(m, u[n - 1]);
      acc += m ? 1.0 : 0.0;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const uint8_t m = mask[i];
      u[i] = sel(m, u[i]);
      acc += m ? 1.0 : 0.0;
    }
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// the start vector's scale from the observed count: v_0 = sV u_0, sV =
// 1 / sqrt(n_obs) (0 for an empty mask: every later scalar is then 0, and the
// host reports the error after the one synchronisation); sP = 0
__global__ void lzm_scale_kernel(double* __restrict__ lzs, const double* __restrict__ count) {
  const double c = *count;
  lzs[0] = c > 0.0 ? 1.0 / sqrt(c) : 0.0;
  lzs[1] = 0.0;
}

// w = select(mask, cy w, 0) + cu v + cp p (in place), partial w.w
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void lzm_update_kernel(
    double* __restrict__ w, const double* __restrict__ v, const double* __restrict__ pv,
    const uint8_t* __restrict__ mask, int64_t n, const double* __restrict__ lzs,
    double* __restrict__ partials) {
  const double cy = lzs[2], cu = lzs[3], cp = lzs[4];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
    const double2* __restrict__ v2 = reinterpret_cast<const double2*>(v);
    const double2* __restrict__ p2 = reinterpret_cast<const double2*>(pv);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const double2 a = w2[i], b = v2[i], c = p2[i];
      double2 r;
      r.x = fma(cp, c.x, fma(cu, b.x, sel(mask[2 * i], cy * a.x)));
      r.y = fma(cp, c.y, fma(cu, b.y, sel(mask[2 * i + 1], cy * a.y)));
      w2[i] = r;
      acc = fma(r.x, r.x, acc);
      acc = fma(r.y, r.y, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const int64_t i = n - 1;
      const double r = fma(cp, pv[i], fma(cu, v[i], sel(mask[i], cy * w[i])));
      w[i] = r;
      acc = fma(r, r, acc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const double r = fma(cp, pv[i], fma(cu, v[i], sel(mask[i], cy * w[i])));
      w[i] = r;
      acc = fma(r, r, acc);
    }
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- per-point noise (gg_lanczos_probe_masked_noise): A = W K W + D, D =
// diag(noise).  The matvec runs with shift 0 (its epilogue gives u.K u); the
// pass that makes a vector u also emits the partials of sum_i noise_i u_i^2 --
// the start pass for u_0, the update pass for every later one -- and the next
// step's alpha is sV^2 (u.K u + sum noise u^2): one more read of N doubles per
// step.  noise at the missing points is dropped by select (NaN allowed).

// u = select(mask, u, 0) in place; partial observed counts (partials) and
// partials of sum_i noise_i u_i^2 (npartials)
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void lzn_start_kernel(
    double* __restrict__ u, const double* __restrict__ noise, const uint8_t* __restrict__ mask,
    int64_t n, double* __restrict__ partials, double* __restrict__ npartials) {
  double acc = 0.0, nacc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    double2* u2 = reinterpret_cast<double2*>(u);
    const double2* d2 = reinterpret_cast<const double2*>(noise);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const uint8_t m0 = mask[2 * i], m1 = mask[2 * i + 1];
      const double2 dv = d2[i];
      double2 uv = u2[i];
      uv.x = sel(m0, uv.x);
      uv.y = sel(m1, uv.y);
      u2[i] = uv;
      acc += (m0 ? 1.0 : 0.0) + (m1 ? 1.0 : 0.0);
      nacc = fma(sel(m0, dv.x) * uv.x, uv.x, nacc);
      nacc = fma(sel(m1, dv.y) * uv.y, uv.y, nacc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const uint8_t m = mask[n - 1];
      const double uv = sel(m, u[n - 1]);
      u[n - 1] = uv;
      acc += m ? 1.0 : 0.0;
      nacc = fma(sel(m, noise[n - 1]) * uv, uv, nacc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const uint8_t m = mask[i];
      const double uv = sel(m, u[i]);
      u[i] = uv;
      acc += m ? 1.0 : 0.0;
      nacc = fma(sel(m, noise[i]) * uv, uv, nacc);
    }
  }
  const double s = block_sum(acc);
  __syncthreads();   // block_sum's shared scratch is reused
  const double sn = block_sum(nacc);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s;
    npartials[blockIdx.x] = sn;
  }
}

// alpha = sV^2 (u.K u + sum noise u^2) and the update's coefficients
// (lz_coef_kernel with the noise's share of the dot)
__global__ void lzn_coef_kernel(double* __restrict__ lzs, const double* __restrict__ dot,
                                const double* __restrict__ ndot, double* __restrict__ alpha_out,
                                const double* __restrict__ beta_prev) {
  const double sV = lzs[0], sP = lzs[1];
  const double a = sV * sV * (*dot + *ndot);
  *alpha_out = a;
  lzs[2] = sV;
  lzs[3] = -a * sV;
  lzs[4] = -(*beta_prev) * sP;
}

// w = select(mask, cy (w + noise v), 0) + cu v + cp p (in place), partial w.w
// (partials) and partials of sum_i noise_i w_i^2 (npartials)
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void lzn_update_kernel(
    double* __restrict__ w, const double* __restrict__ v, const double* __restrict__ pv,
    const double* __restrict__ noise, const uint8_t* __restrict__ mask, int64_t n,
    const double* __restrict__ lzs, double* __restrict__ partials,
    double* __restrict__ npartials) {
  const double cy = lzs[2], cu = lzs[3], cp = lzs[4];
  double acc = 0.0, nacc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
    const double2* __restrict__ v2 = reinterpret_cast<const double2*>(v);
    const double2* __restrict__ p2 = reinterpret_cast<const double2*>(pv);
    const double2* __restrict__ d2 = reinterpret_cast<const double2*>(noise);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const uint8_t m0 = mask[2 * i], m1 = mask[2 * i + 1];
      const double2 a = w2[i], b = v2[i], c = p2[i], dv = d2[i];
      double2 r;
      r.x = fma(cp, c.x, fma(cu, b.x, sel(m0, cy * fma(dv.x, b.x, a.x))));
      r.y = fma(cp, c.y, fma(cu, b.y, sel(m1, cy * fma(dv.y, b.y, a.y))));
      w2[i] = r;
      acc = fma(r.x, r.x, acc);
      acc = fma(r.y, r.y, acc);
      nacc = fma(sel(m0, dv.x) * r.x, r.x, nacc);
      nacc = fma(sel(m1, dv.y) * r.y, r.y, nacc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const int64_t i = n - 1;
      const uint8_t m = mask[i];
      const double r = fma(cp, pv[i], fma(cu, v[i], sel(m, cy * fma(noise[i], v[i], w[i]))));
      w[i] = r;
      acc = fma(r, r, acc);
      nacc = fma(sel(m, noise[i]) * r, r, nacc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const uint8_t m = mask[i];
      const double r = fma(cp, pv[i], fma(cu, v[i], sel(m, cy * fma(noise[i], v[i], w[i]))));
      w[i] = r;
      acc = fma(r, r, acc);
      nacc = fma(sel(m, noise[i]) * r, r, nacc);
    }
  }
  const double s = block_sum(acc);
  __syncthreads();   // block_sum's shared scratch is reused
  const double sn = block_sum(nacc);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s;
    npartials[blockIdx.x] = sn;
  }
}

// gg_lanczos_probe_masked / _timed / _noise: one driver.  noise == nullptr is
// the scalar probe (W K W + shift I) with the launches it always had; with a
// noise vector the matvec runs with shift 0 and the start, coefficient and
// update kernels are the lzn_* ones, plus one reduction of the noise partials
// per vector made.  step_ms (steps entries, may be null): HIP events on the
// stream at every step boundary, the first after the start vector and its
// scale are made.
static void lanczos_masked(const gg_kron* K, double shift, const double* noise,
                           const uint8_t* mask, uint64_t seed, int probe, int steps,
                           double* work_dev, double* alphas_host, double* betas_host,
                           int* steps_done, int64_t* n_observed, double* step_ms,
                           gg_stream stream) {
  GG_REQUIRE(K && work_dev && alphas_host && betas_host, GG_ERR_VALUE, "NULL argument");
  GG_REQUIRE((reinterpret_cast<uintptr_t>(noise) & 7) == 0, GG_ERR_VALUE,
             "the noise must hold doubles (8-byte aligned)");
  GG_REQUIRE(mask != nullptr, GG_ERR_VALUE, "the masked Lanczos needs a mask");
  GG_REQUIRE(steps >= 1, GG_ERR_VALUE, "Lanczos needs steps >= 1");
  GG_REQUIRE(shift >= 0.0, GG_ERR_VALUE, "Lanczos needs shift >= 0");
  int64_t nr = 0, nc = 0, we = 0;
  check_status(gg_kron_shape(K, 0, &nr, &nc, &we));
  GG_REQUIRE(nr == nc, GG_ERR_VALUE, "Lanczos needs a square operator");
  GG_REQUIRE(we <= nr, GG_ERR_VALUE, "non-square factors are not supported here");
  hipStream_t s = as_stream(stream);
  const int64_t n = nr;
  double* P = work_dev;        // u_prev (v_prev = sP u_prev)
  double* V = work_dev + n;    // u      (v = sV u)
  double* W = work_dev + 2 * n;
  double* mvw = work_dev + 3 * n;
  const int nb = vec_blocks(n);
  const int64_t npart = std::max<int64_t>(kron_partials_needed(K, false), kVecBlocks);
  // [alphas | betas | partials | noise partials | zero | dot | ndot | count | lzs(8)]
  double* scal = nullptr;
  GG_HIP(hipMallocAsync(&scal, (2 * (size_t)steps + npart + kVecBlocks + 4 + 8) * sizeof(double),
                        s));
  double* alphas = scal;
  double* betas = scal + steps;
  double* parts = scal + 2 * steps;
  double* nparts = parts + npart;
  double* zero = nparts + kVecBlocks;
  double* dot = zero + 1;
  double* ndot = dot + 1;
  double* count = ndot + 1;
  double* lzs = count + 1;
  GG_HIP(hipMemsetAsync(zero, 0, sizeof(double), s));
  GG_HIP(hipMemsetAsync(P, 0, n * sizeof(double), s));
  const bool d16 = aligned16(noise);
  // u_0 = select(mask, z, 0), z the +-1 probe over all n grid points
  check_status(gg_probe_fill(seed, probe, V, n, stream));
  if (noise == nullptr) {
    if (aligned16(V))
      hipLaunchKernelGGL(lzm_start_kernel<true>, dim3(nb), dim3(kVecThreads), 0, s, V, mask, n,
                         parts);
    else
      hipLaunchKernelGGL(lzm_start_kernel<false>, dim3(nb), dim3(kVecThreads), 0, s, V, mask, n,
                         parts);
  } else if (aligned16(V) && d16) {
    hipLaunchKernelGGL(lzn_start_kernel<true>, dim3(nb), dim3(kVecThreads), 0, s, V, noise, mask,
                       n, parts, nparts);
  } else {
    hipLaunchKernelGGL(lzn_start_kernel<false>, dim3(nb), dim3(kVecThreads), 0, s, V, noise,
                       mask, n, parts, nparts);
  }
  GG_LAUNCH_CHECK();
  launch_reduce_to(parts, nb, count, s);
  if (noise != nullptr) launch_reduce_to(nparts, nb, ndot, s);
  hipLaunchKernelGGL(lzm_scale_kernel, dim3(1), dim3(1), 0, s, lzs, count);
  GG_LAUNCH_CHECK();
  const bool timed = step_ms != nullptr;
  EventSet sev(timed ? (size_t)steps + 1 : 0);
  if (timed) GG_HIP(hipEventRecord(sev.ev[0], s));
  for (int j = 0; j < steps; ++j) {
    // W = K u + shift u (shift 0 with a noise vector), and u.W per block of the
    // last mode product
    int64_t np = 0;
    kron_apply(K, false, V, W, noise ? 0.0 : shift, mvw, parts, nullptr, s, &np, nullptr, 0,
               nullptr);
    launch_reduce_to(parts, np, dot, s);
    const double* beta_prev = (j == 0) ? zero : betas + (j - 1);
    if (noise == nullptr)
      hipLaunchKernelGGL(lz_coef_kernel, dim3(1), dim3(1), 0, s, lzs, dot, alphas + j,
                         beta_prev);
    else
      hipLaunchKernelGGL(lzn_coef_kernel, dim3(1), dim3(1), 0, s, lzs, dot, ndot, alphas + j,
                         beta_prev);
    GG_LAUNCH_CHECK();
    // 16-byte lanes when all three vectors (and the noise) are 16-byte aligned
    const bool v16 = aligned16(W) && aligned16(V) && aligned16(P);
    if (noise == nullptr) {
      if (v16)
        hipLaunchKernelGGL(lzm_update_kernel<true>, dim3(nb), dim3(kVecThreads), 0, s, W, V, P,
                           mask, n, lzs, parts);
      else
        hipLaunchKernelGGL(lzm_update_kernel<false>, dim3(nb), dim3(kVecThreads), 0, s, W, V, P,
                           mask, n, lzs, parts);
    } else if (v16 && d16) {
      hipLaunchKernelGGL(lzn_update_kernel<true>, dim3(nb), dim3(kVecThreads), 0, s, W, V, P,
                         noise, mask, n, lzs, parts, nparts);
    } else {
      hipLaunchKernelGGL(lzn_update_kernel<false>, dim3(nb), dim3(kVecThreads), 0, s, W, V, P,
                         noise, mask, n, lzs, parts, nparts);
    }
    GG_LAUNCH_CHECK();
    launch_reduce_to(parts, nb, betas + j, s);
    if (noise != nullptr) launch_reduce_to(nparts, nb, ndot, s);
    hipLaunchKernelGGL(lz_beta_kernel, dim3(1), dim3(1), 0, s, lzs, betas + j);
    GG_LAUNCH_CHECK();
    if (j + 1 < steps) {
      // rotate: u_prev <- u, u <- w, the old u_prev buffer takes the next matvec
      double* oldP = P;
      P = V;
      V = W;
      W = oldP;
    }
    if (timed) GG_HIP(hipEventRecord(sev.ev[j + 1], s));
  }
  // staged: an empty mask leaves the host arrays untouched
  std::vector<double> ab(2 * (size_t)steps);
  GG_HIP(hipMemcpyAsync(ab.data(), alphas, 2 * (size_t)steps * sizeof(double),
                        hipMemcpyDeviceToHost, s));
  double count_host = 0.0;
  GG_HIP(hipMemcpyAsync(&count_host, count, sizeof(double), hipMemcpyDeviceToHost, s));
  GG_HIP(hipFreeAsync(scal, s));
  GG_HIP(hipStreamSynchronize(s));
  if (n_observed) *n_observed = (int64_t)count_host;
  GG_REQUIRE(count_host > 0.0, GG_ERR_VALUE, "the mask has no observed point");
  for (int j = 0; j < steps; ++j) {
    alphas_host[j] = ab[j];
    betas_host[j] = ab[steps + j];
  }
  if (timed)
    for (int j = 0; j < steps; ++j) {
      float ms = 0.f;
      GG_HIP(hipEventElapsedTime(&ms, sev.ev[j], sev.ev[j + 1]));
      step_ms[j] = ms;
    }
  int done = steps;
  for (int j = 0; j < steps; ++j)
    if (!(betas_host[j] > 1e-300)) {
      done = j + 1;
      break;
    }
  if (steps_done) *steps_done = done;
}

}  // namespace gg

extern "C" {

int gg_lanczos_probe_masked(const gg_kron* K, double shift, const uint8_t* mask_dev,
                            uint64_t seed, int probe, int steps, double* work_dev,
                            double* alphas_host, double* betas_host, int* steps_done,
                            int64_t* n_observed, gg_stream stream) {
  return gg::guard([&] {
    gg::lanczos_masked(K, shift, nullptr, mask_dev, seed, probe, steps, work_dev, alphas_host,
                       betas_host, steps_done, n_observed, nullptr, stream);
  });
}

int gg_lanczos_probe_masked_noise(const gg_kron* K, const double* noise_dev,
                                  const uint8_t* mask_dev, uint64_t seed, int probe, int steps,
                                  double* work_dev, double* alphas_host, double* betas_host,
                                  int* steps_done, int64_t* n_observed, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(noise_dev != nullptr, GG_ERR_VALUE, "the noise vector is NULL");
    gg::lanczos_masked(K, 0.0, noise_dev, mask_dev, seed, probe, steps, work_dev, alphas_host,
                       betas_host, steps_done, n_observed, nullptr, stream);
  });
}

int gg_lanczos_probe_masked_timed(const gg_kron* K, double shift, const uint8_t* mask_dev,
                                  uint64_t seed, int probe, int steps, double* work_dev,
                                  double* alphas_host, double* betas_host, int* steps_done,
                                  int64_t* n_observed, double* step_ms_host,
                                  gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(step_ms_host != nullptr, GG_ERR_VALUE, "step_ms_host is NULL");
    gg::lanczos_masked(K, shift, nullptr, mask_dev, seed, probe, steps, work_dev, alphas_host,
                       betas_host, steps_done, n_observed, step_ms_host, stream);
  });
}

}  // extern "C"
