// ============================================ CG scalars for a host-driven (sharded) CG
// The sharded solve (gp_grief_amd/distributed.py) runs the same recurrence as
// gg_cg_*: local partial dots land in device doubles, the caller all-reduces
// them with RCCL, and these kernels consume the global values.  The update,
// fused-scalars and x-flush kernels are gg_vec.hip's (gg_internal.h).
#include <cmath>

#include "gg_internal.h"

namespace gg {

// q += shift p ; partial p.q -- 16-byte lanes when q and p are 16-byte
// aligned (wide), else 8-byte
__global__ __launch_bounds__(kVecThreads) void shift_dot_kernel(double* __restrict__ q,
                                                                const double* __restrict__ p,
                                                                int64_t n, double shift,
                                                                const CgScalars* __restrict__ sc,
                                                                double* __restrict__ partials,
                                                                int wide) {
  if (sc->done) return;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (wide) {
    const int64_t n2 = n / 2;
    double2* q2 = reinterpret_cast<double2*>(q);
    const double2* p2 = reinterpret_cast<const double2*>(p);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const double2 pv = p2[i];
      double2 v = q2[i];
      v.x = fma(shift, pv.x, v.x);
      v.y = fma(shift, pv.y, v.y);
      q2[i] = v;
      acc = fma(pv.x, v.x, acc);
      acc = fma(pv.y, v.y, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const double v = fma(shift, p[n - 1], q[n - 1]);
      q[n - 1] = v;
      acc = fma(p[n - 1], v, acc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const double pv = p[i];
      const double v = fma(shift, pv, q[i]);
      q[i] = v;
      acc = fma(pv, v, acc);
    }
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// x += alpha p ; r -= alpha q ; partial r.r one double at a time: gg_cgs_update
// on operands that are only 8-byte aligned (cg_xr_update_kernel's 16-byte
// lanes otherwise); the same expressions, so both paths round alike
__global__ __launch_bounds__(kVecThreads) void cgs_xr_update_narrow_kernel(
    double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
    const double* __restrict__ q, int64_t n, const CgScalars* __restrict__ sc,
    double* __restrict__ partials) {
  if (sc->done) return;
  const double a = sc->alpha;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    x[i] += a * p[i];
    const double rv = r[i] - a * q[i];
    r[i] = rv;
    acc = fma(rv, rv, acc);
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// the block partials of a step that the done latch skips were not written:
// its out_dev is 0 (what the caller's all-reduce then sums)
__global__ __launch_bounds__(1024) void cgs_reduce_kernel(const double* __restrict__ partials,
                                                          int64_t count,
                                                          const CgScalars* __restrict__ sc,
                                                          double* __restrict__ out) {
  const double s = sc->done ? 0.0 : sum_partials(partials, count);
  if (threadIdx.x == 0) *out = s;
}

__global__ void cgs_init_kernel(CgScalars* sc, const double* rr, double rtol, double atol) {
  const double s = *rr;
  sc->rho = s;
  sc->rho_prev = 0.0;
  sc->bnorm = sqrt(s);
  sc->tol = fmax(atol, rtol * sc->bnorm);
  sc->iters = 0;
  sc->first = 1;
  sc->pending = 0;
  sc->alpha = sc->beta = sc->pq = 0.0;
  // the fused recurrence's state (unused by the textbook one)
  sc->rq = sc->qq = 0.0;
  sc->repair = 0;
  sc->cancels = 0;
  sc->xpend = 0;
  sc->xh = 2;
  sc->xs = 0;
  sc->done = (s == 0.0 || !(sqrt(s) >= sc->tol)) ? 1 : 0;
}

// ---- fused sharded CG (gg_cgs_fused_*): the single-GPU fused recurrence
// with the dot products reduced across ranks by ONE all-reduce of five
// doubles per iteration, red = [r.r, p.q_old, p.q, 0, q.q] (the caller
// all-reduces it between gg_cgs_fused_post and gg_cgs_fused_scalars)

// block partials of p.q' and q'.q', q' = Y + shift p (Y = K p after the
// exchanges, left unshifted: the next prologue adds shift p_old itself) --
// two read streams, 16-byte lanes (n even, 16-byte aligned vectors)
__global__ __launch_bounds__(kVecThreads) void cgs_post_kernel(
    const double* __restrict__ q, const double* __restrict__ p, int64_t n, double shift,
    const CgScalars* __restrict__ sc, double* __restrict__ part, int64_t pstride) {
  if (sc->done) return;
  double pq = 0.0, qq = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double2* q2 = reinterpret_cast<const double2*>(q);
  const double2* p2 = reinterpret_cast<const double2*>(p);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 2; i += stride) {
    const double2 pv = p2[i];
    double2 v = q2[i];
    v.x = fma(shift, pv.x, v.x);
    v.y = fma(shift, pv.y, v.y);
    pq = fma(pv.x, v.x, pq);
    pq = fma(pv.y, v.y, pq);
    qq = fma(v.x, v.x, qq);
    qq = fma(v.y, v.y, qq);
  }
  const double a = block_sum(pq);
  __syncthreads();
  const double b = block_sum(qq);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = a;
    part[pstride + blockIdx.x] = b;
  }
}

// red = [sum rr_part[0, nrr), sum rr_part[cap, cap + nrr), sum pq, 0, sum qq]
__global__ __launch_bounds__(1024) void cgs_fused_red_kernel(
    const double* __restrict__ rr_part, int64_t nrr, int64_t cap,
    const double* __restrict__ part, int64_t np, int64_t pstride,
    const CgScalars* __restrict__ sc, double* __restrict__ red) {
  // done: neither the prologue nor cgs_post_kernel wrote its partials
  if (sc->done) nrr = np = 0;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < nrr; i += blockDim.x) {
    a[0] += rr_part[i];
    a[1] += rr_part[cap + i];
  }
  for (int64_t i = threadIdx.x; i < np; i += blockDim.x) {
    a[2] += part[i];
    a[3] += part[pstride + i];
  }
  double t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    t[k] = block_sum(a[k]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    red[0] = t[0];
    red[1] = t[1];
    red[2] = t[2];
    red[3] = 0.0;
    red[4] = t[3];
  }
}

// the closing pending update r -= alpha (q + shift p), partial r.r
__global__ __launch_bounds__(kVecThreads) void cgs_close_r_kernel(
    double* __restrict__ r, const double* __restrict__ q, const double* __restrict__ p, int64_t n,
    double shift, const CgScalars* __restrict__ sc, double* __restrict__ partials) {
  if (sc->done || !sc->pending) return;
  const double a = sc->alpha;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double rv = r[i] - a * fma(shift, p[i], q[i]);
    r[i] = rv;
    acc = fma(rv, rv, acc);
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// the closing textbook step (cg_rho_kernel's need_pending 1) from the global
// r.r (all-reduced by the caller)
__global__ void cgs_close_rho_kernel(CgScalars* sc, const double* rr) {
  if (sc->done || !sc->pending) return;
  const double s = *rr;
  sc->rho_prev = sc->rho;
  sc->rho = s;
  sc->beta = s / sc->rho_prev;
  sc->iters += 1;
  sc->first = 0;
  sc->pending = 0;
  sc->repair = 0;
  if (!(sqrt(s) >= sc->tol)) sc->done = 1;
}

__global__ void cgs_alpha_kernel(CgScalars* sc, const double* pq) {
  if (sc->done) return;
  sc->pq = *pq;
  sc->alpha = sc->rho / *pq;
}

__global__ void cgs_rho_kernel(CgScalars* sc, const double* rr) {
  if (sc->done) return;
  const double s = *rr;
  sc->rho_prev = sc->rho;
  sc->rho = s;
  sc->beta = s / sc->rho_prev;
  sc->iters += 1;
  sc->first = 0;
  if (!(sqrt(s) >= sc->tol)) sc->done = 1;
}

}  // namespace gg

struct gg_cgs {
  gg::CgScalars* sc = nullptr;
  gg::CgScalars* host = nullptr;
  double* partials = nullptr;   // kVecBlocks, or 2 x kVecBlocks (fused post)
  // fused recurrence: the prologue launch's r.r / p.q_old partials
  // (2 x rr_cap) and its actual workgroup count
  double* rr_part = nullptr;
  int64_t rr_cap = 0;
  int64_t pro_blocks = 0;
};

namespace gg {

CgScalars* cgs_scalars_ptr(gg_cgs* c) { return c->sc; }

// the prologue partial arrays for launches of up to `cap` workgroups (grown
// on demand, zero-filled)
double* cgs_rr_part(gg_cgs* c, int64_t cap, int64_t* cap_out) {
  if (c->rr_cap < cap) {
    if (c->rr_part) GG_HIP(hipFree(c->rr_part));
    c->rr_part = nullptr;
    GG_HIP(hipMalloc(&c->rr_part, 2 * (size_t)cap * sizeof(double)));
    GG_HIP(hipMemset(c->rr_part, 0, 2 * (size_t)cap * sizeof(double)));
    c->rr_cap = cap;
  }
  *cap_out = c->rr_cap;
  return c->rr_part;
}

void cgs_set_pro_blocks(gg_cgs* c, int64_t nb) { c->pro_blocks = nb; }

}  // namespace gg

extern "C" {

int gg_cgs_create(gg_cgs** out) {
  return gg::guard([&] {
    gg::knobs_reload();   // the handle's switches are the environment's now
    GG_REQUIRE(out, GG_ERR_VALUE, "NULL argument");
    gg_cgs* c = new gg_cgs();
    try {
      GG_HIP(hipMalloc(&c->sc, sizeof(gg::CgScalars)));
      gg::scalars_clear(c->sc);
      GG_HIP(hipHostMalloc(&c->host, sizeof(gg::CgScalars), hipHostMallocDefault));
      GG_HIP(hipMalloc(&c->partials, 2 * gg::kVecBlocks * sizeof(double)));
      GG_HIP(hipMemset(c->partials, 0, 2 * gg::kVecBlocks * sizeof(double)));
    } catch (...) {
      gg_cgs_destroy(c);
      throw;
    }
    *out = c;
  });
}

int gg_cgs_destroy(gg_cgs* c) {
  return gg::guard([&] {
    if (!c) return;
    if (c->sc) (void)hipFree(c->sc);
    if (c->host) (void)hipHostFree(c->host);
    if (c->partials) (void)hipFree(c->partials);
    if (c->rr_part) (void)hipFree(c->rr_part);
    delete c;
  });
}

int gg_cgs_scalars(gg_cgs* c, void** scalars_dev) {
  return gg::guard([&] {
    GG_REQUIRE(c && scalars_dev, GG_ERR_VALUE, "NULL argument");
    *scalars_dev = c->sc;
  });
}

int gg_cgs_local_dot(gg_cgs* c, const double* x_dev, const double* y_dev, int64_t n,
                     double* out_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && x_dev && y_dev && out_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(n >= 0, GG_ERR_VALUE, "n must not be negative");
    hipStream_t s = gg::as_stream(stream);
    const int nb = gg::vec_blocks(n);
    gg::launch_dot_partials(x_dev, y_dev, n, c->partials, nb, s);
    gg::launch_reduce_to(c->partials, nb, out_dev, s);
  });
}

int gg_cgs_init(gg_cgs* c, const double* rr_dev, double rtol, double atol, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && rr_dev && rtol >= 0 && atol >= 0, GG_ERR_VALUE, "bad argument");
    hipLaunchKernelGGL(gg::cgs_init_kernel, dim3(1), dim3(1), 0, gg::as_stream(stream), c->sc,
                       rr_dev, rtol, atol);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_shift_dot(gg_cgs* c, double* q_dev, const double* p_dev, int64_t n, double shift,
                     double* out_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && q_dev && p_dev && out_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(n >= 0, GG_ERR_VALUE, "n must not be negative");
    hipStream_t s = gg::as_stream(stream);
    const int nb = gg::vec_blocks(n);
    const int wide = gg::aligned16(q_dev) && gg::aligned16(p_dev);
    hipLaunchKernelGGL(gg::shift_dot_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, q_dev,
                       p_dev, n, shift, c->sc, c->partials, wide);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gg::cgs_reduce_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                       (int64_t)nb, c->sc, out_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_alpha(gg_cgs* c, const double* pq_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && pq_dev, GG_ERR_VALUE, "NULL argument");
    hipLaunchKernelGGL(gg::cgs_alpha_kernel, dim3(1), dim3(1), 0, gg::as_stream(stream), c->sc,
                       pq_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_update(gg_cgs* c, double* x_dev, double* r_dev, const double* p_dev,
                  const double* q_dev, int64_t n, double* out_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && x_dev && r_dev && p_dev && q_dev && out_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(n >= 0, GG_ERR_VALUE, "n must not be negative");
    hipStream_t s = gg::as_stream(stream);
    const int nb = gg::vec_blocks(n);
    if (gg::aligned16(x_dev) && gg::aligned16(r_dev) && gg::aligned16(p_dev) &&
        gg::aligned16(q_dev))
      hipLaunchKernelGGL(gg::cg_xr_update_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, x_dev,
                         r_dev, p_dev, q_dev, n, c->sc, c->partials, 0);
    else
      hipLaunchKernelGGL(gg::cgs_xr_update_narrow_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                         x_dev, r_dev, p_dev, q_dev, n, c->sc, c->partials);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gg::cgs_reduce_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                       (int64_t)nb, c->sc, out_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_rho(gg_cgs* c, const double* rr_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && rr_dev, GG_ERR_VALUE, "NULL argument");
    hipLaunchKernelGGL(gg::cgs_rho_kernel, dim3(1), dim3(1), 0, gg::as_stream(stream), c->sc,
                       rr_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_fused_post(gg_cgs* c, const double* q_dev, const double* p_dev, int64_t n,
                      double shift, double* red_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && q_dev && p_dev && red_dev && n >= 2 && n % 2 == 0, GG_ERR_VALUE,
               "bad argument");
    GG_REQUIRE(gg::aligned16(q_dev) && gg::aligned16(p_dev), GG_ERR_VALUE,
               "fused post needs 16-byte aligned vectors");
    GG_REQUIRE(c->rr_part && c->pro_blocks > 0, GG_ERR_VALUE,
               "gg_cgs_fused_post needs a fused phase 1 first");
    hipStream_t s = gg::as_stream(stream);
    const int nb = gg::vec_blocks(n);
    hipLaunchKernelGGL(gg::cgs_post_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, q_dev, p_dev,
                       n, shift, c->sc, c->partials, (int64_t)gg::kVecBlocks);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gg::cgs_fused_red_kernel, dim3(1), dim3(1024), 0, s, c->rr_part,
                       c->pro_blocks, c->rr_cap, c->partials, (int64_t)nb,
                       (int64_t)gg::kVecBlocks, c->sc, red_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_fused_scalars(gg_cgs* c, const double* red_dev, const double* p_new_dev,
                         gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && red_dev && p_new_dev, GG_ERR_VALUE, "NULL argument");
    // red = [rr, p.q_old | p.q, (r.q), q.q]: the single-GPU scalars kernel
    // with one-element partial arrays (rr stride 1, matvec stride 1)
    hipLaunchKernelGGL(gg::cg_fused_scalars_kernel, dim3(1), dim3(1024), 0, gg::as_stream(stream),
                       red_dev, (int64_t)1, (int64_t)1, red_dev + 2, (int64_t)1, (int64_t)1,
                       c->sc, p_new_dev, 2, 1, 0);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_fused_close(gg_cgs* c, double* x_dev, double* r_dev, const double* q_dev,
                       const double* p_dev, int64_t n, int64_t half, double shift,
                       double* rr_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && x_dev && r_dev && q_dev && p_dev && rr_dev && n >= 0 && half >= 0 &&
                   half <= n,
               GG_ERR_VALUE, "bad argument");
    hipStream_t s = gg::as_stream(stream);
    const int nb = gg::vec_blocks(n);
    // the deferred x steps, then the pending r update with its r.r partials
    hipLaunchKernelGGL(gg::cg_x_flush2_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, x_dev, n,
                       half, c->sc);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gg::cg_x_flushed_kernel, dim3(1), dim3(1), 0, s, c->sc);
    GG_LAUNCH_CHECK();
    GG_HIP(hipMemsetAsync(c->partials, 0, nb * sizeof(double), s));
    hipLaunchKernelGGL(gg::cgs_close_r_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, r_dev,
                       q_dev, p_dev, n, shift, c->sc, c->partials);
    GG_LAUNCH_CHECK();
    gg::launch_reduce_to(c->partials, nb, rr_dev, s);
  });
}

int gg_cgs_fused_close_rho(gg_cgs* c, const double* rr_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && rr_dev, GG_ERR_VALUE, "NULL argument");
    hipLaunchKernelGGL(gg::cgs_close_rho_kernel, dim3(1), dim3(1), 0, gg::as_stream(stream), c->sc,
                       rr_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_cgs_status(gg_cgs* c, int* iters, int* done, double* rho, double* tol,
                  gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c, GG_ERR_VALUE, "NULL handle");
    hipStream_t s = gg::as_stream(stream);
    GG_HIP(hipMemcpyAsync(c->host, c->sc, sizeof(gg::CgScalars), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    if (iters) *iters = c->host->iters;
    if (done) *done = c->host->done;
    if (rho) *rho = c->host->rho;
    if (tol) *tol = c->host->tol;
  });
}

}  // extern "C"
