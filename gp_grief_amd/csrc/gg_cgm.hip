// Masked CG on a Kronecker grid with missing observations (gg_cgm_*):
//   A = W K W + s I,  W = diag(mask),  A x = W b,  x0 = 0.
// r, p and x are zero off the observed set for every iteration, so
// p.(K p + s p) = p.A p and the shift-and-dot epilogue of the last mode product
// (gg::kron_apply, grid basis) is already the CG's p.A p; only the r update
// needs the mask.  Every select is a select, never a multiply: b may hold NaN
// at the missing points.
//
// One iteration (unpreconditioned): the matvec's launches, then
//   direction  p = u + beta p                (3 passes; u = r, already masked)
//   update     x += alpha p, r -= alpha select(mask, t, 0), r.r partials
//                                            (6 passes + the mask, N / 8 of one)
// and two one-block scalar kernels.  All scalars stay on the device; the host
// polls `done` every check_every iterations, and every kernel returns early
// once it is set.  The vector kernels mirror gg_vec.hip's textbook kernels
// (same grid, same lane order, same fma order), so with a mask of all ones the
// iterates are those of gg_cg_* (textbook recurrence, grid basis).
//
// Preconditioned (gg_cgm_set_precond): z = Q diag(1 / (lam + s)) Q^T r from the
// per-factor eigenpairs of K -- two more Kronecker matvecs, a decoded divide
// and the dot r.z per iteration; the direction kernel applies W (u = z).
//
// Per-point noise (gg_cgm_set_noise): A = W K W + D, D = diag(noise).  The
// matvec runs with shift 0, so its epilogue yields p.K p; the direction pass
// also reads noise and emits partials of sum_i noise_i p_i^2 (its own region of
// the partials buffer, past the matvec's), the alpha kernel sums both sets and
// the update pass uses select(mask, t_i + noise_i p_i, 0): two more reads of N
// doubles per iteration, no more launches.  noise at the missing points is
// dropped by select (it may be NaN there).  `shift` then only feeds the
// preconditioner.
#include <cmath>
#include <vector>

#include "gg_internal.h"

namespace gg {

// the masked CG's device scalars
struct CgmScalars {
  double rho;       // r.z (r.r unpreconditioned) of the current residual
  double rho_prev;
  double rr;        // r.r: the stopping test is on the true residual norm
  double pq;        // p.(A p)
  double alpha;
  double beta;
  double tol;       // stop when sqrt(rr) < tol
  double bnorm;     // |W b|
  int iters;        // completed iterations
  int done;         // 1 = converged / stopped: every kernel becomes a no-op
  int first;        // 1 = the next direction is p = u
};

// r = select(mask, b, 0) ; x = 0 ; partial r.r
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void cgm_start_kernel(
    const double* __restrict__ b, const uint8_t* __restrict__ mask, double* __restrict__ x,
    double* __restrict__ r, int64_t n, double* __restrict__ partials) {
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    const double2* b2 = reinterpret_cast<const double2*>(b);
    double2* x2 = reinterpret_cast<double2*>(x);
    double2* r2 = reinterpret_cast<double2*>(r);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const double2 bv = b2[i];
      double2 rv;
      rv.x = sel(mask[2 * i], bv.x);
      rv.y = sel(mask[2 * i + 1], bv.y);
      r2[i] = rv;
      x2[i] = make_double2(0.0, 0.0);
      acc = fma(rv.x, rv.x, acc);
      acc = fma(rv.y, rv.y, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const double rv = sel(mask[n - 1], b[n - 1]);
      r[n - 1] = rv;
      x[n - 1] = 0.0;
      acc = fma(rv, rv, acc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const double rv = sel(mask[i], b[i]);
      r[i] = rv;
      x[i] = 0.0;
      acc = fma(rv, rv, acc);
    }
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// x += alpha p ; r -= alpha select(mask, t, 0) ; partial r.r
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void cgm_xr_update_kernel(
    double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
    const double* __restrict__ t, const uint8_t* __restrict__ mask, int64_t n,
    const CgmScalars* __restrict__ sc, double* __restrict__ partials) {
  if (sc->done) return;
  const double a = sc->alpha;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    double2* x2 = reinterpret_cast<double2*>(x);
    double2* r2 = reinterpret_cast<double2*>(r);
    const double2* p2 = reinterpret_cast<const double2*>(p);
    const double2* t2 = reinterpret_cast<const double2*>(t);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const double2 pv = p2[i], tv = t2[i];
      double2 xv = x2[i], rv = r2[i];
      xv.x = fma(a, pv.x, xv.x);
      xv.y = fma(a, pv.y, xv.y);
      rv.x = fma(-a, sel(mask[2 * i], tv.x), rv.x);
      rv.y = fma(-a, sel(mask[2 * i + 1], tv.y), rv.y);
      x2[i] = xv;
      r2[i] = rv;
      acc = fma(rv.x, rv.x, acc);
      acc = fma(rv.y, rv.y, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      x[n - 1] = fma(a, p[n - 1], x[n - 1]);
      const double rv = fma(-a, sel(mask[n - 1], t[n - 1]), r[n - 1]);
      r[n - 1] = rv;
      acc = fma(rv, rv, acc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      x[i] = fma(a, p[i], x[i]);
      const double rv = fma(-a, sel(mask[i], t[i]), r[i]);
      r[i] = rv;
      acc = fma(rv, rv, acc);
    }
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// p = select(mask, u, 0) + beta p (p = select(mask, u, 0) on the first
// iteration: p's old contents are never read then); mask == nullptr: u is
// already masked (u = r, unpreconditioned).  p and u are workspace vectors,
// 16-byte aligned.
__global__ __launch_bounds__(kVecThreads) void cgm_direction_kernel(
    double* __restrict__ p, const double* __restrict__ u, const uint8_t* __restrict__ mask,
    int64_t n, const CgmScalars* __restrict__ sc) {
  if (sc->done) return;
  const bool first = sc->first != 0;
  const double beta = sc->beta;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n2 = n / 2;
  double2* p2 = reinterpret_cast<double2*>(p);
  const double2* u2 = reinterpret_cast<const double2*>(u);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    double2 uv = u2[i];
    if (mask != nullptr) {
      uv.x = sel(mask[2 * i], uv.x);
      uv.y = sel(mask[2 * i + 1], uv.y);
    }
    if (!first) {
      const double2 pv = p2[i];
      uv.x = fma(beta, pv.x, uv.x);
      uv.y = fma(beta, pv.y, uv.y);
    }
    p2[i] = uv;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
    double uv = u[n - 1];
    if (mask != nullptr) uv = sel(mask[n - 1], uv);
    p[n - 1] = first ? uv : fma(beta, p[n - 1], uv);
  }
}

// per-point noise: x += alpha p ; r -= alpha select(mask, t + noise p, 0) ;
// partial r.r
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void cgm_xr_update_noise_kernel(
    double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
    const double* __restrict__ t, const double* __restrict__ noise,
    const uint8_t* __restrict__ mask, int64_t n, const CgmScalars* __restrict__ sc,
    double* __restrict__ partials) {
  if (sc->done) return;
  const double a = sc->alpha;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    double2* x2 = reinterpret_cast<double2*>(x);
    double2* r2 = reinterpret_cast<double2*>(r);
    const double2* p2 = reinterpret_cast<const double2*>(p);
    const double2* t2 = reinterpret_cast<const double2*>(t);
    const double2* d2 = reinterpret_cast<const double2*>(noise);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const double2 pv = p2[i], tv = t2[i], dv = d2[i];
      double2 xv = x2[i], rv = r2[i];
      xv.x = fma(a, pv.x, xv.x);
      xv.y = fma(a, pv.y, xv.y);
      rv.x = fma(-a, sel(mask[2 * i], fma(dv.x, pv.x, tv.x)), rv.x);
      rv.y = fma(-a, sel(mask[2 * i + 1], fma(dv.y, pv.y, tv.y)), rv.y);
      x2[i] = xv;
      r2[i] = rv;
      acc = fma(rv.x, rv.x, acc);
      acc = fma(rv.y, rv.y, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const int64_t i = n - 1;
      x[i] = fma(a, p[i], x[i]);
      const double rv = fma(-a, sel(mask[i], fma(noise[i], p[i], t[i])), r[i]);
      r[i] = rv;
      acc = fma(rv, rv, acc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      x[i] = fma(a, p[i], x[i]);
      const double rv = fma(-a, sel(mask[i], fma(noise[i], p[i], t[i])), r[i]);
      r[i] = rv;
      acc = fma(rv, rv, acc);
    }
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// per-point noise: p = select(mask, u, 0) + beta p (p = select(mask, u, 0) on
// the first iteration) and the partials of sum_i noise_i p_i^2, noise selected
// by the mask.  V2: 16-byte lanes on noise (p and u are workspace vectors,
// always 16-byte aligned); every block writes its partial.
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void cgm_direction_noise_kernel(
    double* __restrict__ p, const double* __restrict__ u, const double* __restrict__ noise,
    const uint8_t* __restrict__ mask, int64_t n, const CgmScalars* __restrict__ sc,
    double* __restrict__ partials) {
  if (sc->done) return;
  const bool first = sc->first != 0;
  const double beta = sc->beta;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V2) {
    const int64_t n2 = n / 2;
    double2* p2 = reinterpret_cast<double2*>(p);
    const double2* u2 = reinterpret_cast<const double2*>(u);
    const double2* d2 = reinterpret_cast<const double2*>(noise);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const uint8_t m0 = mask[2 * i], m1 = mask[2 * i + 1];
      const double2 dv = d2[i];
      double2 uv = u2[i];
      uv.x = sel(m0, uv.x);
      uv.y = sel(m1, uv.y);
      if (!first) {
        const double2 pv = p2[i];
        uv.x = fma(beta, pv.x, uv.x);
        uv.y = fma(beta, pv.y, uv.y);
      }
      p2[i] = uv;
      acc = fma(sel(m0, dv.x) * uv.x, uv.x, acc);
      acc = fma(sel(m1, dv.y) * uv.y, uv.y, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
      const int64_t i = n - 1;
      const uint8_t m = mask[i];
      const double uv = first ? sel(m, u[i]) : fma(beta, p[i], sel(m, u[i]));
      p[i] = uv;
      acc = fma(sel(m, noise[i]) * uv, uv, acc);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const uint8_t m = mask[i];
      const double uv = first ? sel(m, u[i]) : fma(beta, p[i], sel(m, u[i]));
      p[i] = uv;
      acc = fma(sel(m, noise[i]) * uv, uv, acc);
    }
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// |W b|^2 -> tolerances, counters; unpreconditioned: rho = r.r
__global__ __launch_bounds__(1024) void cgm_init_kernel(const double* __restrict__ partials,
                                                        int64_t count, CgmScalars* sc,
                                                        double rtol, double atol) {
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) {
    sc->rho = s;
    sc->rho_prev = 0.0;
    sc->rr = s;
    sc->bnorm = sqrt(s);
    sc->tol = fmax(atol, rtol * sc->bnorm);
    sc->iters = 0;
    sc->first = 1;
    sc->alpha = sc->beta = sc->pq = 0.0;
    sc->done = (s == 0.0 || !(sqrt(s) >= sc->tol)) ? 1 : 0;   // also stops on NaN
  }
}

// alpha = rho / (p.t)
__global__ __launch_bounds__(1024) void cgm_alpha_kernel(const double* __restrict__ partials,
                                                         int64_t count, CgmScalars* sc) {
  if (sc->done) return;
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) {
    sc->pq = s;
    sc->alpha = sc->rho / s;
  }
}

// per-point noise: alpha = rho / (p.K p + sum_i noise_i p_i^2), the matvec's
// partials and the direction pass's
__global__ __launch_bounds__(1024) void cgm_alpha_noise_kernel(
    const double* __restrict__ partials, int64_t count, const double* __restrict__ npartials,
    int64_t ncount, CgmScalars* sc) {
  if (sc->done) return;
  const double s = sum_partials(partials, count);
  __syncthreads();   // block_sum's shared scratch is reused
  const double d = sum_partials(npartials, ncount);
  if (threadIdx.x == 0) {
    sc->pq = s + d;
    sc->alpha = sc->rho / sc->pq;
  }
}

// after the update: rr = r.r, the iteration count and the stopping test (the
// rule of cg_rho_kernel and oracle.cg_solve); unpreconditioned (precond == 0)
// also rho = r.r and beta
__global__ __launch_bounds__(1024) void cgm_rr_kernel(const double* __restrict__ partials,
                                                      int64_t count, CgmScalars* sc,
                                                      int precond) {
  if (sc->done) return;
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) {
    sc->rr = s;
    if (!precond) {
      sc->rho_prev = sc->rho;
      sc->rho = s;
      sc->beta = s / sc->rho_prev;
    }
    sc->iters += 1;
    sc->first = 0;
    if (!(sqrt(s) >= sc->tol)) sc->done = 1;   // also stops on NaN
  }
}

// preconditioned: rho = r.z and beta (init: the first rho)
__global__ __launch_bounds__(1024) void cgm_rz_kernel(const double* __restrict__ partials,
                                                      int64_t count, CgmScalars* sc, int init) {
  if (sc->done) return;
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) {
    if (init) {
      sc->rho = s;
    } else {
      sc->rho_prev = sc->rho;
      sc->rho = s;
      sc->beta = s / sc->rho_prev;
    }
  }
}

static int64_t cgm_vec_stride(int64_t n) { return (n + 31) / 32 * 32; }
constexpr int64_t kCgmAlignSlack = 32;   // doubles: room to round the base up to 256 B

}  // namespace gg

struct gg_cgm {
  const gg_kron* K = nullptr;
  double shift = 0.0;
  int64_t n = 0;
  const uint8_t* mask = nullptr;
  double *r = nullptr, *p = nullptr, *t = nullptr, *mv_work = nullptr;
  // preconditioner: z = D Q^T r, u = Q z (one allocation of the handle's, made
  // by gg_cgm_set_precond: an unpreconditioned solve does not pay for them)
  double *zu = nullptr, *z = nullptr, *u = nullptr;
  int64_t mv_work_elems = 0;
  // device: max(kVecBlocks, matvec partials), then kVecBlocks more for the
  // direction pass's noise partials (npartials)
  double* partials = nullptr;
  double* npartials = nullptr;
  const double* noise = nullptr;       // per-point noise (gg_cgm_set_noise), or NULL
  gg::CgmScalars* sc = nullptr;        // device
  gg::CgmScalars* sc_host = nullptr;   // pinned mirror
  double* x = nullptr;
  // Kronecker preconditioner (gg_cgm_set_precond): the eigenvector operator,
  // the concatenated per-factor eigenvalues and the factor orders
  const gg_kron* Q = nullptr;
  const double* lam = nullptr;
  std::vector<int64_t> qm;
};

namespace gg {

// u = Q diag(1 / (lam + shift)) Q^T r, and the partials of r.u
static void cgm_precond(gg_cgm* c, hipStream_t s, int nb) {
  kron_apply(c->Q, true, c->r, c->u, 0.0, c->mv_work, nullptr, nullptr, s, nullptr, nullptr, 0,
             nullptr);
  check_status(gg_kron_diag_scale((int)c->qm.size(), c->qm.data(), c->lam, c->shift,
                               GG_DIAG_DIVIDE, c->u, c->z, s));
  kron_apply(c->Q, false, c->z, c->u, 0.0, c->mv_work, nullptr, nullptr, s, nullptr, nullptr, 0,
             nullptr);
  launch_dot_partials(c->r, c->u, c->n, c->partials, nb, s);
}

}  // namespace gg

extern "C" {

int gg_cgm_work_elems(const gg_kron* K, int64_t* elems) {
  return gg::guard([&] {
    GG_REQUIRE(K && elems, GG_ERR_VALUE, "NULL argument");
    const int64_t vs = gg::cgm_vec_stride(gg::kron_n(K));
    // r, p, t and the matvec scratch (shared with the preconditioner)
    *elems = gg::kCgmAlignSlack + 3 * vs + gg::kron_work_elems(K, false);
  });
}

int gg_cgm_destroy(gg_cgm* c) {
  return gg::guard([&] {
    if (!c) return;
    if (c->partials) (void)hipFree(c->partials);
    if (c->zu) (void)hipFree(c->zu);
    if (c->sc) (void)hipFree(c->sc);
    if (c->sc_host) (void)hipHostFree(c->sc_host);
    delete c;
  });
}

int gg_cgm_create(const gg_kron* K, double shift, const uint8_t* mask_dev, double* work_dev,
                  gg_cgm** out) {
  return gg::guard([&] {
    GG_REQUIRE(K && work_dev && out, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(mask_dev != nullptr, GG_ERR_VALUE, "the masked CG needs a mask");
    GG_REQUIRE(shift > 0.0, GG_ERR_VALUE,
               "the masked CG needs shift > 0 (W K W alone is singular)");
    int64_t nr = 0, nc = 0, we = 0;
    gg::check_status(gg_kron_shape(K, 0, &nr, &nc, &we));
    GG_REQUIRE(nr == nc, GG_ERR_VALUE, "CG needs a square operator");
    GG_REQUIRE((reinterpret_cast<uintptr_t>(work_dev) & 7) == 0, GG_ERR_VALUE,
               "the CG workspace must hold doubles (8-byte aligned)");
    gg_cgm* c = new gg_cgm();
    try {
      c->K = K;
      c->shift = shift;
      c->n = nr;
      c->mask = mask_dev;
      const int64_t vs = gg::cgm_vec_stride(nr);
      work_dev = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work_dev) + 255) &
                                           ~static_cast<uintptr_t>(255));
      c->r = work_dev;
      c->p = work_dev + vs;
      c->t = work_dev + 2 * vs;
      c->mv_work = work_dev + 3 * vs;
      c->mv_work_elems = gg::kron_work_elems(K, false);
      const int64_t np =
          std::max<int64_t>(gg::kVecBlocks, gg::kron_partials_needed(K, false));
      GG_HIP(hipMalloc(&c->partials, (np + gg::kVecBlocks) * sizeof(double)));
      c->npartials = c->partials + np;
      GG_HIP(hipMalloc(&c->sc, sizeof(gg::CgmScalars)));
      GG_HIP(hipMemset(c->sc, 0, sizeof(gg::CgmScalars)));
      GG_HIP(hipHostMalloc(&c->sc_host, sizeof(gg::CgmScalars), hipHostMallocDefault));
    } catch (...) {
      gg_cgm_destroy(c);
      throw;
    }
    *out = c;
  });
}

int gg_cgm_set_precond(gg_cgm* c, const gg_kron* Q, const double* lam_dev) {
  return gg::guard([&] {
    GG_REQUIRE(c, GG_ERR_VALUE, "NULL handle");
    GG_REQUIRE(c->x == nullptr, GG_ERR_VALUE, "set the preconditioner before gg_cgm_start");
    if (Q == nullptr) {
      c->Q = nullptr;
      c->lam = nullptr;
      return;
    }
    GG_REQUIRE(lam_dev != nullptr, GG_ERR_VALUE, "the preconditioner needs the eigenvalues");
    const int d = gg::kron_d(Q);
    GG_REQUIRE(d == gg::kron_d(c->K) && d <= 16, GG_ERR_VALUE,
               "the eigenvector operator must have the operator's factors");
    std::vector<int64_t> qr(d), qc(d), kr(d), kc(d);
    gg::kron_factor_shape(Q, qr.data(), qc.data());
    gg::kron_factor_shape(c->K, kr.data(), kc.data());
    for (int k = 0; k < d; ++k)
      GG_REQUIRE(qr[k] == qc[k] && qr[k] == kr[k] && kr[k] == kc[k], GG_ERR_VALUE,
                 "the eigenvector operator must have the operator's (square) factor orders");
    GG_REQUIRE(std::max(gg::kron_work_elems(Q, false), gg::kron_work_elems(Q, true)) <=
                   c->mv_work_elems,
               GG_ERR_VALUE, "the eigenvector operator needs more matvec scratch");
    const int64_t vs = gg::cgm_vec_stride(c->n);
    if (c->zu == nullptr) GG_HIP(hipMalloc(&c->zu, 2 * vs * sizeof(double)));
    c->z = c->zu;
    c->u = c->zu + vs;
    c->Q = Q;
    c->lam = lam_dev;
    c->qm = qr;
  });
}

int gg_cgm_set_noise(gg_cgm* c, const double* noise_dev) {
  return gg::guard([&] {
    GG_REQUIRE(c, GG_ERR_VALUE, "NULL handle");
    GG_REQUIRE(c->x == nullptr, GG_ERR_VALUE, "set the noise before gg_cgm_start");
    GG_REQUIRE((reinterpret_cast<uintptr_t>(noise_dev) & 7) == 0, GG_ERR_VALUE,
               "the noise must hold doubles (8-byte aligned)");
    c->noise = noise_dev;
  });
}

int gg_cgm_start(gg_cgm* c, const double* b_dev, double* x_dev, double rtol, double atol,
                 gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && b_dev && x_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(rtol >= 0 && atol >= 0, GG_ERR_VALUE,
               "tolerances must be real, non-negative numbers");
    hipStream_t s = gg::as_stream(stream);
    c->x = x_dev;
    const int64_t n = c->n;
    const int nb = gg::vec_blocks(n);
    if (gg::aligned16(b_dev) && gg::aligned16(x_dev))
      hipLaunchKernelGGL(gg::cgm_start_kernel<true>, dim3(nb), dim3(gg::kVecThreads), 0, s,
                         b_dev, c->mask, x_dev, c->r, n, c->partials);
    else
      hipLaunchKernelGGL(gg::cgm_start_kernel<false>, dim3(nb), dim3(gg::kVecThreads), 0, s,
                         b_dev, c->mask, x_dev, c->r, n, c->partials);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gg::cgm_init_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                       (int64_t)nb, c->sc, rtol, atol);
    GG_LAUNCH_CHECK();
    if (c->Q != nullptr) {
      gg::cgm_precond(c, s, nb);
      hipLaunchKernelGGL(gg::cgm_rz_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                         (int64_t)nb, c->sc, 1);
      GG_LAUNCH_CHECK();
    }
  });
}

int gg_cgm_iterate(gg_cgm* c, int max_iters, int check_every, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && c->x, GG_ERR_VALUE, "CG not started");
    hipStream_t s = gg::as_stream(stream);
    const int64_t n = c->n;
    const int nb = gg::vec_blocks(n);
    const bool pre = c->Q != nullptr;
    const bool x16 = gg::aligned16(c->x);
    if (check_every <= 0) check_every = max_iters;
    const double* dn = c->noise;
    const bool d16 = gg::aligned16(dn);
    for (int it = 0; it < max_iters; ++it) {
      if (dn == nullptr)
        hipLaunchKernelGGL(gg::cgm_direction_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                           c->p, pre ? c->u : c->r, pre ? c->mask : (const uint8_t*)nullptr, n,
                           c->sc);
      else if (d16)
        hipLaunchKernelGGL(gg::cgm_direction_noise_kernel<true>, dim3(nb),
                           dim3(gg::kVecThreads), 0, s, c->p, pre ? c->u : c->r, dn, c->mask, n,
                           c->sc, c->npartials);
      else
        hipLaunchKernelGGL(gg::cgm_direction_noise_kernel<false>, dim3(nb),
                           dim3(gg::kVecThreads), 0, s, c->p, pre ? c->u : c->r, dn, c->mask, n,
                           c->sc, c->npartials);
      GG_LAUNCH_CHECK();
      int64_t nparts = 0;
      gg::kron_apply(c->K, false, c->p, c->t, dn ? 0.0 : c->shift, c->mv_work, c->partials,
                     &c->sc->done, s, &nparts, nullptr, 0, nullptr);
      if (dn == nullptr)
        hipLaunchKernelGGL(gg::cgm_alpha_kernel, dim3(1), dim3(1024), 0, s, c->partials, nparts,
                           c->sc);
      else
        hipLaunchKernelGGL(gg::cgm_alpha_noise_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                           nparts, c->npartials, (int64_t)nb, c->sc);
      GG_LAUNCH_CHECK();
      if (dn != nullptr) {
        if (x16 && d16)
          hipLaunchKernelGGL(gg::cgm_xr_update_noise_kernel<true>, dim3(nb),
                             dim3(gg::kVecThreads), 0, s, c->x, c->r, c->p, c->t, dn, c->mask, n,
                             c->sc, c->partials);
        else
          hipLaunchKernelGGL(gg::cgm_xr_update_noise_kernel<false>, dim3(nb),
                             dim3(gg::kVecThreads), 0, s, c->x, c->r, c->p, c->t, dn, c->mask, n,
                             c->sc, c->partials);
      } else if (x16)
        hipLaunchKernelGGL(gg::cgm_xr_update_kernel<true>, dim3(nb), dim3(gg::kVecThreads), 0,
                           s, c->x, c->r, c->p, c->t, c->mask, n, c->sc, c->partials);
      else
        hipLaunchKernelGGL(gg::cgm_xr_update_kernel<false>, dim3(nb), dim3(gg::kVecThreads), 0,
                           s, c->x, c->r, c->p, c->t, c->mask, n, c->sc, c->partials);
      GG_LAUNCH_CHECK();
      hipLaunchKernelGGL(gg::cgm_rr_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                         (int64_t)nb, c->sc, pre ? 1 : 0);
      GG_LAUNCH_CHECK();
      if (pre) {
        gg::cgm_precond(c, s, nb);
        hipLaunchKernelGGL(gg::cgm_rz_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                           (int64_t)nb, c->sc, 0);
        GG_LAUNCH_CHECK();
      }
      if ((it + 1) % check_every == 0 && it + 1 < max_iters) {
        GG_HIP(hipMemcpyAsync(c->sc_host, c->sc, sizeof(gg::CgmScalars), hipMemcpyDeviceToHost,
                              s));
        GG_HIP(hipStreamSynchronize(s));
        if (c->sc_host->done) break;
      }
    }
  });
}

int gg_cgm_status(gg_cgm* c, int* iters, int* converged, double* resid_norm, double* tol,
                  gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c, GG_ERR_VALUE, "NULL handle");
    hipStream_t s = gg::as_stream(stream);
    GG_HIP(hipMemcpyAsync(c->sc_host, c->sc, sizeof(gg::CgmScalars), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    const gg::CgmScalars& h = *c->sc_host;
    if (iters) *iters = h.iters;
    // a created, unstarted handle holds zeroed scalars (bnorm == 0): not converged
    if (converged)
      *converged = c->x != nullptr && ((h.done && std::sqrt(h.rr) < h.tol) || h.bnorm == 0.0);
    if (resid_norm) *resid_norm = std::sqrt(h.rr);
    if (tol) *tol = h.tol;
  });
}

}  // extern "C"
