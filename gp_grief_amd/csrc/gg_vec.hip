// Vector side of the Krylov solvers on MI355X: HBM-bound, coalesced,
// wave-reduced (shfl over 64 lanes -> LDS across waves -> per-block partial ->
// one deterministic single-block reduction).  No float atomics anywhere, so
// every dot product is bitwise reproducible run to run.
//
// Here: dot / reduce / axpby and the single-GPU CG (Lanczos: gg_lanczos.hip;
// diagonal kernels: gg_diag.hip; the sharded CG's scalars: gg_cgs.hip).
//
// The reference has no CG or Lanczos; the CG recurrence is the
// one of scipy.sparse.linalg.cg (oracle/cg.py restates it), driven here with
// every scalar resident on the device so the host only polls convergence.
#include <cmath>
#include <map>
#include <vector>

#include "gg_internal.h"

namespace gg {

__global__ __launch_bounds__(kVecThreads) void dot_partials_kernel(const double* __restrict__ x,
                                                                   const double* __restrict__ y,
                                                                   int64_t n,
                                                                   double* __restrict__ partials) {
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n2 = n / 2;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 a = x2[i], b = y2[i];
    acc = fma(a.x, b.x, acc);
    acc = fma(a.y, b.y, acc);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) acc = fma(x[n - 1], y[n - 1], acc);
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The same partial sums one double at a time: gg_dot on a vector that does not
// start on a 16-byte boundary (a view one double into an allocation).
__global__ __launch_bounds__(kVecThreads) void dot_partials_unaligned_kernel(
    const double* __restrict__ x, const double* __restrict__ y, int64_t n,
    double* __restrict__ partials) {
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    acc = fma(x[i], y[i], acc);
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(1024) void reduce_kernel(const double* __restrict__ partials,
                                                      int64_t count, double* __restrict__ out) {
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) *out = s;
}

void launch_dot_partials(const double* x, const double* y, int64_t n, double* partials,
                         int nblocks, hipStream_t s) {
  GG_REQUIRE(aligned16(x) && aligned16(y), GG_ERR_VALUE, "vectors must be 16-byte aligned");
  hipLaunchKernelGGL(dot_partials_kernel, dim3(nblocks), dim3(kVecThreads), 0, s, x, y, n,
                     partials);
  GG_LAUNCH_CHECK();
}

void launch_reduce_to(const double* partials, int64_t count, double* out, hipStream_t s) {
  hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, s, partials, count, out);
  GG_LAUNCH_CHECK();
}

// x may be y itself (the models scale a vector in place: axpby(0, v, s, v)),
// so neither pointer is __restrict__
__global__ __launch_bounds__(kVecThreads) void axpby_kernel(double a, const double* x, double b,
                                                            double* y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    y[i] = a * x[i] + b * y[i];
}

// ------------------------------------------------------------------ CG kernels
// (p = beta p + r is fused into the first mode product, gg_kron.hip)

// alpha = rho / (p.q)
__global__ __launch_bounds__(1024) void cg_alpha_kernel(const double* __restrict__ partials,
                                                        int64_t count, CgScalars* sc) {
  if (sc->done) return;
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) {
    sc->pq = s;
    sc->alpha = sc->rho / s;
  }
}

// x += alpha p ; r -= alpha q ; partial r.r
__global__ __launch_bounds__(kVecThreads) void cg_xr_update_kernel(
    double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
    const double* __restrict__ q, int64_t n, const CgScalars* __restrict__ sc,
    double* __restrict__ partials, int need_pending) {
  // need_pending: 0 always, 1 only with a pending fused update, 2 only when
  // the fused recurrence asked for a repair (cancelled beta); x == nullptr:
  // r only (x_defer keeps its own x bookkeeping, cg_x_flush_kernel)
  if (sc->done || (need_pending && !sc->pending)) return;
  if (need_pending == 2 && !sc->repair) return;
  if (x == nullptr) {
    const double a = sc->alpha;
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const double rv = r[i] - a * q[i];
      r[i] = rv;
      acc = fma(rv, rv, acc);
    }
    const double s = block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
    return;
  }
  const double a = sc->alpha;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n2 = n / 2;
  double2* x2 = reinterpret_cast<double2*>(x);
  double2* r2 = reinterpret_cast<double2*>(r);
  const double2* p2 = reinterpret_cast<const double2*>(p);
  const double2* q2 = reinterpret_cast<const double2*>(q);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 pv = p2[i], qv = q2[i];
    double2 xv = x2[i], rv = r2[i];
    xv.x += a * pv.x;
    xv.y += a * pv.y;
    rv.x -= a * qv.x;
    rv.y -= a * qv.y;
    x2[i] = xv;
    r2[i] = rv;
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
    x[n - 1] += a * p[n - 1];
    r[n - 1] -= a * q[n - 1];
    acc = fma(r[n - 1], r[n - 1], acc);
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// rho_prev = rho ; rho = r.r ; beta ; iteration count ; convergence
__global__ __launch_bounds__(1024) void cg_rho_kernel(const double* __restrict__ partials,
                                                      int64_t count, CgScalars* sc,
                                                      int need_pending) {
  if (sc->done || (need_pending && !sc->pending)) return;
  if (need_pending == 2 && !sc->repair) return;
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) {
    sc->rho_prev = sc->rho;
    sc->rho = s;
    sc->beta = s / sc->rho_prev;
    sc->iters += 1;
    sc->first = 0;
    sc->pending = 0;
    sc->repair = 0;
    sc->rstored = 1;   // r is in its buffer (the update just wrote it)
    if (!(sqrt(s) >= sc->tol)) sc->done = 1;  // also stops on NaN
  }
}

// derived r (CgScalars::rstored): write the current r into its buffer --
// r = (rstored ? r : p - beta_p p_prev) (- alpha q when pending) -- with its
// r.r partials.  mode 2: only when the recurrence asked for a repair (before
// the prologue); mode 1: the close (whenever r is not stored or an update is
// pending).  cg_rho_kernel / cg_r_stored_kernel then mark it stored.
// The directions are the ones the scalars recorded (sc->rp_cur, rp_prev).
__global__ __launch_bounds__(kVecThreads) void cg_r_materialize_kernel(
    double* __restrict__ r, const double* __restrict__ q, int64_t n,
    const CgScalars* __restrict__ sc, double* __restrict__ partials, int mode) {
  if (sc->done && sc->rstored) return;
  if (mode == 2 && (sc->done || !sc->repair || !sc->pending)) return;
  if (mode == 1 && sc->rstored && !sc->pending) return;
  const bool st = sc->rstored != 0;
  const double bp = sc->beta_p;
  const double* __restrict__ p = sc->rp_cur;
  const double* __restrict__ pprev = sc->rp_prev;
  const double a = sc->pending ? sc->alpha : 0.0;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double rv = st ? r[i] : fma(-bp, pprev[i], p[i]);
    if (a != 0.0) rv -= a * q[i];
    r[i] = rv;
    acc = fma(rv, rv, acc);
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void cg_r_stored_kernel(CgScalars* sc) { sc->rstored = 1; }

// x_defer: fold the deferred steps into x, x += sum_{i < xpend} xc[i] xp[i]
// (also after convergence: x lags r by up to two steps)
__global__ __launch_bounds__(kVecThreads) void cg_x_flush_kernel(double* __restrict__ x,
                                                                 int64_t n,
                                                                 const CgScalars* __restrict__ sc) {
  const int k = sc->xpend;
  if (k <= 0) return;
  const double c0 = sc->xc[0], c1 = k >= 2 ? sc->xc[1] : 0.0;
  const double* __restrict__ p0 = sc->xp[0];
  const double* __restrict__ p1 = k >= 2 ? sc->xp[1] : sc->xp[0];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    x[i] += c0 * p0[i] + c1 * p1[i];
}

// x_defer mode 2 on its own stream: half sc->xh of the active pair, x += c0
// p0 + c1 p1 over [0, H) or [H, n) -- no state change (the scalars kernel
// advances xh).  One 256-thread workgroup per CU, few registers, no LDS: it
// fits beside a ring mode product's workgroup (2 waves / SIMD at 226 VGPRs,
// 131 KB of LDS) and streams while that one computes.  Non-temporal: every
// element is touched once per iteration.
__global__ __launch_bounds__(256) void cg_x_half_kernel(double* __restrict__ x, int64_t n,
                                                        int64_t H,
                                                        const CgScalars* __restrict__ sc) {
  if (sc->done) return;
  const int h = sc->xh;
  if (h >= 2) return;
  const int64_t lo = h ? H : 0, hi = h ? n : H;
  const double c0 = sc->xc[0], c1 = sc->xc[1];
  const double* __restrict__ p0 = sc->xp[0];
  const double* __restrict__ p1 = sc->xp[1];
  typedef double v2 __attribute__((ext_vector_type(2)));
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
  int64_t i = lo + 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  constexpr int kU = 2;
  for (; i + (kU - 1) * stride + 1 < hi; i += kU * stride) {
    v2 xv[kU], a[kU], b[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      xv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2*>(x + i + u * stride));
      a[u] = __builtin_nontemporal_load(reinterpret_cast<const v2*>(p0 + i + u * stride));
      b[u] = __builtin_nontemporal_load(reinterpret_cast<const v2*>(p1 + i + u * stride));
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      xv[u] += c0 * a[u] + c1 * b[u];
      __builtin_nontemporal_store(xv[u], reinterpret_cast<v2*>(x + i + u * stride));
    }
  }
  for (; i < hi; i += stride) {
    x[i] += c0 * p0[i] + c1 * p1[i];
    if (i + 1 < hi) x[i + 1] += c0 * p0[i + 1] + c1 * p1[i + 1];
  }
}

void launch_x_half(double* x, int64_t n, int64_t H, const CgScalars* sc, hipStream_t s) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    GG_HIP(hipGetDevice(&dev));
    GG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  hipLaunchKernelGGL(cg_x_half_kernel, dim3((unsigned)std::max(cus, 1)), dim3(256), 0, s, x, n,
                     H, sc);
  GG_LAUNCH_CHECK();
}

// x_defer mode 2: x += xsc xsp (the waiting single step) + the active pair
// on the halves not yet applied (half 0 = [0, H), half 1 = [H, n))
__global__ __launch_bounds__(kVecThreads) void cg_x_flush2_kernel(double* __restrict__ x,
                                                                  int64_t n, int64_t H,
                                                                  const CgScalars* __restrict__ sc) {
  const int h = sc->xh, xs = sc->xs;
  if (h >= 2 && !xs) return;
  const double cs = xs ? sc->xsc : 0.0;
  const double* __restrict__ ps = xs ? sc->xsp : x;
  const double c0 = h < 2 ? sc->xc[0] : 0.0, c1 = h < 2 ? sc->xc[1] : 0.0;
  const double* __restrict__ p0 = h < 2 ? sc->xp[0] : x;
  const double* __restrict__ p1 = h < 2 ? sc->xp[1] : x;
  const int64_t from = h == 0 ? 0 : H;   // first element the pair still owes
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double v = x[i];
    if (xs) v += cs * ps[i];
    if (h < 2 && i >= from) v += c0 * p0[i] + c1 * p1[i];
    x[i] = v;
  }
}

// The CG prologue's stream pattern alone (gg_cg_calibrate): per element,
// read p_old, r and q, write r, p_new and q -- the six passes of the fused
// prologue launch over the same buffers, with its non-temporal mask (every
// stream but the q write, the launch's output Y); with derived r (RD) the
// five of that prologue: read p_old, p_{j-2} (in r's place) and q, write
// p_new and q.  Values pass through unchanged (r = r, p_new = p_old, q = q;
// the loaded values pass an opaque asm so the compiler cannot drop a store of
// what was just loaded from the same address).  No MFMA work: the launch's
// streams alone on this box.
template <bool RD>
__global__ __launch_bounds__(256) void cg_stream_probe_kernel(double* __restrict__ r,
                                                              const double* __restrict__ p,
                                                              double* __restrict__ p2,
                                                              double* __restrict__ q,
                                                              int64_t n) {
  typedef double v2 __attribute__((ext_vector_type(2)));
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
  constexpr int kU = 2;
  int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  for (; i + (kU - 1) * stride + 1 < n; i += kU * stride) {
    v2 a[kU], b[kU], c[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      a[u] = __builtin_nontemporal_load(reinterpret_cast<const v2*>(p + i + u * stride));
      b[u] = __builtin_nontemporal_load(reinterpret_cast<const v2*>(r + i + u * stride));
      c[u] = __builtin_nontemporal_load(reinterpret_cast<const v2*>(q + i + u * stride));
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) asm volatile("" : "+v"(a[u]), "+v"(b[u]), "+v"(c[u]));
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (RD) {
        // keep the p_{j-2} stream's loads live without changing p_new
        asm volatile("" : : "v"(b[u]));
      } else {
        __builtin_nontemporal_store(b[u], reinterpret_cast<v2*>(r + i + u * stride));
      }
      __builtin_nontemporal_store(a[u], reinterpret_cast<v2*>(p2 + i + u * stride));
      *reinterpret_cast<v2*>(q + i + u * stride) = c[u];
    }
  }
  for (; i < n; i += stride) {
    p2[i] = p[i];
    if (i + 1 < n) p2[i + 1] = p[i + 1];
  }
}

__global__ void cg_x_flushed_kernel(CgScalars* sc) {
  sc->xpend = 0;
  sc->xh = 2;
  sc->xs = 0;
}

// x_defer mode 3: every region gets the steps it has not seen, [wa[r], wn)
// (at most wk of them, all still in the ring) -- the side job's expression
__global__ __launch_bounds__(kVecThreads) void cg_x_flush3_kernel(double* __restrict__ x,
                                                                  int64_t n, int64_t R,
                                                                  const CgScalars* __restrict__ sc) {
  const int K = sc->wk, slots = K + 1, wn = sc->wn;
  if (K <= 0) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int r = (int)(i / R);
    double s = 0.0;
    for (int t = sc->wa[r]; t < wn; ++t) s += sc->wc[t % slots] * sc->wp[t % slots][i];
    x[i] = x[i] + s;
  }
}

__global__ void cg_x_flushed3_kernel(CgScalars* sc) {
  for (int r = 0; r < kXWinMax; ++r) sc->wa[r] = sc->wn;
  sc->warm = 0;
}

// x_defer mode 3 at gg_cg_start: window K, nothing applied or armed
__global__ void cg_xwin_init_kernel(CgScalars* sc, int K) {
  sc->wk = K;
  sc->wn = 0;
  sc->wnext = 0;
  sc->warm = 0;
  sc->sreg = 0;
  sc->scnt = 0;
  for (int r = 0; r < kXWinMax; ++r) sc->wa[r] = 0;
}

// Fused recurrence, end of iteration j (after the last mode product):
//   rho_j = r_j.r_j (partials of the first mode product's prologue, which
//   applied r_j = r_{j-1} - alpha q_{j-1}), stopping test on it;
//   alpha_j = rho_j / (p_j.q_j);
//   beta_j = |r_{j+1}|^2 / rho_j with |r_{j+1}|^2 = rho_j - 2 alpha (r.q) +
//   alpha^2 (q.q), the exact expansion of |r_j - alpha_j q_j|^2.  The true
//   r_{j+1}.r_{j+1} replaces it in the next iteration (stopping test, alpha).
// The x / r updates of iteration j stay pending until the next iteration's
// first two mode products (or gg_cg_iterate's closing update).
//
// x_defer (p_new != nullptr): x is not updated every iteration.  With xpend
// deferred steps at the start of iteration j (the side job folded both into
// x if xpend was 2):  xpend 2 or 0 -> 1 pending, (p_j, alpha_j);  xpend 1 ->
// 2 pending, (p_j, alpha_j) and (p_{j-1}, alpha_{j-1}).  p_new = p_j (this
// iteration's direction buffer); the host keeps three direction buffers so
// p_{j-1} survives the next prologue.
//
// x_defer mode 2 (xmode 2, balanced): the pair of steps (2i, 2i + 1) becomes
// active at the end of iteration 2i + 1 and the side jobs of the next two
// iterations apply it half of x each (sc->xh: 0, 1, then 2 = done), so every
// side launch carries one pass instead of two in every other iteration; four
// direction buffers keep the pair alive.
__global__ __launch_bounds__(1024) void cg_fused_scalars_kernel(
    const double* __restrict__ rr_part, int64_t nrr, int64_t rr_stride,
    const double* __restrict__ mv_part, int64_t nmv, int64_t pstride, CgScalars* sc,
    const double* p_new, int xmode, int rq_ident, int rder) {
  if (sc->done) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t i = threadIdx.x; i < nmv; i += blockDim.x) {
    a0 += mv_part[i];
    if (!rq_ident) a1 += mv_part[pstride + i];
    a2 += mv_part[2 * pstride + i];
  }
  // conjugacy r.q: p_j = r_j + beta_j p_{j-1}, so r_j.q_j = p_j.q_j -
  // beta_j p_{j-1}.A p_j = p_j.q_j - beta_j p_j.q_{j-1} (A symmetric); the
  // prologue summed p_j.q_{j-1} (zero on the first step, where beta = 0)
  if (rq_ident)
    for (int64_t i = threadIdx.x; i < nrr; i += blockDim.x) a1 += rr_part[rr_stride + i];
  const bool pend = sc->pending != 0;
  if (pend)
    for (int64_t i = threadIdx.x; i < nrr; i += blockDim.x) a3 += rr_part[i];
  const double pq = block_sum(a0);
  __syncthreads();
  const double rq_raw = block_sum(a1);   // r.q, or p_j.q_{j-1} (rq_ident)
  __syncthreads();
  const double qq = block_sum(a2);
  __syncthreads();
  const double rr = block_sum(a3);
  if (threadIdx.x == 0) {
    // mode 3: this iteration's pair launch applied the armed side job (it ran:
    // done was 0 then, as it is now)
    if (xmode == 3 && sc->warm) {
      sc->wa[sc->sreg] = sc->wn;
      sc->warm = 0;
    }
    // derived r: this iteration's prologue formed p_j with sc->beta; when an
    // update was pending it computed r_j without storing it
    if (rder) {
      sc->beta_p = sc->beta;
      if (pend) sc->rstored = 0;
      sc->rp_prev = sc->rp_cur;
      sc->rp_cur = p_new;
    }
    if (pend) {
      sc->rho_prev = sc->rho;
      sc->rho = rr;
      sc->iters += 1;
      if (!(sqrt(rr) >= sc->tol)) {  // converged (or NaN): x_j, r_j are final
        sc->done = 1;
        sc->pending = 0;
        // x_defer: xpend 2 was folded into x by this iteration's side job;
        // xpend 1 (alpha_{j-1} p_{j-1}) stays for the closing flush.  Mode 2:
        // this iteration's side job took half xh; the flush does the rest
        if (p_new != nullptr && xmode != 2 && sc->xpend == 2) sc->xpend = 0;
        if (p_new != nullptr && xmode == 2 && sc->xh < 2) sc->xh += 1;
        return;
      }
    }
    const double rho = sc->rho;
    const double alpha = rho / pq;
    const double rq = rq_ident ? pq - sc->beta * rq_raw : rq_raw;   // beta_j: not yet replaced
    double rt = rho - 2.0 * alpha * rq + alpha * alpha * qq;
    sc->pq = pq;
    sc->rq = rq;
    sc->qq = qq;
    sc->alpha = alpha;
    // |r_{j+1}|^2 from three terms of size ~rho: when it is below 1e-6 rho
    // the expansion has lost too many digits for beta -- apply the update
    // and take the true r.r instead (repair kernels before the next matvec)
    sc->repair = rt < (sc->cancel_tol > 0.0 ? sc->cancel_tol : 1e-6) * rho ? 1 : 0;
    sc->cancels += sc->repair;
    sc->beta = sc->repair ? 0.0 : rt / rho;
    sc->first = 0;
    sc->pending = 1;
    if (p_new != nullptr && xmode == 3) {
      // step wn = (alpha_j, p_j) into the ring, then arm the next region with
      // every step it has not seen (wk at most: it was armed wk arms ago)
      const int K = sc->wk, slots = K + 1;
      const int j = sc->wn;
      sc->wc[j % slots] = alpha;
      sc->wp[j % slots] = p_new;
      sc->wn = j + 1;
      const int reg = sc->wnext;
      sc->wnext = reg + 1 == K ? 0 : reg + 1;
      const int a = sc->wa[reg];
      const int cnt = sc->wn - a;
      sc->sreg = reg;
      sc->scnt = cnt;
      for (int t = 0; t < kXWinMax; ++t) {
        const int i = a + (t < cnt ? t : 0);
        sc->scoef[t] = t < cnt ? sc->wc[i % slots] : 0.0;
        sc->sdir[t] = sc->wp[i % slots];
      }
      sc->warm = cnt > 0 ? 1 : 0;
    } else if (p_new != nullptr && xmode == 2) {
      if (sc->xh < 2) sc->xh += 1;   // this iteration's side job took a half
      if (!sc->xs) {
        sc->xs = 1;
        sc->xsc = alpha;
        sc->xsp = p_new;
      } else {   // the pair is complete (the previous one finished just now)
        sc->xc[0] = sc->xsc;
        sc->xp[0] = sc->xsp;
        sc->xc[1] = alpha;
        sc->xp[1] = p_new;
        sc->xh = 0;
        sc->xs = 0;
      }
    } else if (p_new != nullptr) {
      if (sc->xpend == 1) {
        sc->xc[1] = sc->xc[0];
        sc->xp[1] = sc->xp[0];
        sc->xpend = 2;
      } else {
        sc->xpend = 1;
      }
      sc->xc[0] = alpha;
      sc->xp[0] = p_new;
    }
  }
}

// a sharded CG rank's local sums of one fused iteration, red = [r.r (of the
// prologue's r update), p.q_old, p.q, r.q, q.q] (gg_cg_iterate_partial); the
// caller all-reduces red and cg_fused_scalars_kernel takes it as one-element
// partial arrays
__global__ __launch_bounds__(1024) void cg_local_red_kernel(
    const double* __restrict__ rr_part, int64_t nrr, int64_t rr_stride,
    const double* __restrict__ mv_part, int64_t nmv, int64_t pstride, int rq_ident,
    double* __restrict__ red) {
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < nrr; i += blockDim.x) {
    a[0] += rr_part[i];
    if (rq_ident) a[1] += rr_part[rr_stride + i];
  }
  for (int64_t i = threadIdx.x; i < nmv; i += blockDim.x) {
    a[2] += mv_part[i];
    if (!rq_ident) a[3] += mv_part[pstride + i];
    a[4] += mv_part[2 * pstride + i];
  }
  double t[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    t[k] = block_sum(a[k]);
    __syncthreads();
  }
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k] = t[k];
}

// the closing step of a sharded rank: rho from the all-reduced r.r
__global__ void cg_close_rho_kernel(CgScalars* sc, const double* rr) {
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

__global__ void cg_init_kernel(const double* __restrict__ partials, int64_t count,
                               CgScalars* sc, double rtol, double atol) {
  const double s = sum_partials(partials, count);
  if (threadIdx.x == 0) {
    sc->rho = s;
    sc->rho_prev = 0.0;
    sc->bnorm = sqrt(s);
    sc->tol = fmax(atol, rtol * sc->bnorm);
    sc->iters = 0;
    sc->first = 1;
    sc->pending = 0;
    sc->alpha = sc->beta = sc->pq = sc->rq = sc->qq = 0.0;
    sc->repair = 0;
    sc->cancels = 0;
    sc->xpend = 0;
    sc->xh = 2;
    sc->xs = 0;
    sc->wn = 0;
    sc->wnext = 0;
    sc->warm = 0;
    for (int r = 0; r < kXWinMax; ++r) sc->wa[r] = 0;
    sc->beta_p = 0.0;
    sc->rstored = 1;   // r = b (or P b) is in its buffer
    sc->rp_cur = sc->rp_prev = nullptr;
    sc->done = (s == 0.0 || !(sqrt(s) >= sc->tol)) ? 1 : 0;
  }
}

// ------------------------------------------------------------------- CG state
// a handle's scalar block: zeroed, with the cancellation threshold of the
// knob snapshot (GG_CG_CANCEL_TOL, tests: forces the repair / restart paths)
void scalars_clear(CgScalars* sc) {
  GG_HIP(hipMemset(sc, 0, sizeof(CgScalars)));
  const char* e = knob("GG_CG_CANCEL_TOL");
  if (e) {
    const double t = atof(e);
    GG_HIP(hipMemcpy(&sc->cancel_tol, &t, sizeof(double), hipMemcpyHostToDevice));
  }
}
}  // namespace gg

struct gg_cg {
  const gg_kron* K = nullptr;
  double shift = 0.0;
  int64_t n = 0;
  double *r = nullptr, *p = nullptr, *q = nullptr, *mv_work = nullptr;
  double* p2 = nullptr;        // second direction buffer (fused recurrence)
  double* p3 = nullptr;        // third (x_defer: p_{j-1} outlives the next prologue)
  double* p4 = nullptr;        // fourth (x_defer mode 2: p_{j-2} too)
  double* first_dst = nullptr; // odd d: the first mode product's output (not q)
  bool fused = true;           // recurrence: fused (default) or textbook
  int fusion = 0;              // fused layout (gg_cg_set_fusion): 0, 1 or 2
  int xdefer = 2;              // layouts 0 / 1: x updated in deferred pairs (1: every
                               // other iteration; 2: balanced, half a pair per iteration)
  double* partials = nullptr;  // device, max(kVecBlocks, 3 x matvec partials)
  double* rr_part = nullptr;   // device, prologue r.r (+ p_new.q_old) partials (fused)
  int64_t rr_count = 0;
  int rq = 1;                  // layout 0: r.q from the conjugacy identity (gg_cg_set_rq)
  gg::CgScalars* sc = nullptr; // device
  gg::CgScalars* sc_host = nullptr;  // pinned mirror
  const double* b = nullptr;
  double* x = nullptr;
  int64_t mv_partials = 0;
  // rank of a sharded CG (gg_cg_*_partial / _finish): an iteration's local
  // sums await the caller's all-reduce (the p_new of that iteration)
  bool await_finish = false;
  // live timing of the mode products (gg_cg_profile): d + 1 events per
  // profiled iteration, recorded on the CG stream, read back on demand
  bool profiling = false;
  std::vector<hipEvent_t> events;
  size_t events_used = 0;
  // parity-block basis (gg_kronb.hip): the recurrence runs on P b, P x, ...
  // in the block layout -- xb the iterate, q2 the pair launch's q (swapped
  // with q every iteration); x (the caller's) is written by the unfold of
  // each close.  basis: requested (gg_cg_set_basis); block: in effect for the
  // current solve (fixed at gg_cg_start: fused, layout 0, x_defer 2, rq 1)
  const gg::BlockOp* blk = nullptr;
  int basis = 1;
  bool block = false;
  double* xb = nullptr;
  double* q2 = nullptr;
  // a rank of the block-sharded CG (gg_cg_create_blocks): the handle's
  // vectors are blocks [rblk0, rblk0 + rnblk) of the block layout (rnblk > 0);
  // only the _partial / _finish entry points drive it
  int64_t rblk0 = 0, rnblk = -1;
  // A/B (GG_CG_RESTART=1, latched at create): gg_cg_iterate restarts a
  // cancelled beta (p = r) as a sharded rank does instead of repairing it --
  // the restart penalty measured on one GPU with everything else equal
  bool restart = false;
  // x_defer mode 3 (window; block basis with the LDS pair launch): the window
  // requested at create (GG_CG_XWIN, 0 = the balanced pairs of mode 2), the
  // mode in effect for the current solve (gg_cg_start*), and the ring of
  // xwin + 1 direction buffers (slots 0..3 are p, p2, p3, p4 as created; the
  // rest lie past the scratch region) with the current direction at pcur
  int xwin = 0;
  int xphase = 0;   // GG_CG_XWIN_PHASE latched at create (0: the default)
  int xmode = 0;
  double* ring[gg::kXWinMax + 1] = {};
  int pcur = 0;
  double *q_c = nullptr, *q2_c = nullptr;   // q / q2 as created (swapped per iteration)
  // derived r (CgScalars::rstored; with the window in the block basis): the
  // prologue keeps no r -- 5 passes instead of 6.  rder_ok: the knob
  // (GG_CG_RDERIVE, default on) latched at create; rder: in effect this solve
  bool rder_ok = true;
  bool rder = false;
  // the direction before the current one (p_{j-2} for iteration j's prologue)
  double* pprev_buf() const {
    const int ns = nring();
    return ring[(pcur + ns - 1) % ns];
  }
  int launches() const { return block ? gg::block_launches(blk) : gg::kron_d(K); }
  int nring() const { return xmode == 3 ? xwin + 1 : 4; }
  // the length of the recurrence's vectors: the grid's n, or the block
  // layout's (padded pair axes: >= n) for a full handle in the block basis
  // (a block-range handle's n is already its blocks' length)
  int64_t nvec() const { return (block && rnblk < 0) ? gg::block_n(blk) : n; }
  // every solve starts from the buffers as created (a block solve swaps q / q2
  // and rotates the directions)
  void reset_buffers() {
    p = ring[0];
    p2 = ring[1];
    p3 = ring[2];
    p4 = ring[3];
    q = q_c;
    q2 = q2_c;
    pcur = 0;
  }
  // after an iteration's scalars: p_new (p2) becomes the current direction
  void rotate_dirs() {
    if (xmode == 3) {
      const int ns = nring();
      pcur = (pcur + 1) % ns;
      p = ring[pcur];
      p2 = ring[(pcur + 1) % ns];
    } else if (xmode == 2) {
      // (cur, free, p_{j-2}, p_{j-3}) <- (free, p_{j-3}, cur, p_{j-2}): the
      // active pair (at most p_{j-1}, p_{j-2} next iteration) stays alive
      double* cur = p;
      double* o2 = p3;
      p = p2;
      p2 = p4;
      p3 = cur;
      p4 = o2;
    } else if (xmode == 1) {
      // (cur, free, old) <- (free, old, cur): p_j becomes current, p_{j-1}
      // is kept one more iteration for the deferred x update
      double* old_ = p3;
      p3 = p;
      p = p2;
      p2 = old_;
    } else {
      std::swap(p, p2);
    }
  }
};

namespace gg {
// x_defer mode 3's window from the knob snapshot (GG_CG_XWIN; < 2: off)
static int cg_xwin_knob() {
  const char* e = knob("GG_CG_XWIN");
  const int k = e ? atoi(e) : kXWinDefault;
  return k < 2 ? 0 : std::min(k, kXWinMax);
}
// units per window phase of the pair launch (GG_CG_XWIN_PHASE, 1..8; 1: the
// per-unit schedule, an A/B and test switch)
static int cg_xphase_knob() {
  const char* e = knob("GG_CG_XWIN_PHASE");
  const int r = e ? atoi(e) : kXWinPhaseDefault;
  return std::min(std::max(r, 1), kXWinPhaseMax);
}
// direction buffers beyond the four every handle has
static int64_t cg_extra_dirs(int K) { return K >= 2 ? std::max(0, K + 1 - 4) : 0; }
int64_t xwin_region(int64_t n, int K) { return 2 * ceil_div(n, 2 * (int64_t)K); }
}  // namespace gg

extern "C" {

int gg_dot(const double* x_dev, const double* y_dev, int64_t n, double* out_host,
           gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(x_dev && y_dev && out_host && n >= 0, GG_ERR_VALUE, "bad argument");
    hipStream_t s = gg::as_stream(stream);
    double* buf = nullptr;
    GG_HIP(hipMallocAsync(&buf, (gg::kVecBlocks + 1) * sizeof(double), s));
    const int nb = gg::vec_blocks(n);
    if (gg::aligned16(x_dev) && gg::aligned16(y_dev)) {
      gg::launch_dot_partials(x_dev, y_dev, n, buf, nb, s);
    } else {
      hipLaunchKernelGGL(gg::dot_partials_unaligned_kernel, dim3(nb), dim3(gg::kVecThreads), 0,
                         s, x_dev, y_dev, n, buf);
      GG_LAUNCH_CHECK();
    }
    gg::launch_reduce_to(buf, nb, buf + gg::kVecBlocks, s);
    GG_HIP(hipMemcpyAsync(out_host, buf + gg::kVecBlocks, sizeof(double),
                          hipMemcpyDeviceToHost, s));
    GG_HIP(hipFreeAsync(buf, s));
    GG_HIP(hipStreamSynchronize(s));
  });
}

int gg_axpby(double a, const double* x_dev, double b, double* y_dev, int64_t n,
             gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(x_dev && y_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    if (n == 0) return;
    hipLaunchKernelGGL(gg::axpby_kernel, dim3(gg::vec_blocks(2 * n)), dim3(gg::kVecThreads),
                       0, gg::as_stream(stream), a, x_dev, b, y_dev, n);
    GG_LAUNCH_CHECK();
  });
}

// The CG vectors start on 256-byte boundaries: the workspace base is rounded
// up and every vector's stride is a multiple of 32 doubles.  A vector off a
// 128-byte line costs the fused prologue (six streams) 13.0 -> 15.4 ms at
// 200^4 -- the "slow level" of rounds 3-4, reproduced by the diagnostic knob
// GG_CG_VEC_PAD (elements, even; added to the stride: pad 2 = every vector
// 16 bytes further off the line than the previous; tools/prologue_levels.py,
// profiles/r04/n_levels.jsonl).  Read from the snapshot gg_cg_work_elems
// takes, which gg_cg_create lays the workspace out by.
static int64_t cg_vec_pad() {
  const char* e = gg::knob("GG_CG_VEC_PAD");
  const int64_t v = e ? atoll(e) : 0;
  return v > 0 ? 2 * (v / 2) : 0;
}
static int64_t cg_vec_stride(int64_t n) { return (n + 31) / 32 * 32 + cg_vec_pad(); }
constexpr int64_t kCgAlignSlack = 32;   // doubles: room to round the base up to 256 B

// gg_cg_create's layout: r, p, q, p2, p3, p4, then the scratch region (the
// matvec scratch, or xb and q2 in the block basis), then the window's extra
// direction buffers; *extra_off = where those start (from the aligned base)
static int64_t cg_layout_elems(const gg_kron* K, int64_t n, int64_t* extra_off = nullptr,
                               int* xwin = nullptr, int64_t* vstride = nullptr) {
  const gg::BlockOp* B = gg::kron_block(K);
  // every vector holds the grid's n or the block layout's (padded) length
  const int64_t vs = cg_vec_stride(B ? std::max(n, gg::block_n(B)) : n);
  if (vstride) *vstride = vs;
  const int64_t scratch = gg::kron_work_elems(K, false) + (gg::kron_d(K) % 2 == 1 ? n : 0);
  const int64_t region = (std::max(scratch, B ? 2 * vs : 0) + 31) / 32 * 32;
  const int w = (B && gg::block_pair_side(B)) ? gg::cg_xwin_knob() : 0;
  if (extra_off) *extra_off = 6 * vs + region;
  if (xwin) *xwin = w;
  return kCgAlignSlack + 6 * vs + region + gg::cg_extra_dirs(w) * vs;
}

// the workspace each thread's last gg_cg_work_elems sized per operator: a
// gg_cg_create whose layout (read from the snapshot current then) needs more
// -- another handle's creation re-took the GG_* snapshot with, say, a wider
// window in between -- is refused instead of overrunning the caller's buffer
static thread_local std::map<const gg_kron*, int64_t> t_cg_sized;

int gg_cg_work_elems(const gg_kron* K, int64_t* elems) {
  return gg::guard([&] {
    GG_REQUIRE(K && elems, GG_ERR_VALUE, "NULL argument");
    gg::knobs_reload();   // the CG handle made next latches this snapshot
    const int64_t n = gg::kron_n(K);
    // r, p, q, p2, p3, p4 (x_defer) + the matvec scratch (+ the first mode
    // product's own output for an odd number of factors, MpFuse::first_dst);
    // the block basis (gg_kronb.hip) takes the scratch region for xb and q2
    // + the window's extra direction buffers (x_defer mode 3, block basis)
    *elems = cg_layout_elems(K, n);
    t_cg_sized[K] = *elems;
  });
}

int gg_cg_work_elems_blocks(const gg_kron* K, int64_t nblk, int64_t* elems) {
  return gg::guard([&] {
    GG_REQUIRE(K && elems, GG_ERR_VALUE, "NULL argument");
    const gg::BlockOp* B = gg::kron_block(K);
    GG_REQUIRE(B != nullptr, GG_ERR_VALUE, "the operator has no parity-block basis");
    GG_REQUIRE(nblk >= 1 && nblk <= ((int64_t)1 << gg::block_d(B)), GG_ERR_VALUE,
               "block count outside 1..2^d");
    gg::knobs_reload();   // the CG handle made next latches this snapshot
    // r, p, q, p2, p3, p4 and q2 (the pair launch's q), then the window's
    // extra direction buffers (x_defer mode 3)
    const int w = gg::block_pair_side(B) ? gg::cg_xwin_knob() : 0;
    *elems = kCgAlignSlack + (7 + gg::cg_extra_dirs(w)) * cg_vec_stride(nblk * gg::block_nb(B));
  });
}

int gg_cg_create_blocks(const gg_kron* K, int64_t blk0, int64_t nblk, double shift,
                        double* work_dev, gg_cg** out) {
  return gg::guard([&] {
    GG_REQUIRE(K && work_dev && out, GG_ERR_VALUE, "NULL argument");
    const gg::BlockOp* B = gg::kron_block(K);
    GG_REQUIRE(B != nullptr, GG_ERR_VALUE, "the operator has no parity-block basis");
    GG_REQUIRE(gg::block_d(B) >= 3, GG_ERR_VALUE, "the block-sharded CG needs d >= 3");
    GG_REQUIRE(blk0 >= 0 && nblk >= 1 && blk0 + nblk <= ((int64_t)1 << gg::block_d(B)),
               GG_ERR_VALUE, "block range outside the 2^d blocks");
    GG_REQUIRE((reinterpret_cast<uintptr_t>(work_dev) & 15) == 0, GG_ERR_VALUE,
               "the CG workspace must be 16-byte aligned");
    const int64_t n = nblk * gg::block_nb(B);
    gg_cg* cg = new gg_cg();
    try {
      cg->K = K;
      cg->shift = shift;
      cg->n = n;
      const int64_t vs = cg_vec_stride(n);
      work_dev = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work_dev) + 255) &
                                           ~static_cast<uintptr_t>(255));
      cg->r = work_dev;
      cg->p = work_dev + vs;
      cg->q = work_dev + 2 * vs;
      cg->p2 = work_dev + 3 * vs;
      cg->p3 = work_dev + 4 * vs;
      cg->p4 = work_dev + 5 * vs;
      cg->q2 = work_dev + 6 * vs;
      cg->xwin = gg::block_pair_side(B) ? gg::cg_xwin_knob() : 0;
      cg->xphase = gg::cg_xphase_knob();
      cg->ring[0] = cg->p;
      cg->ring[1] = cg->p2;
      cg->ring[2] = cg->p3;
      cg->ring[3] = cg->p4;
      for (int i = 0; i < gg::cg_extra_dirs(cg->xwin); ++i) cg->ring[4 + i] = work_dev + (7 + i) * vs;
      cg->q_c = cg->q;
      cg->q2_c = cg->q2;
      cg->blk = B;
      cg->basis = 1;
      cg->rblk0 = blk0;
      cg->rnblk = nblk;
      cg->fused = true;   // layout 0, x_defer 2, rq 1: the block path's only form
      const char* rde = gg::knob("GG_CG_RDERIVE");  // A/B: 0 keeps r in memory
      cg->rder_ok = !(rde && atoi(rde) == 0);
      cg->mv_partials = gg::block_partials_needed(B);
      GG_HIP(hipMalloc(&cg->partials,
                       std::max<int64_t>(gg::kVecBlocks, 3 * cg->mv_partials) * sizeof(double)));
      cg->rr_count = gg::block_prologue_blocks(B);
      GG_HIP(hipMalloc(&cg->rr_part, 2 * cg->rr_count * sizeof(double)));
      GG_HIP(hipMemset(cg->rr_part, 0, 2 * cg->rr_count * sizeof(double)));
      GG_HIP(hipMalloc(&cg->sc, sizeof(gg::CgScalars)));
      GG_HIP(hipHostMalloc(&cg->sc_host, sizeof(gg::CgScalars), hipHostMallocDefault));
      gg::scalars_clear(cg->sc);
    } catch (...) {
      gg_cg_destroy(cg);
      throw;
    }
    *out = cg;
  });
}

int gg_cg_create(const gg_kron* K, double shift, double* work_dev, gg_cg** out) {
  return gg::guard([&] {
    GG_REQUIRE(K && work_dev && out, GG_ERR_VALUE, "NULL argument");
    // the switches (GG_CG_*) come from the snapshot gg_cg_work_elems took, so
    // the vector stride (GG_CG_VEC_PAD) is the one the workspace was sized for
    int64_t nr = 0, nc = 0, we = 0;
    gg_kron_shape(K, 0, &nr, &nc, &we);
    GG_REQUIRE(nr == nc, GG_ERR_VALUE, "CG needs a square operator");
    gg_cg* cg = new gg_cg();
    try {
      cg->K = K;
      cg->shift = shift;
      cg->n = nr;
      int64_t vs = 0;
      const int64_t need = cg_layout_elems(K, nr, nullptr, nullptr, &vs);
      const auto sized = t_cg_sized.find(K);
      GG_REQUIRE(sized == t_cg_sized.end() || need <= sized->second, GG_ERR_VALUE,
                 "the CG workspace was sized (gg_cg_work_elems) under another GG_* snapshot: "
                 "call gg_cg_work_elems again before gg_cg_create");
      if (sized != t_cg_sized.end()) t_cg_sized.erase(sized);   // one check per sizing
      GG_REQUIRE((reinterpret_cast<uintptr_t>(work_dev) & 7) == 0, GG_ERR_VALUE,
                 "the CG workspace must hold doubles (8-byte aligned)");
      // the caller's own alignment (the 256-byte round-up below would hide it):
      // a base that is only 8-byte aligned takes the textbook recurrence
      const bool base16 = (reinterpret_cast<uintptr_t>(work_dev) & 15) == 0;
      work_dev = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work_dev) + 255) &
                                           ~static_cast<uintptr_t>(255));
      cg->r = work_dev;
      cg->p = work_dev + vs;
      cg->q = work_dev + 2 * vs;
      cg->p2 = work_dev + 3 * vs;
      cg->p3 = work_dev + 4 * vs;
      cg->p4 = work_dev + 5 * vs;
      cg->mv_work = work_dev + 6 * vs;
      if (gg::kron_d(K) % 2 == 1) cg->first_dst = cg->mv_work + gg::kron_work_elems(K, false);
      cg->blk = gg::kron_block(K);
      int64_t extra_off = 0;
      int xwin = 0;
      cg_layout_elems(K, nr, &extra_off, &xwin);
      cg->ring[0] = cg->p;
      cg->ring[1] = cg->p2;
      cg->ring[2] = cg->p3;
      cg->ring[3] = cg->p4;
      cg->q_c = cg->q;
      if (cg->blk != nullptr) {
        cg->xb = work_dev + 6 * vs;
        cg->q2 = work_dev + 7 * vs;
        cg->q2_c = cg->q2;
        const char* be = gg::knob("GG_CG_BASIS");   // read once per handle
        // default: the block basis where its padding costs little
        cg->basis = be ? (atoi(be) != 0 ? 1 : 0) : (gg::block_efficient(cg->blk) ? 1 : 0);
        // the window only where the pair launch carries the side job
        cg->xwin = gg::block_pair_side(cg->blk) ? xwin : 0;
        cg->xphase = gg::cg_xphase_knob();
        for (int i = 0; i < gg::cg_extra_dirs(xwin); ++i)
          cg->ring[4 + i] = work_dev + extra_off + i * vs;
      } else {
        cg->basis = 0;
      }
      const char* xd = gg::knob("GG_CG_XDEFER");   // A/B knob: 0, 1 or 2
      if (xd) cg->xdefer = std::min(2, std::max(0, atoi(xd)));
      const char* rqe = gg::knob("GG_CG_RQ");       // A/B knob: 0 (epilogue reads r) or 1
      if (rqe) cg->rq = std::min(2, std::max(0, atoi(rqe)));   // 2: diagnostic
      const char* rse = gg::knob("GG_CG_RESTART");  // A/B: restart instead of repair
      cg->restart = rse && atoi(rse) == 1;
      const char* rde = gg::knob("GG_CG_RDERIVE");  // A/B: 0 keeps r in memory
      cg->rder_ok = !(rde && atoi(rde) == 0);
      cg->mv_partials = gg::kron_partials_needed(K, false);
      if (cg->blk) cg->mv_partials = std::max(cg->mv_partials, gg::block_partials_needed(cg->blk));
      const int64_t np = std::max<int64_t>(gg::kVecBlocks, 3 * cg->mv_partials);
      GG_HIP(hipMalloc(&cg->partials, np * sizeof(double)));
      // the fused recurrence needs d >= 2 and 16-byte aligned vectors (its
      // side job moves double2); otherwise the textbook recurrence runs
      cg->fused = gg::kron_d(K) >= 2 && (nr % 2) == 0 && base16;
      if (cg->fused) {
        // capacity for any prologue launch shape; each iteration sums exactly
        // the partials its prologue launch wrote (MpFuse::pro_blocks)
        cg->rr_count = gg::kron_prologue_blocks(K);
        if (cg->blk) cg->rr_count = std::max(cg->rr_count, gg::block_prologue_blocks(cg->blk));
        GG_HIP(hipMalloc(&cg->rr_part, 2 * cg->rr_count * sizeof(double)));
        GG_HIP(hipMemset(cg->rr_part, 0, 2 * cg->rr_count * sizeof(double)));
      }
      GG_HIP(hipMalloc(&cg->sc, sizeof(gg::CgScalars)));
      GG_HIP(hipHostMalloc(&cg->sc_host, sizeof(gg::CgScalars), hipHostMallocDefault));
      gg::scalars_clear(cg->sc);
    } catch (...) {
      gg_cg_destroy(cg);
      throw;
    }
    *out = cg;
  });
}

int gg_cg_destroy(gg_cg* cg) {
  return gg::guard([&] {
    if (!cg) return;
    if (cg->partials) (void)hipFree(cg->partials);
    if (cg->rr_part) (void)hipFree(cg->rr_part);
    if (cg->sc) (void)hipFree(cg->sc);
    if (cg->sc_host) (void)hipHostFree(cg->sc_host);
    for (hipEvent_t e : cg->events) (void)hipEventDestroy(e);
    delete cg;
  });
}

int gg_cg_profile(gg_cg* cg, int enable) {
  return gg::guard([&] {
    GG_REQUIRE(cg, GG_ERR_VALUE, "NULL handle");
    cg->profiling = enable != 0;
    cg->events_used = 0;
  });
}

int gg_cg_profile_read(gg_cg* cg, int* n_matvecs, double* mode_ms, int mode_ms_len) {
  return gg::guard([&] {
    GG_REQUIRE(cg && n_matvecs, GG_ERR_VALUE, "NULL argument");
    const int d = cg->launches();
    GG_REQUIRE(mode_ms == nullptr || mode_ms_len >= d, GG_ERR_VALUE, "mode_ms too short");
    const size_t per = (size_t)d + 1;
    const int nm = (int)(cg->events_used / per);
    if (mode_ms)
      for (int k = 0; k < d; ++k) mode_ms[k] = 0.0;
    for (int it = 0; it < nm; ++it) {
      hipEvent_t* ev = cg->events.data() + it * per;
      GG_HIP(hipEventSynchronize(ev[d]));
      for (int k = 0; k < d && mode_ms; ++k) {
        float ms = 0.0f;
        GG_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        mode_ms[k] += ms;
      }
    }
    *n_matvecs = nm;
  });
}

int gg_cg_start(gg_cg* cg, const double* b_dev, double* x_dev, double rtol, double atol,
                gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && b_dev && x_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(rtol >= 0 && atol >= 0, GG_ERR_VALUE,
               "tolerances must be real, non-negative numbers");
    GG_REQUIRE(cg->rnblk < 0, GG_ERR_VALUE,
               "a block-range handle (gg_cg_create_blocks) runs through gg_cg_start_partial");
    // the x / r update and the fused side job move x as 16-byte pairs
    GG_REQUIRE((reinterpret_cast<uintptr_t>(x_dev) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(b_dev) & 7) == 0,
               GG_ERR_VALUE, "x must be 16-byte aligned (b: 8-byte)");
    hipStream_t s = gg::as_stream(stream);
    cg->b = b_dev;
    cg->x = x_dev;
    const int64_t n = cg->n;
    cg->block = cg->blk != nullptr && cg->basis != 0 && cg->fused && cg->fusion == 0 &&
                cg->xdefer == 2 && cg->rq == 1 && gg::block_d(cg->blk) >= 3;
    cg->xmode = (cg->fused && cg->fusion != 2) ? cg->xdefer : 0;
    if (cg->block && cg->xwin >= 2) cg->xmode = 3;
    cg->rder = cg->xmode == 3 && cg->rder_ok && gg::block_rderive_ok(cg->blk);
    cg->reset_buffers();
    hipLaunchKernelGGL(gg::cg_xwin_init_kernel, dim3(1), dim3(1), 0, s, cg->sc,
                       cg->xmode == 3 ? cg->xwin : 0);
    GG_LAUNCH_CHECK();
    GG_HIP(hipMemsetAsync(x_dev, 0, n * sizeof(double), s));
    if (cg->block) {
      // r = P b (the fold, with its |P b|^2 partials), x_b = 0
      gg::block_fold(cg->blk, false, b_dev, cg->r, cg->partials, s);
      GG_HIP(hipMemsetAsync(cg->xb, 0, cg->nvec() * sizeof(double), s));
      // the first prologue reads q_old with nothing pending; the fixed-count
      // block kernel forms r - 0 * q_old there (no select), so whatever the
      // caller's workspace held (a NaN, an Inf) must not be in q
      GG_HIP(hipMemsetAsync(cg->q, 0, cg->nvec() * sizeof(double), s));
      hipLaunchKernelGGL(gg::cg_init_kernel, dim3(1), dim3(1024), 0, s, cg->partials,
                         gg::block_fold_partials(cg->blk), cg->sc, rtol, atol);
      GG_LAUNCH_CHECK();
      return;
    }
    GG_HIP(hipMemcpyAsync(cg->r, b_dev, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    const int nb = gg::vec_blocks(n);
    gg::launch_dot_partials(cg->r, cg->r, n, cg->partials, nb, s);
    hipLaunchKernelGGL(gg::cg_init_kernel, dim3(1), dim3(1024), 0, s, cg->partials,
                       (int64_t)nb, cg->sc, rtol, atol);
    GG_LAUNCH_CHECK();
  });
}

int gg_cg_set_recurrence(gg_cg* cg, int fused) {
  return gg::guard([&] {
    GG_REQUIRE(cg, GG_ERR_VALUE, "NULL handle");
    GG_REQUIRE(cg->x == nullptr, GG_ERR_VALUE, "set the recurrence before gg_cg_start");
    if (!fused) {
      cg->fused = false;
    } else {
      GG_REQUIRE(cg->rr_part != nullptr, GG_ERR_VALUE,
                 "the fused recurrence needs d >= 2, an even n and 16-byte aligned work");
      cg->fused = true;
    }
  });
}

int gg_cg_set_fusion(gg_cg* cg, int layout) {
  return gg::guard([&] {
    GG_REQUIRE(cg, GG_ERR_VALUE, "NULL handle");
    GG_REQUIRE(cg->x == nullptr, GG_ERR_VALUE, "set the fusion layout before gg_cg_start");
    GG_REQUIRE(layout >= 0 && layout <= 2, GG_ERR_VALUE, "fusion layout must be 0, 1 or 2");
    GG_REQUIRE(layout == 0 || gg::kron_first_single_launch(cg->K), GG_ERR_VALUE,
               "fusion layouts 1 / 2 need the first factor within one launch (<= 256 rows)");
    cg->fusion = layout;
  });
}

int gg_cg_get_fusion(const gg_cg* cg, int* layout) {
  return gg::guard([&] {
    GG_REQUIRE(cg && layout, GG_ERR_VALUE, "NULL argument");
    *layout = cg->fusion;
  });
}

int gg_cg_set_xdefer(gg_cg* cg, int on) {
  return gg::guard([&] {
    GG_REQUIRE(cg, GG_ERR_VALUE, "NULL handle");
    GG_REQUIRE(cg->x == nullptr, GG_ERR_VALUE, "set x deferral before gg_cg_start");
    GG_REQUIRE(on >= 0 && on <= 2, GG_ERR_VALUE, "x deferral mode must be 0, 1 or 2");
    cg->xdefer = on;
  });
}

int gg_cg_get_xdefer(const gg_cg* cg, int* on) {
  return gg::guard([&] {
    GG_REQUIRE(cg && on, GG_ERR_VALUE, "NULL argument");
    *on = (cg->fused && cg->fusion != 2) ? cg->xdefer : 0;
  });
}

int gg_cg_get_xwin(const gg_cg* cg, int* K) {
  return gg::guard([&] {
    GG_REQUIRE(cg && K, GG_ERR_VALUE, "NULL argument");
    if (cg->x != nullptr) {
      *K = cg->xmode == 3 ? cg->xwin : 0;
    } else {
      int b = 0;
      gg_cg_get_basis(cg, &b);
      *K = (b && cg->xwin >= 2) ? cg->xwin : 0;
    }
  });
}

int gg_cg_get_rderive(const gg_cg* cg, int* on) {
  return gg::guard([&] {
    GG_REQUIRE(cg && on, GG_ERR_VALUE, "NULL argument");
    if (cg->x != nullptr) {
      *on = cg->rder ? 1 : 0;
    } else {
      int K = 0;
      gg_cg_get_xwin(cg, &K);
      *on = (K >= 2 && cg->rder_ok && gg::block_rderive_ok(cg->blk)) ? 1 : 0;
    }
  });
}

int gg_cg_calibrate(gg_cg* cg, int reps, double* ms_host, int64_t* offsets_host,
                    gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && ms_host && reps >= 1, GG_ERR_VALUE, "bad argument");
    GG_REQUIRE((reinterpret_cast<uintptr_t>(cg->p) & 15) == 0, GG_ERR_VALUE,
               "the CG workspace is not 16-byte aligned");
    hipStream_t s = gg::as_stream(stream);
    int dev = 0, cus = 0;
    GG_HIP(hipGetDevice(&dev));
    GG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    gg::EventSet ev(2);
    // the prologue this solve runs: derived r reads p_{j-2} in r's place
    // (a direction slot the first iterations overwrite anyway)
    const bool rd = cg->rder;
    double* second = rd ? cg->ring[(cg->pcur + 2) % cg->nring()] : cg->r;
    // two untimed passes (first touch in this process), then reps timed
    for (int it = 0; it < reps + 2; ++it) {
      if (it == 2) GG_HIP(hipEventRecord(ev.ev[0], s));
      if (rd)
        hipLaunchKernelGGL(gg::cg_stream_probe_kernel<true>,
                           dim3((unsigned)std::max(cus, 1) * 8), dim3(256), 0, s, second, cg->p,
                           cg->p2, cg->q, cg->nvec());
      else
        hipLaunchKernelGGL(gg::cg_stream_probe_kernel<false>,
                           dim3((unsigned)std::max(cus, 1) * 8), dim3(256), 0, s, second, cg->p,
                           cg->p2, cg->q, cg->nvec());
      GG_LAUNCH_CHECK();
    }
    GG_HIP(hipEventRecord(ev.ev[1], s));
    GG_HIP(hipEventSynchronize(ev.ev[1]));
    float ms = 0.f;
    GG_HIP(hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]));
    *ms_host = ms / reps;
    if (offsets_host) {
      // the buffers' addresses modulo 2 MiB (the allocator's large-page grain)
      const double* b[4] = {second, cg->p, cg->p2, cg->q};
      for (int k = 0; k < 4; ++k)
        offsets_host[k] = (int64_t)(reinterpret_cast<uintptr_t>(b[k]) & ((1u << 21) - 1));
    }
  });
}

int gg_cg_set_rq(gg_cg* cg, int mode) {
  return gg::guard([&] {
    GG_REQUIRE(cg, GG_ERR_VALUE, "NULL handle");
    GG_REQUIRE(cg->x == nullptr, GG_ERR_VALUE, "set the r.q source before gg_cg_start");
    GG_REQUIRE(mode == 0 || mode == 1, GG_ERR_VALUE, "r.q mode must be 0 or 1");
    cg->rq = mode;
  });
}

int gg_cg_get_rq(const gg_cg* cg, int* mode) {
  return gg::guard([&] {
    GG_REQUIRE(cg && mode, GG_ERR_VALUE, "NULL argument");
    *mode = (cg->fused && cg->fusion == 0 && cg->rq) ? 1 : 0;
  });
}

int gg_cg_set_basis(gg_cg* cg, int block) {
  return gg::guard([&] {
    GG_REQUIRE(cg, GG_ERR_VALUE, "NULL handle");
    GG_REQUIRE(cg->x == nullptr, GG_ERR_VALUE, "set the basis before gg_cg_start");
    GG_REQUIRE(block == 0 || cg->blk != nullptr, GG_ERR_VALUE,
               "the operator has no parity-block basis");
    cg->basis = block != 0 ? 1 : 0;
  });
}

int gg_cg_get_basis(const gg_cg* cg, int* block) {
  return gg::guard([&] {
    GG_REQUIRE(cg && block, GG_ERR_VALUE, "NULL argument");
    // in effect once started; before, what gg_cg_start will choose
    *block = cg->x != nullptr ? (cg->block ? 1 : 0)
                              : (cg->blk != nullptr && cg->basis != 0 && cg->fused &&
                                 cg->fusion == 0 && cg->xdefer == 2 && cg->rq == 1 &&
                                 gg::block_d(cg->blk) >= 3)
                                    ? 1
                                    : 0;
  });
}

int gg_cg_launches(const gg_cg* cg, int* launches) {
  return gg::guard([&] {
    GG_REQUIRE(cg && launches, GG_ERR_VALUE, "NULL argument");
    int b = 0;
    gg_cg_get_basis(cg, &b);
    *launches = b ? gg::block_launches(cg->blk) : gg::kron_d(cg->K);
  });
}

int gg_cg_get_recurrence(const gg_cg* cg, int* fused) {
  return gg::guard([&] {
    GG_REQUIRE(cg && fused, GG_ERR_VALUE, "NULL argument");
    *fused = cg->fused ? 1 : 0;
  });
}

// Textbook recurrence, one iteration:
//   q = (K + s I) p with p = r + beta p fused into the first mode product
//   and p.q into the last; alpha; x += alpha p, r -= alpha q, r.r; beta.
// Fused recurrence, one iteration j (every vector pass rides on a mode
// product; the matrix cores bound the kernels and HBM has room):
//   mode product 1: r_j = r_{j-1} - alpha q_{j-1} (in place, r.r partials),
//                   p_j = r_j + beta p_{j-1} (into the other p buffer);
//   mode product 2: side job x_j = x_{j-1} + alpha p_{j-1};
//   mode product d: q_j = K p_j + s p_j, partials p.q, r.q, q.q;
//   scalars: rho_j, stopping test, alpha_j, beta_j (cg_fused_scalars_kernel).
// Leaving gg_cg_iterate applies the pending x / r update with the textbook
// kernels, so the state it leaves (x, r, iteration count) is the textbook's.
int gg_cg_iterate(gg_cg* cg, int max_iters, int check_every, gg_stream stream) {
  const int st = gg_cg_iterate_open(cg, max_iters, check_every, stream);
  return st != GG_OK ? st : gg_cg_close(cg, stream);
}

int gg_cg_iterate_open(gg_cg* cg, int max_iters, int check_every, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && cg->x, GG_ERR_VALUE, "CG not started");
    GG_REQUIRE(cg->rnblk < 0, GG_ERR_VALUE,
               "a block-range handle (gg_cg_create_blocks) runs through gg_cg_iterate_partial");
    hipStream_t s = gg::as_stream(stream);
    const int64_t n = cg->nvec();
    const int nb = gg::vec_blocks(n);
    if (check_every <= 0) check_every = max_iters;
    for (int it = 0; it < max_iters; ++it) {
      int64_t nparts = 0;
      hipEvent_t* ev = nullptr;
      if (cg->profiling) {
        const size_t need = cg->events_used + (size_t)cg->launches() + 1;
        while (cg->events.size() < need) {
          hipEvent_t e;
          GG_HIP(hipEventCreate(&e));
          cg->events.push_back(e);
        }
        ev = cg->events.data() + cg->events_used;
        cg->events_used = need;
      }
      const int xmode = cg->xmode;   // fixed at gg_cg_start
      const bool xdefer = xmode != 0;
      if (cg->fused) {
        // repair (no-op unless the last beta cancelled): x += alpha p,
        // r -= alpha q, rho = r.r, textbook beta; the prologue then sees no
        // pending update (x_defer: r only, x keeps its deferred steps)
        if (!cg->restart) {
          if (cg->rder)   // r derived from the directions (not stored)
            hipLaunchKernelGGL(gg::cg_r_materialize_kernel, dim3(nb), dim3(gg::kVecThreads), 0,
                               s, cg->r, cg->q, n, cg->sc, cg->partials, 2);
          else
            hipLaunchKernelGGL(gg::cg_xr_update_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                               xdefer ? nullptr : cg->x, cg->r, cg->p, cg->q, n, cg->sc,
                               cg->partials, 2);
          GG_LAUNCH_CHECK();
          hipLaunchKernelGGL(gg::cg_rho_kernel, dim3(1), dim3(1024), 0, s, cg->partials,
                             (int64_t)nb, cg->sc, 2);
          GG_LAUNCH_CHECK();
        }
        gg::MpFuse fz;
        fz.r = cg->r;
        fz.q_old = cg->q;
        fz.p_out = cg->fusion == 0 ? cg->p2 : nullptr;
        fz.ep_out = cg->fusion == 0 ? nullptr : cg->p2;
        fz.ex = cg->fusion == 2 ? cg->x : nullptr;
        fz.sc = cg->sc;
        fz.rr_part = cg->rr_part;
        fz.rr_cap = cg->rr_count;
        int64_t pro_blocks = 0;   // the prologue launch's workgroups (kron_apply)
        fz.pro_blocks = &pro_blocks;
        fz.sx = cg->fusion == 2 ? nullptr : cg->x;
        fz.sp = cg->p;
        fz.sn = n;
        fz.xdefer = xmode;
        fz.xwin = cg->xwin;
    fz.xphase = cg->xphase;
        fz.rderive = cg->rder;
        fz.pprev = cg->rder ? cg->pprev_buf() : nullptr;
        fz.first_dst = cg->first_dst;
        // r.q: conjugacy identity (layout 0: the prologue adds p_new.q_old
        // partials, the epilogue skips its pass over r) or read in the epilogue
        const bool rq_ident = cg->rq != 0 && cg->fusion == 0;
        fz.er = (rq_ident && cg->rq != 2) ? nullptr : cg->r;
        fz.pqo_stride = rq_ident ? cg->rr_count : 0;
        fz.pstride = cg->mv_partials;
        if (cg->block) {
          // the block basis: d - 1 launches, q2 <- (K + s I) p_new
          fz.sx = cg->xb;
          fz.blk_q_out = cg->q2;
          gg::block_apply(cg->blk, cg->p, cg->q, cg->shift, nullptr, cg->partials,
                          &cg->sc->done, s, &nparts, &fz, 2, ev);
        } else {
          gg::kron_apply(cg->K, false, cg->p, cg->q, cg->shift, cg->mv_work, cg->partials,
                         &cg->sc->done, s, &nparts, &fz, 2, ev);
        }
        GG_REQUIRE(pro_blocks > 0 && pro_blocks <= cg->rr_count, GG_ERR_RUNTIME,
                   "fused CG: no prologue launch recorded");
        hipLaunchKernelGGL(gg::cg_fused_scalars_kernel, dim3(1), dim3(1024), 0, s, cg->rr_part,
                           pro_blocks, cg->rr_count, cg->partials, nparts, cg->mv_partials,
                           cg->sc,
                           xdefer ? (const double*)cg->p2 : nullptr, xmode, rq_ident ? 1 : 0,
                           cg->rder ? 1 : 0);
        GG_LAUNCH_CHECK();
        if (cg->block) std::swap(cg->q, cg->q2);
        cg->rotate_dirs();
      } else {
        gg::MpFuse fz;
        fz.r = cg->r;
        fz.sc = cg->sc;
        gg::kron_apply(cg->K, false, cg->p, cg->q, cg->shift, cg->mv_work, cg->partials,
                       &cg->sc->done, s, &nparts, &fz, 1, ev);
        hipLaunchKernelGGL(gg::cg_alpha_kernel, dim3(1), dim3(1024), 0, s, cg->partials, nparts,
                           cg->sc);
        GG_LAUNCH_CHECK();
        hipLaunchKernelGGL(gg::cg_xr_update_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                           cg->x, cg->r, cg->p, cg->q, n, cg->sc, cg->partials, 0);
        GG_LAUNCH_CHECK();
        hipLaunchKernelGGL(gg::cg_rho_kernel, dim3(1), dim3(1024), 0, s, cg->partials,
                           (int64_t)nb, cg->sc, 0);
        GG_LAUNCH_CHECK();
      }
      if ((it + 1) % check_every == 0 && it + 1 < max_iters) {
        GG_HIP(hipMemcpyAsync(cg->sc_host, cg->sc, sizeof(gg::CgScalars),
                              hipMemcpyDeviceToHost, s));
        GG_HIP(hipStreamSynchronize(s));
        if (cg->sc_host->done) break;
      }
    }
  });
}

// leaving the fused recurrence: the deferred x steps and the pending r update
// (no-op for the textbook recurrence or when nothing is pending)
int gg_cg_close(gg_cg* cg, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && cg->x, GG_ERR_VALUE, "CG not started");
    GG_REQUIRE(cg->rnblk < 0, GG_ERR_VALUE,
               "a block-range handle (gg_cg_create_blocks) closes through gg_cg_close_partial");
    hipStream_t s = gg::as_stream(stream);
    const int64_t n = cg->nvec();
    const int nb = gg::vec_blocks(n);
    if (cg->fused) {
      const bool xdefer = cg->xmode != 0;
      // closing update (no-op unless pending): x += alpha p, r -= alpha q,
      // rho = r.r, beta, iteration count -- the textbook state.  x_defer: the
      // deferred steps first (also after convergence), then r only
      if (cg->xmode == 3) {
        hipLaunchKernelGGL(gg::cg_x_flush3_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                           cg->block ? cg->xb : cg->x, n, gg::xwin_region(n, cg->xwin), cg->sc);
        GG_LAUNCH_CHECK();
        hipLaunchKernelGGL(gg::cg_x_flushed3_kernel, dim3(1), dim3(1), 0, s, cg->sc);
        GG_LAUNCH_CHECK();
      } else if (cg->xmode == 2) {
        hipLaunchKernelGGL(gg::cg_x_flush2_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                           cg->block ? cg->xb : cg->x, n,
                           cg->block ? gg::block_side_half(n) : gg::kron_side_half(cg->K, n),
                           cg->sc);
        GG_LAUNCH_CHECK();
        hipLaunchKernelGGL(gg::cg_x_flushed_kernel, dim3(1), dim3(1), 0, s, cg->sc);
        GG_LAUNCH_CHECK();
      } else if (xdefer) {
        hipLaunchKernelGGL(gg::cg_x_flush_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, cg->x,
                           n, cg->sc);
        GG_LAUNCH_CHECK();
        hipLaunchKernelGGL(gg::cg_x_flushed_kernel, dim3(1), dim3(1), 0, s, cg->sc);
        GG_LAUNCH_CHECK();
      }
      if (cg->rder)   // r from the directions (- alpha q when pending) into its buffer
        hipLaunchKernelGGL(gg::cg_r_materialize_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                           cg->r, cg->q, n, cg->sc, cg->partials, 1);
      else
        hipLaunchKernelGGL(gg::cg_xr_update_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                           xdefer ? nullptr : cg->x, cg->r, cg->p, cg->q, n, cg->sc,
                           cg->partials, 1);
      GG_LAUNCH_CHECK();
      hipLaunchKernelGGL(gg::cg_rho_kernel, dim3(1), dim3(1024), 0, s, cg->partials,
                         (int64_t)nb, cg->sc, 1);
      GG_LAUNCH_CHECK();
      if (cg->rder) {
        hipLaunchKernelGGL(gg::cg_r_stored_kernel, dim3(1), dim3(1), 0, s, cg->sc);
        GG_LAUNCH_CHECK();
      }
    }
    // the block basis: the caller's x = P^T x_b
    if (cg->block) gg::block_fold(cg->blk, true, cg->xb, cg->x, nullptr, s);
  });
}

// ---- a rank of a sharded CG (include/gp_grief_amd.h, gg_cg_*_partial):
// the fused recurrence on this rank's block of a block-diagonal operator,
// every dot product reduced by the caller between _partial and _finish
int gg_cg_start_partial(gg_cg* cg, const double* b_dev, double* x_dev, double* rr_dev,
                        gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && b_dev && x_dev && rr_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(cg->fused, GG_ERR_VALUE, "the sharded rank runs the fused recurrence");
    hipStream_t s = gg::as_stream(stream);
    cg->b = b_dev;
    cg->x = x_dev;
    // the sharded rank: the handle's own operator layout, or its blocks of
    // the block layout (gg_cg_create_blocks; b and x in that layout)
    cg->block = cg->rnblk > 0;
    cg->await_finish = false;
    cg->xmode = cg->xdefer;
    if (cg->block && cg->xwin >= 2) cg->xmode = 3;
    cg->rder = cg->xmode == 3 && cg->rder_ok && gg::block_rderive_ok(cg->blk);
    cg->reset_buffers();
    hipLaunchKernelGGL(gg::cg_xwin_init_kernel, dim3(1), dim3(1), 0, s, cg->sc,
                       cg->xmode == 3 ? cg->xwin : 0);
    GG_LAUNCH_CHECK();
    const int64_t n = cg->n;
    GG_HIP(hipMemcpyAsync(cg->r, b_dev, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    GG_HIP(hipMemsetAsync(x_dev, 0, n * sizeof(double), s));
    // as in gg_cg_start: the block prologue forms r - 0 * q_old on the first step
    if (cg->block) GG_HIP(hipMemsetAsync(cg->q, 0, n * sizeof(double), s));
    const int nb = gg::vec_blocks(n);
    gg::launch_dot_partials(cg->r, cg->r, n, cg->partials, nb, s);
    gg::launch_reduce_to(cg->partials, nb, rr_dev, s);
  });
}

int gg_cg_start_finish(gg_cg* cg, const double* rr_dev, double rtol, double atol,
                       gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && cg->x && rr_dev, GG_ERR_VALUE, "CG not started (gg_cg_start_partial)");
    GG_REQUIRE(rtol >= 0 && atol >= 0, GG_ERR_VALUE,
               "tolerances must be real, non-negative numbers");
    hipLaunchKernelGGL(gg::cg_init_kernel, dim3(1), dim3(1024), 0, gg::as_stream(stream), rr_dev,
                       (int64_t)1, cg->sc, rtol, atol);
    GG_LAUNCH_CHECK();
  });
}

int gg_cg_iterate_partial(gg_cg* cg, double* red_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && cg->x && red_dev, GG_ERR_VALUE, "CG not started");
    GG_REQUIRE(cg->fused && cg->fusion == 0, GG_ERR_VALUE,
               "the sharded rank runs the fused recurrence, layout 0");
    GG_REQUIRE(!cg->await_finish, GG_ERR_VALUE, "gg_cg_iterate_finish first");
    hipStream_t s = gg::as_stream(stream);
    const int64_t n = cg->n;
    int64_t nparts = 0;
    hipEvent_t* ev = nullptr;
    if (cg->profiling) {
      const size_t need = cg->events_used + (size_t)cg->launches() + 1;
      while (cg->events.size() < need) {
        hipEvent_t e;
        GG_HIP(hipEventCreate(&e));
        cg->events.push_back(e);
      }
      ev = cg->events.data() + cg->events_used;
      cg->events_used = need;
    }
    // no repair kernels: a cancelled beta (set to 0 by the scalars) restarts
    // the recurrence with p = r instead of a second all-reduce
    const int xmode = cg->xmode;
    gg::MpFuse fz;
    fz.r = cg->r;
    fz.q_old = cg->q;
    fz.p_out = cg->p2;
    fz.sc = cg->sc;
    fz.rr_part = cg->rr_part;
    fz.rr_cap = cg->rr_count;
    int64_t pro_blocks = 0;
    fz.pro_blocks = &pro_blocks;
    fz.sx = cg->x;
    fz.sp = cg->p;
    fz.sn = n;
    fz.xdefer = xmode;
    fz.xwin = cg->xwin;
    fz.xphase = cg->xphase;
    fz.rderive = cg->rder;
    fz.pprev = cg->rder ? cg->pprev_buf() : nullptr;
    fz.first_dst = cg->first_dst;
    const bool rq_ident = cg->rq != 0;
    fz.er = rq_ident ? nullptr : cg->r;
    fz.pqo_stride = rq_ident ? cg->rr_count : 0;
    fz.pstride = cg->mv_partials;
    if (cg->block) {
      // the rank's blocks: d - 1 launches, q2 <- (K + s I) p_new
      fz.blk_q_out = cg->q2;
      gg::block_apply(cg->blk, cg->p, cg->q, cg->shift, nullptr, cg->partials, &cg->sc->done, s,
                      &nparts, &fz, 2, ev, cg->rblk0, cg->rnblk);
    } else {
      gg::kron_apply(cg->K, false, cg->p, cg->q, cg->shift, cg->mv_work, cg->partials,
                     &cg->sc->done, s, &nparts, &fz, 2, ev);
    }
    GG_REQUIRE(pro_blocks > 0 && pro_blocks <= cg->rr_count, GG_ERR_RUNTIME,
               "fused CG: no prologue launch recorded");
    if (cg->block) std::swap(cg->q, cg->q2);
    hipLaunchKernelGGL(gg::cg_local_red_kernel, dim3(1), dim3(1024), 0, s, cg->rr_part,
                       pro_blocks, cg->rr_count, cg->partials, nparts, cg->mv_partials,
                       rq_ident ? 1 : 0, red_dev);
    GG_LAUNCH_CHECK();
    cg->await_finish = true;
  });
}

int gg_cg_iterate_finish(gg_cg* cg, const double* red_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && red_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(cg->await_finish, GG_ERR_VALUE, "gg_cg_iterate_partial first");
    hipStream_t s = gg::as_stream(stream);
    const int xmode = cg->xmode;
    const bool rq_ident = cg->rq != 0;
    // red = [rr, p.q_old | p.q, r.q, q.q]: one-element partial arrays
    hipLaunchKernelGGL(gg::cg_fused_scalars_kernel, dim3(1), dim3(1024), 0, s, red_dev,
                       (int64_t)1, (int64_t)1, red_dev + 2, (int64_t)1, (int64_t)1, cg->sc,
                       xmode ? (const double*)cg->p2 : nullptr, xmode, rq_ident ? 1 : 0,
                       cg->rder ? 1 : 0);
    GG_LAUNCH_CHECK();
    cg->rotate_dirs();
    cg->await_finish = false;
  });
}

int gg_cg_close_partial(gg_cg* cg, double* rr_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && cg->x && rr_dev, GG_ERR_VALUE, "CG not started");
    GG_REQUIRE(!cg->await_finish, GG_ERR_VALUE, "gg_cg_iterate_finish first");
    hipStream_t s = gg::as_stream(stream);
    const int64_t n = cg->n;
    const int nb = gg::vec_blocks(n);
    if (cg->xmode == 3) {
      hipLaunchKernelGGL(gg::cg_x_flush3_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, cg->x, n,
                         gg::xwin_region(n, cg->xwin), cg->sc);
      GG_LAUNCH_CHECK();
      hipLaunchKernelGGL(gg::cg_x_flushed3_kernel, dim3(1), dim3(1), 0, s, cg->sc);
      GG_LAUNCH_CHECK();
    } else if (cg->xmode == 2) {
      hipLaunchKernelGGL(gg::cg_x_flush2_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, cg->x, n,
                         cg->block ? gg::block_side_half(n) : gg::kron_side_half(cg->K, n),
                         cg->sc);
      GG_LAUNCH_CHECK();
    } else if (cg->xmode == 1) {
      hipLaunchKernelGGL(gg::cg_x_flush_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, cg->x, n,
                         cg->sc);
      GG_LAUNCH_CHECK();
    }
    if (cg->xmode == 1 || cg->xmode == 2) {
      hipLaunchKernelGGL(gg::cg_x_flushed_kernel, dim3(1), dim3(1), 0, s, cg->sc);
      GG_LAUNCH_CHECK();
    }
    // the pending r update (x: the x_defer bookkeeping above, or here)
    GG_HIP(hipMemsetAsync(cg->partials, 0, nb * sizeof(double), s));
    if (cg->rder) {
      hipLaunchKernelGGL(gg::cg_r_materialize_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                         cg->r, cg->q, n, cg->sc, cg->partials, 1);
      GG_LAUNCH_CHECK();
      hipLaunchKernelGGL(gg::cg_r_stored_kernel, dim3(1), dim3(1), 0, s, cg->sc);
    } else {
      hipLaunchKernelGGL(gg::cg_xr_update_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s,
                         cg->xmode ? nullptr : cg->x, cg->r, cg->p, cg->q, n, cg->sc,
                         cg->partials, 1);
    }
    GG_LAUNCH_CHECK();
    gg::launch_reduce_to(cg->partials, nb, rr_dev, s);
  });
}

int gg_cg_close_finish(gg_cg* cg, const double* rr_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && rr_dev, GG_ERR_VALUE, "NULL argument");
    hipLaunchKernelGGL(gg::cg_close_rho_kernel, dim3(1), dim3(1), 0, gg::as_stream(stream),
                       cg->sc, rr_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_cg_cancels(gg_cg* cg, int* cancels, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg && cancels, GG_ERR_VALUE, "NULL argument");
    hipStream_t s = gg::as_stream(stream);
    GG_HIP(hipMemcpyAsync(cg->sc_host, cg->sc, sizeof(gg::CgScalars), hipMemcpyDeviceToHost,
                          s));
    GG_HIP(hipStreamSynchronize(s));
    *cancels = cg->sc_host->cancels;
  });
}

int gg_cg_status(gg_cg* cg, int* iters, int* converged, double* resid_norm, double* tol,
                 gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(cg, GG_ERR_VALUE, "NULL handle");
    hipStream_t s = gg::as_stream(stream);
    GG_HIP(hipMemcpyAsync(cg->sc_host, cg->sc, sizeof(gg::CgScalars), hipMemcpyDeviceToHost,
                          s));
    GG_HIP(hipStreamSynchronize(s));
    const gg::CgScalars& h = *cg->sc_host;
    if (iters) *iters = h.iters;
    if (converged) *converged = (h.done && std::sqrt(h.rho) < h.tol) || h.bnorm == 0.0;
    if (resid_norm) *resid_norm = std::sqrt(h.rho);
    if (tol) *tol = h.tol;
  });
}

}  // extern "C"
