// Lanczos tridiagonalisation of the shifted Kronecker operator from a
// Rademacher probe (the SLQ log det's inner loop): the recurrence's kernels,
// the grid-basis and block-basis drivers and the gg_lanczos_* C ABI.  The
// masked probe (gg_lzm.hip) shares lz_coef_kernel and lz_beta_kernel.
#include <cmath>

#include "gg_internal.h"

namespace gg {

// ----------------------------------------------------------- Lanczos kernels
// ---- fused Lanczos (gg_lanczos_probe).  The Lanczos vectors are kept
// unnormalised: V holds u with v = sV u, P holds u_prev with v_prev = sP u_prev
// (lzs[0], lzs[1]).  The matvec Y = K u + shift u has alpha's dot u.Y in its
// last epilogue (v.Av = sV^2 u.Y), and ONE streaming pass forms
// w = Av - alpha v - beta v_prev = cy Y + cu u + cp u_prev with |w|^2, in
// place of Y: 13 passes over N per step instead of 18 (no normalisation pass;
// the next step's v is w with sV = 1 / beta).  With an even number of
// factors that pass is the next matvec's prologue instead (CGP 3 in
// gg_kron.hip: w is the MFMA operand, written over u_prev).  alpha = v.Av: the oracle's
// v.(Av - beta v_prev) differs by beta v.v_prev, rounding-level while the
// three-term recurrence keeps local orthogonality.
// lzs: [0] sV, [1] sP, [2] cy, [3] cu, [4] cp
__global__ void lz_coef_kernel(double* __restrict__ lzs, const double* __restrict__ dot,
                               double* __restrict__ alpha_out,
                               const double* __restrict__ beta_prev) {
  const double sV = lzs[0], sP = lzs[1];
  const double a = sV * sV * *dot;
  *alpha_out = a;
  lzs[2] = sV;
  lzs[3] = -a * sV;
  lzs[4] = -(*beta_prev) * sP;
}

// w = cy w + cu v + cp p (in place), partial w.w; 16-byte lanes when all
// three vectors are 16-byte aligned (wide), else 8-byte
__global__ __launch_bounds__(kVecThreads) void lz_update_kernel(
    double* __restrict__ w, const double* __restrict__ v, const double* __restrict__ pv,
    int64_t n, const double* __restrict__ lzs, double* __restrict__ partials, int wide) {
  const double cy = lzs[2], cu = lzs[3], cp = lzs[4];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (!wide) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const double r = fma(cp, pv[i], fma(cu, v[i], cy * w[i]));
      w[i] = r;
      acc = fma(r, r, acc);
    }
    const double s = block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
    return;
  }
  const int64_t n2 = n / 2;
  double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
  const double2* __restrict__ v2 = reinterpret_cast<const double2*>(v);
  const double2* __restrict__ p2 = reinterpret_cast<const double2*>(pv);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 a = w2[i], b = v2[i], c = p2[i];
    double2 r;
    r.x = fma(cp, c.x, fma(cu, b.x, cy * a.x));
    r.y = fma(cp, c.y, fma(cu, b.y, cy * a.y));
    w2[i] = r;
    acc = fma(r.x, r.x, acc);
    acc = fma(r.y, r.y, acc);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    const double r = fma(cp, pv[i], fma(cu, v[i], cy * w[i]));
    w[i] = r;
    acc = fma(r, r, acc);
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// beta = sqrt(|w|^2) ; next step: v_prev = v (sP = sV), v = w (sV = 1 / beta)
__global__ void lz_beta_kernel(double* __restrict__ lzs, double* __restrict__ beta) {
  const double b = sqrt(*beta);
  *beta = b;
  lzs[1] = lzs[0];
  lzs[0] = b > 0.0 ? 1.0 / b : 0.0;
}

// The block-basis Lanczos step's scalars (lanczos_block), after step j's
// three launches: rr = |w_{j-1}|^2 (the prologue's partials; |u_0|^2 = 1 at
// j = 0), dot = u_j.Y_j (the pair launch's p.q partials).  beta_{j-1} =
// sqrt(rr), v_j = u_j / beta_{j-1} (sV), v_{j-1} = sP u_{j-1} (the previous
// sV), alpha_j = sV^2 dot, and the next prologue's w_j = A v_j - alpha_j v_j -
// beta_{j-1} v_{j-1} = cy Y_j + cu u_j + cp u_{j-1}.
// lzs: [0] sV, [1] sP, [2] cy, [3] cu, [4] cp
__global__ __launch_bounds__(1024) void lzb_step_kernel(const double* __restrict__ rr_part,
                                                        int64_t nrr,
                                                        const double* __restrict__ dot_part,
                                                        int64_t ndot, double* __restrict__ lzs,
                                                        double* __restrict__ alpha_out,
                                                        double* __restrict__ beta_out,
                                                        int first) {
  double a0 = 0.0, a1 = 0.0;
  for (int64_t i = threadIdx.x; i < nrr; i += blockDim.x) a0 += rr_part[i];
  for (int64_t i = threadIdx.x; i < ndot; i += blockDim.x) a1 += dot_part[i];
  const double rr = block_sum(a0);
  __syncthreads();
  const double dot = block_sum(a1);
  if (threadIdx.x == 0) {
    const double beta = sqrt(rr);
    if (!first) *beta_out = beta;
    const double sP = lzs[0];
    const double sV = beta > 0.0 ? 1.0 / beta : 0.0;
    const double alpha = sV * sV * dot;
    *alpha_out = alpha;
    lzs[0] = sV;
    lzs[1] = sP;
    lzs[2] = sV;
    lzs[3] = -alpha * sV;
    lzs[4] = first ? 0.0 : -beta * sP;
  }
}

// the block basis for the probe where the operator has one with d >= 3 (the
// Lanczos tridiagonal is invariant under the orthogonal fold P: the probe z
// becomes P z, the operator P K P^T); GG_LZ_BASIS=0 (snapshot) keeps the grid
static bool lanczos_use_block(const gg_kron* K) {
  const BlockOp* B = kron_block(K);
  // unpadded layouts only: the probe's workspace is 4 n (the grid's n)
  if (B == nullptr || block_d(B) < 3 || block_n(B) != kron_n(K)) return false;
  const char* e = knob("GG_LZ_BASIS");
  if (e) return atoi(e) != 0;
  return block_efficient(B);
}

// The fused Lanczos step in the parity-block basis: d - 1 launches and 10
// passes over N per step -- the first launch's prologue forms w_{j-1} = cy Y +
// cu u + cp u_prev (KIND 4: read Y, u, u_prev, write w over u_prev and the
// launch's output over Y), the plain launches 2 each, the pair launch reads
// its slab and w and writes Y_j = (K + shift) w with the u.Y partials.  One
// fold of the probe before, no unfold (only the tridiagonal leaves).
static void lanczos_block(const gg_kron* K, double shift, uint64_t seed, int probe, int steps,
                          double* work_dev, double* alphas_host, double* betas_host,
                          int* steps_done, double* step_ms, double* launch_ms,
                          gg_stream stream) {
  hipStream_t s = gg::as_stream(stream);
  const BlockOp* B = kron_block(K);
  const int64_t n = block_n(B);
  const int L = block_launches(B);
  double* P = work_dev;          // u_prev; w is written over it
  double* V = work_dev + n;      // u (v = sV u)
  double* W = work_dev + 2 * n;  // Y of the previous step (the chain runs in place on it)
  double* W2 = work_dev + 3 * n; // the pair launch's output
  const int nb = vec_blocks(n);
  const int64_t npart = std::max<int64_t>(block_partials_needed(B), kVecBlocks);
  const int64_t nrr = std::max<int64_t>(block_prologue_blocks(B), 1);
  // [alphas | betas | partials (3 x npart: p.q, r.q, q.q) | |w|^2 partials | lzs(8)]
  double* scal = nullptr;
  GG_HIP(hipMallocAsync(&scal, (2 * (size_t)steps + 3 * npart + nrr + 8) * sizeof(double), s));
  double* alphas = scal;
  double* betas = scal + steps;
  double* parts = scal + 2 * steps;
  double* rrparts = parts + 3 * npart;
  double* lzs = rrparts + nrr;
  // step 0's prologue copies u_0: w = 0 Y + 1 u + 0 u_prev (Y, u_prev zeroed)
  const double init[5] = {1.0, 0.0, 0.0, 1.0, 0.0};
  GG_HIP(hipMemcpyAsync(lzs, init, sizeof(init), hipMemcpyHostToDevice, s));
  GG_HIP(hipMemsetAsync(P, 0, n * sizeof(double), s));
  GG_HIP(hipMemsetAsync(W, 0, n * sizeof(double), s));
  // the probe (grid layout, |z| = 1) into W2, folded into V
  launch_probe(seed, probe, 1.0 / std::sqrt((double)n), W2, n, s);
  block_fold(B, false, W2, V, nullptr, s);
  const bool timed = step_ms != nullptr;
  // step boundaries, then the closing pass's end (ev[steps] -> ev[steps + 1])
  EventSet sev(timed ? (size_t)steps + 2 : 0);
  EventSet mev(timed && launch_ms ? (size_t)steps * (L + 1) : 0);
  auto mp_ev = [&](int j) -> hipEvent_t* {
    return mev.ev.empty() ? nullptr : mev.ev.data() + (size_t)j * (L + 1);
  };
  if (timed) GG_HIP(hipEventRecord(sev.ev[0], s));
  for (int j = 0; j < steps; ++j) {
    MpFuse lf;
    lf.r = V;
    lf.q_old = W;
    lf.p_out = P;
    lf.coef = lzs + 2;
    lf.rr_part = rrparts;
    lf.rr_cap = nrr;
    int64_t pro_blocks = 0;
    lf.pro_blocks = &pro_blocks;
    lf.blk_q_out = W2;
    lf.pstride = npart;
    int64_t np = 0;
    block_apply(B, P, W, shift, nullptr, parts, nullptr, s, &np, &lf, 3, mp_ev(j));
    GG_REQUIRE(pro_blocks > 0 && pro_blocks <= nrr, GG_ERR_RUNTIME,
               "Lanczos: no prologue launch recorded");
    hipLaunchKernelGGL(lzb_step_kernel, dim3(1), dim3(1024), 0, s, rrparts, pro_blocks, parts, np,
                       lzs, alphas + j, j > 0 ? betas + (j - 1) : betas, j == 0 ? 1 : 0);
    GG_LAUNCH_CHECK();
    std::swap(P, V);    // u_prev <- u_j's predecessor ... u <- w (= u_j)
    std::swap(W, W2);   // Y_j becomes the next step's chain
    if (timed && j + 1 < steps) GG_HIP(hipEventRecord(sev.ev[j + 1], s));
  }
  // the closing pass, once per probe: beta_{steps-1} = |w_{steps-1}| (one
  // streaming pass, in place of Y; T_k itself needs beta_0 .. beta_{k-2})
  if (timed) GG_HIP(hipEventRecord(sev.ev[steps], s));
  const int wide = aligned16(W) && aligned16(V) && aligned16(P);
  hipLaunchKernelGGL(lz_update_kernel, dim3(nb), dim3(kVecThreads), 0, s, W, V, P, n, lzs + 0,
                     parts, wide);
  GG_LAUNCH_CHECK();
  launch_reduce_to(parts, nb, betas + (steps - 1), s);
  hipLaunchKernelGGL(lz_beta_kernel, dim3(1), dim3(1), 0, s, lzs, betas + (steps - 1));
  GG_LAUNCH_CHECK();
  if (timed) GG_HIP(hipEventRecord(sev.ev[steps + 1], s));
  GG_HIP(hipMemcpyAsync(alphas_host, alphas, steps * sizeof(double), hipMemcpyDeviceToHost, s));
  GG_HIP(hipMemcpyAsync(betas_host, betas, steps * sizeof(double), hipMemcpyDeviceToHost, s));
  GG_HIP(hipFreeAsync(scal, s));
  GG_HIP(hipStreamSynchronize(s));
  if (timed) {
    for (int j = 0; j < steps; ++j) {
      float ms = 0.f;
      GG_HIP(hipEventElapsedTime(&ms, sev.ev[j], sev.ev[j + 1]));
      step_ms[j] = ms;
    }
    if (launch_ms) {
      const int d = kron_d(K);
      for (int k = 0; k < d; ++k) launch_ms[k] = 0.0;
      for (int j = 0; j < steps; ++j)
        for (int k = 0; k < L; ++k) {
          float ms = 0.f;
          GG_HIP(hipEventElapsedTime(&ms, mp_ev(j)[k], mp_ev(j)[k + 1]));
          launch_ms[k] += ms;
        }
      float ms = 0.f;
      GG_HIP(hipEventElapsedTime(&ms, sev.ev[steps], sev.ev[steps + 1]));
      launch_ms[d] = ms;
    }
  }
  int done = steps;
  for (int j = 0; j < steps; ++j)
    if (!(betas_host[j] > 1e-300)) {
      done = j + 1;
      break;
    }
  if (steps_done) *steps_done = done;
}

// gg_lanczos_probe / gg_lanczos_probe_timed.  step_ms (steps entries, may be
// null): HIP events on the stream at every step boundary -- the first after
// the probe is drawn, so allocation, the u_prev memset and the probe kernel
// are outside -- and the last after the final |w|^2 reduction, before the
// alphas / betas are copied back; launch_ms (d entries, may be null): the
// summed time of each mode-product position over the steps.
static void lanczos_probe(const gg_kron* K, double shift, uint64_t seed, int probe, int steps,
                          double* work_dev, double* alphas_host, double* betas_host,
                          int* steps_done, double* step_ms, double* launch_ms,
                          gg_stream stream) {
  {
    GG_REQUIRE(K && work_dev && alphas_host && betas_host && steps >= 1, GG_ERR_VALUE,
               "bad argument");
    int64_t nr = 0, nc = 0, we = 0;
    gg_kron_shape(K, 0, &nr, &nc, &we);
    GG_REQUIRE(nr == nc, GG_ERR_VALUE, "Lanczos needs a square operator");
    GG_REQUIRE(we <= nr, GG_ERR_VALUE, "non-square factors are not supported here");
    if (lanczos_use_block(K)) {
      lanczos_block(K, shift, seed, probe, steps, work_dev, alphas_host, betas_host, steps_done,
                    step_ms, launch_ms, stream);
      return;
    }
    hipStream_t s = gg::as_stream(stream);
    const int64_t n = nr;
    double* P = work_dev;        // u_prev (v_prev = sP u_prev)
    double* V = work_dev + n;    // u      (v = sV u)
    double* W = work_dev + 2 * n;
    double* mvw = work_dev + 3 * n;
    const int nb = gg::vec_blocks(n);
    const int64_t npart = std::max<int64_t>(gg::kron_partials_needed(K, false), gg::kVecBlocks);
    const int64_t nrr = std::max<int64_t>(gg::kron_prologue_blocks(K), 1);
    // [alphas | betas | partials | |w|^2 partials | zero | dot | lzs(8)]
    double* scal = nullptr;
    GG_HIP(hipMallocAsync(&scal, (2 * (size_t)steps + npart + nrr + 10 + 8) * sizeof(double), s));
    double* alphas = scal;
    double* betas = scal + steps;
    double* parts = scal + 2 * steps;
    double* rrparts = parts + npart;
    double* zero = rrparts + nrr;
    double* dot = zero + 1;
    double* lzs = dot + 1;
    const double init[2] = {1.0, 0.0};   // sV = 1 (the probe is normalised), sP = 0
    GG_HIP(hipMemsetAsync(zero, 0, sizeof(double), s));
    GG_HIP(hipMemcpyAsync(lzs, init, sizeof(init), hipMemcpyHostToDevice, s));
    GG_HIP(hipMemsetAsync(P, 0, n * sizeof(double), s));
    gg::launch_probe(seed, probe, 1.0 / std::sqrt((double)n), V, n, s);
    const int d = gg::kron_d(K);
    const bool timed = step_ms != nullptr;
    // step boundaries, then the closing pass's end (ev[steps] -> ev[steps + 1];
    // with the update fused, the last step's update pass is the closing one)
    gg::EventSet sev(timed ? (size_t)steps + 2 : 0);
    gg::EventSet mev(timed && launch_ms ? (size_t)steps * (d + 1) : 0);
    auto mp_ev = [&](int j) -> hipEvent_t* {
      return mev.ev.empty() ? nullptr : mev.ev.data() + (size_t)j * (d + 1);
    };
    if (timed) GG_HIP(hipEventRecord(sev.ev[0], s));
    // w = cy W + cu u + cp u_prev in place of W, |w|^2 -> betas[j], scales
    auto update_beta = [&](int j) {
      const int wide = gg::aligned16(W) && gg::aligned16(V) && gg::aligned16(P);
      hipLaunchKernelGGL(gg::lz_update_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, W, V, P, n,
                         lzs, parts, wide);
      GG_LAUNCH_CHECK();
      gg::launch_reduce_to(parts, nb, betas + j, s);
      hipLaunchKernelGGL(gg::lz_beta_kernel, dim3(1), dim3(1), 0, s, lzs, betas + j);
      GG_LAUNCH_CHECK();
    };
    // The update of step j - 1 rides on step j's first mode product as its
    // prologue (CGP 3: the MFMA operand is w itself, written over u_prev)
    // when the chain's first step writes its scratch, not y (an even number
    // of factors); otherwise it is its own streaming pass.
    const bool fuse = gg::kron_d(K) % 2 == 0;
    for (int j = 0; j < steps; ++j) {
      int64_t np = 0;
      if (j == 0 || !fuse) {
        // W = K u + shift u, and u.W per block of the last mode product
        gg::kron_apply(K, false, V, W, shift, mvw, parts, nullptr, s, &np, nullptr, 0, mp_ev(j));
      } else {
        gg::MpFuse lf;
        lf.r = V;
        lf.q_old = P;
        lf.p_out = P;
        lf.rr_part = rrparts;
        lf.rr_cap = nrr;
        int64_t pro_blocks = 0;
        lf.pro_blocks = &pro_blocks;
        lf.coef = lzs;
        gg::kron_apply(K, false, W, W, shift, mvw, parts, nullptr, s, &np, &lf, 3, mp_ev(j));
        GG_REQUIRE(pro_blocks > 0 && pro_blocks <= nrr, GG_ERR_RUNTIME,
                   "Lanczos: no prologue launch recorded");
        // |w|^2 of the prologue -> beta_{j-1}; w (now in P) is the new u
        gg::launch_reduce_to(rrparts, pro_blocks, betas + (j - 1), s);
        hipLaunchKernelGGL(gg::lz_beta_kernel, dim3(1), dim3(1), 0, s, lzs, betas + (j - 1));
        GG_LAUNCH_CHECK();
        std::swap(P, V);   // u_prev <- u, u <- w
      }
      gg::launch_reduce_to(parts, np, dot, s);
      const double* beta_prev = (j == 0) ? zero : betas + (j - 1);
      hipLaunchKernelGGL(gg::lz_coef_kernel, dim3(1), dim3(1), 0, s, lzs, dot, alphas + j,
                         beta_prev);
      GG_LAUNCH_CHECK();
      const bool closing = fuse && j + 1 == steps;
      if (!fuse || j + 1 == steps) {
        if (timed && closing) GG_HIP(hipEventRecord(sev.ev[steps], s));
        update_beta(j);
        if (j + 1 < steps) {
          // rotate: u_prev <- u, u <- w, the old u_prev buffer takes the next matvec
          double* oldP = P;
          P = V;
          V = W;
          W = oldP;
        }
      }
      if (timed && !closing) GG_HIP(hipEventRecord(sev.ev[j + 1], s));
    }
    if (timed) GG_HIP(hipEventRecord(sev.ev[steps + 1], s));
    GG_HIP(hipMemcpyAsync(alphas_host, alphas, steps * sizeof(double), hipMemcpyDeviceToHost,
                          s));
    GG_HIP(hipMemcpyAsync(betas_host, betas, steps * sizeof(double), hipMemcpyDeviceToHost, s));
    GG_HIP(hipFreeAsync(scal, s));
    GG_HIP(hipStreamSynchronize(s));
    if (timed) {
      for (int j = 0; j < steps; ++j) {
        float ms = 0.f;
        GG_HIP(hipEventElapsedTime(&ms, sev.ev[j], sev.ev[j + 1]));
        step_ms[j] = ms;
      }
      if (launch_ms) {
        for (int k = 0; k < d; ++k) launch_ms[k] = 0.0;
        for (int j = 0; j < steps; ++j)
          for (int k = 0; k < d; ++k) {
            float ms = 0.f;
            GG_HIP(hipEventElapsedTime(&ms, mp_ev(j)[k], mp_ev(j)[k + 1]));
            launch_ms[k] += ms;
          }
        float ms = 0.f;
        GG_HIP(hipEventElapsedTime(&ms, sev.ev[steps], sev.ev[steps + 1]));
        launch_ms[d] = ms;
      }
    }
    int done = steps;
    for (int j = 0; j < steps; ++j)
      if (!(betas_host[j] > 1e-300)) {
        done = j + 1;
        break;
      }
    if (steps_done) *steps_done = done;
  }
}

}  // namespace gg

extern "C" {

int gg_lanczos_probe(const gg_kron* K, double shift, uint64_t seed, int probe, int steps,
                     double* work_dev, double* alphas_host, double* betas_host,
                     int* steps_done, gg_stream stream) {
  return gg::guard([&] {
    gg::lanczos_probe(K, shift, seed, probe, steps, work_dev, alphas_host, betas_host,
                      steps_done, nullptr, nullptr, stream);
  });
}

int gg_lanczos_info(const gg_kron* K, int* block, int* launches) {
  return gg::guard([&] {
    GG_REQUIRE(K && block && launches, GG_ERR_VALUE, "NULL argument");
    const bool b = gg::lanczos_use_block(K);
    *block = b ? 1 : 0;
    *launches = b ? gg::block_launches(gg::kron_block(K)) : gg::kron_d(K);
  });
}

int gg_lanczos_probe_timed(const gg_kron* K, double shift, uint64_t seed, int probe, int steps,
                           double* work_dev, double* alphas_host, double* betas_host,
                           int* steps_done, double* step_ms_host, double* launch_ms_host,
                           gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(step_ms_host != nullptr, GG_ERR_VALUE, "step_ms_host is NULL");
    gg::lanczos_probe(K, shift, seed, probe, steps, work_dev, alphas_host, betas_host,
                      steps_done, step_ms_host, launch_ms_host, stream);
  });
}

}  // extern "C"
