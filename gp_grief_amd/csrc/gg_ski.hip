// Structured kernel interpolation on a Kronecker grid (gg_ski_*, gg_skicg_*):
// the covariance of n scattered points is W K W^T, W the sparse n x N matrix of
// local interpolation weights (Wilson & Nickisch 2015) -- order^d entries per
// row, the tensor product of per-axis stencils: Keys' cubic convolution
// (order 4) or linear (order 2).  W is never stored by rows:
//   stencils  per point and axis the first node (int32) and `order` weights
//   interp    t = W g: every point forms its weights on the fly from the
//             per-axis tables and reads order^(d-1) runs of `order` contiguous
//             doubles along axis 0 (input dimension 0 is fastest)
//   spread    g = W^T p without atomics, through an inverted index built once
//             per (X, grid): the n order^d (node, point, weight product)
//             triples sorted stably by node, an int64 row pointer of N + 1
//             entries.  Eight lanes share a node and add in a fixed order, so
//             every node is written exactly once (0 for an empty row) and the
//             result is bitwise reproducible.  Rows longer than `split`
//             entries (clustered data) are cut into chunks summed by one wave
//             each; a last kernel adds each such row's partial sums in chunk
//             order.
// The CG (gg_skicg_*) solves (W K W^T + shift I) x = b on vectors of length n:
//   direction p = r + beta p, spread, gg::kron_apply (shift 0, grid basis),
//   interp with + shift p and the partials of p.t, alpha, the x / r update of
//   gg_vec.hip with the r.r partials, rho / beta / stopping test.
// Scalars stay on the device (CgScalars), the host polls `done`, and every
// kernel returns early once it is set.  alpha_j and beta_j of every iteration
// are recorded: the Lanczos tridiagonal of the same Krylov space follows from
// them (T_jj = 1 / alpha_j + beta_{j-1} / alpha_{j-1}, T_{j,j+1} = sqrt(beta_j) /
// alpha_j), so one driver serves the solve and the SLQ log det.
#include <cmath>
#include <vector>

#include "gg_internal.h"

namespace gg {

constexpr int kSkiMaxD = 8;
constexpr int kSkiMaxNnzRow = 256;     // order^d
constexpr int kSkiThreads = 256;
constexpr int kSkiRowLanes = 8;        // lanes that share a node in the spread
constexpr double kSkiEdgeTol = 1e-10;  // cells: (x - lo) / h this close to an edge is on it

struct SkiGrid {
  int d;
  int64_t m[kSkiMaxD];
  int64_t stride[kSkiMaxD];   // prod_{e < f} m_e
  double lo[kSkiMaxD];
  double h[kSkiMaxD];
};

template <int ORDER>
__device__ __forceinline__ void ski_weights(double t, double* w) {
  if (ORDER == 4) {
    w[0] = 0.5 * (((-t + 2.0) * t - 1.0) * t);
    w[1] = 0.5 * ((3.0 * t - 5.0) * t * t + 2.0);
    w[2] = 0.5 * (((-3.0 * t + 4.0) * t + 1.0) * t);
    w[3] = 0.5 * ((t - 1.0) * t * t);
  } else {
    w[0] = 1.0 - t;
    w[1] = t;
  }
}

// one thread per point.  WRITE = false: count the points outside the domain
// (one atomic per such point, on an integer counter: the count does not
// depend on the order) and write nothing else.  WRITE = true: the tables.
template <int ORDER, bool WRITE>
__global__ __launch_bounds__(kSkiThreads) void ski_stencil_kernel(
    SkiGrid G, const double* __restrict__ X, int64_t n, int32_t* __restrict__ first,
    double* __restrict__ w, unsigned long long* __restrict__ outside) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double ulo = ORDER == 4 ? 1.0 : 0.0;
  bool out = false;
  for (int f = 0; f < G.d; ++f) {
    const double uhi = (double)(G.m[f] - 1) - ulo;
    double u = (X[i * G.d + f] - G.lo[f]) / G.h[f];
    if (!(u >= ulo - kSkiEdgeTol && u <= uhi + kSkiEdgeTol)) out = true;   // also NaN
    if (WRITE) {
      u = fmin(fmax(u, ulo), uhi);
      const int64_t jmax = G.m[f] - (ORDER == 4 ? 3 : 2);
      int64_t j = (int64_t)floor(u);
      j = j < (int64_t)ulo ? (int64_t)ulo : (j > jmax ? jmax : j);
      double wt[ORDER];
      ski_weights<ORDER>(u - (double)j, wt);
      first[i * G.d + f] = (int32_t)(j - (ORDER == 4 ? 1 : 0));
#pragma unroll
      for (int k = 0; k < ORDER; ++k) w[(i * G.d + f) * ORDER + k] = wt[k];
    }
  }
  if (!WRITE && out) atomicAdd(outside, 1ull);
}

// one thread per entry e = i * S + c, S = ORDER^d; digit f of c (base ORDER,
// axis 0 lowest) is the entry's offset along axis f
template <int ORDER>
__global__ __launch_bounds__(kSkiThreads) void ski_expand_kernel(
    SkiGrid G, const int32_t* __restrict__ first, const double* __restrict__ w, int64_t n,
    int S, int64_t* __restrict__ node, double* __restrict__ wprod) {
  constexpr int LOG = ORDER == 4 ? 2 : 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * S) return;
  const int64_t i = e / S;
  const int c = (int)(e - i * S);
  int64_t nd = 0;
  double wp = 1.0;
  for (int f = G.d - 1; f >= 0; --f) {
    const int dg = (c >> (LOG * f)) & (ORDER - 1);
    nd += ((int64_t)first[i * G.d + f] + dg) * G.stride[f];
    wp *= w[(i * G.d + f) * ORDER + dg];
  }
  node[e] = nd;
  wprod[e] = wp;
}

// t = W g (+ shift p and the block partials of p.t: the CG's p.A p)
template <int ORDER, bool CG>
__global__ __launch_bounds__(kSkiThreads) void ski_interp_kernel(
    SkiGrid G, const int32_t* __restrict__ first, const double* __restrict__ w,
    const double* __restrict__ g, double* __restrict__ t, int64_t n, double shift,
    const double* __restrict__ p, const CgScalars* __restrict__ sc,
    double* __restrict__ partials) {
  constexpr int LOG = ORDER == 4 ? 2 : 1;
  if (CG && sc->done) return;
  const int d = G.d;
  const int combos = 1 << (LOG * (d - 1));
  double dot = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t* fi = first + i * d;
    const double* wi = w + i * d * ORDER;
    double w0[ORDER];
#pragma unroll
    for (int k = 0; k < ORDER; ++k) w0[k] = wi[k];
    int64_t base = fi[0];
    for (int f = 1; f < d; ++f) base += (int64_t)fi[f] * G.stride[f];
    double acc = 0.0;
    for (int c = 0; c < combos; ++c) {
      int64_t off = base;
      double wp = 1.0;
      for (int f = d - 1; f >= 1; --f) {
        const int dg = (c >> (LOG * (f - 1))) & (ORDER - 1);
        off += dg * G.stride[f];
        wp *= wi[f * ORDER + dg];
      }
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < ORDER; ++k) s = fma(w0[k], g[off + k], s);
      acc = fma(wp, s, acc);
    }
    if (CG) {
      const double pv = p[i];
      acc = fma(shift, pv, acc);
      dot = fma(pv, acc, dot);
    }
    t[i] = acc;
  }
  if (CG) {
    const double s = block_sum(dot);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
  }
}

// g = W^T p over the rows of at most `split` entries: kSkiRowLanes lanes per
// node, a fixed butterfly over them
__global__ __launch_bounds__(kSkiThreads) void ski_spread_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ pt,
    const double* __restrict__ wv, const double* __restrict__ p, double* __restrict__ g,
    int64_t N, int64_t split, const int* __restrict__ skip) {
  if (skip != nullptr && *skip) return;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t node = tid / kSkiRowLanes;
  const int lane = (int)(tid % kSkiRowLanes);
  const bool valid = node < N;
  int64_t b = 0, e = 0;
  bool is_long = false;
  if (valid) {
    b = ptr[node];
    e = ptr[node + 1];
    is_long = e - b > split;
    if (is_long) e = b;
  }
  double acc = 0.0;
  for (int64_t j = b + lane; j < e; j += kSkiRowLanes) acc = fma(wv[j], p[pt[j]], acc);
#pragma unroll
  for (int off = kSkiRowLanes / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (valid && lane == 0 && !is_long) g[node] = acc;
}

// one wave per chunk [cb[c], ce[c]) of a long row
__global__ __launch_bounds__(kWave) void ski_spread_chunk_kernel(
    const int64_t* __restrict__ cb, const int64_t* __restrict__ ce,
    const int32_t* __restrict__ pt, const double* __restrict__ wv,
    const double* __restrict__ p, double* __restrict__ cpart, const int* __restrict__ skip) {
  if (skip != nullptr && *skip) return;
  const int64_t c = blockIdx.x;
  const int64_t e = ce[c];
  double acc = 0.0;
  for (int64_t j = cb[c] + threadIdx.x; j < e; j += kWave) acc = fma(wv[j], p[pt[j]], acc);
  acc = wave_sum(acc);
  if (threadIdx.x == 0) cpart[c] = acc;
}

// long row l: its chunks' partial sums, in chunk order
__global__ __launch_bounds__(kSkiThreads) void ski_spread_long_kernel(
    const int64_t* __restrict__ long_node, const int64_t* __restrict__ coff,
    const double* __restrict__ cpart, double* __restrict__ g, int64_t nlong,
    const int* __restrict__ skip) {
  if (skip != nullptr && *skip) return;
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlong) return;
  double acc = 0.0;
  for (int64_t c = coff[l]; c < coff[l + 1]; ++c) acc += cpart[c];
  g[long_node[l]] = acc;
}

// p = r + beta p (p = r on the first iteration)
__global__ __launch_bounds__(kVecThreads) void skicg_direction_kernel(
    double* __restrict__ p, const double* __restrict__ r, int64_t n,
    const CgScalars* __restrict__ sc) {
  if (sc->done) return;
  const bool first = sc->first != 0;
  const double beta = sc->beta;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    p[i] = first ? r[i] : fma(beta, p[i], r[i]);
}

// r = b ; x = 0 ; partial r.r
__global__ __launch_bounds__(kVecThreads) void skicg_start_kernel(
    const double* __restrict__ b, double* __restrict__ x, double* __restrict__ r, int64_t n,
    double* __restrict__ partials) {
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double bv = b[i];
    r[i] = bv;
    x[i] = 0.0;
    acc = fma(bv, bv, acc);
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// after cg_rho_kernel: keep (alpha, beta) of an iteration that just completed
__global__ void skicg_record_kernel(const CgScalars* __restrict__ sc, int* __restrict__ recorded,
                                    double* __restrict__ coef, int max_steps) {
  const int k = *recorded;
  if (sc->iters <= k) return;   // nothing ran (done was already set)
  if (k < max_steps) {
    coef[2 * k] = sc->alpha;
    coef[2 * k + 1] = sc->beta;
  }
  *recorded = sc->iters;
}

static SkiGrid ski_grid(int d, const int64_t* m, int order, const double* lo, const double* h) {
  GG_REQUIRE(order == 2 || order == 4, GG_ERR_VALUE,
             "interpolation order must be 2 (linear) or 4 (cubic)");
  GG_REQUIRE(m != nullptr, GG_ERR_VALUE, "NULL argument");
  GG_REQUIRE(d >= 1 && d <= kSkiMaxD, GG_ERR_VALUE, "1 <= d <= 8 axes supported");
  int64_t S = 1;
  for (int f = 0; f < d; ++f) S *= order;
  GG_REQUIRE(S <= kSkiMaxNnzRow, GG_ERR_VALUE,
             "order^d must be <= 256 (cubic up to d = 4, linear up to d = 8)");
  SkiGrid G{};
  G.d = d;
  int64_t st = 1;
  for (int f = 0; f < d; ++f) {
    GG_REQUIRE(m[f] >= order, GG_ERR_VALUE,
               "every axis needs at least `order` nodes (cubic 4, linear 2)");
    GG_REQUIRE(m[f] < (int64_t(1) << 31), GG_ERR_VALUE, "axis too long");
    GG_REQUIRE(st <= (int64_t(1) << 62) / m[f], GG_ERR_VALUE, "grid too large (N overflows)");
    G.m[f] = m[f];
    G.stride[f] = st;
    st *= m[f];
    if (lo != nullptr) {
      GG_REQUIRE(h[f] > 0.0 && std::isfinite(h[f]) && std::isfinite(lo[f]), GG_ERR_VALUE,
                 "the grid spacing must be positive and finite");
      G.lo[f] = lo[f];
      G.h[f] = h[f];
    }
  }
  return G;
}

static int ski_row_nnz(const SkiGrid& G, int order) {
  int S = 1;
  for (int f = 0; f < G.d; ++f) S *= order;
  return S;
}

}  // namespace gg

struct gg_ski {
  gg::SkiGrid G{};
  int order = 0;
  int64_t n = 0, N = 0, nnz = 0;
  const int32_t* first = nullptr;
  const double* w = nullptr;
  const int64_t* ptr = nullptr;
  const int32_t* pt = nullptr;
  const double* wv = nullptr;
  int64_t split = 0, nlong = 0, nchunks = 0;
  const int64_t *long_node = nullptr, *coff = nullptr, *cb = nullptr, *ce = nullptr;
  double* cpart = nullptr;
};

namespace gg {

static int ski_interp_blocks(int64_t n) {
  return (int)std::min<int64_t>(kVecBlocks, std::max<int64_t>(ceil_div(n, kSkiThreads), 1));
}

// t = W g; p != nullptr: the CG's variant
static void ski_interp(const gg_ski* W, const double* g, double* t, double shift, const double* p,
                       const CgScalars* sc, double* partials, hipStream_t s) {
  const int nb = ski_interp_blocks(W->n);
  const dim3 grid(nb), block(kSkiThreads);
  if (p == nullptr) {
    if (W->order == 4)
      hipLaunchKernelGGL((ski_interp_kernel<4, false>), grid, block, 0, s, W->G, W->first, W->w,
                         g, t, W->n, 0.0, (const double*)nullptr, (const CgScalars*)nullptr,
                         (double*)nullptr);
    else
      hipLaunchKernelGGL((ski_interp_kernel<2, false>), grid, block, 0, s, W->G, W->first, W->w,
                         g, t, W->n, 0.0, (const double*)nullptr, (const CgScalars*)nullptr,
                         (double*)nullptr);
  } else {
    if (W->order == 4)
      hipLaunchKernelGGL((ski_interp_kernel<4, true>), grid, block, 0, s, W->G, W->first, W->w, g,
                         t, W->n, shift, p, sc, partials);
    else
      hipLaunchKernelGGL((ski_interp_kernel<2, true>), grid, block, 0, s, W->G, W->first, W->w, g,
                         t, W->n, shift, p, sc, partials);
  }
  GG_LAUNCH_CHECK();
}

static void ski_spread(const gg_ski* W, const double* p, double* g, const int* skip,
                       hipStream_t s) {
  const int64_t blocks = ceil_div(W->N * kSkiRowLanes, kSkiThreads);
  GG_REQUIRE(blocks < (int64_t(1) << 31), GG_ERR_VALUE, "grid too large for the spread");
  hipLaunchKernelGGL(ski_spread_kernel, dim3((unsigned)blocks), dim3(kSkiThreads), 0, s, W->ptr,
                     W->pt, W->wv, p, g, W->N, W->split, skip);
  GG_LAUNCH_CHECK();
  if (W->nlong == 0) return;
  hipLaunchKernelGGL(ski_spread_chunk_kernel, dim3((unsigned)W->nchunks), dim3(kWave), 0, s,
                     W->cb, W->ce, W->pt, W->wv, p, W->cpart, skip);
  GG_LAUNCH_CHECK();
  hipLaunchKernelGGL(ski_spread_long_kernel, dim3((unsigned)ceil_div(W->nlong, kSkiThreads)),
                     dim3(kSkiThreads), 0, s, W->long_node, W->coff, W->cpart, g, W->nlong, skip);
  GG_LAUNCH_CHECK();
}

static int64_t skicg_vec_stride(int64_t n) { return (n + 31) / 32 * 32; }
constexpr int64_t kSkicgAlignSlack = 32;   // doubles: room to round the base up to 256 B

}  // namespace gg

struct gg_skicg {
  const gg_kron* K = nullptr;
  const gg_ski* W = nullptr;
  double shift = 0.0;
  int64_t n = 0, N = 0;
  double *r = nullptr, *p = nullptr, *t = nullptr, *gp = nullptr, *gq = nullptr,
         *mv_work = nullptr;
  double* partials = nullptr;          // device, kVecBlocks
  gg::CgScalars* sc = nullptr;         // device
  gg::CgScalars* sc_host = nullptr;    // pinned mirror
  int max_steps = 0;
  double* coef = nullptr;              // device: (alpha_j, beta_j), max_steps pairs
  int* recorded = nullptr;             // device: iterations seen by the recorder
  double* x = nullptr;
};

extern "C" {

int gg_ski_stencils(int d, const int64_t* m, const double* lo, const double* h, int order,
                    const double* X_dev, int64_t n, int32_t* first_dev, double* w_dev,
                    int64_t* n_outside, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(lo && h && X_dev && first_dev && w_dev, GG_ERR_VALUE, "NULL argument");
    const gg::SkiGrid G = gg::ski_grid(d, m, order, lo, h);
    GG_REQUIRE(n >= 1 && n < (int64_t(1) << 31), GG_ERR_VALUE, "1 <= n < 2^31 points supported");
    hipStream_t s = gg::as_stream(stream);
    unsigned long long* cnt = nullptr;
    GG_HIP(hipMalloc(&cnt, sizeof *cnt));
    unsigned long long out = 0;
    try {
      GG_HIP(hipMemsetAsync(cnt, 0, sizeof *cnt, s));
      const dim3 grid((unsigned)gg::ceil_div(n, gg::kSkiThreads)), block(gg::kSkiThreads);
      if (order == 4)
        hipLaunchKernelGGL((gg::ski_stencil_kernel<4, false>), grid, block, 0, s, G, X_dev, n,
                           first_dev, w_dev, cnt);
      else
        hipLaunchKernelGGL((gg::ski_stencil_kernel<2, false>), grid, block, 0, s, G, X_dev, n,
                           first_dev, w_dev, cnt);
      GG_LAUNCH_CHECK();
      GG_HIP(hipMemcpyAsync(&out, cnt, sizeof out, hipMemcpyDeviceToHost, s));
      GG_HIP(hipStreamSynchronize(s));
      if (n_outside) *n_outside = (int64_t)out;
      if (out == 0) {
        if (order == 4)
          hipLaunchKernelGGL((gg::ski_stencil_kernel<4, true>), grid, block, 0, s, G, X_dev, n,
                             first_dev, w_dev, cnt);
        else
          hipLaunchKernelGGL((gg::ski_stencil_kernel<2, true>), grid, block, 0, s, G, X_dev, n,
                             first_dev, w_dev, cnt);
        GG_LAUNCH_CHECK();
      }
    } catch (...) {
      (void)hipFree(cnt);
      throw;
    }
    (void)hipFree(cnt);
    GG_REQUIRE(out == 0, GG_ERR_VALUE,
               std::to_string(out) + " point(s) outside the interpolation domain (cubic: one "
               "cell inside the grid's ends; linear: the grid's ends); pad the grid");
  });
}

int gg_ski_expand(int d, const int64_t* m, int order, int64_t n, const int32_t* first_dev,
                  const double* w_dev, int64_t* node_dev, double* wprod_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(first_dev && w_dev && node_dev && wprod_dev, GG_ERR_VALUE, "NULL argument");
    const gg::SkiGrid G = gg::ski_grid(d, m, order, nullptr, nullptr);
    GG_REQUIRE(n >= 1 && n < (int64_t(1) << 31), GG_ERR_VALUE, "1 <= n < 2^31 points supported");
    const int S = gg::ski_row_nnz(G, order);
    const int64_t blocks = gg::ceil_div(n * S, gg::kSkiThreads);
    GG_REQUIRE(blocks < (int64_t(1) << 31), GG_ERR_VALUE, "too many entries");
    const dim3 grid((unsigned)blocks), block(gg::kSkiThreads);
    hipStream_t s = gg::as_stream(stream);
    if (order == 4)
      hipLaunchKernelGGL((gg::ski_expand_kernel<4>), grid, block, 0, s, G, first_dev, w_dev, n, S,
                         node_dev, wprod_dev);
    else
      hipLaunchKernelGGL((gg::ski_expand_kernel<2>), grid, block, 0, s, G, first_dev, w_dev, n, S,
                         node_dev, wprod_dev);
    GG_LAUNCH_CHECK();
  });
}

int gg_ski_destroy(gg_ski* W) {
  return gg::guard([&] { delete W; });
}

int gg_ski_create(int d, const int64_t* m, int order, int64_t n, const int32_t* first_dev,
                  const double* w_dev, const int64_t* rowptr_dev, const int32_t* point_dev,
                  const double* wprod_dev, int64_t split, int64_t nlong,
                  const int64_t* long_node_dev, const int64_t* chunk_off_dev, int64_t nchunks,
                  const int64_t* chunk_begin_dev, const int64_t* chunk_end_dev,
                  double* chunk_sum_dev, gg_ski** out) {
  return gg::guard([&] {
    GG_REQUIRE(first_dev && w_dev && rowptr_dev && point_dev && wprod_dev && out, GG_ERR_VALUE,
               "NULL argument");
    const gg::SkiGrid G = gg::ski_grid(d, m, order, nullptr, nullptr);
    GG_REQUIRE(n >= 1 && n < (int64_t(1) << 31), GG_ERR_VALUE, "1 <= n < 2^31 points supported");
    GG_REQUIRE(split >= 1 && nlong >= 0 && nchunks >= 0, GG_ERR_VALUE,
               "split >= 1, nlong >= 0 and nchunks >= 0 required");
    GG_REQUIRE((nlong == 0) == (nchunks == 0) && nchunks < (int64_t(1) << 31), GG_ERR_VALUE,
               "long rows and their chunks come together");
    if (nlong > 0)
      GG_REQUIRE(long_node_dev && chunk_off_dev && chunk_begin_dev && chunk_end_dev &&
                     chunk_sum_dev,
                 GG_ERR_VALUE, "NULL argument (long rows)");
    gg_ski* W = new gg_ski();
    W->G = G;
    W->order = order;
    W->n = n;
    W->N = G.stride[d - 1] * G.m[d - 1];
    W->nnz = n * gg::ski_row_nnz(G, order);
    W->first = first_dev;
    W->w = w_dev;
    W->ptr = rowptr_dev;
    W->pt = point_dev;
    W->wv = wprod_dev;
    W->split = split;
    W->nlong = nlong;
    W->nchunks = nchunks;
    W->long_node = long_node_dev;
    W->coff = chunk_off_dev;
    W->cb = chunk_begin_dev;
    W->ce = chunk_end_dev;
    W->cpart = chunk_sum_dev;
    *out = W;
  });
}

int gg_ski_interp(const gg_ski* W, const double* g_dev, double* t_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(W && g_dev && t_dev, GG_ERR_VALUE, "NULL argument");
    gg::ski_interp(W, g_dev, t_dev, 0.0, nullptr, nullptr, nullptr, gg::as_stream(stream));
  });
}

int gg_ski_spread(const gg_ski* W, const double* p_dev, double* g_dev, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(W && p_dev && g_dev, GG_ERR_VALUE, "NULL argument");
    gg::ski_spread(W, p_dev, g_dev, nullptr, gg::as_stream(stream));
  });
}

int gg_skicg_work_elems(const gg_kron* K, const gg_ski* W, int64_t* elems) {
  return gg::guard([&] {
    GG_REQUIRE(K && W && elems, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(gg::kron_n(K) == W->N, GG_ERR_VALUE,
               "the operator and the interpolation grid differ in size");
    // r, p, t over the points; W^T p, K W^T p over the grid; the matvec scratch
    *elems = gg::kSkicgAlignSlack + 3 * gg::skicg_vec_stride(W->n) +
             2 * gg::skicg_vec_stride(W->N) + gg::kron_work_elems(K, false);
  });
}

int gg_skicg_destroy(gg_skicg* c) {
  return gg::guard([&] {
    if (!c) return;
    if (c->partials) (void)hipFree(c->partials);
    if (c->sc) (void)hipFree(c->sc);
    if (c->coef) (void)hipFree(c->coef);
    if (c->recorded) (void)hipFree(c->recorded);
    if (c->sc_host) (void)hipHostFree(c->sc_host);
    delete c;
  });
}

int gg_skicg_create(const gg_kron* K, const gg_ski* W, double shift, double* work_dev,
                    int max_steps, gg_skicg** out) {
  return gg::guard([&] {
    GG_REQUIRE(K && W && work_dev && out, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(shift > 0.0, GG_ERR_VALUE,
               "the SKI CG needs shift > 0 (W K W^T alone may be singular)");
    GG_REQUIRE(max_steps >= 0, GG_ERR_VALUE, "max_steps must be >= 0");
    int64_t nr = 0, nc = 0, we = 0;
    gg::check_status(gg_kron_shape(K, 0, &nr, &nc, &we));
    GG_REQUIRE(nr == nc, GG_ERR_VALUE, "CG needs a square operator");
    GG_REQUIRE(nr == W->N, GG_ERR_VALUE,
               "the operator and the interpolation grid differ in size");
    GG_REQUIRE((reinterpret_cast<uintptr_t>(work_dev) & 7) == 0, GG_ERR_VALUE,
               "the CG workspace must hold doubles (8-byte aligned)");
    gg_skicg* c = new gg_skicg();
    try {
      c->K = K;
      c->W = W;
      c->shift = shift;
      c->n = W->n;
      c->N = W->N;
      const int64_t vn = gg::skicg_vec_stride(c->n), vN = gg::skicg_vec_stride(c->N);
      work_dev = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work_dev) + 255) &
                                           ~static_cast<uintptr_t>(255));
      c->r = work_dev;
      c->p = work_dev + vn;
      c->t = work_dev + 2 * vn;
      c->gp = work_dev + 3 * vn;
      c->gq = c->gp + vN;
      c->mv_work = c->gq + vN;
      c->max_steps = max_steps;
      GG_HIP(hipMalloc(&c->partials, gg::kVecBlocks * sizeof(double)));
      GG_HIP(hipMalloc(&c->sc, sizeof(gg::CgScalars)));
      GG_HIP(hipMemset(c->sc, 0, sizeof(gg::CgScalars)));
      GG_HIP(hipMalloc(&c->coef, (size_t)std::max(max_steps, 1) * 2 * sizeof(double)));
      GG_HIP(hipMalloc(&c->recorded, sizeof(int)));
      GG_HIP(hipMemset(c->recorded, 0, sizeof(int)));
      GG_HIP(hipHostMalloc(&c->sc_host, sizeof(gg::CgScalars), hipHostMallocDefault));
    } catch (...) {
      gg_skicg_destroy(c);
      throw;
    }
    *out = c;
  });
}

int gg_skicg_start(gg_skicg* c, const double* b_dev, double* x_dev, double rtol, double atol,
                   gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && b_dev && x_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(rtol >= 0 && atol >= 0, GG_ERR_VALUE,
               "tolerances must be real, non-negative numbers");
    GG_REQUIRE(gg::aligned16(x_dev), GG_ERR_VALUE, "x_dev must be 16-byte aligned");
    hipStream_t s = gg::as_stream(stream);
    c->x = x_dev;
    const int nb = gg::vec_blocks(c->n);
    hipLaunchKernelGGL(gg::skicg_start_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, b_dev,
                       x_dev, c->r, c->n, c->partials);
    GG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gg::cg_init_kernel, dim3(1), dim3(1024), 0, s, c->partials, (int64_t)nb,
                       c->sc, rtol, atol);
    GG_LAUNCH_CHECK();
    GG_HIP(hipMemsetAsync(c->recorded, 0, sizeof(int), s));
  });
}

int gg_skicg_iterate(gg_skicg* c, int max_iters, int check_every, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && c->x, GG_ERR_VALUE, "CG not started");
    hipStream_t s = gg::as_stream(stream);
    const int64_t n = c->n;
    const int nb = gg::vec_blocks(n);
    const int nbi = gg::ski_interp_blocks(n);
    if (check_every <= 0) check_every = max_iters;
    for (int it = 0; it < max_iters; ++it) {
      hipLaunchKernelGGL(gg::skicg_direction_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, c->p,
                         c->r, n, c->sc);
      GG_LAUNCH_CHECK();
      gg::ski_spread(c->W, c->p, c->gp, &c->sc->done, s);
      gg::kron_apply(c->K, false, c->gp, c->gq, 0.0, c->mv_work, nullptr, &c->sc->done, s,
                     nullptr, nullptr, 0, nullptr);
      gg::ski_interp(c->W, c->gq, c->t, c->shift, c->p, c->sc, c->partials, s);
      hipLaunchKernelGGL(gg::cg_alpha_kernel, dim3(1), dim3(1024), 0, s, c->partials,
                         (int64_t)nbi, c->sc);
      GG_LAUNCH_CHECK();
      hipLaunchKernelGGL(gg::cg_xr_update_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, c->x,
                         c->r, c->p, c->t, n, c->sc, c->partials, 0);
      GG_LAUNCH_CHECK();
      hipLaunchKernelGGL(gg::cg_rho_kernel, dim3(1), dim3(1024), 0, s, c->partials, (int64_t)nb,
                         c->sc, 0);
      GG_LAUNCH_CHECK();
      hipLaunchKernelGGL(gg::skicg_record_kernel, dim3(1), dim3(1), 0, s, c->sc, c->recorded,
                         c->coef, c->max_steps);
      GG_LAUNCH_CHECK();
      if ((it + 1) % check_every == 0 && it + 1 < max_iters) {
        GG_HIP(hipMemcpyAsync(c->sc_host, c->sc, sizeof(gg::CgScalars), hipMemcpyDeviceToHost,
                              s));
        GG_HIP(hipStreamSynchronize(s));
        if (c->sc_host->done) break;
      }
    }
  });
}

int gg_skicg_status(gg_skicg* c, int* iters, int* converged, double* resid_norm, double* tol,
                    gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c, GG_ERR_VALUE, "NULL handle");
    hipStream_t s = gg::as_stream(stream);
    GG_HIP(hipMemcpyAsync(c->sc_host, c->sc, sizeof(gg::CgScalars), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    const gg::CgScalars& h = *c->sc_host;
    if (iters) *iters = h.iters;
    // a created, unstarted handle holds zeroed scalars (bnorm == 0): not converged
    if (converged)
      *converged = c->x != nullptr && ((h.done && std::sqrt(h.rho) < h.tol) || h.bnorm == 0.0);
    if (resid_norm) *resid_norm = std::sqrt(h.rho);
    if (tol) *tol = h.tol;
  });
}

int gg_skicg_coefficients(gg_skicg* c, int k, double* alphas, double* betas, int* k_out,
                          gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(c && k_out, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(k >= 0, GG_ERR_VALUE, "k must be >= 0");
    GG_REQUIRE(k == 0 || (alphas && betas), GG_ERR_VALUE, "NULL argument");
    hipStream_t s = gg::as_stream(stream);
    int rec = 0;
    GG_HIP(hipMemcpyAsync(&rec, c->recorded, sizeof(int), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    const int have = std::min(std::min(rec, c->max_steps), k);
    if (have > 0) {
      std::vector<double> buf(2 * (size_t)have);
      GG_HIP(hipMemcpyAsync(buf.data(), c->coef, buf.size() * sizeof(double),
                            hipMemcpyDeviceToHost, s));
      GG_HIP(hipStreamSynchronize(s));
      for (int j = 0; j < have; ++j) {
        alphas[j] = buf[2 * j];
        betas[j] = buf[2 * j + 1];
      }
    }
    *k_out = have;
  });
}

}  // extern "C"
