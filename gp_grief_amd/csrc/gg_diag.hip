// Element-wise and diagonal kernels of the models: row scaling, the divide by
// a precomputed diagonal, the Rademacher probe, and everything that walks the
// Kronecker eigenvalue diagonal (scale / divide / posterior variance, log det,
// the LML gradient's trace pass) -- with their C ABI.
#include <cmath>

#include "gg_internal.h"

namespace gg {

// A[i][j] *= w[i] (mode 0) or /= w[i] (mode 1); square (mode 2): A = A * A
__global__ __launch_bounds__(kVecThreads) void scale_rows_kernel(double* __restrict__ A,
                                                                 int64_t rows, int64_t cols,
                                                                 const double* __restrict__ w,
                                                                 int mode) {
  const int64_t total = rows * cols;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const double a = A[e];
    if (mode == 2) {
      A[e] = a * a;
    } else {
      const double s = w[e / cols];
      A[e] = mode == 0 ? a * s : a / s;
    }
  }
}

__global__ __launch_bounds__(kVecThreads) void diag_divide_kernel(const double* __restrict__ t,
                                                                  double shift,
                                                                  const double* __restrict__ x,
                                                                  double* __restrict__ y,
                                                                  int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    y[i] = x[i] / (t[i] + shift);
}

// Rademacher probe, bit-identical to oracle/cg.py probe_signs (splitmix64;
// probe_mix: gg_internal.h)
__global__ __launch_bounds__(kVecThreads) void probe_kernel(uint64_t base, double scale,
                                                            double* __restrict__ z, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t h = probe_mix(base + (uint64_t)i * 0x9E3779B97F4A7C15ull);
    z[i] = (h >> 63) == 0 ? scale : -scale;
  }
}

static uint64_t probe_base(uint64_t seed, int probe) {
  return (((seed & 0xffffffffull) << 32) ^ (((uint64_t)probe & 0xffffull) << 16) ^
          0x9E3779B97F4A7C15ull);
}

// the Lanczos drivers' start vector (gg_probe_fill's grid is vec_blocks(2 n))
void launch_probe(uint64_t seed, int probe, double scale, double* z, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(probe_kernel, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s,
                     probe_base(seed, probe), scale, z, n);
  GG_LAUNCH_CHECK();
}

// ----------------------------------------------- Kronecker eigenvalue diagonal
// (KronDiag, make_diag: gg_internal.h, shared with gg_sample.hip)
__device__ __forceinline__ double kron_eig_at(const KronDiag& kd, const double* lam, int64_t i) {
  double t = 1.0;
  for (int k = kd.d - 1; k >= 0; --k) {
    const int64_t ik = i % kd.m[k];
    i /= kd.m[k];
    t *= lam[kd.off[k] + ik];
  }
  return t;
}

__global__ __launch_bounds__(kVecThreads) void diag_scale_kernel(KronDiag kd,
                                                                 const double* __restrict__ lam,
                                                                 double shift, int mode,
                                                                 const double* __restrict__ x,
                                                                 double* __restrict__ y,
                                                                 int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double t = kron_eig_at(kd, lam, i);
    double v;
    if (mode == GG_DIAG_DIVIDE)
      v = x[i] / (t + shift);
    else if (mode == GG_DIAG_POSTVAR)
      v = t * shift / (t + shift);
    else
      v = x[i] * (t + shift);
    y[i] = v;
  }
}

__global__ __launch_bounds__(kVecThreads) void logdet_kernel(KronDiag kd,
                                                             const double* __restrict__ lam,
                                                             double shift, int64_t n,
                                                             double* __restrict__ partials) {
  // the last factor varies fastest: decode the head once per run of m_last
  const int64_t ml = kd.m[kd.d - 1];
  const double* lastl = lam + kd.off[kd.d - 1];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t h = i / ml;
    const int64_t l = i - h * ml;
    double t = lastl[l];
    int64_t hh = h;
    for (int k = kd.d - 2; k >= 0; --k) {
      const int64_t ik = hh % kd.m[k];
      hh /= kd.m[k];
      t *= lam[kd.off[k] + ik];
    }
    acc += log(t + shift);
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------- trace pass of the LML gradient
// out[p] = sum_g prod_f num[p][off_f + g_f] / (prod_f lam[off_f + g_f] + shift).
// A work item is (head index, segment of the last factor): the head -- every
// factor but the last -- is decoded once per item, its eigenvalue product and
// the kPC head numerators of this block's row chunk (blockIdx.y) stay in
// registers, and the run over the segment is one FMA and one reciprocal per
// grid point, shared by the kPC accumulators (a multiply and an FMA each).
// No memory stream: the operands are the (P + 1) sum_f m_f table entries.
// kIdx is uint32_t wherever N < 2^31 (the decode's divisions are the cost of
// an item), int64_t beyond.  partials: P rows of gridDim.x.
constexpr int kTraceRows = 8;    // rows of num per block (register accumulators)
constexpr int kTraceSeg = 16;    // shortest segment worth a head decode
constexpr int kTraceSegMax = 128;
constexpr int64_t kTraceItems = 131072;  // items that fill the device

template <int kPC, typename kIdx>
__global__ __launch_bounds__(kVecThreads) void trace_ratio_kernel(
    KronDiag kd, const double* __restrict__ lam, double shift, int P, int64_t rowlen,
    const double* __restrict__ num, kIdx items, kIdx nseg, int seg,
    double* __restrict__ partials) {
  const int d = kd.d;
  const int row0 = blockIdx.y * kPC;
  const kIdx ml = (kIdx)kd.m[d - 1];
  const int64_t offl = kd.off[d - 1];
  // rows past P (the last chunk's tail) read row P - 1 and are never stored
  const double* nrow[kPC];
#pragma unroll
  for (int q = 0; q < kPC; ++q) nrow[q] = num + (int64_t)min(row0 + q, P - 1) * rowlen;
  double acc[kPC];
#pragma unroll
  for (int q = 0; q < kPC; ++q) acc[q] = 0.0;
  const kIdx stride = (kIdx)gridDim.x * blockDim.x;
  for (kIdx it = (kIdx)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    kIdx hh = it / nseg;
    const kIdx sg = it - hh * nseg;
    double hl = 1.0;
    double hn[kPC];
#pragma unroll
    for (int q = 0; q < kPC; ++q) hn[q] = 1.0;
    for (int k = d - 2; k >= 0; --k) {
      const kIdx mk = (kIdx)kd.m[k];
      const kIdx nx = hh / mk;
      const int64_t o = kd.off[k] + (int64_t)(hh - nx * mk);
      hh = nx;
      hl *= lam[o];
#pragma unroll
      for (int q = 0; q < kPC; ++q) hn[q] *= nrow[q][o];
    }
    const kIdx l0 = sg * (kIdx)seg;
    const kIdx l1 = min(l0 + (kIdx)seg, ml);
    for (kIdx l = l0; l < l1; ++l) {
      const int64_t o = offl + (int64_t)l;
      const double r = 1.0 / fma(hl, lam[o], shift);
#pragma unroll
      for (int q = 0; q < kPC; ++q) acc[q] = fma(hn[q] * nrow[q][o], r, acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < kPC; ++q) {
    const double s = block_sum(acc[q]);
    __syncthreads();
    if (threadIdx.x == 0 && row0 + q < P)
      partials[(int64_t)(row0 + q) * gridDim.x + blockIdx.x] = s;
  }
}

// out[blockIdx.x] = sum of row blockIdx.x of partials (rows of `count`)
__global__ __launch_bounds__(1024) void reduce_rows_kernel(const double* __restrict__ partials,
                                                           int64_t count,
                                                           double* __restrict__ out) {
  const double s = sum_partials(partials + (int64_t)blockIdx.x * count, count);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

template <typename kIdx>
static void launch_trace_ratio(int pc, dim3 grid, hipStream_t s, const KronDiag& kd,
                               const double* lam, double shift, int P, int64_t rowlen,
                               const double* num, int64_t items, int64_t nseg, int seg,
                               double* partials) {
#define GG_TRACE_CASE(PC)                                                                  \
  case PC:                                                                                 \
    hipLaunchKernelGGL((trace_ratio_kernel<PC, kIdx>), grid, dim3(kVecThreads), 0, s, kd,  \
                       lam, shift, P, rowlen, num, (kIdx)items, (kIdx)nseg, seg, partials); \
    break;
  switch (pc) {
    GG_TRACE_CASE(1)
    GG_TRACE_CASE(2)
    GG_TRACE_CASE(3)
    GG_TRACE_CASE(4)
    GG_TRACE_CASE(5)
    GG_TRACE_CASE(6)
    GG_TRACE_CASE(7)
    default:
      GG_TRACE_CASE(8)
  }
#undef GG_TRACE_CASE
  GG_LAUNCH_CHECK();
}

}  // namespace gg

extern "C" {

int gg_diag_divide(const double* t_dev, double shift, const double* x_dev, double* y_dev,
                   int64_t n, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(t_dev && x_dev && y_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    if (n == 0) return;
    hipLaunchKernelGGL(gg::diag_divide_kernel, dim3(gg::vec_blocks(2 * n)),
                       dim3(gg::kVecThreads), 0, gg::as_stream(stream), t_dev, shift, x_dev,
                       y_dev, n);
    GG_LAUNCH_CHECK();
  });
}

int gg_scale_rows(double* A_dev, int64_t rows, int64_t cols, const double* w_dev, int mode,
                  gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(A_dev && rows >= 0 && cols >= 0 && mode >= 0 && mode <= 2, GG_ERR_VALUE,
               "bad argument");
    GG_REQUIRE(mode == 2 || w_dev, GG_ERR_VALUE, "w required");
    if (rows * cols == 0) return;
    hipLaunchKernelGGL(gg::scale_rows_kernel, dim3(gg::vec_blocks(2 * rows * cols)),
                       dim3(gg::kVecThreads), 0, gg::as_stream(stream), A_dev, rows, cols, w_dev,
                       mode);
    GG_LAUNCH_CHECK();
  });
}

int gg_kron_diag_scale(int d, const int64_t* m, const double* lam_dev, double shift, int mode,
                       const double* x_dev, double* y_dev, gg_stream stream) {
  return gg::guard([&] {
    int64_t n = 0;
    gg::KronDiag kd = gg::make_diag(d, m, &n);
    GG_REQUIRE(lam_dev && y_dev, GG_ERR_VALUE, "NULL argument");
    GG_REQUIRE(mode == GG_DIAG_POSTVAR || x_dev, GG_ERR_VALUE, "x required");
    GG_REQUIRE(mode >= 0 && mode <= 2, GG_ERR_VALUE, "bad mode");
    hipLaunchKernelGGL(gg::diag_scale_kernel, dim3(gg::vec_blocks(2 * n)),
                       dim3(gg::kVecThreads), 0, gg::as_stream(stream), kd, lam_dev, shift,
                       mode, x_dev, y_dev, n);
    GG_LAUNCH_CHECK();
  });
}

int gg_kron_logdet_shifted(int d, const int64_t* m, const double* lam_dev, double shift,
                           double* out_host, gg_stream stream) {
  return gg::guard([&] {
    int64_t n = 0;
    gg::KronDiag kd = gg::make_diag(d, m, &n);
    GG_REQUIRE(lam_dev && out_host, GG_ERR_VALUE, "NULL argument");
    hipStream_t s = gg::as_stream(stream);
    double* buf = nullptr;
    GG_HIP(hipMallocAsync(&buf, (gg::kVecBlocks + 1) * sizeof(double), s));
    const int nb = gg::vec_blocks(2 * n);
    hipLaunchKernelGGL(gg::logdet_kernel, dim3(nb), dim3(gg::kVecThreads), 0, s, kd, lam_dev,
                       shift, n, buf);
    GG_LAUNCH_CHECK();
    gg::launch_reduce_to(buf, nb, buf + gg::kVecBlocks, s);
    GG_HIP(hipMemcpyAsync(out_host, buf + gg::kVecBlocks, sizeof(double),
                          hipMemcpyDeviceToHost, s));
    GG_HIP(hipFreeAsync(buf, s));
    GG_HIP(hipStreamSynchronize(s));
  });
}

int gg_kron_trace_ratio(int d, const int64_t* m, const double* lam_dev, double shift, int P,
                        const double* num_dev, double* out_host, gg_stream stream) {
  return gg::guard([&] {
    int64_t n = 0;
    gg::KronDiag kd = gg::make_diag(d, m, &n);
    GG_REQUIRE(P >= 0, GG_ERR_VALUE, "P must be >= 0");
    GG_REQUIRE(lam_dev && num_dev && out_host, GG_ERR_VALUE, "NULL argument");
    if (P == 0) return;
    hipStream_t s = gg::as_stream(stream);
    // items: (head, segment of the last factor).  Whole runs where the heads
    // alone fill the device; shorter segments (never under kTraceSeg points,
    // the decode's worth) on a grid with few heads, capped so that one
    // thread's chain of additions stays short.
    const int64_t ml = kd.m[d - 1], nhead = n / ml;
    const int64_t want = gg::ceil_div(gg::kTraceItems, nhead);
    int64_t seg = std::max(gg::ceil_div(ml, want), std::min<int64_t>(ml, gg::kTraceSeg));
    seg = std::min<int64_t>(seg, gg::kTraceSegMax);
    const int64_t nseg = gg::ceil_div(ml, seg), items = nhead * nseg;
    const int nb = (int)std::min<int64_t>(gg::kVecBlocks, gg::ceil_div(items, gg::kVecThreads));
    // P rows in equal chunks of at most kTraceRows, one chunk per blockIdx.y
    const int nchunk = (P + gg::kTraceRows - 1) / gg::kTraceRows;
    const int pc = (P + nchunk - 1) / nchunk;
    GG_REQUIRE(nchunk <= 65535, GG_ERR_VALUE, "too many numerator rows");
    int64_t rowlen = 0;
    for (int k = 0; k < d; ++k) rowlen += kd.m[k];
    double* buf = nullptr;
    GG_HIP(hipMallocAsync(&buf, ((int64_t)P * nb + P) * sizeof(double), s));
    double* out_dev = buf + (int64_t)P * nb;
    const dim3 grid(nb, nchunk);
    if (n < (int64_t(1) << 31))
      gg::launch_trace_ratio<uint32_t>(pc, grid, s, kd, lam_dev, shift, P, rowlen, num_dev, items,
                                       nseg, (int)seg, buf);
    else
      gg::launch_trace_ratio<int64_t>(pc, grid, s, kd, lam_dev, shift, P, rowlen, num_dev, items,
                                      nseg, (int)seg, buf);
    hipLaunchKernelGGL(gg::reduce_rows_kernel, dim3(P), dim3(1024), 0, s, buf, (int64_t)nb,
                       out_dev);
    GG_LAUNCH_CHECK();
    GG_HIP(hipMemcpyAsync(out_host, out_dev, P * sizeof(double), hipMemcpyDeviceToHost, s));
    GG_HIP(hipFreeAsync(buf, s));
    GG_HIP(hipStreamSynchronize(s));
  });
}

int gg_probe_fill(uint64_t seed, int probe, double* z_dev, int64_t n, gg_stream stream) {
  return gg::guard([&] {
    GG_REQUIRE(z_dev && n >= 0, GG_ERR_VALUE, "bad argument");
    if (n == 0) return;
    hipLaunchKernelGGL(gg::probe_kernel, dim3(gg::vec_blocks(2 * n)), dim3(gg::kVecThreads),
                       0, gg::as_stream(stream), gg::probe_base(seed, probe), 1.0, z_dev, n);
    GG_LAUNCH_CHECK();
  });
}

}  // extern "C"
