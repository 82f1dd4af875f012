// wrmf.hip — implicit-feedback ALS (WRMFRecommender.py:37-56) for gfx950, all in double on the f64
// matrix pipe (v_mfma_f64_16x16x4_f64).
//
// f64 MFMA operand maps (lane l of the wave): A holds A[m = l & 15][k = l >> 4], B holds
// B[k = l >> 4][n = l & 15], and result register r of C/D holds D[row = (l >> 4) + 4 r][col = l & 15].
//
// k_gram    G parts: each workgroup sums t t^T over kGramRows table rows, one lower 16x16 tile per
//           wave at a time, 4 rows per MFMA; k_gram_sum adds the parts in index order.
// k_rows    one workgroup per row (one wave while d <= 32, four above).  It walks the row's CSR
//           entries 16 at a time: the neighbour rows are gathered into LDS (the next chunk is
//           already in flight in registers), sum c t t^T is (c o T)^T T on the MFMA with the
//           lower tiles' accumulators in registers, b = sum (c + 1) t one thread per column.  Then
//           A = acc + G + lambda I goes to LDS as lower tiles only (padding columns get a unit
//           diagonal), a right-looking blocked Cholesky runs in place (diagonal tile: one wave,
//           a row per lane, columns passed by shuffle; panel: a row per thread; trailing update:
//           MFMA), and the forward and back substitution go tile by tile the same way.
//           mode 1 stops after the accumulation of one CSR sub-range and writes the partial sums;
//           mode 2 starts from the sum of a heavy row's partial sums, added in part order.
// No atomics anywhere: every sum has one fixed order, so results are bit-identical run to run.
#include <hip/hip_runtime.h>

#include "wrmf_kernels.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "wrmf.hip targets gfx950 (v_mfma_f64_16x16x4_f64); build with --offload-arch=gfx950"
#endif

namespace bprmf {
namespace wrmf {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kChunk = 16;   // neighbour rows gathered per step
constexpr int kTileLd = 17;  // LDS row stride of a 16x16 tile (odd: a column walk hits 16 banks)
constexpr int kTileSz = 16 * kTileLd;

__device__ __forceinline__ double4_t mfma(double a, double b, double4_t c) {
#if defined(__gfx950__)
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
#else
  return c;
#endif
}

// lower tile t = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void tile_of(int t, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}
__device__ __forceinline__ int tile_id(int ti, int tj) { return ti * (ti + 1) / 2 + tj; }

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gram(const double* __restrict__ T, int64_t n, int d,
                                              double* __restrict__ parts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nt = (d + 15) >> 4, ntl = nt * (nt + 1) / 2;
  const int64_t r0 = (int64_t)blockIdx.x * kGramRows;
  const int64_t r1 = r0 + kGramRows < n ? r0 + kGramRows : n;
  double* out = parts + (int64_t)blockIdx.x * ntl * 256;
  const int m = lane & 15, kq = lane >> 4;
  for (int t = wave; t < ntl; t += 4) {
    int ti, tj;
    tile_of(t, ti, tj);
    const int ca = ti * 16 + m, cb = tj * 16 + m;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int64_t r = r0; r < r1; r += 4) {
      const int64_t row = r + kq;
      const bool in = row < r1;
      const double a = (in && ca < d) ? T[row * d + ca] : 0.0;
      const double b = (in && cb < d) ? T[row * d + cb] : 0.0;
      acc = mfma(a, b, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) out[t * 256 + r * 64 + lane] = acc[r];
  }
}

__global__ __launch_bounds__(256) void k_gram_sum(const double* __restrict__ parts, int nparts, int d,
                                                  double* __restrict__ G) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e % d;
  if (j > i) return;
  const int nt = (d + 15) >> 4, ntl = nt * (nt + 1) / 2;
  const int row = i & 15, col = j & 15;
  const int off = tile_id(i >> 4, j >> 4) * 256 + (row >> 2) * 64 + (row & 3) * 16 + col;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += parts[(int64_t)p * ntl * 256 + off];
  G[i * d + j] = s;
  G[j * d + i] = s;
}

// ---------------------------------------------------------------------------------------------
template <int NT>
struct Cfg {
  static constexpr int kWaves = NT <= 2 ? 1 : 4;
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kDp = 16 * NT;                               // padded d
  static constexpr int kNtl = NT * (NT + 1) / 2;                    // lower tiles
  static constexpr int kTpw = (kNtl + kWaves - 1) / kWaves;         // tiles per wave
  static constexpr int kCld = (kDp % 32 == 0) ? kDp + 16 : kDp;     // chunk row stride (doubles)
  static constexpr int kCpt = kChunk * kDp / kThreads;              // gathered doubles per thread
  static constexpr int kLds = (kNtl * kTileSz + kChunk * kCld + kChunk + kDp) * 8;
  static_assert(kChunk * kDp % kThreads == 0, "the gather covers the chunk exactly");
  static_assert(kDp <= kThreads && kChunk <= kThreads, "a thread per column");
};

template <int NT>
__global__ __launch_bounds__(Cfg<NT>::kThreads) void k_rows(const Sweep a, const int mode) {
  using C = Cfg<NT>;
  extern __shared__ double lds[];
  double* tiles = lds;                            // [kNtl][16][kTileLd]
  double* chunk = tiles + C::kNtl * kTileSz;      // [kChunk][kCld]
  double* cs = chunk + kChunk * C::kCld;          // [kChunk]
  double* bs = cs + kChunk;                       // [kDp]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const int d = a.d;

  int32_t row;
  int64_t e0 = 0, e1 = 0;
  if (mode == 0) {
    row = a.order[blockIdx.x];
    e0 = a.indptr[row];
    e1 = a.indptr[row + 1];
  } else if (mode == 1) {
    row = a.prow[blockIdx.x];
    e0 = a.pbeg[blockIdx.x];
    e1 = a.pend[blockIdx.x];
  } else {
    row = a.hrow[blockIdx.x];
  }
  if (mode == 0 && e0 == e1) {  // an empty row solves to exactly +0.0
    if (tid < d) a.Tout[(int64_t)row * d + tid] = 0.0;
    return;
  }

  double4_t acc[C::kTpw];
#pragma unroll
  for (int q = 0; q < C::kTpw; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  double bacc = 0.0;

  if (mode != 2) {
    // gather of chunk c: element x of this thread is neighbour k = idx / kDp, column idx % kDp
    double pre[C::kCpt];
    double prec = 0.0;
    auto fetch = [&](int64_t base) {
#pragma unroll
      for (int x = 0; x < C::kCpt; ++x) {
        const int idx = x * C::kThreads + tid;
        const int k = idx / C::kDp, j = idx % C::kDp;
        const int64_t e = base + k;
        pre[x] = (e < e1 && j < d) ? a.Tin[(int64_t)a.indices[e] * d + j] : 0.0;
      }
      if (tid < kChunk) prec = (base + tid < e1) ? a.conf[base + tid] : 0.0;
    };
    fetch(e0);
    for (int64_t base = e0; base < e1; base += kChunk) {
#pragma unroll
      for (int x = 0; x < C::kCpt; ++x) {
        const int idx = x * C::kThreads + tid;
        chunk[(idx / C::kDp) * C::kCld + idx % C::kDp] = pre[x];
      }
      if (tid < kChunk) cs[tid] = prec;
      __syncthreads();
      if (base + kChunk < e1) fetch(base + kChunk);
#pragma unroll
      for (int q = 0; q < C::kTpw; ++q) {
        const int t = wave + q * C::kWaves;
        if (t < C::kNtl) {
          int ti, tj;
          tile_of(t, ti, tj);
#pragma unroll
          for (int k4 = 0; k4 < kChunk; k4 += 4) {
            const int k = k4 + kq;
            const double av = cs[k] * chunk[k * C::kCld + ti * 16 + m];
            const double bv = chunk[k * C::kCld + tj * 16 + m];
            acc[q] = mfma(av, bv, acc[q]);
          }
        }
      }
      if (tid < C::kDp) {
#pragma unroll
        for (int k = 0; k < kChunk; ++k) bacc += (cs[k] + 1.0) * chunk[k * C::kCld + tid];
      }
      __syncthreads();
    }
  } else {
    const int64_t stride = (int64_t)C::kNtl * 256 + C::kDp;
    for (int64_t p = a.hoff[blockIdx.x]; p < a.hoff[blockIdx.x + 1]; ++p) {
      const double* src = a.partial + p * stride;
#pragma unroll
      for (int q = 0; q < C::kTpw; ++q) {
        const int t = wave + q * C::kWaves;
        if (t < C::kNtl) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[q][r] += src[t * 256 + r * 64 + lane];
        }
      }
      if (tid < C::kDp) bacc += src[C::kNtl * 256 + tid];
    }
  }

  if (mode == 1) {
    double* dst = a.partial + (int64_t)blockIdx.x * ((int64_t)C::kNtl * 256 + C::kDp);
#pragma unroll
    for (int q = 0; q < C::kTpw; ++q) {
      const int t = wave + q * C::kWaves;
      if (t < C::kNtl) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[t * 256 + r * 64 + lane] = acc[q][r];
      }
    }
    if (tid < C::kDp) dst[C::kNtl * 256 + tid] = bacc;
    return;
  }

  // A = G + sum c t t^T + lambda I into the lower tiles, unit diagonal in the padding
#pragma unroll
  for (int q = 0; q < C::kTpw; ++q) {
    const int t = wave + q * C::kWaves;
    if (t < C::kNtl) {
      int ti, tj;
      tile_of(t, ti, tj);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = kq + 4 * r, gi = ti * 16 + lr, gj = tj * 16 + m;
        double v = acc[q][r];
        if (gi < d && gj < d) v += a.G[gi * d + gj];
        if (gi == gj) v += gi < d ? a.lam : 1.0;
        tiles[t * kTileSz + lr * kTileLd + m] = v;
      }
    }
  }
  if (tid < C::kDp) bs[tid] = bacc;
  __syncthreads();

  // blocked right-looking Cholesky, in place
  for (int k = 0; k < NT; ++k) {
    double* Lkk = tiles + tile_id(k, k) * kTileSz;
    if (wave == 0) {  // lane (row m, four copies) holds row m of the diagonal tile
      double r_[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) r_[c] = Lkk[m * kTileLd + c];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double ljj = sqrt(__shfl(r_[j], j, 16));
        r_[j] = (m == j) ? ljj : r_[j] / ljj;
#pragma unroll
        for (int c = j + 1; c < 16; ++c) {
          const double lc = __shfl(r_[j], c, 16);
          if (m >= c) r_[c] = fma(-r_[j], lc, r_[c]);
        }
      }
      if (lane < 16) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (c <= m) Lkk[m * kTileLd + c] = r_[c];
      }
    }
    __syncthreads();
    const int below = (NT - 1 - k) * 16;
    if (tid < below) {  // panel: row x of tile (ti, k) <- x Lkk^-T
      double* rowp = tiles + tile_id(k + 1 + (tid >> 4), k) * kTileSz + (tid & 15) * kTileLd;
      double x[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) x[c] = rowp[c];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        double s = x[c];
#pragma unroll
        for (int p = 0; p < c; ++p) s = fma(-x[p], Lkk[c * kTileLd + p], s);
        x[c] = s / Lkk[c * kTileLd + c];
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) rowp[c] = x[c];
    }
    __syncthreads();
    const int mrem = NT - 1 - k, npair = mrem * (mrem + 1) / 2;
    for (int p = wave; p < npair; p += C::kWaves) {  // A_ij -= L_ik L_jk^T
      int pi, pj;
      tile_of(p, pi, pj);
      double* Aij = tiles + tile_id(k + 1 + pi, k + 1 + pj) * kTileSz;
      const double* Li = tiles + tile_id(k + 1 + pi, k) * kTileSz;
      const double* Lj = tiles + tile_id(k + 1 + pj, k) * kTileSz;
      double4_t dd;
#pragma unroll
      for (int r = 0; r < 4; ++r) dd[r] = Aij[(kq + 4 * r) * kTileLd + m];
#pragma unroll
      for (int k4 = 0; k4 < 16; k4 += 4)
        dd = mfma(-Li[m * kTileLd + k4 + kq], Lj[m * kTileLd + k4 + kq], dd);
#pragma unroll
      for (int r = 0; r < 4; ++r) Aij[(kq + 4 * r) * kTileLd + m] = dd[r];
    }
    __syncthreads();
  }

  // L z = b
  for (int k = 0; k < NT; ++k) {
    const double* Lkk = tiles + tile_id(k, k) * kTileSz;
    if (wave == 0) {
      double z = bs[k * 16 + m];
      double l_[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) l_[c] = Lkk[m * kTileLd + c];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double zj = __shfl(z, j, 16) / Lkk[j * kTileLd + j];
        if (m == j) z = zj;
        if (m > j) z = fma(-l_[j], zj, z);
      }
      if (lane < 16) bs[k * 16 + m] = z;
    }
    __syncthreads();
    const int below = (NT - 1 - k) * 16;
    if (tid < below) {
      const int ti = k + 1 + (tid >> 4);
      const double* rowp = tiles + tile_id(ti, k) * kTileSz + (tid & 15) * kTileLd;
      double s = bs[ti * 16 + (tid & 15)];
#pragma unroll
      for (int c = 0; c < 16; ++c) s = fma(-rowp[c], bs[k * 16 + c], s);
      bs[ti * 16 + (tid & 15)] = s;
    }
    __syncthreads();
  }
  // L^T x = z
  for (int k = NT - 1; k >= 0; --k) {
    const double* Lkk = tiles + tile_id(k, k) * kTileSz;
    if (wave == 0) {
      double z = bs[k * 16 + m];
      double l_[16];  // column m of the diagonal tile
#pragma unroll
      for (int c = 0; c < 16; ++c) l_[c] = Lkk[c * kTileLd + m];
#pragma unroll
      for (int j = 15; j >= 0; --j) {
        const double xj = __shfl(z, j, 16) / Lkk[j * kTileLd + j];
        if (m == j) z = xj;
        if (m < j) z = fma(-l_[j], xj, z);
      }
      if (lane < 16) bs[k * 16 + m] = z;
    }
    __syncthreads();
    if (tid < k * 16) {
      const int tj = tid >> 4;
      const double* colp = tiles + tile_id(k, tj) * kTileSz + (tid & 15);
      double s = bs[tj * 16 + (tid & 15)];
#pragma unroll
      for (int c = 0; c < 16; ++c) s = fma(-colp[c * kTileLd], bs[k * 16 + c], s);
      bs[tj * 16 + (tid & 15)] = s;
    }
    __syncthreads();
  }
  if (tid < d) a.Tout[(int64_t)row * d + tid] = bs[tid];
}

__global__ void k_predict(const double* __restrict__ X, const double* __restrict__ Y, int d,
                          const int32_t* __restrict__ us, const int32_t* __restrict__ is, int64_t n,
                          double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double* x = X + (int64_t)us[p] * d;
  const double* y = Y + (int64_t)is[p] * d;
  double s = 0.0;
  for (int f = 0; f < d; ++f) s += x[f] * y[f];
  out[p] = s;
}

template <int NT>
hipError_t launch_rows(const Sweep& a, hipStream_t s) {
  using C = Cfg<NT>;
  auto* fn = k_rows<NT>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, C::kLds);
  if (e != hipSuccess) return e;
  if (a.n_parts > 0) {
    hipLaunchKernelGGL(fn, dim3(a.n_parts), dim3(C::kThreads), C::kLds, s, a, 1);
    hipLaunchKernelGGL(fn, dim3(a.n_heavy), dim3(C::kThreads), C::kLds, s, a, 2);
  }
  if (a.n_light > 0) hipLaunchKernelGGL(fn, dim3(a.n_light), dim3(C::kThreads), C::kLds, s, a, 0);
  return hipGetLastError();
}

}  // namespace

hipError_t gram(const double* T, int64_t n, int d, double* parts, double* G, hipStream_t s) {
  const int nparts = (int)((n + kGramRows - 1) / kGramRows);
  if (nparts > 0) hipLaunchKernelGGL(k_gram, dim3(nparts), dim3(256), 0, s, T, n, d, parts);
  hipLaunchKernelGGL(k_gram_sum, dim3((d * d + 255) / 256), dim3(256), 0, s, parts, nparts, d, G);
  return hipGetLastError();
}

hipError_t sweep(const Sweep& a, hipStream_t s) {
  switch (tiles_of(a.d)) {
    case 1: return launch_rows<1>(a, s);
    case 2: return launch_rows<2>(a, s);
    case 3: return launch_rows<3>(a, s);
    case 4: return launch_rows<4>(a, s);
    case 5: return launch_rows<5>(a, s);
    case 6: return launch_rows<6>(a, s);
    case 7: return launch_rows<7>(a, s);
    case 8: return launch_rows<8>(a, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t predict(const double* X, const double* Y, int d, const int32_t* us, const int32_t* is,
                   int64_t n, double* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_predict, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, Y, d, us, is, n, out);
  return hipGetLastError();
}

}  // namespace wrmf
}  // namespace bprmf
