// slim.hip — gfx950 kernels of the SLIM path (include/slim.h): the reference's item-item elastic
// net (util/slim.pyx:25-126, SLiMRecommender.py:42-46, :116, :123).
//
// Gram: A is 0/1, so G = A^T A is a matrix of integer counts.  A^T is a dense i8 operand
// [p_pad, k_pad], item-major with the users (the K dimension) contiguous; one wave computes 2 x 2
// tiles of 32 x 32 of G with v_mfma_i32_32x32x32_i8 into i32 accumulators (exact below 2^31 users)
// and stores them, and their mirror images, as f64.  Both operands of a tile are rows of the same
// array read with the same lane -> k map, so the product pairs equal k whatever the instruction's
// operand map is; only the C/D map (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
// places the results.
//
// Coordinate descent: one workgroup owns a column.  The reference visits j = 0 .. p - 1 in turn,
// and most visits change nothing; here every thread evaluates one candidate j of a block of 256
// against the current g and w, the workgroup takes the FIRST candidate that moves, applies it
// with all threads on the update over k, and resumes the scan at j + 1.  The candidates before
// it did not move under the values the reference would have shown them, the ones after it are
// evaluated again, so every g[k] and w[j] sees the reference's operations in the reference's
// order.  All arithmetic is double without contraction into fused multiply-adds, and the
// division is the correctly rounded one, so W is the compiled reference's bit for bit.  G is
// symmetric, so both G[:, col] and the G[:, j] of an update are read as contiguous rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slim_kernels.h"

#pragma clang fp contract(off)

namespace bprmf {
namespace slim {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void k_scatter(const int32_t* __restrict__ rows,
                                                 const int32_t* __restrict__ indices, int64_t n,
                                                 int8_t* __restrict__ At, int64_t k_pad) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) At[(int64_t)indices[e] * k_pad + rows[e]] = 1;
}

// workgroup = 4 waves = the 2 x 2 sub-blocks of 64 x 64 of one 128 x 128 block (bi, bj), bj >= bi;
// a wave holds its sub-block as 2 x 2 tiles of 32 x 32, so two A and two B fragments feed four MFMAs
__global__ __launch_bounds__(256) void k_gram(const int8_t* __restrict__ At, int64_t p, int64_t k_pad,
                                              double* __restrict__ G) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t si = 2 * bi + (wv >> 1), sj = 2 * bj + (wv & 1);
  if (sj < si) return;  // the sub-block below the diagonal of a diagonal block: its mirror is stored
  const int r = lane & 31, h = lane >> 5;
  // rows s * 64 + 32 + r < p_pad and 16 h + 16 <= 32 <= k_pad - k0: inside the padded operand
  const int8_t* pa = At + (si * 64 + r) * k_pad + 16 * h;
  const int8_t* pb = At + (sj * 64 + r) * k_pad + 16 * h;
  const int64_t half = 32 * k_pad;
  const i32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  i32x16 acc[2][2] = {{zero, zero}, {zero, zero}};
  for (int64_t k0 = 0; k0 < k_pad; k0 += 32) {
    const i32x4 a0 = *reinterpret_cast<const i32x4*>(pa + k0);
    const i32x4 a1 = *reinterpret_cast<const i32x4*>(pa + half + k0);
    const i32x4 b0 = *reinterpret_cast<const i32x4*>(pb + k0);
    const i32x4 b1 = *reinterpret_cast<const i32x4*>(pb + half + k0);
    acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
  }
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
      const int64_t gj = sj * 64 + 32 * tb + r;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int64_t gi = si * 64 + 32 * ta + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (gi < p && gj < p) {
          const double v = (double)acc[ta][tb][reg];
          G[gi * p + gj] = v;
          G[gj * p + gi] = v;
        }
      }
    }
}

__global__ __launch_bounds__(256) void k_diag(const double* __restrict__ G, int64_t p,
                                              double* __restrict__ diag) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < p) diag[j] = G[j * p + j];
}

struct CdArgs {
  const double* G;
  const double* diag;
  double* W;
  double* ws;
  unsigned long long* stats;
  int32_t p;
  int64_t col_begin, col_end;
  double alpha, lam, N, tol;
  int32_t ratio, max_iter;
};

// CHIP: g and w of the workgroup's column in LDS; otherwise in its slice of the global workspace.
// The code is the same, so are the bits.
template <bool CHIP>
__global__ __launch_bounds__(kCdThreads) void k_cd(CdArgs a) {
  extern __shared__ double s_gw[];
  __shared__ int s_first[2][4];  // per scan round (alternating) and wave: its first moving lane
  __shared__ double s_new[2][4], s_delta[2][4];
  __shared__ double s_max[4];
  const int p = a.p, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* g = CHIP ? s_gw : a.ws + (int64_t)blockIdx.x * 2 * p;
  double* w = g + p;
  unsigned long long n_sweeps = 0, n_moves = 0, n_capped = 0;
  int par = 0;
  for (int64_t col = a.col_begin + blockIdx.x; col < a.col_end; col += gridDim.x) {
    const double* Gc = a.G + col * p;  // G[col, :] = G[:, col]
    for (int k = tid; k < p; k += kCdThreads) {
      g[k] = 0.0;
      w[k] = 0.0;
    }
    double b, c;
    bool run = true;
    if (a.ratio) {  // :90-98
      double m = 0.0;
      for (int k = tid; k < p; k += kCdThreads)
        if (k != col) m = fmax(m, Gc[k]);
      for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
      if (lane == 0) s_max[wv] = m;
      __syncthreads();
      m = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
      run = m != 0.0;
      b = m * a.lam;
      c = ((m * (1.0 - a.alpha)) / a.alpha) * a.lam;
    } else {  // :45-46
      b = (a.lam * a.alpha) * a.N;
      c = (a.lam * (1.0 - a.alpha)) * a.N;
    }
    __syncthreads();  // g and w are zero; s_max is free again
    if (run) {
      int mode = 0, sweeps = 0;
      for (int step = 0; step < a.max_iter; ++step) {
        bool move = false;
        int j0 = 0;
        while (j0 < p) {
          const int j = j0 + tid;
          bool cand = false;
          double nw = 0.0, dl = 0.0;
          if (j < p && j != col) {
            const double wj = w[j];
            if (!(mode == 1 && wj == 0.0)) {
              const double d = a.diag[j];
              const double av = (Gc[j] + d * wj) - g[j];
              const double sv = (b >= fabs(av) || av <= 0.0) ? 0.0 : av - b;
              nw = sv / (c + d);
              dl = nw - wj;
              cand = fabs(dl) > a.tol;  // false for the NaN of 0/0
            }
          }
          const unsigned long long bal = __ballot(cand);
          if (lane == 0) s_first[par][wv] = bal ? __ffsll((long long)bal) - 1 : 64;
          if (cand && (bal & ((1ull << lane) - 1ull)) == 0) {
            s_new[par][wv] = nw;
            s_delta[par][wv] = dl;
          }
          __syncthreads();
          int fw = -1;
#pragma unroll
          for (int x = 3; x >= 0; --x)
            if (s_first[par][x] < 64) fw = x;
          if (fw < 0) {  // nothing in this block moves
            j0 += kCdThreads;
            par ^= 1;
            continue;
          }
          const int jm = j0 + 64 * fw + s_first[par][fw];
          const double nv = s_new[par][fw], dv = s_delta[par][fw];
          par ^= 1;
          const double* Gj = a.G + (int64_t)jm * p;  // G[jm, :] = G[:, jm]
          // four entries per thread and trip, loads first: g may alias nothing the compiler can
          // prove, and one load-multiply-add-store at a time leaves the memory latency exposed
          for (int k0 = tid; k0 < p; k0 += 4 * kCdThreads) {
            double gv[4], cv[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              const int k = k0 + x * kCdThreads;
              gv[x] = k < p ? g[k] : 0.0;
              cv[x] = k < p ? Gj[k] : 0.0;
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              const int k = k0 + x * kCdThreads;
              if (k < p) g[k] = gv[x] + cv[x] * dv;
            }
          }
          if (tid == 0) w[jm] = nv;
          __syncthreads();
          move = true;
          ++n_moves;
          j0 = jm + 1;
        }
        ++sweeps;
        if (!move) {
          if (mode == 0) break;
          mode = 0;
        } else if (mode == 0) {
          mode = 1;
        }
      }
      n_sweeps += (unsigned long long)sweeps;
      n_capped += a.max_iter > 0 && sweeps == a.max_iter;
    }
    for (int k = tid; k < p; k += kCdThreads) a.W[(int64_t)k * p + col] = w[k];
    __syncthreads();
  }
  if (tid == 0) {
    atomicAdd(a.stats + 0, n_sweeps);
    atomicAdd(a.stats + 1, n_moves);
    atomicAdd(a.stats + 2, n_capped);
  }
}

__global__ __launch_bounds__(256) void k_score(const int64_t* __restrict__ indptr,
                                               const int32_t* __restrict__ indices,
                                               const double* __restrict__ W, int64_t p,
                                               const int32_t* __restrict__ us,
                                               const int32_t* __restrict__ is, int64_t n,
                                               double* __restrict__ out) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const int64_t u = us[x], i = is[x];
  double acc = 0.0;
  for (int64_t q = indptr[u]; q < indptr[u + 1]; ++q) acc += W[(int64_t)indices[q] * p + i];
  out[x] = acc;
}

__global__ __launch_bounds__(256) void k_score_rows(const int64_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices,
                                                    const double* __restrict__ W, int64_t p,
                                                    const int32_t* __restrict__ us, int64_t n,
                                                    double* __restrict__ out) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n * p) return;
  const int64_t u = us[x / p], i = x % p;
  double acc = 0.0;
  for (int64_t q = indptr[u]; q < indptr[u + 1]; ++q) acc += W[(int64_t)indices[q] * p + i];
  out[x] = acc;
}

// (score, position) a ranks before b: higher score, then the earlier position; pos < 0 = none
static __device__ __forceinline__ bool before(double sa, int pa, double sb, int pb) {
  if (pa < 0) return false;
  if (pb < 0) return true;
  return sa > sb || (sa == sb && pa < pb);
}

// One workgroup per user: the list's scores (k_score's arithmetic) into sc, then k selection
// rounds; each round takes the best entry that ranks after the previous round's.  The order is
// the stable descending sort of SLiMRecommender.py:116 (topk.hip's keys hold an f32 score and
// break ties the other way, so its sort is not reused; k <= 32 rounds over a list are cheap).
__global__ __launch_bounds__(256) void k_topk(const int64_t* __restrict__ indptr,
                                              const int32_t* __restrict__ indices,
                                              const double* __restrict__ W, int64_t p,
                                              const int32_t* __restrict__ us,
                                              const int64_t* __restrict__ offs,
                                              const int32_t* __restrict__ items, int k,
                                              double* __restrict__ sc, int32_t* __restrict__ out_pos,
                                              double* __restrict__ out_score) {
  __shared__ double s_s[2][4];
  __shared__ int s_p[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t r = blockIdx.x, beg = offs[r];
  const int n = (int)(offs[r + 1] - beg);
  const int64_t u = us[r];
  const int64_t q0 = indptr[u], q1 = indptr[u + 1];
  for (int x = tid; x < n; x += 256) {
    const int64_t i = items[beg + x];
    double acc = 0.0;
    for (int64_t q = q0; q < q1; ++q) acc += W[(int64_t)indices[q] * p + i];
    sc[beg + x] = acc;
  }
  __syncthreads();
  double last_s = 0.0;
  int last_p = -1;  // none yet: every entry is eligible
  for (int t = 0; t < k; ++t) {
    double bs = 0.0;
    int bp = -1;
    for (int x = tid; x < n; x += 256) {
      const double v = sc[beg + x];
      if ((last_p < 0 || before(last_s, last_p, v, x)) && before(v, x, bs, bp)) {
        bs = v;
        bp = x;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o);
      const int op = __shfl_xor(bp, o);
      if (before(os, op, bs, bp)) {
        bs = os;
        bp = op;
      }
    }
    if (lane == 0) {
      s_s[t & 1][wv] = bs;
      s_p[t & 1][wv] = bp;
    }
    __syncthreads();
    bs = s_s[t & 1][0];
    bp = s_p[t & 1][0];
#pragma unroll
    for (int x = 1; x < 4; ++x)
      if (before(s_s[t & 1][x], s_p[t & 1][x], bs, bp)) {
        bs = s_s[t & 1][x];
        bp = s_p[t & 1][x];
      }
    if (tid == 0) {
      out_pos[r * k + t] = bp;
      out_score[r * k + t] = bp < 0 ? -INFINITY : bs;
    }
    if (bp < 0) {  // the list is exhausted (uniform): the rest is -1 / -inf
      for (int x = t + 1 + tid; x < k; x += 256) {
        out_pos[r * k + x] = -1;
        out_score[r * k + x] = -INFINITY;
      }
      break;
    }
    last_s = bs;
    last_p = bp;
  }
}

hipError_t scatter(const int32_t* rows, const int32_t* indices, int64_t n, int8_t* At, int64_t k_pad,
                   hipStream_t s) {
  if (n <= 0) return hipSuccess;
  k_scatter<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(rows, indices, n, At, k_pad);
  return hipGetLastError();
}

hipError_t gram(const int8_t* At, int64_t p, int64_t p_pad, int64_t k_pad, double* G, double* diag,
                hipStream_t s) {
  if (p <= 0) return hipSuccess;
  const unsigned nb = (unsigned)(p_pad / 128);
  if (nb > 65535u) return hipErrorInvalidValue;
  k_gram<<<dim3(nb, nb), 256, 0, s>>>(At, p, k_pad, G);
  if (hipError_t e = hipGetLastError()) return e;
  k_diag<<<(unsigned)((p + 255) / 256), 256, 0, s>>>(G, p, diag);
  return hipGetLastError();
}

hipError_t coordinate_descent(const Cd& c, hipStream_t s) {
  if (c.p <= 0 || c.col_end <= c.col_begin) return hipSuccess;
  CdArgs a{c.G, c.diag, c.W, c.ws, c.stats, c.p, c.col_begin, c.col_end, c.alpha, c.lam, c.N, c.tol,
           c.ratio, c.max_iter};
  if (c.chip) {
    if (c.p > kChipMaxP) return hipErrorInvalidValue;
    const size_t lds = 16 * (size_t)c.p;
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cd<true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
      return e;
    k_cd<true><<<(unsigned)c.blocks, kCdThreads, lds, s>>>(a);
  } else {
    k_cd<false><<<(unsigned)c.blocks, kCdThreads, 0, s>>>(a);
  }
  return hipGetLastError();
}

hipError_t score(const int64_t* indptr, const int32_t* indices, const double* W, int64_t p,
                 const int32_t* us, const int32_t* is, int64_t n, double* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  k_score<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(indptr, indices, W, p, us, is, n, out);
  return hipGetLastError();
}

hipError_t score_rows(const int64_t* indptr, const int32_t* indices, const double* W, int64_t p,
                      const int32_t* us, int64_t n, double* out, hipStream_t s) {
  if (n <= 0 || p <= 0) return hipSuccess;
  const int64_t blocks = (n * p + 255) / 256;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  k_score_rows<<<(unsigned)blocks, 256, 0, s>>>(indptr, indices, W, p, us, n, out);
  return hipGetLastError();
}

hipError_t topk_lists(const int64_t* indptr, const int32_t* indices, const double* W, int64_t p,
                      const int32_t* us, const int64_t* offs, const int32_t* items, int64_t n_users,
                      int k, double* sc, int32_t* out_pos, double* out_score, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  if (k <= 0 || k > kTopkMaxK || n_users > INT32_MAX) return hipErrorInvalidValue;
  k_topk<<<(unsigned)n_users, 256, 0, s>>>(indptr, indices, W, p, us, offs, items, k, sc, out_pos,
                                            out_score);
  return hipGetLastError();
}

}  // namespace slim
}  // namespace bprmf
