// slim_kernels.h — launchers of the SLIM kernels (slim.hip), internal to libbprmf_amd.so; the
// public ABI is include/slim.h (slim_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bprmf {
namespace slim {

constexpr int kCdThreads = 256;     // one workgroup per column; also the width of a scan block
constexpr int kChipMaxP = 9216;     // g and w in LDS: 2 x 9216 x 8 B = 144 KB of the 160 KB
constexpr int kCdMaxBlocks = 2048;  // workgroups of one fit; each walks its columns in turn
constexpr int kTopkMaxK = 32;

// At[indices[e], rows[e]] = 1 for the n entries of A (At [p_pad, k_pad] i8, zeroed before)
hipError_t scatter(const int32_t* rows, const int32_t* indices, int64_t n, int8_t* At, int64_t k_pad,
                   hipStream_t s);
// G [p, p] f64 = At At^T on i8 MFMA (i32 accumulators, exact): the 64 x 64 sub-blocks on or above
// the diagonal, each stored with its mirror image (p_pad a multiple of 128); diag [p] = G's diagonal
hipError_t gram(const int8_t* At, int64_t p, int64_t p_pad, int64_t k_pad, double* G, double* diag,
                hipStream_t s);

struct Cd {
  const double* G;     // [p, p], symmetric
  const double* diag;  // [p]
  double* W;           // [p, p] row-major: W[j, col] at j * p + col
  double* ws;          // [blocks, 2, p] when !chip
  unsigned long long* stats;  // [3] += sweeps, moves, capped
  int32_t p;
  int64_t col_begin, col_end;
  double alpha, lam, N, tol;
  int32_t ratio, max_iter;
  int32_t blocks;
  bool chip;
};
inline int cd_blocks(int64_t cols) { return (int)(cols < kCdMaxBlocks ? cols : kCdMaxBlocks); }
hipError_t coordinate_descent(const Cd& a, hipStream_t s);

// out[n] = sum_{q in row us[n]} W[indices[q], is[n]], added in CSR order from +0.0
hipError_t score(const int64_t* indptr, const int32_t* indices, const double* W, int64_t p,
                 const int32_t* us, const int32_t* is, int64_t n, double* out, hipStream_t s);
// out[n, :] = sum_{q in row us[n]} W[indices[q], :]
hipError_t score_rows(const int64_t* indptr, const int32_t* indices, const double* W, int64_t p,
                      const int32_t* us, int64_t n, double* out, hipStream_t s);
// per user r: the scores of items[offs[r] .. offs[r + 1]) into sc (same indexing), then the k best
// positions: score descending, ties by the earlier position
hipError_t topk_lists(const int64_t* indptr, const int32_t* indices, const double* W, int64_t p,
                      const int32_t* us, const int64_t* offs, const int32_t* items, int64_t n_users,
                      int k, double* sc, int32_t* out_pos, double* out_score, hipStream_t s);

}  // namespace slim
}  // namespace bprmf
