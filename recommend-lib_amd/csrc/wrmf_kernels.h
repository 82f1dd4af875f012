// wrmf_kernels.h — launchers of the implicit-feedback ALS kernels (wrmf.hip), internal to
// libbprmf_amd.so; the public ABI is include/wrmf.h (wrmf_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bprmf {
namespace wrmf {

constexpr int kMaxFactors = 128;
constexpr int kGramRows = 512;  // table rows per Gram part (one workgroup each)

inline int tiles_of(int d) { return (d + 15) / 16; }             // 16-wide tiles per side
inline int lower_tiles(int d) { return tiles_of(d) * (tiles_of(d) + 1) / 2; }
// doubles of one Gram part / one heavy-row partial sum: the lower tiles in the MFMA's own
// register layout [tile][reg][lane], then (partial sums only) the right-hand side
inline int64_t gram_part_stride(int d) { return (int64_t)lower_tiles(d) * 256; }
inline int64_t partial_stride(int d) { return (int64_t)lower_tiles(d) * 256 + tiles_of(d) * 16; }

// one half-sweep: every row of `indptr` solved from the neighbour table Tin and its Gram matrix G
struct Sweep {
  const int64_t* indptr;   // [rows + 1]
  const int32_t* indices;  // [nnz] neighbour rows (of Tin)
  const double* conf;      // [nnz] confidences, all non-zero
  const double* Tin;       // [*, d]
  double* Tout;            // [rows, d]
  const double* G;         // [d, d] Tin^T Tin
  const int32_t* order;    // [n_light] rows solved by one workgroup each, by decreasing nnz
  int32_t n_light;
  const int32_t* hrow;     // [n_heavy] rows above the heavy threshold, by decreasing nnz
  const int64_t* hoff;     // [n_heavy + 1] first part of each heavy row
  int32_t n_heavy;
  const int32_t* prow;     // [n_parts] row of each part
  const int64_t* pbeg;     // [n_parts] its CSR sub-range
  const int64_t* pend;
  int32_t n_parts;
  double* partial;         // [n_parts, partial_stride(d)]
  int32_t d;
  double lam;
};

// G = T^T T for T [n, d]: kGramRows rows per workgroup into parts [ceil(n / kGramRows),
// gram_part_stride(d)], then the parts summed in index order into G [d, d] (both triangles)
hipError_t gram(const double* T, int64_t n, int d, double* parts, double* G, hipStream_t s);
hipError_t sweep(const Sweep& a, hipStream_t s);
// out[p] = X[us[p]] . Y[is[p]], summed in factor order (ids checked by the caller)
hipError_t predict(const double* X, const double* Y, int d, const int32_t* us, const int32_t* is,
                   int64_t n, double* out, hipStream_t s);

}  // namespace wrmf
}  // namespace bprmf
