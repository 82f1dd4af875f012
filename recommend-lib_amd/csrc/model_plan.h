// model_plan.h — the host-only (no HIP) planning logic of the sibling model paths: the rating-SGD
// dependency levels and SVD++ user lists (mf_capi.cpp), WRMF's two CSR sides with their launch
// plans (wrmf_capi.cpp), Item2Vec's noise CDF (sgns_capi.cpp), SLIM's pair validation, CSR and
// operand geometry (slim_capi.cpp) and NCF's Adam catch-up tables (ncf_capi.cpp).  Like host_plan.h
// it stays out of the HIP translation units so tests/sanitize builds it under AddressSanitizer +
// UndefinedBehaviorSanitizer and checks it against restatements.  Every function returns 0 or a
// bprmf_status; `out` is complete only on success and empty otherwise.
#pragma once
#include <stdint.h>

#include <vector>

namespace bprmf {

// Rating SGD (mf_set_train): level(s) = 1 + max(last level of u, last level of i) over the
// samples in train-set order (0-based here), then a stable counting sort by level, so samples of
// one level keep their train-set order and every sample runs after every earlier sample that
// shares its user or item.  loff [levels + 1] is the prefix of the level sizes.
struct MfLevelPlan {
  std::vector<int32_t> su, si, loff;
  std::vector<double> sr;
  int32_t levels = 0;
};
int mf_level_plan(const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
                  int64_t user_num, int64_t item_num, MfLevelPlan* out);

// SVD++ (mf_set_train): ur[u] as CSR, list order = train order; udup[u] = 1 when u's list holds
// an item twice; uslot[q] = the first position of uitems[q] within its user's list.
struct SvdppPlan {
  std::vector<int32_t> uoff, uitems, udup, uslot;
};
int svdpp_plan(const int32_t* users, const int32_t* items, int64_t n, int64_t user_num,
               int64_t item_num, SvdppPlan* out);

// WRMF (wrmf_set_train): one side of the confidence matrix as CSR with its launch plan: the light
// rows by decreasing nnz (ties by row id), and for the rows above `heavy` entries the fixed CSR
// sub-ranges [pbeg, pend) of `heavy` entries (the last one shorter) whose partial sums several
// workgroups compute; hoff[h] .. hoff[h + 1] are the parts of heavy row hrow[h].
struct WrmfSide {
  int64_t rows = 0;
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices;
  std::vector<double> conf;
  std::vector<int32_t> order, hrow, prow;
  std::vector<int64_t> hoff, pbeg, pend;
  int32_t n_light = 0, n_heavy = 0, n_parts = 0;
};
// side[0]: users (the input with zero confidences dropped), side[1]: items (its transpose).
// BPRMF_E_RANGE: indptr not running from 0 to nnz or decreasing, a column out of range, columns
// of a row not strictly increasing.
struct WrmfCsrPlan {
  WrmfSide side[2];
};
int wrmf_csr_plan(const int64_t* indptr, const int32_t* indices, const double* conf, int64_t nnz,
                  int64_t user_num, int64_t item_num, int32_t heavy, WrmfCsrPlan* out);

// Item2Vec (sgns_set_noise): the CDF of weights^0.75 / sum for inverse sampling, summed in double
// and stored as float, the last entry 2.0f so that every u in [0, 1) lands.  BPRMF_E_INVALID: a
// negative or NaN weight, weights summing to 0.
int sgns_noise_cdf(const double* weights, int64_t vocab, std::vector<float>* cdf);

// SLIM (slim_set_train): A as CSR with the items of a user ascending and duplicates collapsed
// (A[u, i] = 1), `rows` = the user of every kept entry, and the geometry of the dense i8 operand
// A^T [p_pad, k_pad]: item-major, the user (K) dimension contiguous, both padded to the MFMA tile.
// BPRMF_E_RANGE: an id out of range; BPRMF_E_UNSUPPORTED: sizes past int32 or an operand whose
// byte count overflows, or host memory that runs out while the plan is built.
constexpr int64_t kSlimTile = 128;  // k_pad and p_pad are multiples of it (k_gram's block)
struct SlimPlan {
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices, rows;
  int64_t p_pad = 0, k_pad = 0, operand_bytes = 0;
};
int slim_plan(const int32_t* users, const int32_t* items, int64_t n, int64_t user_num,
              int64_t item_num, SlimPlan* out);
// slim_score / slim_score_rows arguments: BPRMF_E_RANGE for an id out of range.  `items` null:
// users only.
int slim_check_ids(const int32_t* users, const int32_t* items, int64_t n, int64_t user_num,
                   int64_t item_num);
// slim_topk_lists arguments: BPRMF_E_RANGE for an id out of range, BPRMF_E_INVALID for offsets
// that do not start at >= 0 or decrease.  `items` may be null when no list has any.
int slim_check_lists(const int32_t* users, const int64_t* offsets, const int32_t* items,
                     int64_t n_users, int64_t user_num, int64_t item_num);

// NCF (ncf_create): the tables of the zero-gradient Adam steps a row catches up on (k_ncf_catch_up),
// in double as the step's own AdamArgs, as interleaved float pairs.  step: torch's (step_size(s),
// 1 / bc2_sqrt(s)) for s = 1 .. n, n the smallest power of two with b1^n and b2^n <= 2^-26 (past it
// f32 cannot tell the bias corrections from 1: the pair is (lr, 1)), capped at 2^22.  pw: (b1^j,
// b2^(j/2)) for j = 1 .. terms.  BPRMF_E_INVALID: a beta outside [0, 1) or terms < 0.
int ncf_catch_tables(double lr, double b1, double b2, int terms, std::vector<float>* step,
                     std::vector<float>* pw);

}  // namespace bprmf
