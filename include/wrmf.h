/*
 * wrmf.h — C ABI of the MI355X implicit-feedback ALS path (libbprmf_amd.so): the reference's
 * WRMFRecommender.py WRMF (:24-62), weighted regularised matrix factorisation.
 *
 * One epoch is U + I independent d x d symmetric positive-definite systems.  For a user u with
 * positives N(u) and confidences c (C = alpha * train_set, non-zero entries only):
 *     (YtY + sum_{i in N(u)} c_i y_i y_i^T + lambda I) x_u = sum_{i in N(u)} (c_i + 1) y_i
 * and the same for every item from X.  The reference takes YtY and XtX before the user sweep
 * (:39-40), so its item sweep solves against the XtX of the old X; gram_mode 0 does the same,
 * gram_mode 1 recomputes XtX after the user sweep (textbook ALS).  Rows without entries solve to
 * exactly +0.0.  Tables and all device arithmetic are double: the item systems are too
 * ill-conditioned for float (WRMF section).
 *
 * Results are deterministic: the Gram matrices and the heavy rows' partial sums are added in a
 * fixed order, without atomics; the same inputs and the same heavy_nnz give the same bits.
 * Conventions are those of bprmf.h: 0 = OK, negative bprmf_status, bprmf_last_error() for the
 * message; host buffers caller-owned, row-major; one host thread per handle.
 */
#ifndef WRMF_H
#define WRMF_H

#include <stdint.h>

#include "bprmf.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { WRMF_GRAM_REFERENCE = 0, WRMF_GRAM_FRESH = 1 };

typedef struct wrmf_handle wrmf_handle;

typedef struct {
  int64_t user_num;
  int64_t item_num;
  int32_t factor_num; /* 1..128 (:25 default 20) */
  int32_t device;
  double lambda_val;  /* :25 default 0.1 */
  int32_t gram_mode;  /* WRMF_GRAM_REFERENCE (stale XtX, :39-40) / WRMF_GRAM_FRESH */
  int32_t heavy_nnz;  /* rows with more entries are accumulated by several workgroups over
                         sub-ranges of heavy_nnz entries; 0 = library default (4096) */
} wrmf_config;

typedef struct {
  int64_t solves;     /* rows solved by the call (empty rows included) */
  int64_t heavy_rows; /* of these, rows that took the split path */
  double seconds;     /* device time of the call */
} wrmf_stats;

int wrmf_create(const wrmf_config* cfg, wrmf_handle** out);
int wrmf_destroy(wrmf_handle* h);
/* C = alpha * R as CSR: indptr [user_num + 1], indices / conf [nnz]; column indices strictly
 * increasing within a row (BPRMF_E_RANGE otherwise, and for ids out of range).  Entries whose
 * conf is 0 are dropped, as the reference's `Pu != 0` does.  The by-item structure is built here. */
int wrmf_set_train(wrmf_handle* h, const int64_t* indptr, const int32_t* indices, const double* conf,
                   int64_t nnz);
/* X [user_num, d], Y [item_num, d]; a null table is left as it is */
int wrmf_set_weights(wrmf_handle* h, const double* X, const double* Y);
int wrmf_get_weights(wrmf_handle* h, double* X, double* Y);
/* side 0: G <- XtX, side 1: G <- YtY; stored in the handle and copied to out [d, d] if not null */
int wrmf_gram(wrmf_handle* h, int32_t side, double* out_or_null);
/* side 0: every user row from Y and the stored YtY; side 1: every item row from X and the stored
 * XtX (BPRMF_E_STATE when that Gram matrix or the train set is missing) */
int wrmf_sweep(wrmf_handle* h, int32_t side, wrmf_stats* st);
/* `epochs` epochs of fit() (:38-56), composed from wrmf_gram and wrmf_sweep by gram_mode */
int wrmf_fit(wrmf_handle* h, int32_t epochs, wrmf_stats* st);
/* x_u . y_i for n pairs; ids out of range fail with BPRMF_E_RANGE */
int wrmf_predict(wrmf_handle* h, const int32_t* users, const int32_t* items, int64_t n, double* out);

#ifdef __cplusplus
}
#endif

#endif /* WRMF_H */
