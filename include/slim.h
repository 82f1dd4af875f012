/*
 * slim.h — C ABI of the MI355X SLIM path (libbprmf_amd.so): the reference's SLiMRecommender.py
 * SLIM with util/slim.pyx, the item-item elastic net over implicit feedback.
 *
 * A [user_num, item_num] is 0/1 (:42-46).  G = A^T A is a matrix of integer counts, computed on
 * i8 MFMA with i32 accumulators and stored as f64: exact for any user_num < 2^31, equal in every
 * summation order.  Every column `col` of W [item_num, item_num] is an independent coordinate
 * descent over j != col (slim.pyx:43-126), in f64 with separate multiplies and adds and the
 * reference's operation order, so W equals the compiled reference bit for bit:
 *     absolute:  b = (lam alpha) N,  c = (lam (1 - alpha)) N,  N = user_num
 *     ratio:     m = max_{j != col} G[j, col]; m == 0 leaves the column zero; otherwise
 *                b = m lam,  c = ((m (1 - alpha)) / alpha) lam
 *     a = (G[j, col] + G[j, j] w[j]) - g[j];  s = 0 if b >= |a| or a <= 0, else a - b
 *     new = s / (c + G[j, j]);  a move iff fabs(new - w[j]) > tol (a NaN from 0/0 is no move):
 *     w[j] = new and g[k] += G[k, j] delta for every k.
 * Sweeps alternate between all coordinates (mode 0) and the non-zero ones (mode 1): a mode-0
 * sweep with a move switches to mode 1, a sweep without a move ends the column from mode 0 and
 * switches back to mode 0 from mode 1; max_iter counts sweeps of both modes.
 *
 * One workgroup owns a column.  It keeps g and w in LDS while item_num <= chip_max_p (default
 * 9216: two f64 arrays of 9216 entries are 144 KB of the 160 KB) and in a global workspace of
 * its own above that; both paths run the same code and give the same bits.
 * Scores are (A W)[u, i] = sum_{j in N(u)} W[j, i], added one by one in ascending j from +0.0.
 * Conventions are those of bprmf.h: 0 = OK, negative bprmf_status, bprmf_last_error() for the
 * message; host buffers caller-owned, row-major; one host thread per handle.
 */
#ifndef SLIM_H
#define SLIM_H

#include <stdint.h>

#include "bprmf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slim_handle slim_handle;

typedef struct {
  int64_t user_num;
  int64_t item_num;
  int32_t device;
  int32_t chip_max_p; /* g and w stay in LDS while item_num <= chip_max_p; 0 = library default
                         (9216), larger values are clamped to it */
} slim_config;

typedef struct {
  int64_t columns;      /* columns of the call */
  int64_t sweeps;       /* sweeps of both modes, over all columns */
  int64_t moves;        /* coordinate updates applied */
  int64_t capped;       /* columns that ran max_iter sweeps (none when max_iter is 0) */
  double gram_seconds;  /* device time of the last slim_gram */
  double cd_seconds;    /* device time of this call's coordinate descent */
} slim_stats;

#define SLIM_TOPK_MAX 32

int slim_create(const slim_config* cfg, slim_handle** out);
int slim_destroy(slim_handle* h);
/* nnz (user, item) pairs in any order; duplicates collapse (A[u, i] = 1); ids out of range:
 * BPRMF_E_RANGE.  Builds the dense i8 operand A^T on the device and drops an earlier G and W.
 * BPRMF_E_UNSUPPORTED with a message when the operand does not fit the free device memory. */
int slim_set_train(slim_handle* h, const int32_t* users, const int32_t* items, int64_t nnz);
/* G = A^T A, kept in the handle and copied to out [item_num, item_num] if not null; W is reset to
 * zero.  BPRMF_E_STATE before slim_set_train; BPRMF_E_UNSUPPORTED when G and W do not fit. */
int slim_gram(slim_handle* h, double* out_or_null);
/* device time of the last slim_gram (also in slim_stats); BPRMF_E_STATE before it */
int slim_gram_seconds(slim_handle* h, double* seconds);
/* Columns [col_begin, col_end) of W; the other columns keep what they hold.  BPRMF_E_STATE before
 * slim_gram.  BPRMF_E_INVALID: lam < 0, tol < 0, max_iter < 0, alpha outside [0, 1] (NaN too),
 * alpha == 0 with lambda_is_ratio (the reference divides by zero), a bad column range. */
int slim_fit(slim_handle* h, double alpha, double lam, int32_t lambda_is_ratio, int32_t max_iter,
             double tol, int64_t col_begin, int64_t col_end, slim_stats* st);
/* W[:, col_begin:col_end] as [item_num, col_end - col_begin] */
int slim_get_weights(slim_handle* h, int64_t col_begin, int64_t col_end, double* out);
/* (A W)[u, i] for n pairs; ids out of range fail with BPRMF_E_RANGE */
int slim_score(slim_handle* h, const int32_t* users, const int32_t* items, int64_t n, double* out);
/* rows of A W for n users: out [n, item_num] */
int slim_score_rows(slim_handle* h, const int32_t* users, int64_t n, double* out);
/* The argument shape of bprmf_topk_lists: user r ranks items[offsets[r] .. offsets[r + 1]).
 * out_pos / out_score [n_users, k]: positions within the user's list, score descending, ties by
 * the EARLIER position first (a stable descending sort, SLiMRecommender.py:116); past a list's
 * end -1 and -inf.  1 <= k <= SLIM_TOPK_MAX. */
int slim_topk_lists(slim_handle* h, const int32_t* users, const int64_t* offsets,
                    const int32_t* items, int64_t n_users, int32_t k, int32_t* out_pos,
                    double* out_score);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_H */
