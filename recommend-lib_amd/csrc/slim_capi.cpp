// slim_capi.cpp — C ABI (include/slim.h) of the SLIM path over the kernels of slim.hip.
//
// One handle = one GPU: A as CSR (items ascending within a user, built and checked on the host by
// model_plan.h slim_plan) and as the dense i8 operand A^T, then G, its diagonal and W [p, p] in
// f64.  W is row-major, so a row of A W is the sum of the user's contiguous W[j, :] rows.
#include <algorithm>
#include <cmath>
#include <utility>

#include "../../include/slim.h"
#include "dev.h"
#include "model_plan.h"
#include "slim_kernels.h"

using namespace bprmf;

struct slim_handle {
  slim_config cfg;
  int32_t chip_max_p = slim::kChipMaxP;
  Lane lane;
  DevBuf<int64_t> indptr;
  DevBuf<int32_t> indices;
  DevBuf<int8_t> At;
  int64_t p_pad = 0, k_pad = 0;
  bool have_train = false;
  DevBuf<double> G, diag, W, ws;
  bool have_gram = false;
  double gram_seconds = 0.0;
  DevBuf<unsigned long long> stats;
  DevBuf<int32_t> d_u, d_i, d_pos;  // staging of the scoring calls (grow-only)
  DevBuf<int64_t> d_off;
  DevBuf<double> d_out, d_sc;
};

namespace {
// `bytes` more of device memory, with 64 MB to spare: a clear message instead of a HIP error later
int need_memory(int64_t bytes, const char* what) {
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if ((double)bytes + 64e6 > (double)free_b)
    return fail(BPRMF_E_UNSUPPORTED, "%s needs %.3f GB of device memory, %.3f GB are free", what,
                bytes * 1e-9, free_b * 1e-9);
  return 0;
}
}  // namespace

extern "C" {

int slim_create(const slim_config* cfg, slim_handle** out) {
  if (!cfg || !out) return fail(BPRMF_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->user_num < 0 || cfg->item_num < 0 || cfg->chip_max_p < 0)
    return fail(BPRMF_E_INVALID, "need user_num, item_num, chip_max_p >= 0");
  if (cfg->user_num >= INT32_MAX - kSlimTile || cfg->item_num >= INT32_MAX - kSlimTile)
    return fail(BPRMF_E_UNSUPPORTED, "row counts must fit int32");
  auto* h = new slim_handle();
  h->cfg = *cfg;
  if (cfg->chip_max_p > 0) h->chip_max_p = std::min(cfg->chip_max_p, slim::kChipMaxP);
  int rc = 0;
  if ((rc = h->lane.open(cfg->device)) || (rc = h->stats.alloc(3))) {
    slim_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int slim_destroy(slim_handle* h) {
  if (!h) return 0;
  (void)h->lane.use();
  if (h->lane.stream) (void)hipStreamSynchronize(h->lane.stream);
  delete h;
  return 0;
}

int slim_set_train(slim_handle* h, const int32_t* users, const int32_t* items, int64_t nnz) {
  if (!h || nnz < 0 || (nnz > 0 && (!users || !items))) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  SlimPlan p;
  if (int r = slim_plan(users, items, nnz, h->cfg.user_num, h->cfg.item_num, &p)) return r;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  // the old set goes first, so both never share the device: from here a failure leaves none
  h->have_train = h->have_gram = false;
  h->indptr.reset();
  h->indices.reset();
  h->At.reset();
  h->G.reset();
  h->diag.reset();
  h->W.reset();
  h->ws.reset();
  if (int r = need_memory(p.operand_bytes + 16 * (int64_t)p.indices.size(), "the dense i8 operand"))
    return r;
  DevBuf<int64_t> indptr;
  DevBuf<int32_t> indices, rows;
  DevBuf<int8_t> At;
  int rc = 0;
  if ((rc = indptr.upload(p.indptr)) || (rc = indices.upload(p.indices)) ||
      (rc = rows.upload(p.rows)) || (rc = At.zalloc(p.operand_bytes)))
    return rc;
  HIPCHK(slim::scatter(rows, indices, (int64_t)p.indices.size(), At, p.k_pad, h->lane.stream));
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  h->indptr = std::move(indptr);
  h->indices = std::move(indices);
  h->At = std::move(At);
  h->p_pad = p.p_pad;
  h->k_pad = p.k_pad;
  h->have_train = true;
  return 0;
}

int slim_gram(slim_handle* h, double* out) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = h->lane.use()) return r;
  if (!h->have_train) return fail(BPRMF_E_STATE, "slim_gram needs slim_set_train first");
  const int64_t p = h->cfg.item_num;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  h->have_gram = false;
  if (h->G.size() != p * p || h->W.size() != p * p) {
    h->G.reset();
    h->W.reset();
    h->diag.reset();
    if (p > 0 && p > (INT64_MAX / 16) / p) return fail(BPRMF_E_UNSUPPORTED, "item_num^2 overflows");
    if (int r = need_memory(16 * p * p + 8 * p, "G and W (two item_num^2 f64 matrices)")) return r;
    int rc = 0;
    if ((rc = h->G.alloc(p * p)) || (rc = h->W.alloc(p * p)) || (rc = h->diag.alloc(p))) return rc;
  }
  if (p > 0) HIPCHK(hipMemsetAsync(h->W, 0, 8 * (size_t)(p * p), h->lane.stream));
  if (int r = h->lane.begin()) return r;
  HIPCHK(slim::gram(h->At, p, h->p_pad, h->k_pad, h->G, h->diag, h->lane.stream));
  if (int r = h->lane.end(&h->gram_seconds)) return r;
  h->have_gram = true;
  if (out && p > 0) HIPCHK(hipMemcpy(out, h->G, 8 * (size_t)(p * p), hipMemcpyDeviceToHost));
  return 0;
}

int slim_gram_seconds(slim_handle* h, double* seconds) {
  if (!h || !seconds) return fail(BPRMF_E_INVALID, "null argument");
  if (!h->have_gram) return fail(BPRMF_E_STATE, "slim_gram_seconds needs slim_gram first");
  *seconds = h->gram_seconds;
  return 0;
}

int slim_fit(slim_handle* h, double alpha, double lam, int32_t lambda_is_ratio, int32_t max_iter,
             double tol, int64_t col_begin, int64_t col_end, slim_stats* st) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = h->lane.use()) return r;
  if (!h->have_train) return fail(BPRMF_E_STATE, "slim_fit needs slim_set_train first");
  if (!h->have_gram) return fail(BPRMF_E_STATE, "slim_fit needs slim_gram first");
  const int64_t p = h->cfg.item_num;
  if (!(lam >= 0.0) || !(tol >= 0.0) || max_iter < 0 || !std::isfinite(lam) || !std::isfinite(tol))
    return fail(BPRMF_E_INVALID, "need finite lam >= 0, tol >= 0 and max_iter >= 0");
  if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(BPRMF_E_INVALID, "alpha must be in [0, 1]");
  if (lambda_is_ratio && alpha == 0.0)
    return fail(BPRMF_E_INVALID, "alpha == 0 with lambda_is_ratio divides by zero");
  if (col_begin < 0 || col_end < col_begin || col_end > p)
    return fail(BPRMF_E_INVALID, "columns [%lld, %lld) outside [0, %lld)", (long long)col_begin,
                (long long)col_end, (long long)p);
  const int64_t cols = col_end - col_begin;
  slim::Cd a{};
  a.G = h->G;
  a.diag = h->diag;
  a.W = h->W;
  a.stats = h->stats;
  a.p = (int32_t)p;
  a.col_begin = col_begin;
  a.col_end = col_end;
  a.alpha = alpha;
  a.lam = lam;
  a.N = (double)h->cfg.user_num;
  a.tol = tol;
  a.ratio = lambda_is_ratio ? 1 : 0;
  a.max_iter = max_iter;
  a.blocks = slim::cd_blocks(cols);
  a.chip = p <= h->chip_max_p;
  if (!a.chip && cols > 0) {
    if (int r = h->ws.reserve((int64_t)a.blocks * 2 * p)) return r;
  }
  a.ws = h->ws;
  HIPCHK(hipMemsetAsync(h->stats, 0, 3 * sizeof(unsigned long long), h->lane.stream));
  if (int r = h->lane.begin()) return r;
  HIPCHK(slim::coordinate_descent(a, h->lane.stream));
  double seconds = 0.0;
  if (int r = h->lane.end(&seconds)) return r;
  unsigned long long s3[3];
  HIPCHK(hipMemcpy(s3, h->stats, sizeof(s3), hipMemcpyDeviceToHost));
  if (st) {
    st->columns = cols;
    st->sweeps = (int64_t)s3[0];
    st->moves = (int64_t)s3[1];
    st->capped = (int64_t)s3[2];
    st->gram_seconds = h->gram_seconds;
    st->cd_seconds = seconds;
  }
  return 0;
}

int slim_get_weights(slim_handle* h, int64_t col_begin, int64_t col_end, double* out) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = h->lane.use()) return r;
  if (!h->have_gram) return fail(BPRMF_E_STATE, "slim_get_weights needs slim_gram first");
  const int64_t p = h->cfg.item_num;
  if (col_begin < 0 || col_end < col_begin || col_end > p || (col_end > col_begin && !out))
    return fail(BPRMF_E_INVALID, "bad column range or null output");
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  const size_t wbytes = 8 * (size_t)(col_end - col_begin);
  if (wbytes && p)
    HIPCHK(hipMemcpy2D(out, wbytes, h->W.get() + col_begin, 8 * (size_t)p, wbytes, (size_t)p,
                       hipMemcpyDeviceToHost));
  return 0;
}

int slim_score(slim_handle* h, const int32_t* users, const int32_t* items, int64_t n, double* out) {
  if (!h || n < 0 || (n > 0 && (!users || !items || !out))) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  if (!h->have_gram) return fail(BPRMF_E_STATE, "slim_score needs slim_gram first");
  if (!n) return 0;
  if (int r = slim_check_ids(users, items, n, h->cfg.user_num, h->cfg.item_num)) return r;
  int rc = 0;
  if ((rc = h->d_u.reserve(n)) || (rc = h->d_i.reserve(n)) || (rc = h->d_out.reserve(n))) return rc;
  HIPCHK(hipMemcpyAsync(h->d_u, users, 4 * n, hipMemcpyHostToDevice, h->lane.stream));
  HIPCHK(hipMemcpyAsync(h->d_i, items, 4 * n, hipMemcpyHostToDevice, h->lane.stream));
  HIPCHK(slim::score(h->indptr, h->indices, h->W, h->cfg.item_num, h->d_u, h->d_i, n, h->d_out,
                     h->lane.stream));
  HIPCHK(hipMemcpyAsync(out, h->d_out, 8 * n, hipMemcpyDeviceToHost, h->lane.stream));
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  return 0;
}

int slim_score_rows(slim_handle* h, const int32_t* users, int64_t n, double* out) {
  if (!h || n < 0 || (n > 0 && (!users || !out))) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  if (!h->have_gram) return fail(BPRMF_E_STATE, "slim_score_rows needs slim_gram first");
  const int64_t p = h->cfg.item_num;
  if (!n || !p) return 0;
  if (int r = slim_check_ids(users, nullptr, n, h->cfg.user_num, h->cfg.item_num)) return r;
  int rc = 0;
  if ((rc = h->d_u.reserve(n)) || (rc = h->d_out.reserve(n * p))) return rc;
  HIPCHK(hipMemcpyAsync(h->d_u, users, 4 * n, hipMemcpyHostToDevice, h->lane.stream));
  HIPCHK(slim::score_rows(h->indptr, h->indices, h->W, p, h->d_u, n, h->d_out, h->lane.stream));
  HIPCHK(hipMemcpyAsync(out, h->d_out, 8 * n * p, hipMemcpyDeviceToHost, h->lane.stream));
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  return 0;
}

int slim_topk_lists(slim_handle* h, const int32_t* users, const int64_t* offsets,
                    const int32_t* items, int64_t n_users, int32_t k, int32_t* out_pos,
                    double* out_score) {
  if (!h || n_users < 0 || (n_users > 0 && (!users || !offsets || !out_pos || !out_score)))
    return fail(BPRMF_E_INVALID, "bad arguments");
  if (k < 1 || k > SLIM_TOPK_MAX) return fail(BPRMF_E_INVALID, "k must be in 1..%d", SLIM_TOPK_MAX);
  if (int r = h->lane.use()) return r;
  if (!h->have_gram) return fail(BPRMF_E_STATE, "slim_topk_lists needs slim_gram first");
  if (!n_users) return 0;
  if (offsets[n_users] > offsets[0] && !items) return fail(BPRMF_E_INVALID, "null items");
  if (int r = slim_check_lists(users, offsets, items, n_users, h->cfg.user_num, h->cfg.item_num))
    return r;
  for (int64_t r = 0; r < n_users; ++r)
    if (offsets[r + 1] - offsets[r] > INT32_MAX) return fail(BPRMF_E_UNSUPPORTED, "a list is too long");
  const int64_t total = offsets[n_users];
  int rc = 0;
  if ((rc = h->d_u.reserve(n_users)) || (rc = h->d_off.reserve(n_users + 1)) ||
      (rc = h->d_i.reserve(total)) || (rc = h->d_sc.reserve(total)) ||
      (rc = h->d_pos.reserve(n_users * k)) || (rc = h->d_out.reserve(n_users * k)))
    return rc;
  hipStream_t s = h->lane.stream;
  HIPCHK(hipMemcpyAsync(h->d_u, users, 4 * n_users, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->d_off, offsets, 8 * (n_users + 1), hipMemcpyHostToDevice, s));
  if (total > 0) HIPCHK(hipMemcpyAsync(h->d_i, items, 4 * total, hipMemcpyHostToDevice, s));
  HIPCHK(slim::topk_lists(h->indptr, h->indices, h->W, h->cfg.item_num, h->d_u, h->d_off, h->d_i,
                          n_users, k, h->d_sc, h->d_pos, h->d_out, s));
  HIPCHK(hipMemcpyAsync(out_pos, h->d_pos, 4 * n_users * k, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(out_score, h->d_out, 8 * n_users * k, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
