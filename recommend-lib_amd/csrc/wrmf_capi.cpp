// wrmf_capi.cpp — C ABI (include/wrmf.h) of the implicit-feedback ALS path over the kernels of
// wrmf.hip.
//
// One handle = one GPU: X, Y and the two Gram matrices (double, row-major) in HBM, the confidence
// matrix as CSR (user sweep) and its transpose (item sweep), both built on the host with their
// launch plans (model_plan.h wrmf_csr_plan): the light rows by decreasing nnz, and for the rows
// above the heavy threshold the fixed CSR sub-ranges of heavy_nnz entries whose partial sums
// several workgroups compute before one workgroup adds them in part order and solves the row.
#include <algorithm>
#include <utility>

#include "../../include/wrmf.h"
#include "dev.h"
#include "model_plan.h"
#include "wrmf_kernels.h"

using namespace bprmf;

namespace {
constexpr int32_t kDefaultHeavyNnz = 4096;

struct SidePlan {  // a WrmfSide on the device
  int64_t rows = 0;
  DevBuf<int64_t> indptr;
  DevBuf<int32_t> indices;
  DevBuf<double> conf;
  DevBuf<int32_t> order, hrow, prow;
  DevBuf<int64_t> hoff, pbeg, pend;
  int32_t n_light = 0, n_heavy = 0, n_parts = 0;
};
}  // namespace

struct wrmf_handle {
  wrmf_config cfg;
  int32_t heavy = kDefaultHeavyNnz;
  Lane lane;
  DevBuf<double> X, Y;
  DevBuf<double> G[2];  // XtX, YtY
  bool have_G[2] = {false, false};  // wrmf_gram has stored it (a sweep uses it as stored, however
                                    // old: the reference's item sweep sees the XtX of the old X)
  DevBuf<double> gram_parts;
  DevBuf<double> partial;
  SidePlan side[2];  // 0: users (CSR), 1: items (its transpose)
  bool have_train = false;  // side[] and partial hold a whole train set
  DevBuf<int32_t> d_u, d_i;  // predict's staging (grow-only)
  DevBuf<double> d_out;
};

namespace {
int upload_side(SidePlan& s, const WrmfSide& p) {
  s.rows = p.rows;
  s.n_light = p.n_light;
  s.n_heavy = p.n_heavy;
  s.n_parts = p.n_parts;
  int rc = 0;
  (void)((rc = s.indptr.upload(p.indptr)) || (rc = s.indices.upload(p.indices)) ||
         (rc = s.conf.upload(p.conf)) || (rc = s.order.upload(p.order)) ||
         (rc = s.hrow.upload(p.hrow)) || (rc = s.prow.upload(p.prow)) ||
         (rc = s.hoff.upload(p.hoff)) || (rc = s.pbeg.upload(p.pbeg)) || (rc = s.pend.upload(p.pend)));
  return rc;
}
int do_gram(wrmf_handle* h, int side) {
  const double* T = side == 0 ? h->X : h->Y;
  const int64_t n = side == 0 ? h->cfg.user_num : h->cfg.item_num;
  HIPCHK(wrmf::gram(T, n, h->cfg.factor_num, h->gram_parts, h->G[side], h->lane.stream));
  h->have_G[side] = true;
  return 0;
}
int do_sweep(wrmf_handle* h, int side) {
  if (!h->have_train) return fail(BPRMF_E_STATE, "wrmf_sweep needs wrmf_set_train first");
  if (!h->have_G[1 - side])
    return fail(BPRMF_E_STATE, "wrmf_sweep(side %d) needs wrmf_gram(side %d) first", side, 1 - side);
  const SidePlan& s = h->side[side];
  wrmf::Sweep a{};
  a.indptr = s.indptr;
  a.indices = s.indices;
  a.conf = s.conf;
  a.Tin = side == 0 ? h->Y : h->X;
  a.Tout = side == 0 ? h->X : h->Y;
  a.G = h->G[1 - side];
  a.order = s.order;
  a.n_light = s.n_light;
  a.hrow = s.hrow;
  a.hoff = s.hoff;
  a.n_heavy = s.n_heavy;
  a.prow = s.prow;
  a.pbeg = s.pbeg;
  a.pend = s.pend;
  a.n_parts = s.n_parts;
  a.partial = h->partial;
  a.d = h->cfg.factor_num;
  a.lam = h->cfg.lambda_val;
  HIPCHK(wrmf::sweep(a, h->lane.stream));
  return 0;
}
// the end of a timed call: waits for it and fills the stats
int finish(wrmf_handle* h, wrmf_stats* st, int64_t solves, int64_t heavy_rows) {
  double seconds = 0.0;
  if (int r = h->lane.end(&seconds)) return r;
  if (st) {
    st->solves = solves;
    st->heavy_rows = heavy_rows;
    st->seconds = seconds;
  }
  return 0;
}
}  // namespace

extern "C" {

int wrmf_create(const wrmf_config* cfg, wrmf_handle** out) {
  if (!cfg || !out) return fail(BPRMF_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->user_num < 0 || cfg->item_num < 0 || cfg->heavy_nnz < 0)
    return fail(BPRMF_E_INVALID, "need user_num, item_num, heavy_nnz >= 0");
  if (cfg->factor_num < 1 || cfg->factor_num > wrmf::kMaxFactors)
    return fail(BPRMF_E_UNSUPPORTED, "factor_num must be in 1..%d", wrmf::kMaxFactors);
  if (cfg->gram_mode != WRMF_GRAM_REFERENCE && cfg->gram_mode != WRMF_GRAM_FRESH)
    return fail(BPRMF_E_INVALID, "unknown gram_mode");
  if (cfg->user_num >= INT32_MAX || cfg->item_num >= INT32_MAX)
    return fail(BPRMF_E_UNSUPPORTED, "row counts must fit int32");
  auto* h = new wrmf_handle();
  h->cfg = *cfg;
  h->heavy = cfg->heavy_nnz > 0 ? cfg->heavy_nnz : kDefaultHeavyNnz;
  const int64_t d = cfg->factor_num;
  const int64_t rows = std::max(cfg->user_num, cfg->item_num);
  const int64_t parts = std::max<int64_t>(1, (rows + wrmf::kGramRows - 1) / wrmf::kGramRows);
  int rc = 0;
  if ((rc = h->lane.open(cfg->device)) || (rc = h->X.zalloc(cfg->user_num * d)) ||
      (rc = h->Y.zalloc(cfg->item_num * d)) || (rc = h->G[0].alloc(d * d)) ||
      (rc = h->G[1].alloc(d * d)) ||
      (rc = h->gram_parts.alloc(parts * wrmf::gram_part_stride((int)d)))) {
    wrmf_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int wrmf_destroy(wrmf_handle* h) {
  if (!h) return 0;
  (void)h->lane.use();
  if (h->lane.stream) (void)hipStreamSynchronize(h->lane.stream);
  delete h;
  return 0;
}

int wrmf_set_train(wrmf_handle* h, const int64_t* indptr, const int32_t* indices, const double* conf,
                   int64_t nnz) {
  if (!h || !indptr || nnz < 0 || (nnz > 0 && (!indices || !conf)))
    return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  WrmfCsrPlan p;
  if (int r = wrmf_csr_plan(indptr, indices, conf, nnz, h->cfg.user_num, h->cfg.item_num, h->heavy, &p))
    return r;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  // the old set goes first, so both never share the device: from here a failure leaves none
  h->have_train = false;
  h->side[0] = SidePlan();
  h->side[1] = SidePlan();
  h->partial.reset();
  SidePlan side[2];
  DevBuf<double> partial;
  const int64_t parts = std::max(p.side[0].n_parts, p.side[1].n_parts);
  int rc = 0;
  if ((rc = upload_side(side[0], p.side[0])) || (rc = upload_side(side[1], p.side[1])) ||
      (rc = partial.alloc(parts * wrmf::partial_stride(h->cfg.factor_num))))
    return rc;
  h->side[0] = std::move(side[0]);
  h->side[1] = std::move(side[1]);
  h->partial = std::move(partial);
  h->have_train = true;
  return 0;
}

int wrmf_set_weights(wrmf_handle* h, const double* X, const double* Y) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = h->lane.use()) return r;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num, d = h->cfg.factor_num;
  if (X && U) HIPCHK(hipMemcpy(h->X, X, 8 * U * d, hipMemcpyHostToDevice));
  if (Y && I) HIPCHK(hipMemcpy(h->Y, Y, 8 * I * d, hipMemcpyHostToDevice));
  return 0;
}

int wrmf_get_weights(wrmf_handle* h, double* X, double* Y) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = h->lane.use()) return r;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num, d = h->cfg.factor_num;
  if (X && U) HIPCHK(hipMemcpy(X, h->X, 8 * U * d, hipMemcpyDeviceToHost));
  if (Y && I) HIPCHK(hipMemcpy(Y, h->Y, 8 * I * d, hipMemcpyDeviceToHost));
  return 0;
}

int wrmf_gram(wrmf_handle* h, int32_t side, double* out) {
  if (!h || (side != 0 && side != 1)) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  if (int r = do_gram(h, side)) return r;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  const int64_t d = h->cfg.factor_num;
  if (out) HIPCHK(hipMemcpy(out, h->G[side], 8 * d * d, hipMemcpyDeviceToHost));
  return 0;
}

int wrmf_sweep(wrmf_handle* h, int32_t side, wrmf_stats* st) {
  if (!h || (side != 0 && side != 1)) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  if (int r = h->lane.begin()) return r;
  if (int r = do_sweep(h, side)) return r;
  return finish(h, st, h->side[side].rows, h->side[side].n_heavy);
}

int wrmf_fit(wrmf_handle* h, int32_t epochs, wrmf_stats* st) {
  if (!h || epochs < 0) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  if (!h->have_train) return fail(BPRMF_E_STATE, "wrmf_fit needs wrmf_set_train first");
  if (int r = h->lane.begin()) return r;
  const bool fresh = h->cfg.gram_mode == WRMF_GRAM_FRESH;
  for (int32_t e = 0; e < epochs; ++e) {
    int rc = 0;
    // :39-40 both Gram matrices before the user sweep; fresh: XtX after it
    if ((rc = do_gram(h, 1)) || (!fresh && (rc = do_gram(h, 0))) || (rc = do_sweep(h, 0)) ||
        (fresh && (rc = do_gram(h, 0))))
      return rc;
    if ((rc = do_sweep(h, 1))) return rc;
  }
  return finish(h, st, (int64_t)epochs * (h->side[0].rows + h->side[1].rows),
                   (int64_t)epochs * (h->side[0].n_heavy + h->side[1].n_heavy));
}

int wrmf_predict(wrmf_handle* h, const int32_t* users, const int32_t* items, int64_t n, double* out) {
  if (!h || n < 0 || (n > 0 && (!users || !items || !out))) return fail(BPRMF_E_INVALID, "bad arguments");
  if (!n) return 0;
  if (int r = h->lane.use()) return r;
  for (int64_t p = 0; p < n; ++p)
    if (users[p] < 0 || users[p] >= h->cfg.user_num || items[p] < 0 || items[p] >= h->cfg.item_num)
      return fail(BPRMF_E_RANGE, "pair %lld = (%d, %d) out of range", (long long)p, users[p], items[p]);
  int rc = 0;
  if ((rc = h->d_u.reserve(n)) || (rc = h->d_i.reserve(n)) || (rc = h->d_out.reserve(n))) return rc;
  HIPCHK(hipMemcpyAsync(h->d_u, users, 4 * n, hipMemcpyHostToDevice, h->lane.stream));
  HIPCHK(hipMemcpyAsync(h->d_i, items, 4 * n, hipMemcpyHostToDevice, h->lane.stream));
  HIPCHK(wrmf::predict(h->X, h->Y, h->cfg.factor_num, h->d_u, h->d_i, n, h->d_out, h->lane.stream));
  HIPCHK(hipMemcpyAsync(out, h->d_out, 8 * n, hipMemcpyDeviceToHost, h->lane.stream));
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  return 0;
}

}  // extern "C"
