// wrmf_capi.cpp — C ABI (include/wrmf.h) of the implicit-feedback ALS path over the kernels of
// wrmf.hip.
//
// One handle = one GPU: X, Y and the two Gram matrices (double, row-major) in HBM, the confidence
// matrix as CSR (user sweep) and, built here on the host, its transpose (item sweep).  Each side
// carries its launch plan: the light rows by decreasing nnz (ties by row id), and for the rows
// above the heavy threshold the fixed CSR sub-ranges of heavy_nnz entries whose partial sums
// several workgroups compute before one workgroup adds them in part order and solves the row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/wrmf.h"
#include "handle.h"
#include "wrmf_kernels.h"

using namespace bprmf;

namespace {
constexpr int32_t kDefaultHeavyNnz = 4096;

struct SidePlan {
  int64_t rows = 0, nnz = 0;
  int64_t* indptr = nullptr;
  int32_t* indices = nullptr;
  double* conf = nullptr;
  int32_t *order = nullptr, *hrow = nullptr, *prow = nullptr;
  int64_t *hoff = nullptr, *pbeg = nullptr, *pend = nullptr;
  int32_t n_light = 0, n_heavy = 0, n_parts = 0;
};
}  // namespace

struct wrmf_handle {
  wrmf_config cfg;
  int32_t heavy = kDefaultHeavyNnz;
  double *X = nullptr, *Y = nullptr;
  double* G[2] = {nullptr, nullptr};  // XtX, YtY
  bool have_G[2] = {false, false};  // wrmf_gram has stored it (a sweep uses it as stored, however
                                    // old: the reference's item sweep sees the XtX of the old X)
  double* gram_parts = nullptr;
  double* partial = nullptr;
  SidePlan side[2];  // 0: users (CSR), 1: items (its transpose)
  bool have_train = false;
  int32_t *d_u = nullptr, *d_i = nullptr;  // predict's staging
  double* d_out = nullptr;
  int64_t pred_cap = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {
int wset_dev(wrmf_handle* h) {
  HIPCHK(hipSetDevice(h->cfg.device));
  return 0;
}
template <typename T>
int up(T** p, const std::vector<T>& v) {
  if (int r = dalloc(p, (int64_t)v.size())) return r;
  if (!v.empty()) HIPCHK(hipMemcpy(*p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return 0;
}
void free_side(SidePlan& s) {
  void* ptrs[] = {s.indptr, s.indices, s.conf, s.order, s.hrow, s.prow, s.hoff, s.pbeg, s.pend};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  s = SidePlan();
}
// the launch plan of one side and its upload
int build_side(SidePlan& s, int64_t rows, const std::vector<int64_t>& indptr,
               const std::vector<int32_t>& indices, const std::vector<double>& conf, int32_t heavy) {
  s.rows = rows;
  s.nnz = (int64_t)indices.size();
  std::vector<int32_t> by(rows);
  std::iota(by.begin(), by.end(), 0);
  std::stable_sort(by.begin(), by.end(), [&](int32_t a, int32_t b) {
    return indptr[a + 1] - indptr[a] > indptr[b + 1] - indptr[b];
  });
  std::vector<int32_t> order, hrow, prow;
  std::vector<int64_t> hoff{0}, pbeg, pend;
  for (int32_t r : by) {
    const int64_t b = indptr[r], e = indptr[r + 1];
    if (e - b <= heavy) {
      order.push_back(r);
      continue;
    }
    hrow.push_back(r);
    for (int64_t x = b; x < e; x += heavy) {
      prow.push_back(r);
      pbeg.push_back(x);
      pend.push_back(std::min<int64_t>(x + heavy, e));
    }
    hoff.push_back((int64_t)prow.size());
  }
  if (prow.size() >= (size_t)INT32_MAX) return fail(BPRMF_E_UNSUPPORTED, "too many heavy-row parts");
  s.n_light = (int32_t)order.size();
  s.n_heavy = (int32_t)hrow.size();
  s.n_parts = (int32_t)prow.size();
  int rc = 0;
  (void)((rc = up(&s.indptr, indptr)) || (rc = up(&s.indices, indices)) || (rc = up(&s.conf, conf)) ||
         (rc = up(&s.order, order)) || (rc = up(&s.hrow, hrow)) || (rc = up(&s.prow, prow)) ||
         (rc = up(&s.hoff, hoff)) || (rc = up(&s.pbeg, pbeg)) || (rc = up(&s.pend, pend)));
  return rc;
}
int do_gram(wrmf_handle* h, int side) {
  const double* T = side == 0 ? h->X : h->Y;
  const int64_t n = side == 0 ? h->cfg.user_num : h->cfg.item_num;
  HIPCHK(wrmf::gram(T, n, h->cfg.factor_num, h->gram_parts, h->G[side], h->stream));
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
  HIPCHK(wrmf::sweep(a, h->stream));
  return 0;
}
int timed_begin(wrmf_handle* h) {
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  return 0;
}
int timed_end(wrmf_handle* h, wrmf_stats* st, int64_t solves, int64_t heavy_rows) {
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipEventSynchronize(h->ev1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (st) {
    st->solves = solves;
    st->heavy_rows = heavy_rows;
    st->seconds = ms * 1e-3;
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
  int rc = 0;
  auto bail = [&](int r) {
    wrmf_destroy(h);
    return r;
  };
  if ((rc = wset_dev(h))) return bail(rc);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess)
    return bail(fail(BPRMF_E_HIP, "stream/event creation failed"));
  const int64_t d = cfg->factor_num;
  const int64_t rows = std::max(cfg->user_num, cfg->item_num);
  const int64_t parts = std::max<int64_t>(1, (rows + wrmf::kGramRows - 1) / wrmf::kGramRows);
  if ((rc = dalloc(&h->X, cfg->user_num * d)) || (rc = dalloc(&h->Y, cfg->item_num * d)) ||
      (rc = dalloc(&h->G[0], d * d)) || (rc = dalloc(&h->G[1], d * d)) ||
      (rc = dalloc(&h->gram_parts, parts * wrmf::gram_part_stride((int)d))))
    return bail(rc);
  auto z = [&](void* p, size_t bytes) { return p && bytes ? hipMemset(p, 0, bytes) : hipSuccess; };
  if (z(h->X, 8 * cfg->user_num * d) || z(h->Y, 8 * cfg->item_num * d))
    return bail(fail(BPRMF_E_HIP, "hipMemset failed"));
  *out = h;
  return 0;
}

int wrmf_destroy(wrmf_handle* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  void* ptrs[] = {h->X, h->Y, h->G[0], h->G[1], h->gram_parts, h->partial, h->d_u, h->d_i, h->d_out};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  free_side(h->side[0]);
  free_side(h->side[1]);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int wrmf_set_train(wrmf_handle* h, const int64_t* indptr, const int32_t* indices, const double* conf,
                   int64_t nnz) {
  if (!h || !indptr || nnz < 0 || (nnz > 0 && (!indices || !conf)))
    return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = wset_dev(h)) return r;
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num;
  if (indptr[0] != 0 || indptr[U] != nnz) return fail(BPRMF_E_RANGE, "indptr must run from 0 to nnz");
  // validate, drop zero confidences (the reference's Pu != 0), count the columns
  std::vector<int64_t> up_(U + 1, 0), ip(I + 1, 0);
  std::vector<int32_t> ui;
  std::vector<double> uc;
  ui.reserve(nnz);
  uc.reserve(nnz);
  for (int64_t u = 0; u < U; ++u) {
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b > e || e > nnz) return fail(BPRMF_E_RANGE, "indptr decreases at row %lld", (long long)u);
    for (int64_t x = b; x < e; ++x) {
      const int32_t i = indices[x];
      if (i < 0 || i >= I) return fail(BPRMF_E_RANGE, "column %d of row %lld out of range", i, (long long)u);
      if (x > b && indices[x - 1] >= i)
        return fail(BPRMF_E_RANGE, "row %lld: column indices must be strictly increasing", (long long)u);
      if (conf[x] == 0.0) continue;
      ui.push_back(i);
      uc.push_back(conf[x]);
      ip[i + 1]++;
    }
    up_[u + 1] = (int64_t)ui.size();
  }
  for (int64_t i = 0; i < I; ++i) ip[i + 1] += ip[i];
  const int64_t kept = (int64_t)ui.size();
  std::vector<int32_t> ii(kept);
  std::vector<double> ic(kept);
  std::vector<int64_t> pos(ip.begin(), ip.end() - 1);
  for (int64_t u = 0; u < U; ++u)
    for (int64_t x = up_[u]; x < up_[u + 1]; ++x) {
      const int64_t q = pos[ui[x]]++;
      ii[q] = (int32_t)u;
      ic[q] = uc[x];
    }
  HIPCHK(hipStreamSynchronize(h->stream));
  free_side(h->side[0]);
  free_side(h->side[1]);
  h->have_train = false;
  if (h->partial) HIPCHK(hipFree(h->partial));
  h->partial = nullptr;
  if (int r = build_side(h->side[0], U, up_, ui, uc, h->heavy)) return r;
  if (int r = build_side(h->side[1], I, ip, ii, ic, h->heavy)) return r;
  const int64_t parts = std::max(h->side[0].n_parts, h->side[1].n_parts);
  if (int r = dalloc(&h->partial, parts * wrmf::partial_stride(h->cfg.factor_num))) return r;
  h->have_train = true;
  return 0;
}

int wrmf_set_weights(wrmf_handle* h, const double* X, const double* Y) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = wset_dev(h)) return r;
  HIPCHK(hipStreamSynchronize(h->stream));
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num, d = h->cfg.factor_num;
  if (X && U) HIPCHK(hipMemcpy(h->X, X, 8 * U * d, hipMemcpyHostToDevice));
  if (Y && I) HIPCHK(hipMemcpy(h->Y, Y, 8 * I * d, hipMemcpyHostToDevice));
  return 0;
}

int wrmf_get_weights(wrmf_handle* h, double* X, double* Y) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = wset_dev(h)) return r;
  HIPCHK(hipStreamSynchronize(h->stream));
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num, d = h->cfg.factor_num;
  if (X && U) HIPCHK(hipMemcpy(X, h->X, 8 * U * d, hipMemcpyDeviceToHost));
  if (Y && I) HIPCHK(hipMemcpy(Y, h->Y, 8 * I * d, hipMemcpyDeviceToHost));
  return 0;
}

int wrmf_gram(wrmf_handle* h, int32_t side, double* out) {
  if (!h || (side != 0 && side != 1)) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = wset_dev(h)) return r;
  if (int r = do_gram(h, side)) return r;
  HIPCHK(hipStreamSynchronize(h->stream));
  const int64_t d = h->cfg.factor_num;
  if (out) HIPCHK(hipMemcpy(out, h->G[side], 8 * d * d, hipMemcpyDeviceToHost));
  return 0;
}

int wrmf_sweep(wrmf_handle* h, int32_t side, wrmf_stats* st) {
  if (!h || (side != 0 && side != 1)) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = wset_dev(h)) return r;
  if (int r = timed_begin(h)) return r;
  if (int r = do_sweep(h, side)) return r;
  return timed_end(h, st, h->side[side].rows, h->side[side].n_heavy);
}

int wrmf_fit(wrmf_handle* h, int32_t epochs, wrmf_stats* st) {
  if (!h || epochs < 0) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = wset_dev(h)) return r;
  if (!h->have_train) return fail(BPRMF_E_STATE, "wrmf_fit needs wrmf_set_train first");
  if (int r = timed_begin(h)) return r;
  const bool fresh = h->cfg.gram_mode == WRMF_GRAM_FRESH;
  for (int32_t e = 0; e < epochs; ++e) {
    int rc = 0;
    // :39-40 both Gram matrices before the user sweep; fresh: XtX after it
    if ((rc = do_gram(h, 1)) || (!fresh && (rc = do_gram(h, 0))) || (rc = do_sweep(h, 0)) ||
        (fresh && (rc = do_gram(h, 0))))
      return rc;
    if ((rc = do_sweep(h, 1))) return rc;
  }
  return timed_end(h, st, (int64_t)epochs * (h->side[0].rows + h->side[1].rows),
                   (int64_t)epochs * (h->side[0].n_heavy + h->side[1].n_heavy));
}

int wrmf_predict(wrmf_handle* h, const int32_t* users, const int32_t* items, int64_t n, double* out) {
  if (!h || n < 0 || (n > 0 && (!users || !items || !out))) return fail(BPRMF_E_INVALID, "bad arguments");
  if (!n) return 0;
  if (int r = wset_dev(h)) return r;
  for (int64_t p = 0; p < n; ++p)
    if (users[p] < 0 || users[p] >= h->cfg.user_num || items[p] < 0 || items[p] >= h->cfg.item_num)
      return fail(BPRMF_E_RANGE, "pair %lld = (%d, %d) out of range", (long long)p, users[p], items[p]);
  if (n > h->pred_cap) {
    void* olds[] = {h->d_u, h->d_i, h->d_out};
    for (void* p : olds)
      if (p) HIPCHK(hipFree(p));
    h->d_u = h->d_i = nullptr;
    h->d_out = nullptr;
    h->pred_cap = 0;
    if (int r = dalloc(&h->d_u, n)) return r;
    if (int r = dalloc(&h->d_i, n)) return r;
    if (int r = dalloc(&h->d_out, n)) return r;
    h->pred_cap = n;
  }
  HIPCHK(hipMemcpyAsync(h->d_u, users, 4 * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_i, items, 4 * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(wrmf::predict(h->X, h->Y, h->cfg.factor_num, h->d_u, h->d_i, n, h->d_out, h->stream));
  HIPCHK(hipMemcpyAsync(out, h->d_out, 8 * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
