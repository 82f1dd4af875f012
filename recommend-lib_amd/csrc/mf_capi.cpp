// mf_capi.cpp — C ABI (include/mf.h) of the rating-SGD path over the kernels of mf.hip.
//
// One handle = one GPU: P, Q (double, row-major) and the two bias vectors in HBM, the train
// samples laid out by dependency level (model_plan.h mf_level_plan; SVDpp: train order, one level
// per sample, with the per-user lists of svdpp_plan).  After a failed mf_set_train the handle
// holds the previous train set whole.
#include <utility>

#include "../../include/mf.h"
#include "dev.h"
#include "mf_kernels.h"
#include "model_plan.h"

using namespace bprmf;

namespace {
struct TrainSet {
  DevBuf<int32_t> su, si, loff;
  DevBuf<double> sr;
  DevBuf<int32_t> uoff, uitems, udup, uslot;  // SVDpp
  int64_t n = 0;
  int32_t levels = 0;
};
}  // namespace

struct mf_handle {
  mf_config cfg;
  Lane lane;
  DevBuf<double> P, Q, bu, bi;
  DevBuf<double> Y;  // SVDpp: yj [I, k]
  TrainSet t;
  double gm = 0.0;
  DevBuf<int32_t> d_err;
};

namespace {
mf::Args args_of(const mf_handle* h) {
  mf::Args a{};
  a.su = h->t.su;
  a.si = h->t.si;
  a.sr = h->t.sr;
  a.loff = h->t.loff;
  a.levels = h->t.levels;
  a.k = h->cfg.n_factors;
  a.P = h->P;
  a.Q = h->Q;
  a.bu = h->bu;
  a.bi = h->bi;
  // SVD.fit: global_mean = 0 when not biased (:121-124); RSVD keeps it for the bias decay, and
  // SVDpp always adds it (:199, :246)
  a.gm = (h->cfg.model == MF_SVD && !h->cfg.variant) ? 0.0 : h->gm;
  a.variant = h->cfg.variant;
  for (int x = 0; x < 4; ++x) {
    a.lr[x] = h->cfg.lr[x];
    a.reg[x] = h->cfg.reg[x];
  }
  a.Y = h->Y;
  a.uoff = h->t.uoff;
  a.uitems = h->t.uitems;
  a.udup = h->t.udup;
  a.uslot = h->t.uslot;
  a.lr_yj = h->cfg.lr_yj;
  a.reg_yj = h->cfg.reg_yj;
  return a;
}
}  // namespace

extern "C" {

int mf_create(const mf_config* cfg, mf_handle** out) {
  if (!cfg || !out) return fail(BPRMF_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->user_num < 0 || cfg->item_num < 0 || cfg->n_factors <= 0)
    return fail(BPRMF_E_INVALID, "need user_num, item_num >= 0 and n_factors > 0");
  if (cfg->n_factors > 1024) return fail(BPRMF_E_UNSUPPORTED, "n_factors must be <= 1024");
  if (cfg->model != MF_SVD && cfg->model != MF_RSVD && cfg->model != MF_SVDPP)
    return fail(BPRMF_E_INVALID, "unknown model");
  if (cfg->model == MF_RSVD && cfg->variant != 1 && cfg->variant != 2)
    return fail(BPRMF_E_INVALID, "RSVD version must be 1 or 2");
  if (cfg->user_num >= INT32_MAX || cfg->item_num >= INT32_MAX)
    return fail(BPRMF_E_UNSUPPORTED, "row counts must fit int32");
  auto* h = new mf_handle();
  h->cfg = *cfg;
  const int64_t k = cfg->n_factors;
  int rc = 0;
  if ((rc = h->lane.open(cfg->device)) || (rc = h->P.zalloc(cfg->user_num * k)) ||
      (rc = h->Q.zalloc(cfg->item_num * k)) || (rc = h->bu.zalloc(cfg->user_num)) ||
      (rc = h->bi.zalloc(cfg->item_num)) || (rc = h->d_err.zalloc(1)) ||
      (cfg->model == MF_SVDPP && (rc = h->Y.zalloc(cfg->item_num * k)))) {
    mf_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int mf_destroy(mf_handle* h) {
  if (!h) return 0;
  (void)h->lane.use();
  if (h->lane.stream) (void)hipStreamSynchronize(h->lane.stream);
  delete h;
  return 0;
}

int mf_set_train(mf_handle* h, const int32_t* users, const int32_t* items, const double* ratings,
                 int64_t n, double global_mean) {
  if (!h || n < 0 || (n > 0 && (!users || !items || !ratings))) return fail(BPRMF_E_INVALID, "bad arguments");
  if (n >= INT32_MAX) return fail(BPRMF_E_UNSUPPORTED, "at most 2^31 - 1 train rows");
  if (int r = h->lane.use()) return r;
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num;
  TrainSet t;  // built beside the handle's, which it replaces only when whole
  int rc = 0;
  if (h->cfg.model == MF_SVDPP) {
    // samples in train order (one level each) and ur[u] (:222-224) as CSR
    SvdppPlan p;
    if ((rc = svdpp_plan(users, items, n, U, I, &p)) || (rc = t.su.upload(users, n)) ||
        (rc = t.si.upload(items, n)) || (rc = t.sr.upload(ratings, n)) ||
        (rc = t.uoff.upload(p.uoff)) || (rc = t.uitems.upload(p.uitems)) ||
        (rc = t.udup.upload(p.udup)) || (rc = t.uslot.upload(p.uslot)))
      return rc;
    t.levels = (int32_t)n;
  } else {
    MfLevelPlan p;
    if ((rc = mf_level_plan(users, items, ratings, n, U, I, &p)) || (rc = t.su.upload(p.su)) ||
        (rc = t.si.upload(p.si)) || (rc = t.sr.upload(p.sr)) || (rc = t.loff.upload(p.loff)))
      return rc;
    t.levels = p.levels;
  }
  t.n = n;
  h->t = std::move(t);
  h->gm = global_mean;
  return 0;
}

int mf_set_weights(mf_handle* h, const double* P, const double* Q, const double* bu, const double* bi) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = h->lane.use()) return r;
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num, k = h->cfg.n_factors;
  if (P && U) HIPCHK(hipMemcpy(h->P, P, 8 * U * k, hipMemcpyHostToDevice));
  if (Q && I) HIPCHK(hipMemcpy(h->Q, Q, 8 * I * k, hipMemcpyHostToDevice));
  if (U) HIPCHK(bu ? hipMemcpy(h->bu, bu, 8 * U, hipMemcpyHostToDevice) : hipMemset(h->bu, 0, 8 * U));
  if (I) HIPCHK(bi ? hipMemcpy(h->bi, bi, 8 * I, hipMemcpyHostToDevice) : hipMemset(h->bi, 0, 8 * I));
  return 0;
}

int mf_get_weights(mf_handle* h, double* P, double* Q, double* bu, double* bi) {
  if (!h) return fail(BPRMF_E_INVALID, "null handle");
  if (int r = h->lane.use()) return r;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  const int64_t U = h->cfg.user_num, I = h->cfg.item_num, k = h->cfg.n_factors;
  if (P && U) HIPCHK(hipMemcpy(P, h->P, 8 * U * k, hipMemcpyDeviceToHost));
  if (Q && I) HIPCHK(hipMemcpy(Q, h->Q, 8 * I * k, hipMemcpyDeviceToHost));
  if (bu && U) HIPCHK(hipMemcpy(bu, h->bu, 8 * U, hipMemcpyDeviceToHost));
  if (bi && I) HIPCHK(hipMemcpy(bi, h->bi, 8 * I, hipMemcpyDeviceToHost));
  return 0;
}

int mf_set_implicit(mf_handle* h, const double* Y) {
  if (!h || !Y) return fail(BPRMF_E_INVALID, "bad arguments");
  if (h->cfg.model != MF_SVDPP) return fail(BPRMF_E_STATE, "only SVDpp has an implicit table");
  if (int r = h->lane.use()) return r;
  const int64_t bytes = 8 * h->cfg.item_num * h->cfg.n_factors;
  if (bytes) HIPCHK(hipMemcpy(h->Y, Y, bytes, hipMemcpyHostToDevice));
  return 0;
}

int mf_get_implicit(mf_handle* h, double* Y) {
  if (!h || !Y) return fail(BPRMF_E_INVALID, "bad arguments");
  if (h->cfg.model != MF_SVDPP) return fail(BPRMF_E_STATE, "only SVDpp has an implicit table");
  if (int r = h->lane.use()) return r;
  HIPCHK(hipStreamSynchronize(h->lane.stream));
  const int64_t bytes = 8 * h->cfg.item_num * h->cfg.n_factors;
  if (bytes) HIPCHK(hipMemcpy(Y, h->Y, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int mf_fit(mf_handle* h, int32_t epochs, mf_stats* st) {
  if (!h || epochs < 0) return fail(BPRMF_E_INVALID, "bad arguments");
  if (int r = h->lane.use()) return r;
  const mf::Args a = args_of(h);
  if (int r = h->lane.begin()) return r;
  for (int32_t e = 0; e < epochs; ++e) HIPCHK(mf::epoch(a, h->cfg.model, h->lane.stream));
  double seconds = 0.0;
  if (int r = h->lane.end(&seconds)) return r;
  if (st) {
    st->samples = (int64_t)epochs * h->t.n;
    st->levels = h->t.levels;
    st->seconds = seconds;
  }
  return 0;
}

int mf_predict(mf_handle* h, const int32_t* users, const int32_t* items, int64_t n, double* out) {
  if (!h || n < 0 || (n > 0 && (!users || !items || !out))) return fail(BPRMF_E_INVALID, "bad arguments");
  if (!n) return 0;
  if (int r = h->lane.use()) return r;
  if (h->cfg.model == MF_SVDPP && !h->t.uoff) return fail(BPRMF_E_STATE, "SVDpp predict needs the train set");
  DevBuf<int32_t> du, di;
  DevBuf<double> dout;
  int rc = 0;
  if ((rc = du.alloc(n)) || (rc = di.alloc(n)) || (rc = dout.alloc(n))) return rc;
  hipStream_t s = h->lane.stream;
  int32_t bad = 0;
  HIPCHK(hipMemcpyAsync(du, users, 4 * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(di, items, 4 * n, hipMemcpyHostToDevice, s));
  HIPCHK(mf::predict(args_of(h), h->cfg.model, du, di, n, h->cfg.user_num, h->cfg.item_num, dout,
                     h->d_err, s));
  HIPCHK(hipMemcpyAsync(out, dout, 8 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&bad, h->d_err, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (bad) {
    (void)hipMemset(h->d_err, 0, 4);
    return fail(BPRMF_E_RANGE, "Invalid user or item code");
  }
  return 0;
}

}  // extern "C"
