// TEST SCAFFOLDING, not product code.  The host stand-ins of s2_contract_host.cpp beside this file, plus what rg_s2_set_coding adds to the hard-call
// contraction (include/rg_step2.h, "--test dominant | recessive"): rg_s2_contract_packed stages and counts the rows as the additive stand-in does, then
// -- as rg_s2_apply_coding of regenie_amd/csrc/step2_qt.hip -- takes the additive per-trait counts against ctx->contract_mask, relabels the staged
// 2-bit codes in place (dominant 00 -> 10; recessive 10 -> 11, 00 -> 10) and returns the sums / squares of the relabelled row; counts stay additive.
// With step2_bt.hip compiled against the shim, its coded branch (rg_s2_bt_score_packed, score_from_sums, k_bt_prep and the corrections reading the
// relabelled staged row) runs on the host.
#include "../../regenie_amd/csrc/step2_internal.h"
#define rg_s2_contract_packed rg_s2_contract_packed_additive
#include "s2_contract_host.cpp"
#undef rg_s2_contract_packed

extern "C" {

int rg_s2_set_coding(rg_s2_ctx* ctx, int32_t coding) {
  if (!ctx || coding < RG_S2_ADDITIVE || coding > RG_S2_RECESSIVE) return RG_S2_ERR_ARG;
  ctx->coding = coding;
  return RG_S2_OK;
}

int rg_s2_contract_packed(rg_s2_ctx* ctx, const uint8_t* rows, int64_t ld, int32_t bs, int32_t on_device, int32_t flip, const rg_s2_contract_out* out) {
  int rc = rg_s2_contract_packed_additive(ctx, rows, ld, bs, on_device, flip, out);      // stages the rows (flip applied), additive counts
  ctx->staged_bs = bs;
  ctx->tcnt_valid = false;
  if (rc || ctx->coding == RG_S2_ADDITIVE) return rc;
  const HostCols& h = cols_of(ctx);
  const int64_t n = ctx->n;
  const int P = ctx->P;
  const int64_t Np = (n + 128 * RG_MAX_SEG - 1) / (128 * RG_MAX_SEG) * (128 * RG_MAX_SEG), ldp = Np / 4;
  uint8_t* pk = (uint8_t*)ctx->pbuf[RG_S2_Q_PK];
  if (ctx->contract_mask) {
    free(ctx->d_tcnt);
    ctx->d_tcnt = (int32_t*)calloc((size_t)bs * P * 2, sizeof(int32_t));
    ctx->tcnt_valid = true;
  }
  for (int j = 0; j < bs; ++j) {
    std::vector<double> g0(n), ms(n);
    for (int64_t i = 0; i < n; ++i) {
      uint8_t& b = pk[(size_t)j * ldp + (i >> 2)];
      unsigned code = (b >> (2 * (i & 3))) & 3u;
      if (ctx->contract_mask)
        for (int p = 0; p < P; ++p)
          if (ctx->contract_mask[(size_t)p * n + i]) {
            ctx->d_tcnt[((size_t)j * P + p) * 2] += code == 0 ? 2 : code == 2 ? 1 : 0;
            ctx->d_tcnt[((size_t)j * P + p) * 2 + 1] += code != 1;
          }
      if (ctx->coding == RG_S2_DOMINANT) { if (code == 0) code = 2; }
      else { if (code == 2) code = 3; else if (code == 0) code = 2; }
      b = (uint8_t)((b & ~(3u << (2 * (i & 3)))) | (code << (2 * (i & 3))));
      g0[i] = code == 2 ? 1.0 : 0.0;
      ms[i] = code == 1 ? 1.0 : 0.0;
    }
    for (int c = 0; c < h.ncol; ++c) {
      const double* col = h.cols.data() + (size_t)c * n;
      double s = 0.0, sm = 0.0, s2 = 0.0;
      for (int64_t i = 0; i < n; ++i) { s += g0[i] * col[i]; sm += ms[i] * col[i]; s2 += g0[i] * g0[i] * col[i]; }
      if (out->sums) { out->sums[((size_t)j * 2) * h.ncol + c] = s; out->sums[((size_t)j * 2 + 1) * h.ncol + c] = sm; }
      if (out->sq && c < h.nsq) out->sq[(size_t)j * h.nsq + c] = s2;
    }
  }
  return RG_S2_OK;
}

}  // extern "C"
