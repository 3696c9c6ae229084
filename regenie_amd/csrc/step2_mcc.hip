// rg_s2_qt_moments (include/rg_step2.h): the masked power sums the moment-matched correlation test of a quantitative trait needs
// (`regenie --step 2 --qt --mcc`; MCCResults::dkat, MCC.cpp:500-645, works on Gmat.col(isnp) -- Data.cpp:2501-2515).
//
// For a listed row v of the block LAST scored and every trait t:  S_k = sum_i mask_t(i) r_v(i)^k (k = 1..6)  and  sum_i r_v(i) yres_t(i),
// where r_v is the vector the reference's test sees:
//   sparse variant (check_sparse_G)  the mean-imputed raw genotype g~ (not residualised, scale_fac = 1)
//   dense variant                    residualize_geno's output (g~ - X b) / scale_fac,  b = X^T g~
// The verdict, the mean and scale_fac are the score call's (rg_s2_ctx::last_qt); b is RECOMPUTED here from the row (one more pass over it and
// over X, in fp64 with a fixed summation tree): the three score entries leave b in three different forms (fp64 partial sums, integer
// contractions against digit planes, per mean and missing indicator), and the test is applied to few rows of a block.
//
// Mapping (gfx950): the sample axis is the long one and everything is a reduction over it, so a workgroup of 256 threads takes one row and a
// chunk of MCC_CHUNK = 2048 samples, 8 per thread at a stride of 256 (coalesced 2 KB rows of X / yres, 256 B of a mask, 64 B of a 2-bit row):
//   k_s2_mcc_proj   partial b_c of the chunk, one value per covariate     -> part [row][chunk][C]
//   k_s2_mcc_beta   b_c = the chunks' partial sums in chunk order
//   k_s2_mcc_sums   r of the chunk's samples in registers (c = x . b as C fused multiply-adds per sample from b in LDS), then per trait the seven
//                   sums of the chunk                                     -> part [row][chunk][P][7]
//   k_s2_mcc_final  the chunks' partial sums in chunk order
// Within a chunk a sum goes thread (8 terms in order) -> wave (shuffle tree) -> workgroup (4 waves in order): no floating-point atomics, the
// same bits on every run.  The covariate part is C FMAs per sample on the vector units, not the fp64 MFMA.  That follows from the mapping chosen
// here -- one row per workgroup, the simplest one with a fixed summation order -- under which the product is matrix x VECTOR and every listed
// row re-reads X twice and yres / the masks once through L2 (20 GB of cache traffic for 37 MB of unique data at 1,024 rows x 100,000 samples,
// profiles/mcc.md).  A workgroup that took a tile of rows would read X and yres once per tile and turn c = X b into a small fp64 GEMM the MFMA
// could take; that mapping has not been built or measured.
#include "step2_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int MCC_EPT = 8;
constexpr int MCC_CHUNK = 256 * MCC_EPT;
constexpr int MCC_NS = 7;

// the mean-imputed entry i of a row as the score entries read it
template <int KIND>
__device__ __forceinline__ double mcc_geno(const void* __restrict__ row, int64_t i, double mu, double scale) {
  if (KIND == 1) {                // fp64, missing = NaN or negative
    const double v = reinterpret_cast<const double*>(row)[i];
    return v >= 0.0 ? v : mu;
  } else if (KIND == 2) {         // staged .bed codes (flip applied): 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0
    const int code = (reinterpret_cast<const uint8_t*>(row)[i >> 2] >> (2 * (int)(i & 3))) & 3;
    return code == 0 ? 2.0 : (code == 1 ? mu : (code == 2 ? 1.0 : 0.0));
  } else {                        // uint16 in units of 1 / scale, 0xFFFF = missing
    const uint16_t q = reinterpret_cast<const uint16_t*>(row)[i];
    return q == 0xFFFFu ? mu : (double)q / scale;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// grid (chunk, listed row); dense rows only
template <int KIND>
__global__ __launch_bounds__(256) void k_s2_mcc_proj(const void* __restrict__ rows, int64_t ld_bytes, const int32_t* __restrict__ variant, int64_t n,
                                                     const double* __restrict__ X, int C, const double* __restrict__ mu, const int32_t* __restrict__ sparse,
                                                     double scale, double* __restrict__ part) {
  __shared__ double red[4][RG_S2_MAX_COV];
  const int v = blockIdx.y, ch = blockIdx.x, nchunk = gridDim.x, j = variant[v], tid = threadIdx.x;
  if (sparse[j]) return;
  const char* row = reinterpret_cast<const char*>(rows) + (int64_t)j * ld_bytes;
  const double m = mu[j];
  const int64_t i0 = (int64_t)ch * MCC_CHUNK + tid;
  double g[MCC_EPT];
#pragma unroll
  for (int e = 0; e < MCC_EPT; ++e) {
    const int64_t i = i0 + e * 256;
    g[e] = i < n ? mcc_geno<KIND>(row, i, m, scale) : 0.0;
  }
  for (int c = 0; c < C; ++c) {
    const double* x = X + (int64_t)c * n;
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < MCC_EPT; ++e) {
      const int64_t i = i0 + e * 256;
      s = fma(i < n ? x[i] : 0.0, g[e], s);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6][c] = s;
  }
  __syncthreads();
  if (tid < C) part[((int64_t)v * nchunk + ch) * C + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// thread = (listed row, covariate)
__global__ void k_s2_mcc_beta(const double* __restrict__ part, int nchunk, int C, int nv, const int32_t* __restrict__ variant, const int32_t* __restrict__ sparse,
                              double* __restrict__ b /*[nv][RG_S2_MAX_COV]*/) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nv * C) return;
  const int v = t / C, c = t - v * C;
  double s = 0.0;
  if (!sparse[variant[v]])
    for (int ch = 0; ch < nchunk; ++ch) s += part[((int64_t)v * nchunk + ch) * C + c];
  b[(int64_t)v * RG_S2_MAX_COV + c] = s;
}

// grid (chunk, listed row)
template <int KIND>
__global__ __launch_bounds__(256) void k_s2_mcc_sums(const void* __restrict__ rows, int64_t ld_bytes, const int32_t* __restrict__ variant, int64_t n,
                                                     const double* __restrict__ X, int C, const double* __restrict__ Y, const uint8_t* __restrict__ M, int P,
                                                     const double* __restrict__ mu, const double* __restrict__ sf, const int32_t* __restrict__ sparse,
                                                     double scale, const double* __restrict__ b, double* __restrict__ part) {
  __shared__ double sb[RG_S2_MAX_COV];
  __shared__ double red[4][MCC_NS + 1];
  const int v = blockIdx.y, ch = blockIdx.x, nchunk = gridDim.x, j = variant[v], tid = threadIdx.x;
  const bool dense = !sparse[j];
  const char* row = reinterpret_cast<const char*>(rows) + (int64_t)j * ld_bytes;
  const double m = mu[j], s_fac = sf[j];
  const int64_t i0 = (int64_t)ch * MCC_CHUNK + tid;
  if (tid < C) sb[tid] = b[(int64_t)v * RG_S2_MAX_COV + tid];
  __syncthreads();
  double r[MCC_EPT];
#pragma unroll
  for (int e = 0; e < MCC_EPT; ++e) {
    const int64_t i = i0 + e * 256;
    r[e] = i < n ? mcc_geno<KIND>(row, i, m, scale) : 0.0;
  }
  if (dense) {
    double cx[MCC_EPT];
#pragma unroll
    for (int e = 0; e < MCC_EPT; ++e) cx[e] = 0.0;
    for (int c = 0; c < C; ++c) {
      const double* x = X + (int64_t)c * n;
      const double bc = sb[c];
#pragma unroll
      for (int e = 0; e < MCC_EPT; ++e) {
        const int64_t i = i0 + e * 256;
        cx[e] = fma(i < n ? x[i] : 0.0, bc, cx[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < MCC_EPT; ++e) r[e] = (r[e] - cx[e]) / s_fac;
  }
  for (int t = 0; t < P; ++t) {
    const double* y = Y + (int64_t)t * n;
    const uint8_t* mk = M + (int64_t)t * n;
    double a[MCC_NS];
#pragma unroll
    for (int k = 0; k < MCC_NS; ++k) a[k] = 0.0;
#pragma unroll
    for (int e = 0; e < MCC_EPT; ++e) {
      const int64_t i = i0 + e * 256;
      if (i < n) {
        const double q = r[e], q2 = q * q, q3 = q2 * q;
        a[6] = fma(q, y[i], a[6]);
        if (mk[i]) { a[0] += q; a[1] += q2; a[2] += q3; a[3] += q2 * q2; a[4] += q2 * q3; a[5] += q3 * q3; }
      }
    }
#pragma unroll
    for (int k = 0; k < MCC_NS; ++k) {
      const double s = wave_sum(a[k]);
      if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < MCC_NS) part[(((int64_t)v * nchunk + ch) * P + t) * MCC_NS + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    __syncthreads();
  }
}

// thread = (listed row, trait, sum)
__global__ void k_s2_mcc_final(const double* __restrict__ part, int nchunk, int64_t total /* nv * P * 7 */, int PS, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t v = t / PS;
  const int q = (int)(t - v * PS);
  double s = 0.0;
  for (int ch = 0; ch < nchunk; ++ch) s += part[((int64_t)v * nchunk + ch) * PS + q];
  out[t] = s;
}

enum { M_VAR = 0, M_PART = 1, M_B = 2, M_OUT = 3 };

template <int KIND>
void launch_rows(rg_s2_ctx* ctx, int nv, int nchunk, int64_t ld_bytes, const int32_t* dvar, double* part, double* b, double* dout) {
  const rg_s2_ctx::LastQt& lq = ctx->last_qt;
  const int C = ctx->C, P = ctx->P;
  const double scale = (double)lq.scale;
  hipLaunchKernelGGL((k_s2_mcc_proj<KIND>), dim3(nchunk, nv), dim3(256), 0, ctx->st, lq.rows, ld_bytes, dvar, ctx->n, (const double*)ctx->dX, C, lq.mu, lq.sparse, scale, part);
  hipLaunchKernelGGL(k_s2_mcc_beta, dim3((nv * C + 255) / 256), dim3(256), 0, ctx->st, (const double*)part, nchunk, C, nv, dvar, lq.sparse, b);
  hipLaunchKernelGGL((k_s2_mcc_sums<KIND>), dim3(nchunk, nv), dim3(256), 0, ctx->st, lq.rows, ld_bytes, dvar, ctx->n, (const double*)ctx->dX, C, (const double*)ctx->dY,
                     (const uint8_t*)ctx->dM, P, lq.mu, lq.sf, lq.sparse, scale, (const double*)b, part);
  const int64_t total = (int64_t)nv * P * MCC_NS;
  hipLaunchKernelGGL(k_s2_mcc_final, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->st, (const double*)part, nchunk, total, P * MCC_NS, dout);
}

}  // namespace

void rg_s2_mcc_free(rg_s2_ctx* ctx) {
  for (void*& p : ctx->mbuf) { if (p) (void)hipFree(p); p = nullptr; }
  for (size_t& c : ctx->mcap) c = 0;
}

extern "C" int rg_s2_qt_moments(rg_s2_ctx* ctx, int32_t nv, const int32_t* variant, const rg_s2_mcc_out* out) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_moments: context was not created");
  const rg_s2_ctx::LastQt& lq = ctx->last_qt;
  if (lq.kind == 0 || !ctx->have_null) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_moments: no block has been scored by rg_s2_qt_block / _packed / _int");
  if (nv < 0 || (nv > 0 && (!variant || !out || !out->sums))) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_moments: bad arguments");
  for (int v = 0; v < nv; ++v)
    if (variant[v] < 0 || variant[v] >= lq.bs) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_moments: a listed row is outside the block last scored");
  ctx->last_ms = 0.0;
  if (nv == 0) return RG_S2_OK;
  S2_HIP(hipSetDevice(ctx->dev));
  const int64_t n = ctx->n;
  const int C = ctx->C, P = ctx->P, nchunk = (int)((n + MCC_CHUNK - 1) / MCC_CHUNK);
  const int W = std::max(C, P * MCC_NS);                      // doubles of a (row, chunk) in the partial-sum buffer, whichever kernel fills it
  // rows per pass: at most 65,535 (grid.y), and partial sums of at most 64 MB
  const int per_pass = (int)std::max<int64_t>(1, std::min<int64_t>(65535, ((int64_t)64 << 20) / ((int64_t)nchunk * W * (int64_t)sizeof(double))));
  const int np = std::min(per_pass, (int)nv);
  int rc;
  if ((rc = rg_s2_ensure_in(ctx, ctx->mbuf, ctx->mcap, M_VAR, (size_t)nv * sizeof(int32_t)))) return rc;
  if ((rc = rg_s2_ensure_in(ctx, ctx->mbuf, ctx->mcap, M_PART, (size_t)np * nchunk * W * sizeof(double)))) return rc;
  if ((rc = rg_s2_ensure_in(ctx, ctx->mbuf, ctx->mcap, M_B, (size_t)np * RG_S2_MAX_COV * sizeof(double)))) return rc;
  if ((rc = rg_s2_ensure_in(ctx, ctx->mbuf, ctx->mcap, M_OUT, (size_t)nv * P * MCC_NS * sizeof(double)))) return rc;
  int32_t* dvar = (int32_t*)ctx->mbuf[M_VAR];
  double* part = (double*)ctx->mbuf[M_PART];
  double* b = (double*)ctx->mbuf[M_B];
  double* dout = (double*)ctx->mbuf[M_OUT];
  S2_HIP(hipMemcpyAsync(dvar, variant, (size_t)nv * sizeof(int32_t), hipMemcpyHostToDevice, ctx->st));
  for (const auto& fx : lq.sf_fix)      // rows rg_s2_qt_block_packed scored a second time: the scale_fac it handed out (the vector outlives the copies: synchronised below)
    S2_HIP(hipMemcpyAsync(const_cast<double*>(lq.sf) + fx.first, &fx.second, sizeof(double), hipMemcpyHostToDevice, ctx->st));
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  for (int v0 = 0; v0 < nv; v0 += np) {
    const int nvp = std::min(np, (int)nv - v0);
    double* o = dout + (size_t)v0 * P * MCC_NS;
    if (lq.kind == 1) launch_rows<1>(ctx, nvp, nchunk, lq.ld * (int64_t)sizeof(double), dvar + v0, part, b, o);
    else if (lq.kind == 2) launch_rows<2>(ctx, nvp, nchunk, lq.ld, dvar + v0, part, b, o);
    else launch_rows<3>(ctx, nvp, nchunk, lq.ld * (int64_t)sizeof(uint16_t), dvar + v0, part, b, o);
  }
  S2_HIP(hipEventRecord(ctx->e1, ctx->st));
  S2_HIP(hipGetLastError());
  S2_HIP(hipMemcpyAsync(out->sums, dout, (size_t)nv * P * MCC_NS * sizeof(double), hipMemcpyDeviceToHost, ctx->st));
  S2_HIP(hipStreamSynchronize(ctx->st));
  float ms = 0.f;
  S2_HIP(hipEventElapsedTime(&ms, ctx->e0, ctx->e1));
  ctx->last_ms = ms;
  return RG_S2_OK;
}
