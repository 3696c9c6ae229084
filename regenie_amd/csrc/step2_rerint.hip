// rg_s2_qt_rerint (include/rg_step2.h): the two-stage rank-inverse-normal transformation of the Step-2 residuals of quantitative traits
// (`regenie --step 2 --qt --apply-rerint | --apply-rerint-cov`; Data::residualize_res and the tail of compute_res, Data.cpp:2393-2436, ranks as
// rint_pheno, Pheno.cpp:1975-2011).  It works IN PLACE on the context's residuals dY [P][n] (masked, unscaled: Y - LOCO prediction) between
// rg_s2_set_null and the first block of the chromosome:
//   1. per trait the observed samples' values become 64-bit keys whose unsigned order is the order of the doubles (sign flip of the bit
//      pattern; -0 is taken as +0, as the reference's `==` takes it), unobserved samples and the padding up to a power of two become the
//      largest key, and a bitonic network sorts the keys alone -- no payload: every sample then finds, by two binary searches in its trait's
//      sorted keys, how many observed values lie below it (lo) and how many are not above it (hi).  Its rank is rint_pheno's
//      (lo + 1) + (hi - lo - 1) / 2, the mean position of its block of ties: a function of the multiset of values only, so the order in
//      which the samples arrive cannot change it.
//   2. y = Phi^-1((rank - 3/8) / (nvals + 1/4))  (kc = 3/8, denominator nvals - 2 kc + 1), Wichura's AS241 (PPND16) in fp64
//   3. RG_S2_RERINT_COV: beta = res^T X, res -= mask .* (X beta^T)
//   4. scale_Y = |res_p| / sqrt(Neff_p - C) (1 for a trait the caller dropped), res /= scale_Y; then compute_res's own
//      p_sd_yres = |res_p| / sqrt(Neff_p - C), res /= p_sd_yres, scf_sv = scale_Y * p_sd_yres (to the context's dscf and to the caller)
// The block entries find the residuals where they always do; the planes of the res columns and res^T X are rebuilt by the first hard-call /
// integer-dosage block after any rg_s2_set_null (ensure_planes, step2_qt.hip), so nothing new is launched there.
//
// Mapping (gfx950).  Sort: a workgroup of 256 threads owns a tile of 2,048 keys, 8 per thread, element e * 256 + t of the tile in register e of
// thread t.  A compare-exchange at distance j then needs: j >= 256 the thread's own registers; j = 128, 64 another wave (one trip through 16 KB
// of LDS); j <= 32 another lane of the wave (64-lane shuffles).  k_rr_tile<false> runs the stages k = 2 .. 2,048 of the network on its tile,
// k_rr_global one step at distance j >= 2,048 over the whole array (two coalesced streams), k_rr_tile<true> the steps j = 1,024 .. 1 of a stage
// k > 2,048.  Sums (beta, norms): chunk of 2,048 samples per workgroup -> thread (8 terms in order) -> wave (shuffle tree) -> 4 waves in order
// -> the chunks in chunk order; no atomics, the same bits on every run (as step2_mcc.hip).
#include "step2_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int RR_EPT = 8;
constexpr int RR_TILE = 256 * RR_EPT;
constexpr uint64_t RR_PAD = ~0ull;

__device__ __forceinline__ uint64_t rr_key(double v) {
  if (v == 0.0) v = 0.0;      // -0 -> +0
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ uint64_t rr_shfl_xor(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}

// compare-exchange between registers e and e | JE (distance JE * 256); gi0 = index of register 0's element in the trait's array
template <int JE>
__device__ __forceinline__ void rr_in_thread(uint64_t (&r)[RR_EPT], uint32_t kdir, uint32_t gi0) {
#pragma unroll
  for (int e = 0; e < RR_EPT; ++e) {
    if (e & JE) continue;
    const bool asc = ((gi0 + e * 256) & kdir) == 0;
    const uint64_t a = r[e], b = r[e | JE];
    const bool sw = (a > b) == asc;
    r[e] = sw ? b : a;
    r[e | JE] = sw ? a : b;
  }
}

// the element keeps the smaller of the pair when it is the lower index of an ascending pair or the upper index of a descending one
__device__ __forceinline__ uint64_t rr_pick(uint64_t mine, uint64_t other, bool lower, bool asc) {
  const uint64_t mn = mine < other ? mine : other, mx = mine < other ? other : mine;
  return lower == asc ? mn : mx;
}

// the steps j = K / 2 .. 1 of the stage whose direction bit is kdir (K <= RR_TILE: the steps that stay inside a tile)
template <int K>
__device__ __forceinline__ void rr_stage(uint64_t (&r)[RR_EPT], uint64_t* lds, uint32_t kdir, uint32_t gi0, int t) {
  if (K >= 2048) rr_in_thread<4>(r, kdir, gi0);
  if (K >= 1024) rr_in_thread<2>(r, kdir, gi0);
  if (K >= 512) rr_in_thread<1>(r, kdir, gi0);
#pragma unroll
  for (int sh = 7; sh >= 6; --sh) {
    const int j = 1 << sh;
    if (K < 2 * j) continue;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < RR_EPT; ++e) lds[e * 256 + t] = r[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < RR_EPT; ++e) r[e] = rr_pick(r[e], lds[e * 256 + (t ^ j)], (t & j) == 0, ((gi0 + e * 256) & kdir) == 0);
  }
#pragma unroll
  for (int sh = 5; sh >= 0; --sh) {
    const int j = 1 << sh;
    if (K < 2 * j) continue;
#pragma unroll
    for (int e = 0; e < RR_EPT; ++e) r[e] = rr_pick(r[e], rr_shfl_xor(r[e], j), (t & j) == 0, ((gi0 + e * 256) & kdir) == 0);
  }
}

// keys [trait of the pass][Npad]; grid (Npad / 256, traits of the pass)
__global__ __launch_bounds__(256) void k_rr_keys(const double* __restrict__ Y, const uint8_t* __restrict__ M, int64_t n, int64_t Npad, int p0,
                                                 uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t src = (int64_t)(p0 + blockIdx.y) * n + i;
  keys[(int64_t)blockIdx.y * Npad + i] = (i < n && M[src]) ? rr_key(Y[src]) : RR_PAD;
}

// grid (Npad / RR_TILE, traits of the pass): MERGE = false sorts the tile (stages 2 .. 2,048), true runs the in-tile steps of stage kdir
template <bool MERGE>
__global__ __launch_bounds__(256) void k_rr_tile(uint64_t* __restrict__ keys, int64_t Npad, uint32_t kdir) {
  __shared__ uint64_t lds[RR_TILE];
  const int t = threadIdx.x;
  const uint32_t gi0 = blockIdx.x * (uint32_t)RR_TILE + t;
  uint64_t* a = keys + (int64_t)blockIdx.y * Npad + gi0;
  uint64_t r[RR_EPT];
#pragma unroll
  for (int e = 0; e < RR_EPT; ++e) r[e] = a[e * 256];
  if (MERGE) rr_stage<2048>(r, lds, kdir, gi0, t);
  else {
    rr_stage<2>(r, lds, 2, gi0, t); rr_stage<4>(r, lds, 4, gi0, t); rr_stage<8>(r, lds, 8, gi0, t); rr_stage<16>(r, lds, 16, gi0, t);
    rr_stage<32>(r, lds, 32, gi0, t); rr_stage<64>(r, lds, 64, gi0, t); rr_stage<128>(r, lds, 128, gi0, t); rr_stage<256>(r, lds, 256, gi0, t);
    rr_stage<512>(r, lds, 512, gi0, t); rr_stage<1024>(r, lds, 1024, gi0, t); rr_stage<2048>(r, lds, 2048, gi0, t);
  }
#pragma unroll
  for (int e = 0; e < RR_EPT; ++e) a[e * 256] = r[e];
}

// one step at distance j >= RR_TILE of stage kdir; thread = pair; grid (Npad / 512, traits of the pass)
__global__ __launch_bounds__(256) void k_rr_global(uint64_t* __restrict__ keys, int64_t Npad, uint32_t j, uint32_t kdir) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const uint32_t i = 2u * q - (q & (j - 1u));
  uint64_t* a = keys + (int64_t)blockIdx.y * Npad;
  const uint64_t x = a[i], y = a[i + j];
  if ((x > y) == ((i & kdir) == 0)) { a[i] = y; a[i + j] = x; }
}

// Wichura (1988), Algorithm AS241, PPND16: the standard-normal quantile to about 1 part in 10^16
__device__ double rr_ndtri(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                           1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                           5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  double r = sqrt(-log(q <= 0.0 ? p : 1.0 - p)), num, den;
  if (r <= 5.0) {
    r -= 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
              3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
              6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r + 2.05319162663775882187e+0) * r + 1.0);
  } else {
    r -= 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
              2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
              1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555888793769e-1) * r + 1.0);
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// rank and quantile of every sample of the pass's traits from the sorted keys; grid (ceil(n / 256), traits of the pass)
__global__ __launch_bounds__(256) void k_rr_rank(const uint64_t* __restrict__ keys, int64_t Npad, const int32_t* __restrict__ nvals, const uint8_t* __restrict__ M,
                                                 int64_t n, int p0, double* __restrict__ Y, double* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = p0 + blockIdx.y;
  const int64_t at = (int64_t)p * n + i;
  if (!M[at]) { Y[at] = 0.0; if (rank) rank[at] = 0.0; return; }
  const uint64_t* s = keys + (int64_t)blockIdx.y * Npad;
  const int nv = nvals[p];
  const uint64_t key = rr_key(Y[at]);
  int lo = 0, hi = nv;      // first position whose key is not below `key`
  while (lo < hi) { const int m = (lo + hi) >> 1; if (s[m] < key) lo = m + 1; else hi = m; }
  int up = lo, top = nv;    // first position whose key is above `key`
  while (up < top) { const int m = (up + top) >> 1; if (s[m] <= key) up = m + 1; else top = m; }
  const double rk = (double)(lo + 1) + (double)(up - lo - 1) / 2.0;
  if (rank) rank[at] = rk;      // null: the caller did not ask for the ranks
  Y[at] = rr_ndtri((rk - 0.375) / ((double)nv - 2.0 * 0.375 + 1.0));
}

__device__ __forceinline__ double rr_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// part [p][chunk][C] = the chunk's share of res_p . x_c; grid (chunk, P)
__global__ __launch_bounds__(256) void k_rr_dot_part(const double* __restrict__ Y, const double* __restrict__ X, int64_t n, int C, double* __restrict__ part) {
  __shared__ double red[4][RG_S2_MAX_COV];
  const int ch = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const int64_t i0 = (int64_t)ch * RR_TILE + tid;
  double y[RR_EPT];
#pragma unroll
  for (int e = 0; e < RR_EPT; ++e) { const int64_t i = i0 + e * 256; y[e] = i < n ? Y[(int64_t)p * n + i] : 0.0; }
  for (int c = 0; c < C; ++c) {
    const double* x = X + (int64_t)c * n;
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < RR_EPT; ++e) { const int64_t i = i0 + e * 256; s = fma(i < n ? x[i] : 0.0, y[e], s); }
    s = rr_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6][c] = s;
  }
  __syncthreads();
  if (tid < C) part[((int64_t)p * gridDim.x + ch) * C + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// beta [p][RG_S2_MAX_COV]: the chunks' shares in chunk order; thread = (p, c)
__global__ void k_rr_dot_final(const double* __restrict__ part, int nchunk, int C, int P, double* __restrict__ beta) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P * C) return;
  const int p = t / C, c = t - p * C;
  double s = 0.0;
  for (int ch = 0; ch < nchunk; ++ch) s += part[((int64_t)p * nchunk + ch) * C + c];
  beta[p * RG_S2_MAX_COV + c] = s;
}

// res_p(i) -= mask_p(i) * sum_c x_c(i) beta_p(c); grid (chunk, P)
__global__ __launch_bounds__(256) void k_rr_project(double* __restrict__ Y, const double* __restrict__ X, const uint8_t* __restrict__ M, int64_t n, int C,
                                                    const double* __restrict__ beta) {
  __shared__ double sb[RG_S2_MAX_COV];
  const int p = blockIdx.y, tid = threadIdx.x;
  if (tid < C) sb[tid] = beta[p * RG_S2_MAX_COV + tid];
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * RR_TILE + tid;
  double cx[RR_EPT];
#pragma unroll
  for (int e = 0; e < RR_EPT; ++e) cx[e] = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* x = X + (int64_t)c * n;
    const double bc = sb[c];
#pragma unroll
    for (int e = 0; e < RR_EPT; ++e) { const int64_t i = i0 + e * 256; cx[e] = fma(i < n ? x[i] : 0.0, bc, cx[e]); }
  }
#pragma unroll
  for (int e = 0; e < RR_EPT; ++e) {
    const int64_t i = i0 + e * 256;
    if (i < n) { const int64_t at = (int64_t)p * n + i; Y[at] = M[at] ? Y[at] - cx[e] : 0.0; }
  }
}

// part [p][chunk] = the chunk's share of |res_p|^2; grid (chunk, P)
__global__ __launch_bounds__(256) void k_rr_sq_part(const double* __restrict__ Y, int64_t n, double* __restrict__ part) {
  __shared__ double red[4];
  const int ch = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const int64_t i0 = (int64_t)ch * RR_TILE + tid;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < RR_EPT; ++e) { const int64_t i = i0 + e * 256; const double v = i < n ? Y[(int64_t)p * n + i] : 0.0; s = fma(v, v, s); }
  s = rr_wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) part[(int64_t)p * gridDim.x + ch] = (red[0] + red[1]) + (red[2] + red[3]);
}

// thread = trait: sd = |res_p| / sqrt(Neff_p - C).  second == 0: scale_Y (1 for a dropped trait); else p_sd_yres and scf_sv = scale_Y * p_sd_yres
__global__ void k_rr_sd(const double* __restrict__ part, int nchunk, int P, int C, const int32_t* __restrict__ nvals, const uint8_t* __restrict__ pass, int second,
                        double* __restrict__ scale_y, double* __restrict__ sd2, double* __restrict__ scf) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double s = 0.0;
  for (int ch = 0; ch < nchunk; ++ch) s += part[(int64_t)p * nchunk + ch];
  const double sd = sqrt(s) / sqrt((double)(nvals[p] - C));
  if (!second) scale_y[p] = pass[p] ? sd : 1.0;
  else { sd2[p] = sd; scf[p] = scale_y[p] * sd; }
}

// res_p /= d_p; grid (ceil(n / 256), P)
__global__ __launch_bounds__(256) void k_rr_div(double* __restrict__ Y, int64_t n, const double* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) Y[(int64_t)blockIdx.y * n + i] /= d[blockIdx.y];
}

enum { R_KEYS = 0, R_RANK = 1, R_PART = 2, R_SMALL = 3 };

}  // namespace

void rg_s2_rerint_free(rg_s2_ctx* ctx) {
  for (void*& p : ctx->rbuf) { if (p) (void)hipFree(p); p = nullptr; }
  for (size_t& c : ctx->rcap) c = 0;
}

extern "C" int rg_s2_qt_rerint(rg_s2_ctx* ctx, int32_t mode, const uint8_t* pass, double numtol, const rg_s2_rerint_out* out) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_rerint: context was not created");
  if (!ctx->have_null) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_rerint: rg_s2_set_null has not been called");
  if (mode != RG_S2_RERINT && mode != RG_S2_RERINT_COV) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_rerint: mode must be RG_S2_RERINT or RG_S2_RERINT_COV");
  const int64_t n = ctx->n;
  const int C = ctx->C, P = ctx->P;
  std::vector<int32_t> nvals(P, 0);
  for (int p = 0; p < P; ++p) {
    const uint8_t* m = ctx->hM.data() + (size_t)p * n;
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i) k += m[i] ? 1 : 0;
    if (k <= C) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_qt_rerint: a trait has no more observed samples than covariates");
    nvals[p] = (int32_t)k;
  }
  S2_HIP(hipSetDevice(ctx->dev));
  ctx->last_qt.kind = 0;      // a scored block belongs to the residuals it was scored under
  ctx->res_ready = false;     // the planes of the res columns and res^T X: rebuilt from the transformed residuals by the next block that reads them
  ctx->last_ms = 0.0;
  int64_t Npad = RR_TILE;
  while (Npad < n) Npad *= 2;      // n < 2^26 (rg_s2_create)
  const int per_pass = (int)std::max<int64_t>(1, std::min<int64_t>(P, ((int64_t)256 << 20) / (Npad * (int64_t)sizeof(uint64_t))));   // keys of at most 256 MB (one trait when a single one is larger)
  const int nchunk = (int)((n + RR_TILE - 1) / RR_TILE);
  const size_t small_bytes = ((size_t)P * RG_S2_MAX_COV + 3 * (size_t)P) * sizeof(double) + (size_t)P * sizeof(int32_t) + (size_t)P;
  int rc;
  if ((rc = rg_s2_ensure_in(ctx, ctx->rbuf, ctx->rcap, R_KEYS, (size_t)per_pass * Npad * sizeof(uint64_t)))) return rc;
  const bool want_ranks = out && out->ranks;      // [P][n] doubles: held only for a caller that reads them (the driver does not)
  if (want_ranks && (rc = rg_s2_ensure_in(ctx, ctx->rbuf, ctx->rcap, R_RANK, (size_t)P * n * sizeof(double)))) return rc;
  if ((rc = rg_s2_ensure_in(ctx, ctx->rbuf, ctx->rcap, R_PART, (size_t)P * nchunk * std::max(C, 1) * sizeof(double)))) return rc;
  if ((rc = rg_s2_ensure_in(ctx, ctx->rbuf, ctx->rcap, R_SMALL, small_bytes))) return rc;
  uint64_t* keys = (uint64_t*)ctx->rbuf[R_KEYS];
  double* rank = want_ranks ? (double*)ctx->rbuf[R_RANK] : nullptr;
  double* part = (double*)ctx->rbuf[R_PART];
  double* beta = (double*)ctx->rbuf[R_SMALL];
  double* scale_y = beta + (size_t)P * RG_S2_MAX_COV;
  double* sd2 = scale_y + P;
  double* scf = sd2 + P;
  int32_t* dnv = (int32_t*)(scf + P);
  uint8_t* dpass = (uint8_t*)(dnv + P);
  std::vector<uint8_t> hpass(P, 1);
  if (pass) hpass.assign(pass, pass + P);
  S2_HIP(hipMemcpyAsync(dnv, nvals.data(), (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, ctx->st));
  S2_HIP(hipMemcpyAsync(dpass, hpass.data(), (size_t)P, hipMemcpyHostToDevice, ctx->st));
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  const unsigned gn = (unsigned)((n + 255) / 256);
  for (int p0 = 0; p0 < P; p0 += per_pass) {
    const int np = std::min(per_pass, P - p0);
    hipLaunchKernelGGL(k_rr_keys, dim3((unsigned)(Npad / 256), np), dim3(256), 0, ctx->st, (const double*)ctx->dY, (const uint8_t*)ctx->dM, n, Npad, p0, keys);
    hipLaunchKernelGGL(k_rr_tile<false>, dim3((unsigned)(Npad / RR_TILE), np), dim3(256), 0, ctx->st, keys, Npad, 0u);
    for (int64_t k = 2 * RR_TILE; k <= Npad; k *= 2) {
      for (int64_t j = k / 2; j >= RR_TILE; j /= 2)
        hipLaunchKernelGGL(k_rr_global, dim3((unsigned)(Npad / 512), np), dim3(256), 0, ctx->st, keys, Npad, (uint32_t)j, (uint32_t)k);
      hipLaunchKernelGGL(k_rr_tile<true>, dim3((unsigned)(Npad / RR_TILE), np), dim3(256), 0, ctx->st, keys, Npad, (uint32_t)k);
    }
    hipLaunchKernelGGL(k_rr_rank, dim3(gn, np), dim3(256), 0, ctx->st, (const uint64_t*)keys, Npad, (const int32_t*)dnv, (const uint8_t*)ctx->dM, n, p0, ctx->dY, rank);
  }
  if (mode == RG_S2_RERINT_COV) {
    hipLaunchKernelGGL(k_rr_dot_part, dim3(nchunk, P), dim3(256), 0, ctx->st, (const double*)ctx->dY, (const double*)ctx->dX, n, C, part);
    hipLaunchKernelGGL(k_rr_dot_final, dim3((P * C + 255) / 256), dim3(256), 0, ctx->st, (const double*)part, nchunk, C, P, beta);
    hipLaunchKernelGGL(k_rr_project, dim3(nchunk, P), dim3(256), 0, ctx->st, ctx->dY, (const double*)ctx->dX, (const uint8_t*)ctx->dM, n, C, (const double*)beta);
  }
  for (int second = 0; second < 2; ++second) {
    hipLaunchKernelGGL(k_rr_sq_part, dim3(nchunk, P), dim3(256), 0, ctx->st, (const double*)ctx->dY, n, part);
    hipLaunchKernelGGL(k_rr_sd, dim3(1), dim3(64), 0, ctx->st, (const double*)part, nchunk, P, C, (const int32_t*)dnv, (const uint8_t*)dpass, second, scale_y, sd2, scf);
    hipLaunchKernelGGL(k_rr_div, dim3(gn, P), dim3(256), 0, ctx->st, ctx->dY, n, (const double*)(second ? sd2 : scale_y));
  }
  S2_HIP(hipMemcpyAsync(ctx->dscf, scf, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, ctx->st));
  S2_HIP(hipEventRecord(ctx->e1, ctx->st));
  S2_HIP(hipGetLastError());
  std::vector<double> hs(2 * (size_t)P);
  S2_HIP(hipMemcpyAsync(hs.data(), scale_y, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, ctx->st));
  S2_HIP(hipMemcpyAsync(hs.data() + P, scf, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, ctx->st));
  if (out && out->res) S2_HIP(hipMemcpyAsync(out->res, ctx->dY, (size_t)P * n * sizeof(double), hipMemcpyDeviceToHost, ctx->st));
  if (want_ranks) S2_HIP(hipMemcpyAsync(out->ranks, rank, (size_t)P * n * sizeof(double), hipMemcpyDeviceToHost, ctx->st));
  S2_HIP(hipStreamSynchronize(ctx->st));
  float ms = 0.f;
  S2_HIP(hipEventElapsedTime(&ms, ctx->e0, ctx->e1));
  ctx->last_ms = ms;
  if (out && out->scale_Y) memcpy(out->scale_Y, hs.data(), (size_t)P * sizeof(double));
  if (out && out->scf_sv) memcpy(out->scf_sv, hs.data() + P, (size_t)P * sizeof(double));
  for (int p = 0; p < P; ++p)
    if (hs[p] < numtol) {      // Data.cpp:2431-2433 (the residuals were divided by it: the null model is gone)
      ctx->have_null = false;
      return rg_s2_fail(ctx, RG_S2_ERR_ARG, "some phenotype residuals has sd=0.");
    }
  return RG_S2_OK;
}
