// Step 2, counts of a block restricted to a SAMPLE GROUP (include/rg_step2.h: rg_s2_set_group, rg_s2_group_counts_packed, rg_s2_group_sums_int).
//
// What it is for: outside the pseudo-autosomal regions of chromosome X the reference counts a male's call at half its value in the minor-allele
// count (parseSnpfromBed / parseSnpfromBGEN / readChunkFromPGENFileToG, e.g. Geno.cpp:2445-2471; compute_mac, Geno.cpp:3077-3108; per trait
// update_trait_counts, :2948-2959).  With the group = the males, the driver needs per variant the males' calls equal to 1, equal to 2 and observed
// (hard calls) or their dosage sum and observed count (integer dosages), overall and among the samples each trait is observed for.
//
// The membership, and membership AND mask_p for each of the P trait masks, are packed once into bit planes laid out like a 2-bit row: sample i is
// bit 2 (i & 15) of 32-bit word i >> 4, zeros at the odd positions and at positions >= n.  A hard-call count is then a popcount of the row word's
// low / high half-planes under the plane word; the plane words (P + 1 per row word, the same for every row of the block) come from L2.
// One workgroup of 256 per (row, chunk of 8 planes): a block with at most 7 traits reads each row once.  No atomics; LDS only for the four-wave
// reduction.  The entries take the caller's rows (host rows are staged into a buffer of this file's own): they do not touch the block a score entry
// staged, and a context without a group never reaches this file's kernels or allocations.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "step2_internal.h"

#define GRP_PL 8      // planes per workgroup

struct GroupState {
  std::vector<uint8_t> member;      // [n] host copy
  std::vector<uint8_t> masks;       // [P][n] caller's masks (empty: those of rg_s2_set_null)
  int mask_gen = -1;                // rg_s2_ctx::mask_gen the planes were packed at
  int64_t nw = 0;                   // words per plane: ceil(n / 16)
  uint32_t* d_planes = nullptr;     // [1 + P][nw]
  void* d_rows = nullptr; size_t rows_cap = 0;
  void* d_out = nullptr; size_t out_cap = 0;
};

// the row word i (samples 16 i .. 16 i + 15) of a row of nbytes = ceil(n / 4) bytes: a 4-byte load where the row allows it
__device__ __forceinline__ uint32_t grp_row_word(const uint8_t* __restrict__ row, int64_t i, int64_t nbytes, bool aligned) {
  const int64_t b = i * 4;
  if (aligned && b + 4 <= nbytes) return *reinterpret_cast<const uint32_t*>(row + b);
  uint32_t x = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (b + k < nbytes) x |= (uint32_t)row[b + k] << (8 * k);
  return x;
}

template <int NV>
__device__ __forceinline__ void grp_reduce_store(int (&v)[NV], int (*red)[4]) {
#pragma unroll
  for (int a = 0; a < NV; ++a)
    for (int o = 32; o > 0; o >>= 1) v[a] += __shfl_down(v[a], o);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < NV; ++a) red[a][threadIdx.x >> 6] = v[a];
  }
  __syncthreads();
}

// grid (bs, ceil((1 + P) / GRP_PL)); out [bs][1 + P][3] = calls equal to 1, equal to 2, observed among the plane's samples (.bed coding:
// 00 -> 2 copies, 01 -> missing, 10 -> 1, 11 -> 0; flip counts the other allele: 00 <-> 11)
__global__ __launch_bounds__(256) void k_s2_group_counts(const uint8_t* __restrict__ rows, int64_t ld, int64_t n, int flip,
                                                         const uint32_t* __restrict__ planes, int64_t nw, int npl, int32_t* __restrict__ out) {
  __shared__ int red[3 * GRP_PL][4];
  const uint8_t* row = rows + (int64_t)blockIdx.x * ld;
  const int q0 = blockIdx.y * GRP_PL;
  const int nq = min(GRP_PL, npl - q0);
  const int64_t nbytes = (n + 3) / 4;
  const bool aligned = ((reinterpret_cast<uintptr_t>(rows) | (uintptr_t)ld) & 3) == 0;
  int acc[3 * GRP_PL];
#pragma unroll
  for (int a = 0; a < 3 * GRP_PL; ++a) acc[a] = 0;
  for (int64_t i = threadIdx.x; i < nw; i += 256) {
    const uint32_t x = grp_row_word(row, i, nbytes, aligned);
    const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
    const uint32_t one = hi & ~lo, obs = ~(lo & ~hi) & 0x55555555u;
    const uint32_t two = flip ? (lo & hi) : (~lo & ~hi & 0x55555555u);
#pragma unroll
    for (int q = 0; q < GRP_PL; ++q) {
      if (q < nq) {
        const uint32_t m = planes[(int64_t)(q0 + q) * nw + i];
        acc[3 * q] += __popc(one & m); acc[3 * q + 1] += __popc(two & m); acc[3 * q + 2] += __popc(obs & m);
      }
    }
  }
  grp_reduce_store<3 * GRP_PL>(acc, red);
  if ((int)threadIdx.x < 3 * nq) {
    const int a = threadIdx.x;
    out[((int64_t)blockIdx.x * npl + q0) * 3 + a] = red[a][0] + red[a][1] + red[a][2] + red[a][3];
  }
}

// Integer dosages: rows [bs][ld] uint16, 0xFFFF = missing.  grid as above; out [bs][1 + P][2] int64 = exact sum, observed count among the plane's samples.
__global__ __launch_bounds__(256) void k_s2_group_sums_int(const uint16_t* __restrict__ G, int64_t ld, int64_t n, const uint32_t* __restrict__ planes,
                                                           int64_t nw, int npl, int64_t* __restrict__ out) {
  __shared__ unsigned long long reds[GRP_PL][4];
  __shared__ int redc[GRP_PL][4];
  const uint16_t* row = G + (int64_t)blockIdx.x * ld;
  const int q0 = blockIdx.y * GRP_PL;
  const int nq = min(GRP_PL, npl - q0);
  unsigned long long sum[GRP_PL];
  int cnt[GRP_PL];
#pragma unroll
  for (int q = 0; q < GRP_PL; ++q) { sum[q] = 0; cnt[q] = 0; }
  for (int64_t i = threadIdx.x; i < nw; i += 256) {
    uint32_t m[GRP_PL];
#pragma unroll
    for (int q = 0; q < GRP_PL; ++q) m[q] = q < nq ? planes[(int64_t)(q0 + q) * nw + i] : 0u;
    const int64_t s0 = i * 16;
    const int ns = (int)min((int64_t)16, n - s0);
    uint32_t part[GRP_PL];
#pragma unroll
    for (int q = 0; q < GRP_PL; ++q) part[q] = 0;
    for (int k = 0; k < ns; ++k) {
      const uint32_t v = row[s0 + k];
      const uint32_t ob = v != 0xFFFFu ? 1u : 0u;
      const uint32_t val = ob ? v : 0u;
#pragma unroll
      for (int q = 0; q < GRP_PL; ++q) {
        const uint32_t bit = (m[q] >> (2 * k)) & ob;      // (the planes hold nothing at odd positions)
        part[q] += val & (0u - bit);                       // at most 16 * 65534 per word
        cnt[q] += (int)bit;
      }
    }
#pragma unroll
    for (int q = 0; q < GRP_PL; ++q) sum[q] += part[q];
  }
#pragma unroll
  for (int q = 0; q < GRP_PL; ++q)
    for (int o = 32; o > 0; o >>= 1) { sum[q] += __shfl_down(sum[q], o); cnt[q] += __shfl_down(cnt[q], o); }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < GRP_PL; ++q) { reds[q][threadIdx.x >> 6] = sum[q]; redc[q][threadIdx.x >> 6] = cnt[q]; }
  }
  __syncthreads();
  if ((int)threadIdx.x < nq) {
    const int q = threadIdx.x;
    int64_t* o = out + ((int64_t)blockIdx.x * npl + q0 + q) * 2;
    o[0] = (int64_t)(reds[q][0] + reds[q][1] + reds[q][2] + reds[q][3]);
    o[1] = (int64_t)(redc[q][0] + redc[q][1] + redc[q][2] + redc[q][3]);
  }
}

static int grp_ensure(rg_s2_ctx* ctx, void** buf, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return RG_S2_OK;
  if (*buf) S2_HIP(hipFree(*buf));
  *buf = nullptr; *cap = 0;
  S2_HIP(hipMalloc(buf, bytes));
  *cap = bytes;
  return RG_S2_OK;
}

// membership (and membership AND mask_p) -> bit planes, uploaded
static int grp_pack(rg_s2_ctx* ctx) {
  GroupState& g = *ctx->grp;
  const int64_t n = ctx->n;
  const int P = ctx->P;
  const uint8_t* masks = g.masks.empty() ? ctx->hM.data() : g.masks.data();
  std::vector<uint32_t> pl((size_t)(1 + P) * g.nw, 0u);
  for (int64_t i = 0; i < n; ++i) {
    if (!g.member[i]) continue;
    const uint32_t bit = 1u << (2 * (i & 15));
    pl[(size_t)(i >> 4)] |= bit;
    for (int q = 0; q < P; ++q)
      if (masks[(size_t)q * n + i]) pl[(size_t)(1 + q) * g.nw + (i >> 4)] |= bit;
  }
  S2_HIP(hipMemcpyAsync(g.d_planes, pl.data(), pl.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->st));
  S2_HIP(hipStreamSynchronize(ctx->st));
  g.mask_gen = ctx->mask_gen;
  return RG_S2_OK;
}

static int grp_ready(rg_s2_ctx* ctx, const char* who) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, std::string(who) + ": context was not created");
  if (!ctx->grp) return rg_s2_fail(ctx, RG_S2_ERR_ARG, std::string(who) + ": no group has been set (rg_s2_set_group)");
  S2_HIP(hipSetDevice(ctx->dev));
  if (ctx->grp->masks.empty() && ctx->grp->mask_gen != ctx->mask_gen) return grp_pack(ctx);      // rg_s2_set_null brought new masks
  return RG_S2_OK;
}

void rg_s2_group_free(rg_s2_ctx* ctx) {
  if (!ctx || !ctx->grp) return;
  GroupState* g = ctx->grp;
  if (g->d_planes) (void)hipFree(g->d_planes);
  if (g->d_rows) (void)hipFree(g->d_rows);
  if (g->d_out) (void)hipFree(g->d_out);
  delete g;
  ctx->grp = nullptr;
}

extern "C" {

int rg_s2_set_group(rg_s2_ctx* ctx, const uint8_t* member, const uint8_t* mask) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_set_group: context was not created");
  S2_HIP(hipSetDevice(ctx->dev));
  S2_HIP(hipStreamSynchronize(ctx->st));
  rg_s2_group_free(ctx);
  if (!member) return RG_S2_OK;
  const size_t n = (size_t)ctx->n, nm = n * (size_t)ctx->P;
  if (!mask && ctx->hM.size() != nm)
    return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_set_group: the trait masks are not there (call rg_s2_set_null first, or hand over the masks)");
  ctx->grp = new GroupState();
  GroupState& g = *ctx->grp;
  g.member.assign(member, member + n);
  if (mask) g.masks.assign(mask, mask + nm);
  g.nw = (ctx->n + 15) / 16;
  S2_HIP(hipMalloc((void**)&g.d_planes, sizeof(uint32_t) * (size_t)(1 + ctx->P) * g.nw));
  return grp_pack(ctx);
}

int rg_s2_group_counts_packed(rg_s2_ctx* ctx, const uint8_t* rows, int64_t ld, int32_t bs, int32_t rows_on_device, int32_t flip, int32_t* counts) {
  int rc = grp_ready(ctx, "rg_s2_group_counts_packed");
  if (rc != RG_S2_OK) return rc;
  const int64_t n = ctx->n, nbytes = (n + 3) / 4;
  if (!rows || !counts || bs < 1 || ld < nbytes) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_counts_packed: need rows, counts, bs >= 1 and ld >= ceil(n / 4)");
  GroupState& g = *ctx->grp;
  const int npl = 1 + ctx->P;
  const uint8_t* d = rows;
  int64_t ldd = ld;
  if (!rows_on_device) {
    ldd = (nbytes + 3) / 4 * 4;
    if ((rc = grp_ensure(ctx, &g.d_rows, &g.rows_cap, (size_t)bs * ldd)) != RG_S2_OK) return rc;
    S2_HIP(hipMemcpy2DAsync(g.d_rows, (size_t)ldd, rows, (size_t)ld, (size_t)nbytes, (size_t)bs, hipMemcpyHostToDevice, ctx->st));
    d = (const uint8_t*)g.d_rows;
  }
  const size_t ob = sizeof(int32_t) * 3 * (size_t)npl * bs;
  if ((rc = grp_ensure(ctx, &g.d_out, &g.out_cap, ob)) != RG_S2_OK) return rc;
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  hipLaunchKernelGGL(k_s2_group_counts, dim3(bs, (npl + GRP_PL - 1) / GRP_PL), dim3(256), 0, ctx->st, d, ldd, n, flip ? 1 : 0, g.d_planes, g.nw, npl, (int32_t*)g.d_out);
  S2_HIP(hipGetLastError());
  S2_HIP(hipEventRecord(ctx->e1, ctx->st));
  S2_HIP(hipMemcpyAsync(counts, g.d_out, ob, hipMemcpyDeviceToHost, ctx->st));
  S2_HIP(hipStreamSynchronize(ctx->st));
  float ms = 0.f;
  S2_HIP(hipEventElapsedTime(&ms, ctx->e0, ctx->e1));
  ctx->last_ms = ms;
  return RG_S2_OK;
}

int rg_s2_group_sums_int(rg_s2_ctx* ctx, const uint16_t* G, int64_t ld, int32_t bs, int32_t g_on_device, int64_t* sums) {
  int rc = grp_ready(ctx, "rg_s2_group_sums_int");
  if (rc != RG_S2_OK) return rc;
  const int64_t n = ctx->n;
  if (!G || !sums || bs < 1 || ld < n) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_sums_int: need G, sums, bs >= 1 and ld >= n");
  GroupState& g = *ctx->grp;
  const int npl = 1 + ctx->P;
  const uint16_t* d = G;
  int64_t ldd = ld;
  if (!g_on_device) {
    ldd = n;
    if ((rc = grp_ensure(ctx, &g.d_rows, &g.rows_cap, sizeof(uint16_t) * (size_t)bs * n)) != RG_S2_OK) return rc;
    S2_HIP(hipMemcpy2DAsync(g.d_rows, sizeof(uint16_t) * (size_t)n, G, sizeof(uint16_t) * (size_t)ld, sizeof(uint16_t) * (size_t)n, (size_t)bs, hipMemcpyHostToDevice, ctx->st));
    d = (const uint16_t*)g.d_rows;
  }
  const size_t ob = sizeof(int64_t) * 2 * (size_t)npl * bs;
  if ((rc = grp_ensure(ctx, &g.d_out, &g.out_cap, ob)) != RG_S2_OK) return rc;
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  hipLaunchKernelGGL(k_s2_group_sums_int, dim3(bs, (npl + GRP_PL - 1) / GRP_PL), dim3(256), 0, ctx->st, d, ldd, n, g.d_planes, g.nw, npl, (int64_t*)g.d_out);
  S2_HIP(hipGetLastError());
  S2_HIP(hipEventRecord(ctx->e1, ctx->st));
  S2_HIP(hipMemcpyAsync(sums, g.d_out, ob, hipMemcpyDeviceToHost, ctx->st));
  S2_HIP(hipStreamSynchronize(ctx->st));
  float ms = 0.f;
  S2_HIP(hipEventElapsedTime(&ms, ctx->e0, ctx->e1));
  ctx->last_ms = ms;
  return RG_S2_OK;
}

}  // extern "C"
