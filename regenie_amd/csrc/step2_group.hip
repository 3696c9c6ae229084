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
//
// The same planes serve a second member set (rg_s2_set_cases, rg_s2_case_counts_packed, rg_s2_case_sums_int; `--af-cc`): update_af_cc (Geno.cpp:3069-3075)
// adds a sample's call to af_case[p] and 1 to ns_case[p] when it is a case of trait p and observed for it, so the member of plane p is "case of trait p
// AND mask_p" -- no plane 0.  GroupState owns both sets in ONE device buffer, the group's 1 + P planes first, the cases' P planes after them, packed by
// one function; the kernels take (planes, npl) and do not know which set they count.  With both sets there, a case entry launches once over all
// 1 + 2 P planes, so a block's rows are read once, and keeps the group's part for rg_s2_group_counts_last / rg_s2_group_sums_last.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "step2_internal.h"

#define GRP_PL 8      // planes per workgroup

struct GroupState {
  bool has_group = false, has_cases = false;
  std::vector<uint8_t> member;      // [n] host copy
  std::vector<uint8_t> masks;       // [P][n] caller's masks (empty: those of rg_s2_set_null)
  std::vector<uint8_t> is_case;     // [P][n] host copy (rg_s2_set_cases)
  std::vector<uint8_t> cmasks;      // [P][n] the masks handed over with the cases (empty: those of rg_s2_set_null)
  int mask_gen = -1;                // rg_s2_ctx::mask_gen the planes were packed at
  int64_t nw = 0;                   // words per plane: ceil(n / 16)
  int npl_g = 0, npl_c = 0;         // planes [0, npl_g) = the group's (0 or 1 + P), [npl_g, npl_g + npl_c) = the cases' (0 or P)
  uint32_t* d_planes = nullptr;     // [npl_g + npl_c][nw]
  void* d_rows = nullptr; size_t rows_cap = 0;
  void* d_out = nullptr; size_t out_cap = 0;
  // the group's part of the last case-entry launch (both sets there): what rg_s2_group_counts_last / rg_s2_group_sums_last hand out
  int last_kind = 0, last_bs = 0;   // 0: none, 1: counts, 2: sums
  int staged_kind = 0;              // d_rows holds the host rows of the last case entry (1: 2-bit, 2: uint16) at pitch staged_ld: rg_s2_case_rows_staged
  int64_t staged_ld = 0;
  std::vector<int32_t> last_gc;
  std::vector<int64_t> last_gs;
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

// Integer dosages against any plane set, eight samples per lane and pass (the case entries; rg_s2_group_sums_int keeps the kernel above): lane t of pass k
// takes samples 8 h .. 8 h + 7, h = t + 256 k -- ONE 16-byte load of the row (a wave reads 1 KiB contiguous) and the half h & 1 of plane word h >> 1.
// The observed bits of the eight values are gathered into the planes' layout once (bit 2 k), so a plane costs one AND and one popcount for the count
// and a bit-extract and a multiply-add per value for the sum.  Rows whose base or pitch is not a multiple of 16 bytes, and the last partial eight of
// a row, are read value by value (never past sample n - 1).  grid (bs, ceil(npl / GRP_PL)); out [bs][npl][2] int64 = exact sum, observed count.
__global__ __launch_bounds__(256) void k_s2_plane_sums_int8(const uint16_t* __restrict__ G, int64_t ld, int64_t n, const uint32_t* __restrict__ planes,
                                                            int64_t nw, int npl, int64_t* __restrict__ out) {
  __shared__ unsigned long long reds[GRP_PL][4];
  __shared__ int redc[GRP_PL][4];
  const uint16_t* row = G + (int64_t)blockIdx.x * ld;
  const int q0 = blockIdx.y * GRP_PL;
  const int nq = min(GRP_PL, npl - q0);
  const bool vec = ((reinterpret_cast<uintptr_t>(G) | (uintptr_t)(ld * 2)) & 15) == 0;
  const int64_t nh = (n + 7) / 8;
  unsigned long long sum[GRP_PL];
  int cnt[GRP_PL];
#pragma unroll
  for (int q = 0; q < GRP_PL; ++q) { sum[q] = 0; cnt[q] = 0; }
  for (int64_t h = threadIdx.x; h < nh; h += 256) {
    const int64_t s0 = h * 8;
    uint32_t v[8];
    if (vec && s0 + 8 <= n) {
      const uint4 x = *reinterpret_cast<const uint4*>(row + s0);
      v[0] = x.x & 0xFFFFu; v[1] = x.x >> 16; v[2] = x.y & 0xFFFFu; v[3] = x.y >> 16;
      v[4] = x.z & 0xFFFFu; v[5] = x.z >> 16; v[6] = x.w & 0xFFFFu; v[7] = x.w >> 16;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = s0 + k < n ? (uint32_t)row[s0 + k] : 0xFFFFu;
    }
    uint32_t ob = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t o = v[k] != 0xFFFFu ? 1u : 0u;
      ob |= o << (2 * k);
      v[k] = o ? v[k] : 0u;
    }
    const int sh = (int)(h & 1) * 16;
    const int64_t w = h >> 1;
#pragma unroll
    for (int q = 0; q < GRP_PL; ++q) {
      if (q < nq) {
        const uint32_t m = (planes[(int64_t)(q0 + q) * nw + w] >> sh) & ob;      // (the planes hold nothing at odd positions)
        cnt[q] += __popc(m);
        uint32_t part = 0;                                                         // at most 8 * 65534
#pragma unroll
        for (int k = 0; k < 8; ++k) part += v[k] * ((m >> (2 * k)) & 1u);
        sum[q] += part;
      }
    }
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

// nq planes of one set into pl [nq][nw]: bit i of plane q = sel(q, i) AND mask(q, i).  sel: [n] shared by the planes (sel_stride 0) or [nq][n]
// (sel_stride n); masks: [nq][n] or null (no mask).  The one place a membership becomes plane bits.
static void grp_pack_set(uint32_t* pl, int64_t nw, int64_t n, int nq, const uint8_t* sel, int64_t sel_stride, const uint8_t* masks) {
  for (int q = 0; q < nq; ++q) {
    const uint8_t* s = sel + (size_t)q * sel_stride;
    const uint8_t* m = masks ? masks + (size_t)q * n : nullptr;
    uint32_t* p = pl + (size_t)q * nw;
    for (int64_t i = 0; i < n; ++i)
      if (s[i] && (!m || m[i])) p[i >> 4] |= 1u << (2 * (i & 15));
  }
}

// both sets -> bit planes, uploaded
static int grp_pack(rg_s2_ctx* ctx) {
  GroupState& g = *ctx->grp;
  const int64_t n = ctx->n;
  const int P = ctx->P;
  std::vector<uint32_t> pl((size_t)(g.npl_g + g.npl_c) * g.nw, 0u);
  if (g.has_group) {
    grp_pack_set(pl.data(), g.nw, n, 1, g.member.data(), 0, nullptr);
    grp_pack_set(pl.data() + g.nw, g.nw, n, P, g.member.data(), 0, g.masks.empty() ? ctx->hM.data() : g.masks.data());
  }
  if (g.has_cases) grp_pack_set(pl.data() + (size_t)g.npl_g * g.nw, g.nw, n, P, g.is_case.data(), n, g.cmasks.empty() ? ctx->hM.data() : g.cmasks.data());
  S2_HIP(hipMemcpyAsync(g.d_planes, pl.data(), pl.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->st));
  S2_HIP(hipStreamSynchronize(ctx->st));
  g.mask_gen = ctx->mask_gen;
  g.last_kind = 0; g.staged_kind = 0;
  return RG_S2_OK;
}

// after a set call changed which sets are there: the plane buffer at its new size, packed; nothing left of the state when both are gone
static int grp_rebuild(rg_s2_ctx* ctx) {
  GroupState& g = *ctx->grp;
  if (!g.has_group && !g.has_cases) { rg_s2_group_free(ctx); return RG_S2_OK; }
  g.nw = (ctx->n + 15) / 16;
  g.npl_g = g.has_group ? 1 + ctx->P : 0;
  g.npl_c = g.has_cases ? ctx->P : 0;
  if (g.d_planes) S2_HIP(hipFree(g.d_planes));
  g.d_planes = nullptr;
  S2_HIP(hipMalloc((void**)&g.d_planes, sizeof(uint32_t) * (size_t)(g.npl_g + g.npl_c) * g.nw));
  return grp_pack(ctx);
}

static int grp_ready(rg_s2_ctx* ctx, const char* who, bool cases) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, std::string(who) + ": context was not created");
  if (!cases && !(ctx->grp && ctx->grp->has_group)) return rg_s2_fail(ctx, RG_S2_ERR_ARG, std::string(who) + ": no group has been set (rg_s2_set_group)");
  if (cases && !(ctx->grp && ctx->grp->has_cases)) return rg_s2_fail(ctx, RG_S2_ERR_ARG, std::string(who) + ": no cases have been set (rg_s2_set_cases)");
  S2_HIP(hipSetDevice(ctx->dev));
  const GroupState& g = *ctx->grp;
  const bool ctx_masks = (g.has_group && g.masks.empty()) || (g.has_cases && g.cmasks.empty());
  if (ctx_masks && g.mask_gen != ctx->mask_gen) return grp_pack(ctx);      // rg_s2_set_null brought new masks
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

// the rows of a hard-call block where the kernel reads them: the caller's device rows, or a staged copy of its host rows
static int grp_stage_packed(rg_s2_ctx* ctx, const uint8_t* rows, int64_t ld, int32_t bs, int32_t rows_on_device, const uint8_t** d, int64_t* ldd) {
  GroupState& g = *ctx->grp;
  const int64_t nbytes = (ctx->n + 3) / 4;
  *d = rows; *ldd = ld;
  if (rows_on_device) return RG_S2_OK;
  *ldd = (nbytes + 3) / 4 * 4;
  int rc = grp_ensure(ctx, &g.d_rows, &g.rows_cap, (size_t)bs * *ldd);
  if (rc != RG_S2_OK) return rc;
  S2_HIP(hipMemcpy2DAsync(g.d_rows, (size_t)*ldd, rows, (size_t)ld, (size_t)nbytes, (size_t)bs, hipMemcpyHostToDevice, ctx->st));
  *d = (const uint8_t*)g.d_rows;
  return RG_S2_OK;
}

// the same for uint16 rows; pitch: the staged copy's row length is rounded up to that many elements (8: the 16-byte loads of k_s2_plane_sums_int8)
static int grp_stage_int(rg_s2_ctx* ctx, const uint16_t* G, int64_t ld, int32_t bs, int32_t g_on_device, int64_t pitch, const uint16_t** d, int64_t* ldd) {
  GroupState& g = *ctx->grp;
  const int64_t n = ctx->n;
  *d = G; *ldd = ld;
  if (g_on_device) return RG_S2_OK;
  *ldd = (n + pitch - 1) / pitch * pitch;
  int rc = grp_ensure(ctx, &g.d_rows, &g.rows_cap, sizeof(uint16_t) * (size_t)bs * *ldd);
  if (rc != RG_S2_OK) return rc;
  S2_HIP(hipMemcpy2DAsync(g.d_rows, sizeof(uint16_t) * (size_t)*ldd, G, sizeof(uint16_t) * (size_t)ld, sizeof(uint16_t) * (size_t)n, (size_t)bs, hipMemcpyHostToDevice, ctx->st));
  *d = (const uint16_t*)g.d_rows;
  return RG_S2_OK;
}

// what every count entry does after its launch: results to the host, the kernel's time
template <typename T>
static int grp_finish(rg_s2_ctx* ctx, T* host, size_t bytes) {
  GroupState& g = *ctx->grp;
  S2_HIP(hipGetLastError());
  S2_HIP(hipEventRecord(ctx->e1, ctx->st));
  S2_HIP(hipMemcpyAsync(host, g.d_out, bytes, hipMemcpyDeviceToHost, ctx->st));
  S2_HIP(hipStreamSynchronize(ctx->st));
  float ms = 0.f;
  S2_HIP(hipEventElapsedTime(&ms, ctx->e0, ctx->e1));
  ctx->last_ms = ms;
  return RG_S2_OK;
}

// a case entry's results [bs][npl][w] split into the caller's [bs][P][w] and, with a group there, the kept [bs][1 + P][w]
template <typename T>
static void grp_split(const GroupState& g, const std::vector<T>& all, int bs, int w, T* cases, std::vector<T>& group) {
  const size_t npl = (size_t)(g.npl_g + g.npl_c), ng = (size_t)g.npl_g * w, nc = (size_t)g.npl_c * w;
  group.resize((size_t)bs * ng);
  for (int j = 0; j < bs; ++j) {
    const T* src = all.data() + (size_t)j * npl * w;
    if (ng) std::memcpy(group.data() + (size_t)j * ng, src, ng * sizeof(T));
    std::memcpy(cases + (size_t)j * nc, src + ng, nc * sizeof(T));
  }
}

extern "C" {

int rg_s2_set_group(rg_s2_ctx* ctx, const uint8_t* member, const uint8_t* mask) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_set_group: context was not created");
  S2_HIP(hipSetDevice(ctx->dev));
  S2_HIP(hipStreamSynchronize(ctx->st));
  if (!member) {
    if (!ctx->grp) return RG_S2_OK;
    ctx->grp->has_group = false;
    ctx->grp->member.clear(); ctx->grp->masks.clear();
    return grp_rebuild(ctx);
  }
  const size_t n = (size_t)ctx->n, nm = n * (size_t)ctx->P;
  if (!mask && ctx->hM.size() != nm) {
    if (ctx->grp) {      // a refused call leaves no group behind (the cases stay)
      ctx->grp->has_group = false;
      ctx->grp->member.clear(); ctx->grp->masks.clear();
      (void)grp_rebuild(ctx);
    }
    return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_set_group: the trait masks are not there (call rg_s2_set_null first, or hand over the masks)");
  }
  if (!ctx->grp) ctx->grp = new GroupState();
  GroupState& g = *ctx->grp;
  g.has_group = true;
  g.member.assign(member, member + n);
  g.masks.clear();
  if (mask) g.masks.assign(mask, mask + nm);
  return grp_rebuild(ctx);
}

int rg_s2_set_cases(rg_s2_ctx* ctx, const uint8_t* is_case, const uint8_t* mask) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_set_cases: context was not created");
  S2_HIP(hipSetDevice(ctx->dev));
  S2_HIP(hipStreamSynchronize(ctx->st));
  if (!is_case) {
    if (!ctx->grp) return RG_S2_OK;
    ctx->grp->has_cases = false;
    ctx->grp->is_case.clear(); ctx->grp->cmasks.clear();
    return grp_rebuild(ctx);
  }
  const size_t nm = (size_t)ctx->n * (size_t)ctx->P;
  if (!mask && ctx->hM.size() != nm)
    return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_set_cases: the trait masks are not there (call rg_s2_set_null first, or hand over the masks)");
  if (!ctx->grp) ctx->grp = new GroupState();
  GroupState& g = *ctx->grp;
  g.has_cases = true;
  g.is_case.assign(is_case, is_case + nm);
  g.cmasks.clear();
  if (mask) g.cmasks.assign(mask, mask + nm);
  return grp_rebuild(ctx);
}

int rg_s2_group_counts_packed(rg_s2_ctx* ctx, const uint8_t* rows, int64_t ld, int32_t bs, int32_t rows_on_device, int32_t flip, int32_t* counts) {
  int rc = grp_ready(ctx, "rg_s2_group_counts_packed", false);
  if (rc != RG_S2_OK) return rc;
  const int64_t n = ctx->n, nbytes = (n + 3) / 4;
  if (!rows || !counts || bs < 1 || ld < nbytes) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_counts_packed: need rows, counts, bs >= 1 and ld >= ceil(n / 4)");
  GroupState& g = *ctx->grp;
  const int npl = g.npl_g;
  const uint8_t* d;
  int64_t ldd;
  g.staged_kind = 0;
  if ((rc = grp_stage_packed(ctx, rows, ld, bs, rows_on_device, &d, &ldd)) != RG_S2_OK) return rc;
  const size_t ob = sizeof(int32_t) * 3 * (size_t)npl * bs;
  if ((rc = grp_ensure(ctx, &g.d_out, &g.out_cap, ob)) != RG_S2_OK) return rc;
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  hipLaunchKernelGGL(k_s2_group_counts, dim3(bs, (npl + GRP_PL - 1) / GRP_PL), dim3(256), 0, ctx->st, d, ldd, n, flip ? 1 : 0, g.d_planes, g.nw, npl, (int32_t*)g.d_out);
  return grp_finish(ctx, counts, ob);
}

int rg_s2_group_sums_int(rg_s2_ctx* ctx, const uint16_t* G, int64_t ld, int32_t bs, int32_t g_on_device, int64_t* sums) {
  int rc = grp_ready(ctx, "rg_s2_group_sums_int", false);
  if (rc != RG_S2_OK) return rc;
  const int64_t n = ctx->n;
  if (!G || !sums || bs < 1 || ld < n) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_sums_int: need G, sums, bs >= 1 and ld >= n");
  GroupState& g = *ctx->grp;
  const int npl = g.npl_g;
  const uint16_t* d;
  int64_t ldd;
  g.staged_kind = 0;
  if ((rc = grp_stage_int(ctx, G, ld, bs, g_on_device, 1, &d, &ldd)) != RG_S2_OK) return rc;
  const size_t ob = sizeof(int64_t) * 2 * (size_t)npl * bs;
  if ((rc = grp_ensure(ctx, &g.d_out, &g.out_cap, ob)) != RG_S2_OK) return rc;
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  hipLaunchKernelGGL(k_s2_group_sums_int, dim3(bs, (npl + GRP_PL - 1) / GRP_PL), dim3(256), 0, ctx->st, d, ldd, n, g.d_planes, g.nw, npl, (int64_t*)g.d_out);
  return grp_finish(ctx, sums, ob);
}

int rg_s2_case_counts_packed(rg_s2_ctx* ctx, const uint8_t* rows, int64_t ld, int32_t bs, int32_t rows_on_device, int32_t flip, int32_t* counts) {
  int rc = grp_ready(ctx, "rg_s2_case_counts_packed", true);
  if (rc != RG_S2_OK) return rc;
  const int64_t n = ctx->n, nbytes = (n + 3) / 4;
  if (!rows || !counts || bs < 1 || ld < nbytes) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_case_counts_packed: need rows, counts, bs >= 1 and ld >= ceil(n / 4)");
  GroupState& g = *ctx->grp;
  const int npl = g.npl_g + g.npl_c;      // one launch over both sets: the rows are read once
  const uint8_t* d;
  int64_t ldd;
  g.last_kind = 0; g.staged_kind = 0;
  if ((rc = grp_stage_packed(ctx, rows, ld, bs, rows_on_device, &d, &ldd)) != RG_S2_OK) return rc;
  std::vector<int32_t> all((size_t)bs * npl * 3);
  const size_t ob = sizeof(int32_t) * all.size();
  if ((rc = grp_ensure(ctx, &g.d_out, &g.out_cap, ob)) != RG_S2_OK) return rc;
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  hipLaunchKernelGGL(k_s2_group_counts, dim3(bs, (npl + GRP_PL - 1) / GRP_PL), dim3(256), 0, ctx->st, d, ldd, n, flip ? 1 : 0, g.d_planes, g.nw, npl, (int32_t*)g.d_out);
  if ((rc = grp_finish(ctx, all.data(), ob)) != RG_S2_OK) return rc;
  grp_split(g, all, bs, 3, counts, g.last_gc);
  if (g.has_group) { g.last_kind = 1; g.last_bs = bs; }
  if (!rows_on_device) { g.staged_kind = 1; g.staged_ld = ldd; }
  return RG_S2_OK;
}

int rg_s2_case_sums_int(rg_s2_ctx* ctx, const uint16_t* G, int64_t ld, int32_t bs, int32_t g_on_device, int64_t* sums) {
  int rc = grp_ready(ctx, "rg_s2_case_sums_int", true);
  if (rc != RG_S2_OK) return rc;
  const int64_t n = ctx->n;
  if (!G || !sums || bs < 1 || ld < n) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_case_sums_int: need G, sums, bs >= 1 and ld >= n");
  GroupState& g = *ctx->grp;
  const int npl = g.npl_g + g.npl_c;
  const uint16_t* d;
  int64_t ldd;
  g.last_kind = 0; g.staged_kind = 0;
  if ((rc = grp_stage_int(ctx, G, ld, bs, g_on_device, 8, &d, &ldd)) != RG_S2_OK) return rc;
  std::vector<int64_t> all((size_t)bs * npl * 2);
  const size_t ob = sizeof(int64_t) * all.size();
  if ((rc = grp_ensure(ctx, &g.d_out, &g.out_cap, ob)) != RG_S2_OK) return rc;
  S2_HIP(hipEventRecord(ctx->e0, ctx->st));
  hipLaunchKernelGGL(k_s2_plane_sums_int8, dim3(bs, (npl + GRP_PL - 1) / GRP_PL), dim3(256), 0, ctx->st, d, ldd, n, g.d_planes, g.nw, npl, (int64_t*)g.d_out);
  if ((rc = grp_finish(ctx, all.data(), ob)) != RG_S2_OK) return rc;
  grp_split(g, all, bs, 2, sums, g.last_gs);
  if (g.has_group) { g.last_kind = 2; g.last_bs = bs; }
  if (!g_on_device) { g.staged_kind = 2; g.staged_ld = ldd; }
  return RG_S2_OK;
}

int rg_s2_group_counts_last(rg_s2_ctx* ctx, int32_t bs, int32_t* counts) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_counts_last: context was not created");
  if (!counts || !ctx->grp || ctx->grp->last_kind != 1)
    return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_counts_last: no rg_s2_case_counts_packed call with a group set since the planes were last packed");
  if (bs != ctx->grp->last_bs) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_counts_last: bs is not that of the last rg_s2_case_counts_packed call");
  std::memcpy(counts, ctx->grp->last_gc.data(), ctx->grp->last_gc.size() * sizeof(int32_t));
  return RG_S2_OK;
}

int rg_s2_group_sums_last(rg_s2_ctx* ctx, int32_t bs, int64_t* sums) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_sums_last: context was not created");
  if (!sums || !ctx->grp || ctx->grp->last_kind != 2)
    return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_sums_last: no rg_s2_case_sums_int call with a group set since the planes were last packed");
  if (bs != ctx->grp->last_bs) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_group_sums_last: bs is not that of the last rg_s2_case_sums_int call");
  std::memcpy(sums, ctx->grp->last_gs.data(), ctx->grp->last_gs.size() * sizeof(int64_t));
  return RG_S2_OK;
}

int rg_s2_case_rows_staged(rg_s2_ctx* ctx, const void** rows, int64_t* ld) {
  if (!ctx || !ctx->st) return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_case_rows_staged: context was not created");
  if (!rows || !ld || !ctx->grp || !ctx->grp->staged_kind)
    return rg_s2_fail(ctx, RG_S2_ERR_ARG, "rg_s2_case_rows_staged: the last count entry was no case entry on host rows");
  *rows = ctx->grp->d_rows; *ld = ctx->grp->staged_ld;
  return RG_S2_OK;
}

}  // extern "C"
