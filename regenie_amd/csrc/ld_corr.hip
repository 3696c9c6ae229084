// The Step-2 LD matrix of a region (include/rg_ld.h): Data::print_ld (reference src/Data.cpp:4368-4449) on the matrix cores.
//
//   sum_s g_i g_j = A_ij + m_j B_ij + m_i B_ji + m_i m_j D_ij      A = g0 g0^T, B_ij = sum g0_i miss_j, D = miss miss^T   (exact int32)
//   LD_ij         = sum_s g_i g_j - sum_c (X^T g_i)_c (X^T g_j)_c                                                          (fp64)
//
// k_ld_gram is the hot kernel: a 128 x 128 tile of row-panel variants against column-panel variants over all samples, both operands
// read from the row store at 2 bits per genotype and expanded to int8 on the way to LDS (v_perm_b32 as a 4-entry byte LUT, as
// gram_i8.hip does), contracted with v_mfma_i32_32x32x32_i8.  Against gram_i8.hip's tile it keeps the next K-step's 16 packed bytes
// in flight in registers while the current one is multiplied, and double-buffers the LDS image so that a K-step costs one barrier.
// Rows of the store are padded with code 11 (-> 0 for the dosage and for the indicator) to a multiple of 64 samples: the sample
// tail is zero fill, there is no second kernel.  Only tile pairs on or above the diagonal are computed; the B / D passes leave at
// once for tiles without a missing call.  X^T g_i comes from rg_s2_contract_packed (step2_qt.hip, exact digit planes).
#include "rg_internal.h"
#include "../../include/rg_ld.h"
#include "../../include/rg_step2.h"

#include <algorithm>
#include <string>
#include <vector>

#define LT 128
#define LPITCH 80  // 64 data bytes + 16 pad (gram_i8.hip: conflict-free ds_read_b128 fragment reads)
#define LD_LUT_DOSAGE 0x00010002u  // 00 -> 2, 01 -> missing (0), 10 -> 1, 11 -> 0
#define LD_LUT_MISS 0x00000100u

namespace {

__device__ __forceinline__ unsigned ld_expand4(unsigned b, unsigned lut) {
  unsigned x = b | (b << 6);
  x = x | (x << 12);
  x &= 0x03030303u;
  return __builtin_amdgcn_perm(lut, lut, x);
}

__device__ __forceinline__ void ld_stage(uint4 w, unsigned lut, uint8_t* lds_row) {
  unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint4 o;
    o.x = ld_expand4(ws[d] & 0xFFu, lut);
    o.y = ld_expand4((ws[d] >> 8) & 0xFFu, lut);
    o.z = ld_expand4((ws[d] >> 16) & 0xFFu, lut);
    o.w = ld_expand4(ws[d] >> 24, lut);
    *reinterpret_cast<uint4*>(lds_row + d * 16) = o;
  }
}

// One 128 x 128 tile: C[r][c] = sum_k lutA(A[r][k]) * lutB(B[c][k]); rows of A and B are ld bytes apart, ld a multiple of 16.
__device__ __forceinline__ void ld_tile(const uint8_t* __restrict__ A, int a_rows, unsigned a_lut, const uint8_t* __restrict__ B, int b_rows,
                                        unsigned b_lut, bool same, int64_t ld, int32_t* __restrict__ C, int64_t ldc, uint8_t* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  v16i acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  const bool isA = tid < LT;
  const int srow = isA ? tid : tid - LT;
  const bool do_stage = isA || !same;
  const bool valid = do_stage && (isA ? srow < a_rows : srow < b_rows);
  const uint8_t* gbase = isA ? A + (int64_t)srow * ld : B + (int64_t)srow * ld;
  const unsigned lut = isA ? a_lut : b_lut;
  const int my_off = (isA ? 0 : LT * LPITCH) + srow * LPITCH;
  const int b_off = same ? 0 : LT * LPITCH;
  const int64_t nk = ld / 16;
  const uint4 pad = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);  // code 11 -> 0
  uint4 w = pad;
  if (valid) w = *reinterpret_cast<const uint4*>(gbase);
  for (int64_t k = 0; k < nk; ++k) {
    uint8_t* buf = smem + (k & 1) * (2 * LT * LPITCH);
    if (do_stage) ld_stage(w, lut, buf + my_off);
    if (valid && k + 1 < nk) w = *reinterpret_cast<const uint4*>(gbase + (k + 1) * 16);   // in flight while this step is multiplied
    __syncthreads();   // the other buffer was read before the previous barrier: one barrier per step is enough
    const uint8_t* sA = buf;
    const uint8_t* sB = buf + b_off;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v4i af[2], bf[2];
      const int koff = ks * 32 + (lane >> 5) * 16;
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const v4i*>(sA + (wr * 64 + i * 32 + (lane & 31)) * LPITCH + koff);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const v4i*>(sB + (wc * 64 + j * 32 + (lane & 31)) * LPITCH + koff);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }
  // C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int col = wc * 64 + j * 32 + (lane & 31);
        if (row < a_rows && col < b_rows) C[(int64_t)row * ldc + col] = acc[i][j][r];
      }
}

// The tile pair (tr, tc) of workgroup blockIdx.x over nta x ntb tiles; tri: pairs tr <= tc only.  false: no such pair.
__device__ __forceinline__ bool ld_tile_pair(int nta, int ntb, int tri, int& tr, int& tc) {
  int tidx = blockIdx.x;
  {  // XCD-aware remap (gram_i8.hip): consecutive tile ids share an operand panel; keep them on one XCD's L2
    const int nwg = gridDim.x;
    const int q = nwg / 8, r = nwg % 8, xcd = tidx % 8, k = tidx / 8;
    tidx = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  if (tri) {  // unrank over tc >= tr: pair index = tc (tc + 1) / 2 + tr
    tc = (int)((sqrtf(8.0f * tidx + 1.0f) - 1.0f) * 0.5f);
    while ((tc + 1) * (tc + 2) / 2 <= tidx) ++tc;
    while (tc * (tc + 1) / 2 > tidx) --tc;
    tr = tidx - tc * (tc + 1) / 2;
  } else {
    tr = tidx / ntb;
    tc = tidx - tr * ntb;
  }
  return tr < nta && tc < ntb;
}

// The body of the Gram kernels: grid.x = tile pair, grid.y = which sum (0: A, 1: B, 2: B of the mirrored pair / Bt, 3: D).
//   tri != 0 (rg_ld_finish): rows [0, na) against themselves, tile pairs tr <= tc only; SA, SD [na][na] (upper tiles written),
//     SB [na][na] full: y = 1 writes tile (tr, tc) of it, y = 2 tile (tc, tr); tile_miss[t] != 0: tile t has a missing call.
//   kinds: bit k set = sum k is wanted.
//   tri == 0 (rg_ld_pair_sums): rows [a0, a0 + na) against [b0, b0 + nb), every tile pair and every sum; SBt [na][nb] is y = 2.
// Store: the row store and its tile routine -- run<MA, MB>(ra, a_rows, rb, b_rows, same, C, ldc, smem): the tile of the rows from ra on
// against the rows from rb on into C; MA / MB: the operand is the missing indicator of its rows, not their dosage.
template <class Store, class Sum = typename Store::Sum>
__device__ __forceinline__ void ld_sums(const Store& s, int a0, int na, int b0, int nb, int tri, int kinds, const uint8_t* __restrict__ tile_miss, Sum* SA, Sum* SB,
                                        Sum* SBt, Sum* SD, int64_t ldc, uint8_t* smem) {
  int tr, tc;
  if (!ld_tile_pair((na + LT - 1) / LT, (nb + LT - 1) / LT, tri, tr, tc)) return;
  const int kind = blockIdx.y;
  if (!((kinds >> kind) & 1)) return;      // a sum the caller did not ask for
  const int ra = a0 + tr * LT, rb = b0 + tc * LT;
  const int ar = min(LT, na - tr * LT), bc = min(LT, nb - tc * LT);
  const bool diag = tri && tr == tc;
  const int64_t at = (int64_t)tr * LT * ldc + (int64_t)tc * LT;      // tile (tr, tc) of an output
  if (kind == 0) {
    s.template run<false, false>(ra, ar, rb, bc, diag, SA + at, ldc, smem);
  } else if (kind == 1) {
    if (tile_miss && !tile_miss[tc]) return;
    s.template run<false, true>(ra, ar, rb, bc, false, SB + at, ldc, smem);
  } else if (kind == 2) {
    if (tri) {  // B of the mirrored pair: dosage of tile tc against the indicator of tile tr
      if (diag || (tile_miss && !tile_miss[tr])) return;
      s.template run<false, true>(rb, bc, ra, ar, false, SB + (int64_t)tc * LT * ldc + (int64_t)tr * LT, ldc, smem);
    } else {
      s.template run<true, false>(ra, ar, rb, bc, false, SBt + at, ldc, smem);
    }
  } else {
    if (tile_miss && !(tile_miss[tr] && tile_miss[tc])) return;
    s.template run<true, true>(ra, ar, rb, bc, diag, SD + at, ldc, smem);
  }
}

struct LdRows {      // the 2-bit row store: the LUT that expands the codes makes an operand the dosage or the indicator
  using Sum = int32_t;
  const uint8_t* rows;
  int64_t ld;
  template <bool MA, bool MB>
  __device__ __forceinline__ void run(int ra, int a_rows, int rb, int b_rows, bool same, Sum* C, int64_t ldc, uint8_t* smem) const {
    ld_tile(rows + (int64_t)ra * ld, a_rows, MA ? LD_LUT_MISS : LD_LUT_DOSAGE, rows + (int64_t)rb * ld, b_rows, MB ? LD_LUT_MISS : LD_LUT_DOSAGE, same, ld, C, ldc, smem);
  }
};

__global__ __launch_bounds__(256) void k_ld_gram(const uint8_t* __restrict__ rows, int64_t ld, int a0, int na, int b0, int nb, int tri, int kinds,
                                                 const uint8_t* __restrict__ tile_miss, int32_t* SA, int32_t* SB, int32_t* SBt, int32_t* SD, int64_t ldc) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * 2 * LT * LPITCH];
  ld_sums(LdRows{rows, ld}, a0, na, b0, nb, tri, kinds, tile_miss, SA, SB, SBt, SD, ldc, smem);
}

// Rows as they arrive (nbytes = ceil(n / 4) bytes used, ld bytes apart, already copied into the store) -> the store's form:
// the other allele when flip, the codes past sample n and the padding up to ld set to 11.  One workgroup per row.
__global__ __launch_bounds__(256) void k_ld_store(uint8_t* __restrict__ rows, int64_t ld, int64_t n, int flip) {
  uint8_t* row = rows + (int64_t)blockIdx.x * ld;
  const int64_t nbytes = (n + 3) / 4;
  for (int64_t b = threadIdx.x; b < ld; b += blockDim.x) {
    unsigned v = b < nbytes ? row[b] : 0xFFu;
    if (flip) {  // 00 <-> 11, 01 and 10 stay
      const unsigned eq = ~((v >> 1) ^ v) & 0x55u;
      v ^= eq | (eq << 1);
    }
    if (b == nbytes - 1 && (n & 3)) v |= (0xFFu << (2 * (n & 3))) & 0xFFu;
    if (b >= nbytes) v = 0xFFu;
    row[b] = (uint8_t)v;
  }
}

// ---- integer dosages (rg_ld_append_int) ---------------------------------------------------------------------------------------------
// The store: int8 planes [NP + 1][M][Kp], Kp = n rounded up to the K-step of 64: the NP balanced base-128 digits of a row
// (g0 = sum_p 128^p d_p, d_p in [-64, 63]; the split of k_s2_int_rows, step2_qt.hip) and its missing indicator as plane NP, zero
// past sample n.  The split is done once per row on append, not per K-step in the Gram kernel: profiles/ld_corr.md found k_ld_gram
// held back by expanding its operands on the vector units at every K-step, and here a row is read by every tile pair of its panel.
// bad: set when a value other than 0xFFFF exceeds vmax.  One workgroup per row.
__global__ __launch_bounds__(256) void k_ld_store_int(const uint16_t* __restrict__ G, int64_t ldg, int64_t n, int64_t Kp, int NP, unsigned vmax,
                                                      int8_t* __restrict__ planes, int64_t plane_stride, int32_t* __restrict__ bad) {
  const uint16_t* g = G + (int64_t)blockIdx.x * ldg;
  int8_t* out = planes + (int64_t)blockIdx.x * Kp;
  bool over = false;
  for (int64_t i0 = (int64_t)threadIdx.x * 4; i0 < Kp; i0 += 256 * 4) {
    unsigned dig[3] = {0u, 0u, 0u}, mb = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned raw = i0 + e < n ? g[i0 + e] : 0u;
      const bool miss = raw == 0xFFFFu;
      over |= !miss && raw > vmax;
      int v = (miss || raw > vmax) ? 0 : (int)raw;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int d = ((v & 127) ^ 64) - 64;
        dig[k] |= (unsigned)(uint8_t)(int8_t)d << (8 * e);
        v = (v - d) >> 7;
      }
      mb |= (miss ? 1u : 0u) << (8 * e);
    }
    for (int k = 0; k < NP; ++k) *reinterpret_cast<unsigned*>(out + (int64_t)k * plane_stride + i0) = dig[k];
    *reinterpret_cast<unsigned*>(out + (int64_t)NP * plane_stride + i0) = mb;
  }
  if (over) atomicOr(bad, 1);
}

// A digit product is at most 64 * 64 and at most three plane pairs share an accumulator (those of equal weight p + q), so an int32
// accumulator is safe for floor((2^31 - 1) / (3 * 4096)) = 174,762 samples: it is flushed into the 64-bit sum every 2,048 K-steps
// (131,072 samples).
#define LDI_FLUSH 2048

// One 128 x 128 tile of 64-bit sums: C[r][c] = sum_k (sum_p 128^p A_p[r][k]) (sum_q 128^q B_q[c][k]) for NA planes of the row
// operand and NB of the column operand (a plane is ps bytes after the one before; rows are Kp bytes apart, Kp a multiple of 64).
// A K-step's planes are staged in LDS once and every plane pair runs against that image; the pairs of equal weight p + q share an
// accumulator.  512 threads: wave w owns rows [32 (w >> 1), +32) x columns [64 (w & 1), +64), so NA + NB - 1 accumulators are
// 32 (NA + NB - 1) registers and two waves fit a SIMD (a 64 x 64 wave tile would need 320 accumulator registers for three digits).
template <int NA, int NB>
__device__ __forceinline__ void ldi_tile(const int8_t* __restrict__ A, int a_rows, const int8_t* __restrict__ B, int b_rows, bool same, int64_t Kp,
                                         int64_t ps, long long* __restrict__ C, int64_t ldc, uint8_t* smem) {
  constexpr int NW = NA + NB - 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  v16i acc[NW][2];
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[w][j][r] = 0;

  // staging: thread -> (operand, row, half of the 64-byte K-step)
  const bool isA = tid < 2 * LT;
  const int srow = (tid & (2 * LT - 1)) >> 1, half = tid & 1;
  constexpr int NS = NA > NB ? NA : NB;
  const int my_np = isA ? NA : NB;
  const bool do_stage = isA || !same;
  const bool valid = do_stage && (isA ? srow < a_rows : srow < b_rows);
  const int8_t* gbase = (isA ? A : B) + (int64_t)srow * Kp + half * 32;
  const int b_off = same ? 0 : NA * LT * LPITCH;
  const int my_off = (isA ? 0 : NA * LT * LPITCH) + srow * LPITCH + half * 32;
  const int64_t nk = Kp / 64;
  uint4 w0[NS], w1[NS];
#pragma unroll
  for (int p = 0; p < NS; ++p) {
    w0[p] = make_uint4(0u, 0u, 0u, 0u);
    w1[p] = w0[p];
    if (valid && p < my_np) {
      w0[p] = *reinterpret_cast<const uint4*>(gbase + (int64_t)p * ps);
      w1[p] = *reinterpret_cast<const uint4*>(gbase + (int64_t)p * ps + 16);
    }
  }
  bool first = true;
  for (int64_t k = 0; k < nk; ++k) {
    if (k) __syncthreads();   // the image of the previous step has been read
    if (do_stage) {
#pragma unroll
      for (int p = 0; p < NS; ++p)
        if (p < my_np) {
          *reinterpret_cast<uint4*>(smem + my_off + p * LT * LPITCH) = w0[p];
          *reinterpret_cast<uint4*>(smem + my_off + p * LT * LPITCH + 16) = w1[p];
        }
    }
    if (valid && k + 1 < nk) {   // in flight while this step is multiplied
#pragma unroll
      for (int p = 0; p < NS; ++p)
        if (p < my_np) {
          w0[p] = *reinterpret_cast<const uint4*>(gbase + (int64_t)p * ps + (k + 1) * 64);
          w1[p] = *reinterpret_cast<const uint4*>(gbase + (int64_t)p * ps + (k + 1) * 64 + 16);
        }
    }
    __syncthreads();
    const uint8_t* sA = smem;
    const uint8_t* sB = smem + b_off;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int koff = ks * 32 + (lane >> 5) * 16;
      v4i af[NA], bf[NB][2];
#pragma unroll
      for (int p = 0; p < NA; ++p) af[p] = *reinterpret_cast<const v4i*>(sA + (p * LT + wr * 32 + (lane & 31)) * LPITCH + koff);
#pragma unroll
      for (int q = 0; q < NB; ++q)
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[q][j] = *reinterpret_cast<const v4i*>(sB + (q * LT + wc * 64 + j * 32 + (lane & 31)) * LPITCH + koff);
#pragma unroll
      for (int p = 0; p < NA; ++p)
#pragma unroll
        for (int q = 0; q < NB; ++q)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[p + q][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[p], bf[q][j], acc[p + q][j], 0, 0, 0);
    }
    if (((k + 1) % LDI_FLUSH) == 0 || k + 1 == nk) {
      // C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const int col = wc * 64 + j * 32 + (lane & 31);
          long long v = 0;
#pragma unroll
          for (int w = NW - 1; w >= 0; --w) { v = v * 128 + (long long)acc[w][j][r]; acc[w][j][r] = 0; }
          if (row < a_rows && col < b_rows) {
            long long* c = C + (int64_t)row * ldc + col;
            *c = first ? v : *c + v;   // the tile is this workgroup's alone
          }
        }
      first = false;
    }
  }
}

// k_ld_gram for the plane store: the same grid, tile-pair order and meaning of tri, kinds, tile_miss and the four sums (64-bit
// here); row r of the matrix is row r of every plane: of the NP digit planes for the dosage, of the one after them for the indicator.
template <int NP>
struct LdPlanes {
  using Sum = long long;
  const int8_t* planes;
  int64_t Kp, ps;
  template <bool MA, bool MB>
  __device__ __forceinline__ void run(int ra, int a_rows, int rb, int b_rows, bool same, Sum* C, int64_t ldc, uint8_t* smem) const {
    ldi_tile<MA ? 1 : NP, MB ? 1 : NP>(planes + (int64_t)ra * Kp + (MA ? NP * ps : 0), a_rows, planes + (int64_t)rb * Kp + (MB ? NP * ps : 0), b_rows, same, Kp, ps, C,
                                       ldc, smem);
  }
};

template <int NP>
__global__ __launch_bounds__(512) void k_ld_gram_int(const int8_t* __restrict__ planes, int64_t Kp, int64_t ps, int a0, int na, int b0, int nb, int tri,
                                                     int kinds, const uint8_t* __restrict__ tile_miss, long long* SA, long long* SB, long long* SBt,
                                                     long long* SD, int64_t ldc) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * NP * LT * LPITCH];
  ld_sums(LdPlanes<NP>{planes, Kp, ps}, a0, na, b0, nb, tri, kinds, tile_miss, SA, SB, SBt, SD, ldc, smem);
}


// LD[ci][cj] for the row pair (i, j), i <= j, written to both triangles of the M x M matrix.  T = int32_t: hard calls (scale 1, no
// division); T = long long: integer dosages, A / scale^2 and B / scale in genotype units (means are in genotype units already).
template <class T>
__global__ __launch_bounds__(256) void k_ld_combine(const T* __restrict__ SA, const T* __restrict__ SB, const T* __restrict__ SD, int R, double scale,
                                                    const double* __restrict__ mean, const double* __restrict__ gx, int C,
                                                    const int32_t* __restrict__ col, double* __restrict__ LD, int M) {
  constexpr bool kInt = sizeof(T) == 8;
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= R || j >= R || i > j) return;
  double v = (double)SA[(int64_t)i * R + j];
  if (kInt) v = __ddiv_rn(v, __dmul_rn(scale, scale));
  if (SB) {
    const double mi = mean[i], mj = mean[j];
    double bij = (double)SB[(int64_t)i * R + j], bji = (double)SB[(int64_t)j * R + i];
    if (kInt) { bij = __ddiv_rn(bij, scale); bji = __ddiv_rn(bji, scale); }
    v = __dadd_rn(v, __dmul_rn(mj, bij));
    v = __dadd_rn(v, __dmul_rn(mi, bji));
    v = __dadd_rn(v, __dmul_rn(__dmul_rn(mi, mj), (double)SD[(int64_t)i * R + j]));
  }
  double p = 0.0;
  for (int c = 0; c < C; ++c) p = fma(gx[(int64_t)i * C + c], gx[(int64_t)j * C + c], p);
  v -= p;
  const int ci = col[i], cj = col[j];
  LD[(int64_t)ci * M + cj] = v;
  LD[(int64_t)cj * M + ci] = v;
}

// Data.cpp:4386-4397: zero[c] = diagonal in (-tol, 0); sds[c] = sqrt(numtol) for a non-positive diagonal (a zeroed one included)
__global__ void k_ld_diag(const double* __restrict__ LD, int M, double tol, double numtol, uint8_t* __restrict__ zero, double* __restrict__ inv_sd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= M) return;
  const double d = LD[(int64_t)c * M + c];
  const bool z = d < 0 && fabs(d) < tol;
  zero[c] = z ? 1 : 0;
  const double sd = (z || d <= 0) ? sqrt(numtol) : sqrt(d);
  inv_sd[c] = 1.0 / sd;
}

__device__ __forceinline__ double ld_corr_at(const double* __restrict__ LD, int M, const uint8_t* __restrict__ zero, const double* __restrict__ inv_sd,
                                             int i, int j) {
  if (i == j) {  // the diagonal becomes sds^2 before the scaling
    const double sd = 1.0 / inv_sd[i];
    return __dmul_rn(__dmul_rn(inv_sd[i], __dmul_rn(sd, sd)), inv_sd[i]);
  }
  const double v = (zero[i] || zero[j]) ? 0.0 : LD[(int64_t)i * M + j];
  return __dmul_rn(__dmul_rn(inv_sd[i], v), inv_sd[j]);
}

__global__ __launch_bounds__(256) void k_ld_corr(const double* __restrict__ LD, int M, const uint8_t* __restrict__ zero, const double* __restrict__ inv_sd,
                                                 double* __restrict__ out) {
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= M || j >= M) return;
  out[(int64_t)i * M + j] = ld_corr_at(LD, M, zero, inv_sd, min(i, j), max(i, j));
}

// print_ld's binary body: vals(k++) = r * r * 65535 + 0.5 over i < j, truncated to 16 bits (no fused multiply-add: the value is
// the one the host would compute from the correlation)
__global__ __launch_bounds__(256) void k_ld_r2(const double* __restrict__ LD, int M, const uint8_t* __restrict__ zero, const double* __restrict__ inv_sd,
                                               uint16_t* __restrict__ out) {
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= M || j >= M || i >= j) return;
  const double r = ld_corr_at(LD, M, zero, inv_sd, i, j);
  const double v = __dadd_rn(__dmul_rn(__dmul_rn(r, r), 65535.0), 0.5);
  const int64_t k = (int64_t)i * M - (int64_t)i * (i + 1) / 2 + (j - i - 1);
  out[k] = (uint16_t)(v < 65535.0 ? (unsigned)v : 65535u);
}

// ---- the unscaled matrix (--skip-scaleG) and its sparse form (--sparse-thr) -----------------------------------------------------------
// Data.cpp:4386-4391 and :4400: zero[c] as k_ld_diag; diag[c] = max(diagonal after the zeroing, numtol); sd[c] = sqrt(diag[c])
__global__ void k_ld_diag_gtg(const double* __restrict__ LD, int M, double tol, double numtol, uint8_t* __restrict__ zero, double* __restrict__ diag,
                              double* __restrict__ sd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= M) return;
  const double d = LD[(int64_t)c * M + c];
  const bool z = d < 0 && fabs(d) < tol;
  zero[c] = z ? 1 : 0;
  const double dd = fmax(z ? 0.0 : d, numtol);
  diag[c] = dd;
  sd[c] = sqrt(dd);
}

__global__ __launch_bounds__(256) void k_ld_gtg(const double* __restrict__ LD, int M, const uint8_t* __restrict__ zero, const double* __restrict__ diag,
                                                double* __restrict__ out) {
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= M || j >= M) return;
  out[(int64_t)i * M + j] = i == j ? diag[i] : ((zero[i] || zero[j]) ? 0.0 : LD[(int64_t)i * M + j]);
}

// The one predicate of the count pass and the write pass: v = LD[i][j] / sd[i] / sd[j] (Data.cpp:4417, the divisions as written),
// kept when fabs(v) >= thr.  ldrow: row i of LD; sdi = sd[i].
__device__ __forceinline__ bool ld_sparse_keep(const double* __restrict__ ldrow, bool zi, double sdi, const uint8_t* __restrict__ zero,
                                               const double* __restrict__ sd, int j, double thr, double& v) {
  const double x = (zi || zero[j]) ? 0.0 : ldrow[j];
  v = __ddiv_rn(__ddiv_rn(x, sdi), sd[j]);
  return fabs(v) >= thr;
}

#define LDS_WAVES 4      // rows per workgroup of the two sparse passes: one 64-lane wavefront per row

// Both passes walk row i over j in (i, M) in steps of 64 columns, lane l at column j0 + l (coalesced along the row); the kept
// entries of a step are ordered by the prefix popcount of the wavefront's ballot, the steps by a running base: no atomics, so the
// order is (i, j) row-major and the same from run to run.
// WRITE false: nrow[i] = kept entries of row i.  WRITE true: off[i] = exclusive scan of nrow; the triplets go to [off[i], off[i + 1]).
template <bool WRITE>
__global__ __launch_bounds__(64 * LDS_WAVES) void k_ld_sparse(const double* __restrict__ LD, int M, const uint8_t* __restrict__ zero, const double* __restrict__ sd,
                                                              double thr, long long* __restrict__ nrow, const long long* __restrict__ off,
                                                              int32_t* __restrict__ orow, int32_t* __restrict__ ocol, double* __restrict__ oval) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * LDS_WAVES + (threadIdx.x >> 6);      // (uniform over the wavefront)
  if (i >= M) return;
  const double* ldrow = LD + (int64_t)i * M;
  const bool zi = zero[i] != 0;
  const double sdi = sd[i];
  long long base = WRITE ? off[i] : 0;
  for (int j0 = i + 1; j0 < M; j0 += 64) {
    const int j = j0 + lane;
    double v = 0.0;
    const bool keep = j < M && ld_sparse_keep(ldrow, zi, sdi, zero, sd, j, thr, v);
    const unsigned long long mask = __ballot(keep);
    if (WRITE && keep) {
      const long long at = base + __popcll(mask & ((1ull << lane) - 1ull));
      orow[at] = i;
      ocol[at] = j;
      oval[at] = v;
    }
    base += __popcll(mask);
  }
  if (!WRITE && lane == 0) nrow[i] = base;
}

// off[0 .. M] = exclusive scan of nrow[0 .. M) (off[M] = the total).  One workgroup: thread t owns the chunk [t * per, (t + 1) * per).
__global__ __launch_bounds__(256) void k_ld_scan(const long long* __restrict__ nrow, int M, long long* __restrict__ off) {
  __shared__ long long part[256];
  const int t = threadIdx.x, per = (M + 255) / 256;
  const int lo = min(t * per, M), hi = min(lo + per, M);
  long long s = 0;
  for (int k = lo; k < hi; ++k) s += nrow[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int k = 0; k < 256; ++k) { const long long x = part[k]; part[k] = run; run += x; }
    off[M] = run;
  }
  __syncthreads();
  long long run = part[t];
  for (int k = lo; k < hi; ++k) { off[k] = run; run += nrow[k]; }
}

}  // namespace

enum { LD_EMPTY = 0, LD_CALLS, LD_INTS };

struct rg_ld_ctx {
  int dev = 0;
  int64_t n = 0, ld = 0;
  int C = 0, M = 0, nrows = 0;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint8_t* rows = nullptr;            // [M][ld] in the order appended
  int kind = LD_EMPTY;                // the store in use: no panel yet, 2-bit hard calls (rows), integer dosages (planes)
  int scale = 0, np = 0;              // integer dosages: units of 1 / scale, np digit planes
  int64_t kp = 0;                     // n rounded up to 64
  int8_t* planes = nullptr;           // [planes_np + 1][M][kp], allocated by the first rg_ld_append_int
  int planes_np = 0;                  // the plane count the store was sized for (np once a panel is held)
  rg_s2_ctx* s2 = nullptr;            // the contraction primitive (X^T g), created by rg_ld_set_basis
  std::vector<int32_t> col_of_row;    // [nrows]
  std::vector<uint8_t> col_state;     // [M] 0: open, 1: appended, 2: forced
  std::vector<double> mean, gx;       // [nrows], [nrows][C]
  std::vector<int32_t> nmiss;         // [nrows]
  int32_t* sp_row = nullptr;          // the triplets of the last rg_ld_finish_sparse: [sp_count] each, device memory
  int32_t* sp_col = nullptr;
  double* sp_val = nullptr;
  int64_t sp_count = -1;              // -1: no sparse result is held
  double last_ms = 0.0;
  int64_t last_tiles = 0;
  std::string err;
};

static int ld_fail(rg_ld_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}
#define LD_HIP(x)                                                                                                              \
  do {                                                                                                                         \
    hipError_t e_ = (x);                                                                                                       \
    if (e_ != hipSuccess) return ld_fail(ctx, RG_LD_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                   \
  } while (0)

namespace {
struct DevBuf {  // device memory of one call
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T> T* as() const { return (T*)p; }
};
}  // namespace

// The Gram kernel of the store the context holds (hard calls, two or three digit planes), on the context's stream.  The outputs are
// [na][nb] of the store's sum type (int32_t / long long).
static void ld_launch_gram(rg_ld_ctx* ctx, dim3 grid, int a0, int na, int b0, int nb, int tri, int kinds, const uint8_t* tile_miss, void* SA, void* SB, void* SBt,
                           void* SD) {
  if (ctx->kind == LD_CALLS) {
    hipLaunchKernelGGL(k_ld_gram, grid, dim3(256), 0, ctx->st, ctx->rows, ctx->ld, a0, na, b0, nb, tri, kinds, tile_miss, (int32_t*)SA, (int32_t*)SB, (int32_t*)SBt,
                       (int32_t*)SD, (int64_t)nb);
  } else {
    const auto k = ctx->np == 2 ? k_ld_gram_int<2> : k_ld_gram_int<3>;
    hipLaunchKernelGGL(k, grid, dim3(512), 0, ctx->st, ctx->planes, ctx->kp, (int64_t)ctx->M * ctx->kp, a0, na, b0, nb, tri, kinds, tile_miss, (long long*)SA,
                       (long long*)SB, (long long*)SBt, (long long*)SD, (int64_t)nb);
  }
}

// rg_ld_pair_sums / rg_ld_pair_sums_int after their argument checks; T: the sum type of the store
template <class T>
static int ld_pair_sums(rg_ld_ctx* ctx, int a0, int na, int b0, int nb, T* const (&outs)[4]) {
  LD_HIP(hipSetDevice(ctx->dev));
  const size_t cnt = (size_t)na * nb;
  DevBuf S;
  LD_HIP(S.alloc(4 * cnt * sizeof(T)));
  T* s = S.as<T>();
  const int nt = ((na + LT - 1) / LT) * ((nb + LT - 1) / LT);
  const int kinds = (outs[0] ? 1 : 0) | (outs[1] ? 2 : 0) | (outs[2] ? 4 : 0) | (outs[3] ? 8 : 0);
  LD_HIP(hipEventRecord(ctx->e0, ctx->st));
  ld_launch_gram(ctx, dim3(nt, 4), a0, na, b0, nb, 0, kinds, nullptr, s, s + cnt, s + 2 * cnt, s + 3 * cnt);
  LD_HIP(hipGetLastError());
  LD_HIP(hipEventRecord(ctx->e1, ctx->st));
  for (int k = 0; k < 4; ++k)
    if (outs[k]) LD_HIP(hipMemcpyAsync(outs[k], s + k * cnt, cnt * sizeof(T), hipMemcpyDeviceToHost, ctx->st));
  LD_HIP(hipStreamSynchronize(ctx->st));
  float ms = 0.f;
  LD_HIP(hipEventElapsedTime(&ms, ctx->e0, ctx->e1));
  ctx->last_ms = ms;
  ctx->last_tiles = (int64_t)nt * __builtin_popcount(kinds);
  return RG_LD_OK;
}

// What the two append entries check alike, after their own arguments: room for bs more rows, every column in range and open.
static int ld_append_check(rg_ld_ctx* ctx, const std::string& who, int32_t bs, const int32_t* cols) {
  if ((int64_t)ctx->nrows + bs > ctx->M) return ld_fail(ctx, RG_LD_ERR_ARG, who + ": more rows than the " + std::to_string(ctx->M) + " columns of the matrix");
  std::vector<uint8_t> seen(ctx->col_state);
  for (int j = 0; j < bs; ++j) {
    if (cols[j] < 0 || cols[j] >= ctx->M) return ld_fail(ctx, RG_LD_ERR_ARG, who + ": column index out of range");
    if (seen[cols[j]]) return ld_fail(ctx, RG_LD_ERR_ARG, who + ": column " + std::to_string(cols[j]) + " is used twice");
    seen[cols[j]] = 1;
  }
  return RG_LD_OK;
}

// The bs rows just stored become rows of the matrix.  Without a basis (rg_ld_set_basis) obs and sums are empty; otherwise obs [bs][2]:
// per row the sum (genotype units) and the number of its observed entries; sums [bs][2][C]: X^T g0 and X^T miss in genotype units.
static void ld_append_commit(rg_ld_ctx* ctx, int32_t bs, const int32_t* cols, const std::vector<double>& obs, const std::vector<double>& sums) {
  const int r0 = ctx->nrows, C = ctx->C;
  ctx->mean.resize((size_t)r0 + bs, 0.0);
  ctx->nmiss.resize((size_t)r0 + bs, 0);
  ctx->gx.resize(((size_t)r0 + bs) * C, 0.0);
  for (int j = 0; j < bs && !obs.empty(); ++j) {
    const double nobs = obs[2 * j + 1], m = nobs > 0 ? obs[2 * j] / nobs : 0.0;
    ctx->mean[r0 + j] = m;
    ctx->nmiss[r0 + j] = (int32_t)(ctx->n - (int64_t)nobs);
    for (int c = 0; c < C; ++c) ctx->gx[(size_t)(r0 + j) * C + c] = sums[((size_t)j * 2) * C + c] + m * sums[((size_t)j * 2 + 1) * C + c];
  }
  for (int j = 0; j < bs; ++j) { ctx->col_of_row.push_back(cols[j]); ctx->col_state[cols[j]] = 1; }
  ctx->nrows += bs;
}

// the triplets rg_ld_finish_sparse left in device memory
static void ld_sparse_release(rg_ld_ctx* ctx) {
  (void)hipSetDevice(ctx->dev);
  if (ctx->sp_row) (void)hipFree(ctx->sp_row);
  if (ctx->sp_col) (void)hipFree(ctx->sp_col);
  if (ctx->sp_val) (void)hipFree(ctx->sp_val);
  ctx->sp_row = ctx->sp_col = nullptr;
  ctx->sp_val = nullptr;
  ctx->sp_count = -1;
}

extern "C" {

int rg_ld_create(rg_ld_ctx** out, int device, int64_t n, int32_t n_cov, int32_t n_col) {
  if (!out) return RG_LD_ERR_ARG;
  rg_ld_ctx* ctx = new rg_ld_ctx();
  *out = ctx;
  if (n < 1 || n >= ((int64_t)1 << 29)) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_create: need 1 <= n < 2^29 samples (int32 sums)");
  if (n_col < 1 || n_col > (1 << 19)) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_create: need 1 <= M <= 2^19 columns");
  if (n_cov < 1 || n_cov > RG_S2_MAX_COV) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_create: need 1 <= n_cov <= 64");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ld_fail(ctx, RG_LD_ERR_HIP, "rg_ld_create: no HIP device (this library has no CPU path)");
  if (device < 0 || device >= ndev) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_create: device index out of range");
  ctx->dev = device; ctx->n = n; ctx->C = n_cov; ctx->M = n_col;
  ctx->ld = (n + 63) / 64 * 16;
  ctx->kp = (n + 63) / 64 * 64;
  LD_HIP(hipSetDevice(device));
  LD_HIP(hipStreamCreateWithFlags(&ctx->st, hipStreamNonBlocking));
  LD_HIP(hipEventCreate(&ctx->e0));
  LD_HIP(hipEventCreate(&ctx->e1));
  LD_HIP(hipMalloc((void**)&ctx->rows, (size_t)n_col * ctx->ld));
  ctx->col_state.assign(n_col, 0);
  return RG_LD_OK;
}

void rg_ld_destroy(rg_ld_ctx* ctx) {
  if (!ctx) return;
  if (ctx->st) {
    (void)hipSetDevice(ctx->dev);
    (void)hipStreamSynchronize(ctx->st);
    if (ctx->s2) rg_s2_destroy(ctx->s2);
    if (ctx->rows) (void)hipFree(ctx->rows);
    if (ctx->planes) (void)hipFree(ctx->planes);
    ld_sparse_release(ctx);
    if (ctx->e0) (void)hipEventDestroy(ctx->e0);
    if (ctx->e1) (void)hipEventDestroy(ctx->e1);
    (void)hipStreamDestroy(ctx->st);
  }
  delete ctx;
}

const char* rg_ld_last_error(const rg_ld_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
double rg_ld_last_kernel_ms(const rg_ld_ctx* ctx) { return ctx ? ctx->last_ms : 0.0; }
int64_t rg_ld_last_tiles(const rg_ld_ctx* ctx) { return ctx ? ctx->last_tiles : 0; }

int rg_ld_set_basis(rg_ld_ctx* ctx, const double* X) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_set_basis: context was not created");
  if (!X) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_set_basis: null argument");
  if (ctx->nrows > 0) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_set_basis: the basis must be set before the first panel is appended");
  if (ctx->n <= ctx->C) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_set_basis: need n > n_cov");
  if (!ctx->s2) {
    if (rg_s2_create(&ctx->s2, ctx->dev, ctx->n, ctx->C, 1) != RG_S2_OK) {
      const std::string m = std::string("rg_ld_set_basis: ") + rg_s2_last_error(ctx->s2);
      rg_s2_destroy(ctx->s2);
      ctx->s2 = nullptr;
      return ld_fail(ctx, RG_LD_ERR_HIP, m);
    }
  }
  if (rg_s2_set_columns(ctx->s2, ctx->C, X, 0) != RG_S2_OK) return ld_fail(ctx, RG_LD_ERR_HIP, std::string("rg_ld_set_basis: ") + rg_s2_last_error(ctx->s2));
  return RG_LD_OK;
}

int rg_ld_force_columns(rg_ld_ctx* ctx, int32_t k, const int32_t* cols) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_force_columns: context was not created");
  if (k < 0 || (k > 0 && !cols)) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_force_columns: bad arguments");
  for (int t = 0; t < k; ++t) {
    if (cols[t] < 0 || cols[t] >= ctx->M) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_force_columns: column index out of range");
    if (ctx->col_state[cols[t]] == 1) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_force_columns: column " + std::to_string(cols[t]) + " holds a variant already");
  }
  for (int t = 0; t < k; ++t) ctx->col_state[cols[t]] = 2;
  return RG_LD_OK;
}

int rg_ld_append(rg_ld_ctx* ctx, const uint8_t* rows, int64_t ld, int32_t bs, int32_t rows_on_device, int32_t flip, const int32_t* cols) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append: context was not created");
  const int64_t n = ctx->n, nbytes = (n + 3) / 4;
  if (!rows || !cols || bs < 1 || ld < nbytes) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append: bad arguments (need bs >= 1, ld >= ceil(n / 4))");
  if (ctx->kind == LD_INTS) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append: the matrix holds integer-dosage panels (rg_ld_append_int); the two kinds cannot be mixed");
  if (int rc = ld_append_check(ctx, "rg_ld_append", bs, cols)) return rc;
  LD_HIP(hipSetDevice(ctx->dev));
  uint8_t* dst = ctx->rows + (int64_t)ctx->nrows * ctx->ld;
  LD_HIP(hipMemcpy2DAsync(dst, ctx->ld, rows, ld, nbytes, bs, rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->st));
  hipLaunchKernelGGL(k_ld_store, dim3(bs), dim3(256), 0, ctx->st, dst, ctx->ld, n, flip ? 1 : 0);
  LD_HIP(hipGetLastError());
  LD_HIP(hipStreamSynchronize(ctx->st));
  std::vector<double> obs, sums;
  if (ctx->s2) {  // X^T g0, X^T miss and the call counts of the stored rows (the allele is already the one counted)
    obs.resize((size_t)bs * 2);
    sums.resize((size_t)bs * 2 * ctx->C);
    std::vector<int32_t> counts((size_t)bs * 4);
    rg_s2_contract_out co = {sums.data(), nullptr, counts.data(), nullptr};
    if (rg_s2_contract_packed(ctx->s2, dst, ctx->ld, bs, 1, 0, &co) != RG_S2_OK)
      return ld_fail(ctx, RG_LD_ERR_HIP, std::string("rg_ld_append: ") + rg_s2_last_error(ctx->s2));
    for (int j = 0; j < bs; ++j) {
      const int32_t* c4 = counts.data() + (size_t)j * 4;
      obs[2 * j] = (double)((int64_t)c4[0] + 2 * (int64_t)c4[1]);
      obs[2 * j + 1] = (double)(n - c4[2]);
    }
  }
  ld_append_commit(ctx, bs, cols, obs, sums);
  ctx->kind = LD_CALLS;
  return RG_LD_OK;
}

int rg_ld_append_int(rg_ld_ctx* ctx, const uint16_t* G, int64_t ld, int32_t bs, int32_t g_on_device, int32_t scale, const int32_t* cols) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append_int: context was not created");
  const int64_t n = ctx->n;
  if (!G || !cols || bs < 1 || ld < n) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append_int: bad arguments (need bs >= 1, ld >= n)");
  if (scale < 1 || scale > 16384) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append_int: need 1 <= scale <= 16384");
  if (ctx->kind == LD_CALLS) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append_int: the matrix holds 2-bit panels (rg_ld_append); the two kinds cannot be mixed");
  if (ctx->kind == LD_INTS && scale != ctx->scale)
    return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append_int: the matrix holds panels of scale " + std::to_string(ctx->scale) + "; one matrix has one scale");
  if (int rc = ld_append_check(ctx, "rg_ld_append_int", bs, cols)) return rc;
  LD_HIP(hipSetDevice(ctx->dev));
  const int np = 2 * scale <= 8127 ? 2 : 3;      // the rule of rg_s2_qt_block_int: two balanced base-128 digits reach 63 + 63 * 128
  const int64_t kp = ctx->kp, ps = (int64_t)ctx->M * kp;
  if (ctx->planes && ctx->planes_np != np) {      // left by a first append that failed at a scale with another plane count
    LD_HIP(hipFree(ctx->planes));
    ctx->planes = nullptr;
  }
  if (!ctx->planes) {      // M * kp * (np + 1) bytes; a matrix that does not fit is an error, there is no second route
    const size_t need = (size_t)ps * (np + 1);
    size_t free_b = 0, total_b = 0;
    LD_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
      return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append_int: the digit planes of the matrix need " + std::to_string(need) + " bytes (M * n * " + std::to_string(np + 1) +
                                             "), the device has " + std::to_string(free_b) + " free");
    LD_HIP(hipMalloc((void**)&ctx->planes, need));
    ctx->planes_np = np;
  }
  DevBuf dG, dBad;
  const uint16_t* src = G;
  int64_t lds = ld;
  if (!g_on_device) {
    lds = (n + 7) / 8 * 8;
    LD_HIP(dG.alloc((size_t)bs * lds * sizeof(uint16_t)));
    LD_HIP(hipMemcpy2DAsync(dG.p, lds * sizeof(uint16_t), G, ld * sizeof(uint16_t), n * sizeof(uint16_t), bs, hipMemcpyHostToDevice, ctx->st));
    src = dG.as<uint16_t>();
  }
  LD_HIP(dBad.alloc(sizeof(int32_t)));
  LD_HIP(hipMemsetAsync(dBad.p, 0, sizeof(int32_t), ctx->st));
  hipLaunchKernelGGL(k_ld_store_int, dim3(bs), dim3(256), 0, ctx->st, src, lds, n, kp, np, (unsigned)(2 * scale), ctx->planes + (int64_t)ctx->nrows * kp, ps,
                     dBad.as<int32_t>());
  LD_HIP(hipGetLastError());
  int32_t bad = 0;
  LD_HIP(hipMemcpyAsync(&bad, dBad.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
  LD_HIP(hipStreamSynchronize(ctx->st));
  if (bad) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_append_int: a dosage is above 2 * scale = " + std::to_string(2 * scale) + " (0xFFFF is the missing value)");
  std::vector<double> obs, sums;
  if (ctx->s2) {  // X^T g0 and X^T miss in genotype units, the sum and the number of the observed entries
    obs.resize((size_t)bs * 2);
    sums.resize((size_t)bs * 2 * ctx->C);
    std::vector<double> vstat((size_t)bs * 4);
    rg_s2_contract_out co = {sums.data(), nullptr, nullptr, vstat.data()};
    if (rg_s2_contract_int(ctx->s2, src, lds, bs, 1, scale, &co) != RG_S2_OK)
      return ld_fail(ctx, RG_LD_ERR_HIP, std::string("rg_ld_append_int: ") + rg_s2_last_error(ctx->s2));
    for (int j = 0; j < bs; ++j) { obs[2 * j] = vstat[(size_t)j * 4] / (double)scale; obs[2 * j + 1] = vstat[(size_t)j * 4 + 2]; }
  }
  ld_append_commit(ctx, bs, cols, obs, sums);
  ctx->kind = LD_INTS; ctx->scale = scale; ctx->np = np;
  return RG_LD_OK;
}

int rg_ld_pair_sums_int(rg_ld_ctx* ctx, int32_t a0, int32_t na, int32_t b0, int32_t nb, int64_t* A, int64_t* B, int64_t* Bt, int64_t* D) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_pair_sums_int: context was not created");
  if (ctx->kind != LD_INTS) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_pair_sums_int: the matrix holds no integer-dosage panel");
  if (a0 < 0 || b0 < 0 || na < 1 || nb < 1 || (int64_t)a0 + na > ctx->nrows || (int64_t)b0 + nb > ctx->nrows)
    return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_pair_sums_int: row range outside the panels appended");
  return ld_pair_sums<int64_t>(ctx, a0, na, b0, nb, {A, B, Bt, D});
}

int rg_ld_pair_sums(rg_ld_ctx* ctx, int32_t a0, int32_t na, int32_t b0, int32_t nb, int32_t* A, int32_t* B, int32_t* Bt, int32_t* D) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_pair_sums: context was not created");
  if (a0 < 0 || b0 < 0 || na < 1 || nb < 1 || (int64_t)a0 + na > ctx->nrows || (int64_t)b0 + nb > ctx->nrows)
    return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_pair_sums: row range outside the panels appended");
  if (ctx->kind == LD_INTS) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_pair_sums: the matrix holds integer-dosage panels (rg_ld_pair_sums_int)");
  return ld_pair_sums<int32_t>(ctx, a0, na, b0, nb, {A, B, Bt, D});
}

}  // extern "C"

// What rg_ld_finish and rg_ld_finish_sparse share: the checks of the context, then LD [M][M] (both triangles, forced columns zero) into
// dLD on the context's stream -- the Gram of the panels and the fp64 combination; not synchronised.  started: the Gram kernel ran.
struct LdBuildTmp {      // what the stream reads until the caller synchronises it
  DevBuf SA, SB, SD, Tm, Mean, Gx, Col;
  std::vector<uint8_t> tile_miss;
};

static int ld_build(rg_ld_ctx* ctx, const std::string& who, DevBuf& dLD, LdBuildTmp& tmp, bool& started) {
  started = false;
  if (!ctx->s2) return ld_fail(ctx, RG_LD_ERR_ARG, who + ": rg_ld_set_basis has not been called");
  const int M = ctx->M, R = ctx->nrows, C = ctx->C;
  for (int c = 0; c < M; ++c)
    if (!ctx->col_state[c]) return ld_fail(ctx, RG_LD_ERR_ARG, who + ": column " + std::to_string(c) + " was neither appended nor forced");
  LD_HIP(hipSetDevice(ctx->dev));
  const int nt = (R + LT - 1) / LT;
  std::vector<uint8_t>& tile_miss = tmp.tile_miss;
  tile_miss.assign(std::max(1, nt), 0);
  bool any_miss = false;
  for (int r = 0; r < R; ++r) if (ctx->nmiss[r] > 0) { tile_miss[r / LT] = 1; any_miss = true; }
  DevBuf &dSA = tmp.SA, &dSB = tmp.SB, &dSD = tmp.SD, &dTm = tmp.Tm, &dMean = tmp.Mean, &dGx = tmp.Gx, &dCol = tmp.Col;
  const size_t MM = (size_t)M * M, RR = (size_t)R * R;
  LD_HIP(dLD.alloc(MM * sizeof(double)));
  LD_HIP(hipMemsetAsync(dLD.p, 0, MM * sizeof(double), ctx->st));
  ctx->last_ms = 0.0;
  ctx->last_tiles = 0;
  const size_t ssz = ctx->kind == LD_INTS ? sizeof(long long) : sizeof(int32_t);      // the sums of the store
  if (R > 0) {
    LD_HIP(dSA.alloc(RR * ssz));
    if (any_miss) {
      LD_HIP(dSB.alloc(RR * ssz));
      LD_HIP(dSD.alloc(RR * ssz));
      LD_HIP(hipMemsetAsync(dSB.p, 0, RR * ssz, ctx->st));
      LD_HIP(hipMemsetAsync(dSD.p, 0, RR * ssz, ctx->st));
    }
    LD_HIP(dTm.alloc(tile_miss.size()));
    LD_HIP(dMean.alloc(sizeof(double) * R));
    LD_HIP(dGx.alloc(sizeof(double) * R * C));
    LD_HIP(dCol.alloc(sizeof(int32_t) * R));
    LD_HIP(hipMemcpyAsync(dTm.p, tile_miss.data(), tile_miss.size(), hipMemcpyHostToDevice, ctx->st));
    LD_HIP(hipMemcpyAsync(dMean.p, ctx->mean.data(), sizeof(double) * R, hipMemcpyHostToDevice, ctx->st));
    LD_HIP(hipMemcpyAsync(dGx.p, ctx->gx.data(), sizeof(double) * R * C, hipMemcpyHostToDevice, ctx->st));
    LD_HIP(hipMemcpyAsync(dCol.p, ctx->col_of_row.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, ctx->st));
    const int npair = nt * (nt + 1) / 2;
    LD_HIP(hipEventRecord(ctx->e0, ctx->st));
    ld_launch_gram(ctx, dim3(npair, any_miss ? 4 : 1), 0, R, 0, R, 1, 0xF, dTm.as<uint8_t>(), dSA.p, dSB.p, nullptr, dSD.p);
    LD_HIP(hipGetLastError());
    LD_HIP(hipEventRecord(ctx->e1, ctx->st));
    int64_t tiles = npair;
    if (any_miss)
      for (int a = 0; a < nt; ++a)
        for (int b = a; b < nt; ++b) tiles += (tile_miss[b] ? 1 : 0) + ((a != b && tile_miss[a]) ? 1 : 0) + ((tile_miss[a] && tile_miss[b]) ? 1 : 0);
    ctx->last_tiles = tiles;
    const dim3 g2((R + 15) / 16, (R + 15) / 16);
    if (ctx->kind == LD_CALLS)      // (dSB, dSD are null without a missing call)
      hipLaunchKernelGGL(k_ld_combine<int32_t>, g2, dim3(256), 0, ctx->st, dSA.as<int32_t>(), dSB.as<int32_t>(), dSD.as<int32_t>(), R, 1.0, dMean.as<double>(),
                         dGx.as<double>(), C, dCol.as<int32_t>(), dLD.as<double>(), M);
    else
      hipLaunchKernelGGL(k_ld_combine<long long>, g2, dim3(256), 0, ctx->st, dSA.as<long long>(), dSB.as<long long>(), dSD.as<long long>(), R, (double)ctx->scale,
                         dMean.as<double>(), dGx.as<double>(), C, dCol.as<int32_t>(), dLD.as<double>(), M);
    LD_HIP(hipGetLastError());
    started = true;
  }
  return RG_LD_OK;
}

// after the stream of ld_build has been synchronised
static int ld_build_time(rg_ld_ctx* ctx, bool started) {
  if (started) {
    float ms = 0.f;
    LD_HIP(hipEventElapsedTime(&ms, ctx->e0, ctx->e1));
    ctx->last_ms = ms;
  }
  return RG_LD_OK;
}

extern "C" {

int rg_ld_finish(rg_ld_ctx* ctx, int32_t form, void* out, int32_t out_on_device, double tol, double numtol) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_finish: context was not created");
  if (!out || (form != RG_LD_R2_U16 && form != RG_LD_CORR_F64 && form != RG_LD_COV_F64 && form != RG_LD_GTG_F64) || !(numtol > 0) || !(tol >= 0))
    return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_finish: bad arguments");
  const int M = ctx->M;
  const size_t MM = (size_t)M * M;
  DevBuf dLD, dZero, dInv, dDiag, dOut;
  LdBuildTmp tmp;
  bool started = false;
  if (int rc = ld_build(ctx, "rg_ld_finish", dLD, tmp, started)) return rc;
  const dim3 gM((M + 15) / 16, (M + 15) / 16);
  const size_t out_bytes = form == RG_LD_R2_U16 ? (size_t)M * (M - 1) / 2 * sizeof(uint16_t) : MM * sizeof(double);
  void* dres = nullptr;
  if (form == RG_LD_COV_F64) dres = dLD.p;
  else {
    LD_HIP(dZero.alloc(M));
    LD_HIP(dInv.alloc(sizeof(double) * M));
    if (form == RG_LD_GTG_F64) {
      LD_HIP(dDiag.alloc(sizeof(double) * M));
      hipLaunchKernelGGL(k_ld_diag_gtg, dim3((M + 255) / 256), dim3(256), 0, ctx->st, dLD.as<double>(), M, tol, numtol, dZero.as<uint8_t>(), dDiag.as<double>(),
                         dInv.as<double>());
    } else {
      hipLaunchKernelGGL(k_ld_diag, dim3((M + 255) / 256), dim3(256), 0, ctx->st, dLD.as<double>(), M, tol, numtol, dZero.as<uint8_t>(), dInv.as<double>());
    }
    LD_HIP(hipGetLastError());
    if (out_on_device) dres = out;
    else { LD_HIP(dOut.alloc(out_bytes)); dres = dOut.p; }
    if (form == RG_LD_CORR_F64) hipLaunchKernelGGL(k_ld_corr, gM, dim3(256), 0, ctx->st, dLD.as<double>(), M, dZero.as<uint8_t>(), dInv.as<double>(), (double*)dres);
    else if (form == RG_LD_GTG_F64) hipLaunchKernelGGL(k_ld_gtg, gM, dim3(256), 0, ctx->st, dLD.as<double>(), M, dZero.as<uint8_t>(), dDiag.as<double>(), (double*)dres);
    else if (M > 1) hipLaunchKernelGGL(k_ld_r2, gM, dim3(256), 0, ctx->st, dLD.as<double>(), M, dZero.as<uint8_t>(), dInv.as<double>(), (uint16_t*)dres);
    LD_HIP(hipGetLastError());
  }
  if (dres != out && out_bytes > 0) LD_HIP(hipMemcpyAsync(out, dres, out_bytes, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->st));
  LD_HIP(hipStreamSynchronize(ctx->st));
  return ld_build_time(ctx, started);
}

int rg_ld_finish_sparse(rg_ld_ctx* ctx, double thr, double tol, double numtol, double* sd, int64_t* count) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_finish_sparse: context was not created");
  if (!sd || !count || !(numtol > 0) || !(tol >= 0)) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_finish_sparse: bad arguments");
  if (!(thr > 0 && thr < 1)) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_finish_sparse: the threshold must lie in (0, 1)");
  ld_sparse_release(ctx);
  const int M = ctx->M;
  DevBuf dLD, dZero, dSd, dDiag, dNrow, dOff;
  long long total = 0;
  {
    LdBuildTmp tmp;      // the integer sums are freed before the triplets are allocated
    bool started = false;
    if (int rc = ld_build(ctx, "rg_ld_finish_sparse", dLD, tmp, started)) return rc;
    LD_HIP(dZero.alloc(M));
    LD_HIP(dSd.alloc(sizeof(double) * M));
    LD_HIP(dDiag.alloc(sizeof(double) * M));
    LD_HIP(dNrow.alloc(sizeof(long long) * M));
    LD_HIP(dOff.alloc(sizeof(long long) * ((size_t)M + 1)));
    hipLaunchKernelGGL(k_ld_diag_gtg, dim3((M + 255) / 256), dim3(256), 0, ctx->st, dLD.as<double>(), M, tol, numtol, dZero.as<uint8_t>(), dDiag.as<double>(),
                       dSd.as<double>());
    LD_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ld_sparse<false>, dim3((M + LDS_WAVES - 1) / LDS_WAVES), dim3(64 * LDS_WAVES), 0, ctx->st, dLD.as<double>(), M, dZero.as<uint8_t>(),
                       dSd.as<double>(), thr, dNrow.as<long long>(), nullptr, nullptr, nullptr, nullptr);
    LD_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ld_scan, dim3(1), dim3(256), 0, ctx->st, dNrow.as<long long>(), M, dOff.as<long long>());
    LD_HIP(hipGetLastError());
    LD_HIP(hipMemcpyAsync(&total, dOff.as<long long>() + M, sizeof(long long), hipMemcpyDeviceToHost, ctx->st));
    LD_HIP(hipMemcpyAsync(sd, dSd.p, sizeof(double) * M, hipMemcpyDeviceToHost, ctx->st));
    LD_HIP(hipStreamSynchronize(ctx->st));
    if (int rc = ld_build_time(ctx, started)) return rc;
  }
  if (total > 0) {
    const size_t need = (size_t)total * (2 * sizeof(int32_t) + sizeof(double));
    size_t free_b = 0, total_b = 0;
    LD_HIP(hipMemGetInfo(&free_b, &total_b));
    const bool fits = need <= free_b && hipMalloc((void**)&ctx->sp_row, (size_t)total * sizeof(int32_t)) == hipSuccess &&
                      hipMalloc((void**)&ctx->sp_col, (size_t)total * sizeof(int32_t)) == hipSuccess &&
                      hipMalloc((void**)&ctx->sp_val, (size_t)total * sizeof(double)) == hipSuccess;
    if (!fits) {
      (void)hipGetLastError();
      ld_sparse_release(ctx);
      return ld_fail(ctx, RG_LD_ERR_HIP, "rg_ld_finish_sparse: the " + std::to_string(total) + " entries at or above the threshold need " + std::to_string(need) +
                                             " bytes of device memory, the device has " + std::to_string(free_b) + " free: raise the threshold");
    }
    hipLaunchKernelGGL(k_ld_sparse<true>, dim3((M + LDS_WAVES - 1) / LDS_WAVES), dim3(64 * LDS_WAVES), 0, ctx->st, dLD.as<double>(), M, dZero.as<uint8_t>(),
                       dSd.as<double>(), thr, nullptr, dOff.as<long long>(), ctx->sp_row, ctx->sp_col, ctx->sp_val);
    LD_HIP(hipGetLastError());
    LD_HIP(hipStreamSynchronize(ctx->st));
  }
  ctx->sp_count = total;
  *count = total;
  return RG_LD_OK;
}

int rg_ld_sparse_fetch(rg_ld_ctx* ctx, int32_t* row, int32_t* col, double* val) {
  if (!ctx || !ctx->rows) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_sparse_fetch: context was not created");
  if (ctx->sp_count < 0) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_sparse_fetch: no sparse result is held (rg_ld_finish_sparse)");
  if (ctx->sp_count == 0) return RG_LD_OK;
  if (!row || !col || !val) return ld_fail(ctx, RG_LD_ERR_ARG, "rg_ld_sparse_fetch: null argument");
  LD_HIP(hipSetDevice(ctx->dev));
  LD_HIP(hipMemcpyAsync(row, ctx->sp_row, (size_t)ctx->sp_count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
  LD_HIP(hipMemcpyAsync(col, ctx->sp_col, (size_t)ctx->sp_count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
  LD_HIP(hipMemcpyAsync(val, ctx->sp_val, (size_t)ctx->sp_count * sizeof(double), hipMemcpyDeviceToHost, ctx->st));
  LD_HIP(hipStreamSynchronize(ctx->st));
  return RG_LD_OK;
}

}  // extern "C"
