/* rg_ld.h -- C ABI of the Step-2 LD matrix of a region (`regenie --step 2 --compute-corr`, hard calls or dosages).
 *
 * What it replaces in the reference: Data::print_ld (Data.cpp:4368-4449) and the sparse matrix get_G_svs fills for it
 * (Data.cpp:4227-4304): for M variants and n analysed samples
 *     LD = G^T G - (G^T X)(G^T X)^T        G [n][M] hard calls, every variant mean-imputed (mean_impute_g, Data.cpp:4278-4279),
 *                                          X [n][C] the orthonormal covariate basis (new_cov, intercept included)
 * then the reference's treatment of the diagonal and the scaling to correlations (Data.cpp:4386-4397), and the 16-bit R^2
 * quantisation of the binary file (Data.cpp:4431-4436); or, for --skip-scaleG, the unscaled matrix after the diagonal rules
 * (Data.cpp:4400) and its sparse form under --sparse-thr (Data.cpp:4407-4421), thresholded on the device.
 *
 * How: with g0 = the call with 0 at a missing entry, miss = its indicator and m_j the mean of the observed calls of variant j,
 *     sum_s g_i g_j = A_ij + m_j B_ij + m_i B_ji + m_i m_j D_ij,    A = g0 g0^T,  B_ij = sum_s g0_i miss_j,  D = miss miss^T
 * A, B, D are integers, computed exactly on the i8 matrix cores from the 2-bit rows (int32 sums: n < 2^29); B and D only for tile
 * pairs in which a tile has a missing call.  X^T g comes from the contraction primitive of rg_step2.h (exact digit planes).  The
 * combination, the subtraction, the scaling and the quantisation are fp64 on the vector units (csrc/ld_corr.hip).
 *
 * Layout: rows are 2-bit hard calls in .bed coding, sample-fastest, 4 per byte, low bits first (00 -> 2, 01 -> missing, 10 -> 1,
 * 11 -> 0 copies of the counted allele), as rg_s2_qt_block_packed takes them; flip != 0 counts the other allele.
 * Dosages (the reference's Data::compute_ld_dosages, Data.cpp:3887-3980): rows of integers in units of 1 / scale (rg_ld_append_int).
 * The same decomposition with g0 the integer dosage; A, B, D are exact: each row is split once into balanced base-128 int8 digit
 * planes and a missing plane, A = sum_{p,q} 128^(p+q) P_p P_q^T on the i8 matrix cores, the int32 accumulators flushed into int64
 * sums every 131,072 samples (a digit product reaches 4,096 and three plane pairs share an accumulator), so every n < 2^29 is exact.
 * The fp64 epilogue divides A by scale^2 and B by scale; 8 M^2 bytes per integer sum instead of 4.
 * Conventions: 0 on success, < 0 on error with rg_ld_last_error(ctx); the library never falls back to the CPU.
 */
#ifndef RG_LD_H
#define RG_LD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rg_ld_ctx rg_ld_ctx;

#define RG_LD_OK 0
#define RG_LD_ERR_ARG (-1)
#define RG_LD_ERR_HIP (-2)

/* the four forms rg_ld_finish returns */
#define RG_LD_R2_U16 0   /* uint16 [M (M - 1) / 2]: r * r * 65535 + 0.5 truncated, row-major over i < j (the binary .corr body) */
#define RG_LD_CORR_F64 1 /* double [M][M]: the correlation matrix (the text .corr)                                             */
#define RG_LD_COV_F64 2  /* double [M][M]: LD before the diagonal is looked at and before scaling                               */
#define RG_LD_GTG_F64 3  /* double [M][M]: LD unscaled after the two diagonal rules (--skip-scaleG: Data.cpp:4118 / :4400)          */

/* n analysed samples (1 <= n < 2^29), C covariate basis columns (intercept included; 1 <= C <= 64), M columns of the matrix
 * (1 <= M <= 2^19; the M x M results and sums must fit the device: 8 M^2 bytes for LD, 4 M^2 per integer sum).  The packed rows
 * of the M variants stay in device memory: M * 16 * ceil(n / 64) bytes. */
int rg_ld_create(rg_ld_ctx** out, int device, int64_t n, int32_t n_cov, int32_t n_col);
void rg_ld_destroy(rg_ld_ctx* ctx);
const char* rg_ld_last_error(const rg_ld_ctx* ctx);

/* X [C][n], orthonormal, sample-fastest (host pointer).  Needs n > C.  Before the first rg_ld_append that rg_ld_finish is to see. */
int rg_ld_set_basis(rg_ld_ctx* ctx, const double* X);

/* Columns that no variant fills (IDs forced into the matrix that the genotype file does not have): zero vectors, correlation 0
 * with everything, diagonal 1.  cols: host, [k]. */
int rg_ld_force_columns(rg_ld_ctx* ctx, int32_t k, const int32_t* cols);

/* A panel of bs variants; row j (ld >= ceil(n / 4) bytes apart; host pointer, or device when rows_on_device) takes column cols[j]
 * (host, [bs]) of the matrix.  A column can be given once. */
int rg_ld_append(rg_ld_ctx* ctx, const uint8_t* rows, int64_t ld, int32_t bs, int32_t rows_on_device, int32_t flip, const int32_t* cols);

/* A panel of bs variants as integer dosages: G [bs][ld >= n] uint16 in units of 1 / scale, 0xFFFF = missing, every other value
 * <= 2 * scale, 1 <= scale <= 16384 (8-bit .bgen probabilities: scale 255; .pgen dosages: scale 16384); host pointer, or device when
 * g_on_device.  A matrix holds either 2-bit panels or integer-dosage panels of one scale: anything else is RG_LD_ERR_ARG.  On append
 * a row is split into balanced base-128 int8 digit planes (two when 2 * scale <= 8127, else three) and a 0/1 missing plane, which
 * stay in device memory: M * 64 * ceil(n / 64) * (planes + 1) bytes, allocated by the first call; a matrix that does not fit the
 * device is RG_LD_ERR_ARG (the bound covers the planes alone: the transient buffers of an append and the 8 M^2-byte sums and result of
 * rg_ld_finish come on top, and running out of memory there is RG_LD_ERR_HIP).  A first call that fails after the allocation keeps
 * it; a later call at a scale with another plane count replaces it. */
int rg_ld_append_int(rg_ld_ctx* ctx, const uint16_t* G, int64_t ld, int32_t bs, int32_t g_on_device, int32_t scale, const int32_t* cols);

/* The result in one of the four forms; out is a host pointer, or a device pointer when out_on_device (the quantisation runs on the
 * device either way: M (M - 1) bytes leave it, not 8 M^2).  tol: a diagonal entry in (-tol, 0) zeroes its row and column
 * (params.tol = 1e-8); numtol: a non-positive diagonal entry becomes numtol (params.numtol = 1e-6) -- Data.cpp:4386-4397.
 * RG_LD_GTG_F64 keeps the zeroing rule and then sets diag = max(diag, numtol); nothing is scaled.
 * Every column must have been appended or forced. */
int rg_ld_finish(rg_ld_ctx* ctx, int32_t form, void* out, int32_t out_on_device, double tol, double numtol);

/* The sparse form of the unscaled matrix (--skip-scaleG --sparse-thr, Data.cpp:4407-4421): sd [M] (host) = sqrt of the diagonal of
 * RG_LD_GTG_F64, and the entries v = LD[i][j] / sd[i] / sd[j] over i < j (LD after the zeroing rule, the two divisions as written)
 * with fabs(v) >= thr, in row-major order of (i, j); *count is their number.  The M x M matrix is thresholded where it lies: the
 * triplets stay in device memory, owned by the context, until the next rg_ld_finish_sparse or rg_ld_destroy, and
 * rg_ld_sparse_fetch copies them out.  Count and order are the same from run to run.  thr must lie in (0, 1): anything else is
 * RG_LD_ERR_ARG; a triplet buffer (16 bytes per entry) that does not fit the device is RG_LD_ERR_HIP, and the message names the count. */
int rg_ld_finish_sparse(rg_ld_ctx* ctx, double thr, double tol, double numtol, double* sd, int64_t* count);

/* The triplets of the last rg_ld_finish_sparse: row, col (0-based, row < col) and val, each [count] on the host. */
int rg_ld_sparse_fetch(rg_ld_ctx* ctx, int32_t* row, int32_t* col, double* val);

/* Test entry: the raw integer sums of one panel pair, rows [a0, a0 + na) against rows [b0, b0 + nb) in the order they were
 * appended (no basis needed): A[i][j] = sum g0_i g0_j, B[i][j] = sum g0_i miss_j, Bt[i][j] = sum miss_i g0_j, D[i][j] = sum miss_i miss_j,
 * each int32 [na][nb] on the host; a NULL pointer skips that sum. */
int rg_ld_pair_sums(rg_ld_ctx* ctx, int32_t a0, int32_t na, int32_t b0, int32_t nb, int32_t* A, int32_t* B, int32_t* Bt, int32_t* D);

/* The same for integer-dosage panels, g0 in integer units (A in units of 1 / scale^2, B and Bt of 1 / scale): int64 [na][nb]. */
int rg_ld_pair_sums_int(rg_ld_ctx* ctx, int32_t a0, int32_t na, int32_t b0, int32_t nb, int64_t* A, int64_t* B, int64_t* Bt, int64_t* D);

/* Device time of the panel-pair Gram kernel of the last rg_ld_finish / rg_ld_pair_sums, in ms, and the tiles it computed. */
double rg_ld_last_kernel_ms(const rg_ld_ctx* ctx);
int64_t rg_ld_last_tiles(const rg_ld_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
