// regenie-amd: C++ host driver for `--step 1` / `--step 2` on MI355X: declarations shared by its translation units.
//
// Keeps the reference's command-line surface for Step 1 (src/Regenie.cpp:146-371 option table, subset
// listed in SURVEY.md section 2 row 1) and its outputs (<out>.log, <out>_pred.list, <out>_<k>.loco,
// optional <out>_<k>.prs / <out>_prs.list; src/Data.cpp:956-1129, :1795-1975) and calls the HIP library
// through the C ABI of include/rg_step1.h for everything Data::level_0_calculations, ridge_level_1 and
// make_predictions do.  Host-side prerequisites (text parsing, masks, covariate basis, phenotype
// residualisation, fold / block bookkeeping, LOCO assembly, writers) follow the reference functions
// cited next to each routine.  There is no CPU compute fallback for the hot path.
//
// Served: --qt / --bt, K-fold CV / --loocv (and the reference's automatic LOOCV for --bt below 5,000 samples), and the
// file protocol of the level-0 job split: --split-l0 PFX,N / --run-l0 PFX.master,k / --run-l1 PFX.master [--keep-l0]
// (src/Data.cpp:232-309, :818-908; raw double N x (blocks*R0) files of Step1_Models.cpp:728-734).
// Genotype input: --bed PFX (bed/bim/fam), --pgen PFX (pgen/pvar/psam: hardcalls decoded to the same 2-bit rows, dosage files
// to doubles for the fp64 level 0; include/rg_pgen.h) or --bgen FILE [--sample FILE] (BGEN v1.2, 8-bit; include/rg_bgen.h);
// gzipped text inputs and --gz outputs through zlib (Files.cpp:38-160).  Not served (explicit errors, never silent): BGEN files
// other than layout 2 with 8-bit probabilities.
//   driver_common.cpp  text helpers, the option table (Regenie.cpp:146-371 subset), small utilities
//   driver_models.cpp  covariate-only null models and the host-side statistics (logistic / Poisson / Cox null fits, Firth, p-values)
//   driver_inputs.cpp  genotype metadata (.bim/.fam, .pvar/.psam, .bgen), phenotype / covariate files, LOCO files, the level-0 job files
//   driver_step2.cpp   `--step 2`: single-variant tests on the rg_step2.h kernels, one part per GPU (driver_step2.h: what it shares with the next)
//   driver_step2_bgen.cpp  the BGEN read-ahead of `--step 2` (BgenAhead), the planning of its groups
//   driver_ld.cpp      `--step 2 --compute-corr`: the LD matrix of a region on the rg_ld.h kernels
//   driver_step1_plan.cpp    `--step 1` without a device: the plan of a run (blocks, folds, ridge grids, penalties, GPU ranges), `--split-l0`, the
//                            .loco / .prs / .firth writer and the lists (driver_step1.h: what the Step-1 units share)
//   driver_step1_ingest.cpp  `--step 1`: the genotype ingest under one owner (mapped .bed, its copy in device memory, the ring of host buffers)
//   driver_step1.cpp   `--step 1`: contexts, level 0, the multi-GPU exchange, level 1, the level-0 job files; run()
//   driver_main.cpp    main()
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <fstream>
#include <functional>
#include <future>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <fcntl.h>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include <charconv>
#include <climits>
#include <unistd.h>
#include <zlib.h>

#include "../../include/rg_bgen.h"
#include "../../include/rg_pgen.h"
#include "../../include/rg_step1.h"
#include "../../include/rg_step2.h"
#include "../../include/rg_ld.h"

namespace rgdrv {

constexpr double MISSING = -999.0;  // Regenie.hpp:215

struct Params {
  int step = 0;
  std::string bed, pgen, bgen, sample_file, pheno_file, covar_file, out = "regenie_out";
  std::vector<std::string> keep, remove, extract, exclude, pheno_cols, covar_cols, cat_covar;
  int max_cat_levels = 10;
  bool rint = false;
  // --apply-rerint / --apply-rerint-cov: the two-stage rank-inverse-normal transformation of the Step-2 residuals of quantitative traits
  // (Regenie.cpp:433-434, :1251-1252; Data::residualize_res, Data.cpp:2407-2436).  Off under --bt; set but without effect under --ct and in step 1.
  bool rerint = false, rerintcov = false;
  int bsize = 0, cv_folds = 5, n_ridge_l0 = 5, n_ridge_l1 = 5, nchrom = 23, threads = 0;
  int n_block = 0;                         // --nb: total number of blocks, taken chromosome by chromosome (0: all)
  bool firth = false, firth_approx = false, firth_se = false;   // --firth --approx [--firth-se] (step 2, binary traits)
  bool write_null_firth = false;          // --write-null-firth (step 1 or 2): the null approximate-Firth estimates per chromosome, PFX_<k>.firth + PFX_firth.list
  std::string use_null_firth;             // --use-null-firth LIST (step 2): start values of the null Firth fits
  bool spa = false;                                             // --spa (step 2, binary traits)
  double pthresh = 0.05;                                        // --pThresh: score tests below it get the correction
  double min_info = 0.0; bool set_min_info = false;             // --minINFO (step 2, dosages)
  bool bt = false, ct = false, loocv = false, strict = false, ref_first = false, use_rel_path = false,
       print_prs = false, force_step1 = false, lowmem = false, force_qt = false, cc12 = false, gz = false;
  bool t2e = false;                        // --t2e: time-to-event traits (step 1: Cox ridge at level 1)
  bool t2e_event_l0 = false;               // --t2e-event-l0: which level-0 FILE a --lowmem / --run-l1 run of the reference reads for a time-to-event trait
                                           // (l0_idx, Step1_Models.cpp:2259-2261); level 1 itself fits on the time column's predictors either way (:2258,
                                           // :2269-2282) and this driver keeps them in HBM, so the switch is accepted and changes nothing -- regenie's own
                                           // in-memory outputs with and without it are byte-identical (tests/golden/ref_outputs/t2e_kfold_synth_event_l0)
  bool t2e_l1_pi6 = false;                 // --t2e-l1-pi6: level-1 penalties L (1 - h) / h * 6 / pi^2 from the heritability grid (check_l0, :2106-2110)
  std::vector<std::string> event_cols;     // --eventColList, matching --phenoColList (the time columns) in order
  int min_case_count = 10, niter_max = 50, niter_max_line_search = 25, niter_max_ridge = 100;
  // level-0 job split (Data.cpp:232-309, :818-908)
  std::string split_file;              // --split-l0 prefix / --run-l0, --run-l1 master file
  int njobs = 0, job_num = 0;
  bool split_l0 = false, run_l0 = false, run_l1 = false, keep_l0 = false;
  std::vector<double> setl0, setl1;
  int device = 0;
  // one node, several GPUs (no counterpart option in the reference, whose job split goes through files): --gpus N deals the
  // SNP blocks to N GPUs like write_l0_master (Data.cpp:270-302), one host thread per GPU, and replaces the job files by one
  // exchange of the level-0 predictors (rg_l0_finish).  --transport rccl (default) | peer; --single-device puts every rank on
  // --device (test mode, needs --transport peer); --force-collectives runs the exchange code with a single GPU as well.
  int gpus = 1;
  int transport = RG_TRANSPORT_RCCL;
  bool single_device = false, force_collectives = false;
  bool l1_shared = false;   // --l1-shared: all-gather + shared level 1 even when every GPU could own a phenotype
  // --step 2 (single-variant association test, quantitative traits: Data::test_snps_fast, Data.cpp:2230-2360)
  std::string pred_list;    // --pred: the _pred.list of step 1
  double min_mac = 5;       // --minMAC (Regenie.hpp:311)
  // --chr / --chrList / --range: the variant filter of read_bim / read_pvar / the .bgen index (Geno.cpp:106-110, :582-587, :857-859)
  std::set<int> chr_keep;   // empty: every chromosome
  bool set_range = false;
  int range_chr = -1;
  double range_min = 0, range_max = 0;
  // --step 2 --compute-corr: the LD matrix of a region (Data::ld_comp, Data.cpp:3807-3848; driver_ld.cpp)
  bool compute_corr = false, corr_text = false, forcein_vars = false;
  bool skip_scaleG = false;  // --skip-scaleG: the unscaled matrix (= GtG) with its `M n_samples` header line; text output only
  bool saw_sparse_thr = false;
  double sparse_thr = 0;     // --sparse-thr t: its sparse form, the sd line and the `i j r` lines with |r| >= t (0: no sparsifying); needs --skip-scaleG
  bool ld_dosages = false;   // --ld-dosages: the LD matrix of dosage input (--bgen, a .pgen dosage track), Data::compute_ld_dosages; refused without it
  // --step 2 --condition-list FILE [--condition-file FORMAT,FILE [--condition-file-sample FILE]] [--max-condition-vars N]: the listed variants become
  // covariates and leave the tested set (Regenie.cpp:217-219, :277, :516, :714-722; condition_variants in driver_inputs.cpp)
  std::string condition_list, condition_fmt, condition_file, condition_sample;
  uint32_t max_condition_vars = 10000;
  // --step 2 --qt --mcc [--mcc-thr p] [--mcc-skew s]: the moment-matched correlation test of skewed quantitative traits (Regenie.cpp:343-345, :489,
  // :1262-1277; compute_score_qt_mcc, Step2_Models.cpp:237-341)
  bool mcc = false;
  double mcc_thr = 0.01, mcc_skew = 0.0;
  // --step 2 --test additive|dominant|recessive [--minHOMs N] (Regenie.cpp:282, :735-740, :906-907): the genotype coding of the single-variant tests
  // (params.test_type 0 / 1 / 2 = RG_S2_ADDITIVE / RG_S2_DOMINANT / RG_S2_RECESSIVE of include/rg_step2.h); the recessive test ignores a variant whose
  // recoded sum over the observed samples -- the homALT carriers -- is below --minHOMs (Geno.cpp:2517-2521)
  int test_type = 0;
  bool saw_test = false;
  double min_homs = 0.0;
  // --step 2 --par-region hg38|hg19|hg18|b38|b37|b36|<end_par1>,<start_par2> (Regenie.cpp:253, check_build_code :1643-1660): the bounds of the
  // pseudo-autosomal regions of chromosome X.  A variant of chromosome X with par1_max < pos < par2_min is non-PAR (in_non_par, Geno.cpp:2802-2814):
  // there a male's call counts half in the minor-allele count.  The reference defaults to hg38 without a word; here chromosome X with males is
  // tested only when the build is named.
  bool par_set = false;
  std::string build_code;
  int64_t par1_max = 0, par2_min = 0;
  // --af-cc (Regenie.cpp:214, :458): A1FREQ_CASES A1FREQ_CONTROLS N_CASES N_CONTROLS in the result files of `--step 2 --bt`; switched off with the
  // reference's warning in every other mode (:1076-1079)
  bool af_cc = false;
};

// a worker thread of a multi-GPU step-2 run logs into its own buffer (tl_log): the parts' logs are appended in order afterwards
extern thread_local std::ostringstream* tl_log;
struct Log {  // mstream (Regenie.hpp:120-142): tee to stdout and <out>.log
  std::ofstream f;
  template <class T>
  Log& operator<<(const T& v) { if (tl_log) { *tl_log << v; return *this; } std::cout << v; if (f.is_open()) f << v; return *this; }
  Log& operator<<(std::ostream& (*m)(std::ostream&)) { if (tl_log) { *tl_log << m; return *this; } std::cout << m; if (f.is_open()) f << m; return *this; }
};
extern Log sout;
bool full_teardown();               // RG_TEARDOWN=1, or a tool that finalises at exit: device memory, page-locked buffers and the runtime are released in order
extern bool fast_exit;              // set at the successful end of a run: main() then leaves through _exit once the log is closed
extern std::mutex g_reader_mu;      // the .pgen / .bgen readers keep per-handle state: one block read at a time (multi-GPU step 2)

// Files (Files.cpp:38-160): a file whose name ends in ".gz" and starts with the gzip magic is read through zlib, anything
// else as plain text; `--gz` writes the .loco / .prs outputs through zlib.  (The reference needs Boost Iostreams for this.)
inline bool ends_with_gz(const std::string& fn) { return fn.size() > 3 && fn.compare(fn.size() - 3, 3, ".gz") == 0; }
inline bool file_exists(const std::string& fn) { return access(fn.c_str(), F_OK) == 0; }

class GzInBuf : public std::streambuf {
 public:
  explicit GzInBuf(const std::string& fn) : f_(gzopen(fn.c_str(), "rb")), buf_(1 << 16) {}
  ~GzInBuf() override { if (f_) gzclose(f_); }
  bool ok() const { return f_ != nullptr; }
 protected:
  int_type underflow() override {
    if (gptr() < egptr()) return traits_type::to_int_type(*gptr());
    const int n = f_ ? gzread(f_, buf_.data(), (unsigned)buf_.size()) : 0;
    if (n <= 0) return traits_type::eof();
    setg(buf_.data(), buf_.data(), buf_.data() + n);
    return traits_type::to_int_type(*gptr());
  }
 private:
  gzFile f_;
  std::vector<char> buf_;
};

class TextIn : public std::istream {  // Files::openForRead
 public:
  explicit TextIn(const std::string& fn) : std::istream(nullptr) {
    bool gz = false;
    if (ends_with_gz(fn)) {  // isGzipped(filename, true): extension first, then the two magic bytes
      std::ifstream t(fn, std::ios::binary);
      unsigned char h[2] = {0, 0};
      t.read((char*)h, 2);
      gz = t && h[0] == 0x1f && h[1] == 0x8b;
    }
    if (gz) {
      gz_.reset(new GzInBuf(fn));
      if (gz_->ok()) rdbuf(gz_.get()); else setstate(std::ios::failbit);
    } else {
      if (plain_.open(fn, std::ios::in)) rdbuf(&plain_); else setstate(std::ios::failbit);
    }
  }
 private:
  std::filebuf plain_;
  std::unique_ptr<GzInBuf> gz_;
};

class GzOutBuf : public std::streambuf {
 public:
  explicit GzOutBuf(const std::string& fn) : f_(gzopen(fn.c_str(), "wb")) {}
  ~GzOutBuf() override { if (f_) gzclose(f_); }
  bool ok() const { return f_ != nullptr; }
 protected:
  int_type overflow(int_type c) override {
    if (c == traits_type::eof()) return traits_type::not_eof(c);
    const char ch = traits_type::to_char_type(c);
    return (f_ && gzwrite(f_, &ch, 1) == 1) ? c : traits_type::eof();
  }
  std::streamsize xsputn(const char* p, std::streamsize n) override {
    if (!f_ || n <= 0) return 0;
    return gzwrite(f_, p, (unsigned)n) > 0 ? n : 0;
  }
 private:
  gzFile f_;
};

class TextOut : public std::ostream {  // Files::openForWrite
 public:
  TextOut(const std::string& fn, bool gz) : std::ostream(nullptr) {
    if (gz) {
      gz_.reset(new GzOutBuf(fn));
      if (gz_->ok()) rdbuf(gz_.get()); else setstate(std::ios::failbit);
    } else {
      if (plain_.open(fn, std::ios::out)) rdbuf(&plain_); else setstate(std::ios::failbit);
    }
  }
 private:
  std::filebuf plain_;
  std::unique_ptr<GzOutBuf> gz_;
};

struct Run {
  Params p;
  std::vector<double> bhat_start;        // [P][C] null logistic estimates (--write-null-firth in step 1: start of the null Firth fits)
  // genotype meta
  std::vector<std::string> fam_ids;      // FID_IID, file order
  std::vector<int> snp_chrom;            // kept variants
  std::vector<int64_t> snp_offset;
  std::vector<int> chr_read;             // chromosomes in file order
  std::vector<std::string> snp_ids;      // kept variants
  std::vector<int64_t> snp_pos;          // kept variants: physpos, and the two alleles in output order (Geno.cpp:546-553)
  std::vector<std::string> snp_a0, snp_a1;
  // --step 2: the LOCO files of step 1 (blup_read, Pheno.cpp:1241-1391)
  struct Blup { std::string file; std::vector<int64_t> col_sample; std::vector<int64_t> line_off;
                std::vector<std::string> lines; };     // lines: the chromosome rows of a gzipped file (no seeking there), else empty
  std::vector<Blup> blups;               // per phenotype
  // --run-l0 / --run-l1 (prep_parallel_l0 / prep_parallel_l1)
  int64_t parallel_nGeno = 0;            // global number of variants (lambda uses it, Data.cpp:607)
  int parallel_nBlocks = 0, parallel_nSnps = 0;
  std::string job_prefix;
  std::vector<std::string> mprefix; std::vector<int> bstart, btot;
  int64_t n_file = 0, bpr = 0;
  rg_pgen* pgen = nullptr;               // --pgen: open reader (bed rows come from rg_pgen_read_bed_rows)
  bool dosage_mode = false;              // --pgen with dosage tracks / --bgen: rows of doubles, level 0 from rg_l0_blocks_f64
  bool has_male = false;                 // a sample with sex code 1 in the .fam / .psam / .sample (Step 2 on chromosome X needs it)
  std::vector<uint8_t> sex;              // per sample of the file: the sex code (0: unknown / NA, 1: male, 2: female; params->sex)
  rg_bgen* bgenh = nullptr;              // --bgen: open reader
  // --condition-list: the conditioning variants in ascending id order (filters->condition_snp_names is a std::map, Geno.cpp:4151-4179) with their
  // index in the main genotype file (-1: not met among the variants the chromosome / range filter leaves)
  std::map<std::string, int64_t> cond_snps;
  int n_cond = 0;                        // columns appended to the covariates (not counted in the log's n_cov, as in the reference)
  // --mcc: params.mcc_test once the phenotypes are read (off when --mcc-skew leaves no trait), pheno_data.mcc_Y per trait (Pheno.cpp:117-131)
  bool mcc_test = false;
  std::vector<uint8_t> mcc_Y;
  Run() = default;
  Run(const Run&) = delete;
  ~Run() { if (pgen) rg_pgen_close(pgen); if (bgenh) rg_bgen_close(bgenh); }
  // samples
  std::vector<uint8_t> ind_ignore, ain;  // N_file, N
  std::vector<std::string> ids;          // kept, file order
  int64_t N = 0, n_analyzed = 0;
  // phenotypes / covariates
  std::vector<std::string> pheno_names;
  int P = 0, C = 0;
  std::vector<double> Y, X, neff, scale_Y;  // col-major N x P, N x C
  std::vector<uint8_t> mask;                // col-major N x P
  std::vector<double> Yraw, offset;         // BT: phenotypes_raw (0/1) and offset_nullreg, col-major N x P
  std::vector<uint8_t> pheno_pass;          // BT: null logistic model converged
  // --t2e: the phenotypes of the run are the TIME columns; Yraw = their raw values, Yevent the matching event columns (0 / 1),
  // t2e_num[q] = 1-based position of time column q among the selected (time and event) columns of the file: the reference counts
  // both as phenotypes, and names its outputs by that number (out_<num>.loco)
  std::vector<double> Yevent;
  std::vector<int> t2e_num;
  int outnum(int q) const { return t2e_num.empty() ? q + 1 : t2e_num[q]; }
};

constexpr double NUMTOL = 1e-6;                                   // Regenie.hpp numtol
constexpr double NUMTOL_EPS = 10 * 2.220446049250313e-16;         // Regenie.hpp:225

// a loop spread over host threads (step 2's variant loop is the reference's OpenMP loop in compute_tests_mt, Data.cpp:2484-2486)
template <class F>
void parallel_for(int n, int nthreads, F&& fn) {
  nthreads = std::max(1, std::min(nthreads, n));
  if (nthreads == 1) { for (int j = 0; j < n; ++j) fn(j); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t)
    th.emplace_back([&, t]() { for (int j = t; j < n; j += nthreads) fn(j); });
  for (auto& x : th) x.join();
}

// ---- driver_common.cpp
// A whole text file in memory with its line table (the remainder of a TextIn after the header line): the sample files of a 500,000-sample
// run are tokenised, matched to their samples and converted by several threads from here, without a string per token.
struct TextLines {
  std::string buf;
  std::vector<std::pair<size_t, size_t>> span;      // [begin, end) of every line, '\n' excluded (std::getline's lines)
  size_t size() const { return span.size(); }
  const char* begin(size_t l) const { return buf.data() + span[l].first; }
  const char* end(size_t l) const { return buf.data() + span[l].second; }
  std::string line(size_t l) const { return buf.substr(span[l].first, span[l].second - span[l].first); }
};
void slurp_lines(std::istream& f, TextLines& t);     // everything the stream still holds
int usable_cpus();      // hardware threads worth using: affinity mask and cgroup CPU quota taken into account
struct Tok { const char* b; const char* e; };
// whitespace-separated tokens of [b, e) (what `is >> t` would give); returns their number, stores the first `maxtok` of them
int tokenize(const char* b, const char* e, Tok* out, int maxtok);
double convert_double_tok(const char* b, const char* e);   // convert_double on a token that is not NUL-terminated
// "FID_IID" -> sample index without building the key: open addressing over the id strings
class IdIndex {
 public:
  explicit IdIndex(const std::vector<std::string>& ids);
  int64_t find(const char* fb, const char* fe, const char* ib, const char* ie) const;      // -1: no such sample
 private:
  static uint64_t hash(const char* fb, const char* fe, const char* ib, const char* ie);
  const std::vector<std::string>& ids_;
  std::vector<int32_t> slot_;
  uint64_t mask_;
};
std::vector<std::string> split_ws(const std::string& s);
std::vector<std::string> split_char(const std::string& s, char c);
int chr_str_to_int(std::string s, int nchrom);
double convert_double(const std::string& v);
std::string cpp_double(double v);
std::set<std::string> read_id_files(const std::vector<std::string>& files);
std::set<std::string> read_snp_files(const std::vector<std::string>& files);
void jacobi_eigh(std::vector<double> A, int n, std::vector<double>& d, std::vector<double>& V);
[[noreturn]] void usage_error(const std::string& m);
Params parse_args(int argc, char** argv);
std::string get_fullpath(const std::string& f);
void check(rg_ctx* ctx, int rc);
// ---- driver_models.cpp
double get_pvec1(double eta);
bool solve_dense(std::vector<double> A, std::vector<double> b, int n, std::vector<double>& x);
double norm_quantile(double p);
double get_logp(double t);
// --mcc: the closed-form part of the moment-matched correlation test (MCC::setup_y / precomp_sumy, MCCResults::dkat)
struct MccTrait { double n_mask, ni, ybar, ynorm, y2, y3, y4, y6; };      // per trait and chromosome: counts, mean and norm of yres, power sums of the normalised yres
MccTrait mcc_setup_trait(const double* yres, const uint8_t* mask, int64_t n, int n_cov);
// sums: S_1 .. S_6 and r . yres of rg_s2_qt_moments.  -> the p-value; ok = false when the gamma fit is not defined (skewness of D <= 0) or p is 0 or 1
double mcc_pvalue(const MccTrait& t, const double* sums, bool* ok);
double gamma_q(double a, double x);            // regularised upper incomplete gamma Q(a, x)
double gamma_p(double a, double x);            // ... and the lower one
double chisq1_upper_quantile(double p);        // x with P(chi-square(1) > x) = p
bool spd_logdet_inv(const std::vector<double>& A, int n, double& logdet, std::vector<double>* inv);
struct LogisticState { std::vector<double> beta, pv, eta; };      // what an attempt of fit_logistic leaves for the next one (the reference's in-place arguments)
bool fit_logistic(const double* y, const double* X, const uint8_t* mask, int64_t N, int C, const Params& prm, bool check_hs_dev, std::vector<double>& eta,
                  const double* offset = nullptr, std::vector<double>* pv_out = nullptr, std::vector<double>* beta_out = nullptr, LogisticState* resume = nullptr);
bool fit_poisson(const double* y, const double* X, const uint8_t* mask, int64_t N, int C, const Params& prm, std::vector<double>& eta,
                 const double* offset = nullptr, std::vector<double>* pv_out = nullptr);
bool cox_null_fit(const double* time, const double* event, const uint8_t* mask, const double* X, int64_t N, int C, const Params& prm, std::vector<double>& eta);
bool cox_null_newton(const double* time, const double* event, const uint8_t* mask, const double* X, int64_t N, int C, const Params& prm, double stephalf_tol,
                     std::vector<double>& eta);   // the reference's Newton fall-back (cox_firth.cpp without the Firth term)
bool firth_fit_cols(const double* y, const std::vector<const double*>& cols, const uint8_t* mask, const double* offset, int64_t n, int nfree, double maxstep,
                    std::vector<double>& beta, double* dev_out = nullptr, std::vector<double>* inv_out = nullptr, double stop_tol = 0.0);   // stop_tol > 0: fit_firth_nr's stopping rule
bool firth_null_fit(const double* y, const double* X, const uint8_t* mask, const double* offset, int64_t n, int C, std::vector<double>& beta);
// ---- driver_inputs.cpp
void read_bgen_meta(Run& r);
void read_bim_fam(Run& r);
void apply_sample_and_variant_filters(Run& r);
void blup_read(Run& r, const std::unordered_map<std::string, int64_t>& idx);
void read_condition_list(Run& r);
void condition_variants(Run& r, const std::vector<uint8_t>& in_cov, std::vector<double>& Xraw, int& ncols);
void read_pheno_cov(Run& r);
void prep_parallel_l0(Run& r);
void prep_parallel_l1(Run& r, int total_n_block, int64_t n_variants);
// ---- driver_step2.cpp / driver_step1.cpp
int run_step2_all(Run& r, std::chrono::steady_clock::time_point t_start);
// driver_ld.cpp registers its entry here when it is linked in: a build of the driver without that unit (the host-emulated test binary) still
// links, and says so when asked for the mode
extern int (*run_ld_entry)(Run& r, std::chrono::steady_clock::time_point t_start);
int run(int argc, char** argv);

}  // namespace rgdrv
