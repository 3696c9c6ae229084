// regenie-amd, the C++ host driver (see driver.h): what the two translation units of `--step 2` share (driver_step2.cpp, driver_step2_bgen.cpp).
#pragma once
#include "driver.h"

namespace rgdrv {

// One part of a `--step 2` run: the blocks [blk_lo, blk_hi) of the run's block list (chromosomes in file order, ceil(n_chr / bsize) blocks
// each) on one device.  A run on G GPUs is G parts on G host threads -- the blocks are independent, there is no exchange -- whose result
// lines go to part files that are concatenated in block order afterwards (run_step2_all).
struct S2Part {
  int part = 0, nparts = 1, device = 0;
  int blk_lo = 0, blk_hi = INT_MAX;
  int64_t n_ignored_snps = 0, n_ignored_tests = 0;     // out
  std::vector<std::string> firth_body;                 // out: --write-null-firth lines per trait
  std::vector<std::string> files;                      // out: the part's result files, one per trait
};

enum class In { Bed, PgenHard, Dosage };

// the environment switches of Step 2, read once
struct S2Env {
  bool dense = getenv("RG_S2_DENSE") != nullptr;                 // the fp64 route of the library (rg_s2_qt_block), kept for comparison
  bool bgen_rows = getenv("RG_S2_BGEN_ROWS") != nullptr;         // BGEN through the general dosage rows
  bool bgen_host = getenv("RG_S2_BGEN_HOST") != nullptr;         // BGEN read-ahead without the device decoder
  bool timing = getenv("RG_TIMING") != nullptr;
  int prep_threads = getenv("RG_S2_PREP_THREADS") ? std::max(1, atoi(getenv("RG_S2_PREP_THREADS"))) : 0;      // 0: not set
  int bgen_group = getenv("RG_S2_BGEN_GROUP") ? atoi(getenv("RG_S2_BGEN_GROUP")) : 3072;                      // the streams the GPU holds at once
  double bgen_host_share = getenv("RG_S2_BGEN_HOST_SHARE") ? std::min(0.9, std::max(0.0, atof(getenv("RG_S2_BGEN_HOST_SHARE")))) : 0.0;
};

// The analysed samples of a run: sample k of the analysis (the rows handed to the device) is kept sample an[k] and sample file_idx[k] of the
// genotype file.
struct SampleMap {
  explicit SampleMap(const Run& r) {
    for (int64_t i = 0; i < r.N; ++i) if (r.ain[i]) an.push_back(i);
    n = (int64_t)an.size();
    file_idx.assign(n, 0);
    int64_t kept = 0, k = 0;
    for (int64_t i = 0; i < r.n_file && k < n; ++i) {
      if (r.ind_ignore[i]) continue;
      if (kept == an[k]) file_idx[k++] = i;
      ++kept;
    }
    identity = n == r.n_file;
    for (int64_t k = 0; identity && k < n; ++k) identity = file_idx[k] == k;
  }
  std::vector<int64_t> an;                      // analysed samples among the kept ones, file order
  int64_t n = 0;
  std::vector<int64_t> file_idx;                // file index of every analysed sample
  bool identity = false;                        // every sample of the file is analysed, in file order
};

// A dosage as the exact integer the device takes (uint16 rows, 0xFFFF = missing); DOSAGE_NOT_INTEGRAL: the file's value is no such integer.
constexpr unsigned DOSAGE_NOT_INTEGRAL = 0x10000u;
// 8-bit .bgen probabilities (b0, b1) in units of 1 / 255: G * 255 = prob1 + 2 prob0, or with --ref-first prob1 + 2 max(1 - prob0 - prob1, 0)
// (Geno.cpp:2286-2290).  Above 510 (prob0 + prob1 > 1 in the file) it is no dosage in [0, 2]; the value is returned as it is.
inline unsigned bgen_dosage_255(unsigned b0, unsigned b1, bool ref_first) { return ref_first ? b1 + 2u * (b0 + b1 < 255u ? 255u - b0 - b1 : 0u) : b1 + 2u * b0; }
inline bool bgen_dosage_integral(unsigned q) { return q <= 510u; }
// `--test dominant | recessive` (coding 1 | 2), parseSnpfromBGEN's second pass (Geno.cpp:2384-2389), in units of 1 / 255: prob0 + prob1 | prob0, with
// --ref-first prob1 + prob2 | prob2 (prob2 = max(1 - prob0 - prob1, 0)).  At most 255 in a file whose probabilities sum to at most 1.
inline unsigned bgen_coded_255(unsigned b0, unsigned b1, bool ref_first, int coding) {
  const unsigned b2 = b0 + b1 < 255u ? 255u - b0 - b1 : 0u;
  return coding == 1 ? (ref_first ? b1 + b2 : b0 + b1) : (ref_first ? b2 : b0);
}
// the same relabelling of a hard call 0 / 1 / 2 (parseSnpfromBed, Geno.cpp:2511-2515; the .pgen reader rounds a dosage to a hard call first, :2672-2678)
inline double recode_hard_call(double hc, int coding) { return coding == 1 ? (hc == 2.0 ? 1.0 : hc) : coding == 2 ? (hc >= 1.0 ? hc - 1.0 : hc) : hc; }
// a .pgen dosage in units of 1 / 16384; -3 is the missing value
inline unsigned pgen_dosage_16384(double g) {
  if (g == -3.0) return 0xFFFFu;
  const double v = g * 16384.0, rv = std::nearbyint(v);
  if (std::fabs(v - rv) > 1e-6 || rv < 0 || rv > 2.0 * 16384.0) return DOSAGE_NOT_INTEGRAL;
  return (unsigned)rv;
}

// The run-wide facts of a part, built once and only read afterwards (by the workers of the read-ahead too).
struct S2Common : SampleMap {
  S2Common(Run& r, const S2Part& part);
  Run& r;
  const Params& p;
  const S2Part& part;
  const S2Env env;
  const int64_t N;
  const int P, C;
  bool any_missing = false;                     // filters->has_missing: a sample masked for at least one trait
  std::vector<uint8_t> has_missing;
  std::vector<double> Xc, Yc;                   // compact, sample-fastest copies for the C ABI
  std::vector<uint8_t> Mc;
  std::map<int, std::vector<int64_t>> chr_snps; // blocks per chromosome (set_blocks_for_testing: ceil(n_chr / bsize))
  int total_blocks = 0;
  bool glm, mcc, firth, spa, correct, per_trait, show_info, multi, fast_bgen;
  int rerint = 0;                               // --apply-rerint (RG_S2_RERINT) / --apply-rerint-cov (RG_S2_RERINT_COV), quantitative traits only; 0: off
  double z_thr;
  In in;
  int flip, dscale, nthreads, nt_prep;
  int coding;                                   // --test: 0 additive, 1 dominant, 2 recessive (= RG_S2_ADDITIVE / _DOMINANT / _RECESSIVE)
  const char* test_name;                        // the TEST column: ADD / DOM / REC (Data.cpp:2077-2089)
  int64_t ld16;                                 // leading dimension of the host threads' uint16 dosage rows
  // chromosome X outside the pseudo-autosomal regions (--par-region): a male's call counts half in the minor-allele count
  bool sex_aware = false;                       // chromosome X is tested, the sample file has males and --par-region names the bounds
  std::vector<uint8_t> male;                    // per analysed sample: sex code 1 (params->sex subset to the analysis, Geno.cpp:1330-1332)
  // --af-cc (binary traits): per (trait, analysed sample), 1 = an observed case -- mask_p * y_p of update_af_cc (Geno.cpp:3069-3075)
  bool af_cc = false;
  std::vector<uint8_t> Cc, any_case;            // [P][n]; [n]: a case of at least one trait
  bool non_par(int64_t snp) const { return sex_aware && r.snp_chrom[snp] == p.nchrom && r.snp_pos[snp] > p.par1_max && r.snp_pos[snp] < p.par2_min; }   // in_non_par (Geno.cpp:2802-2814)
};

inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
// compute_mac (Geno.cpp:3077-3108), autosomes
inline bool below_min_mac(double total, double ns, double min_mac) { return std::min(total, 2.0 * ns - total) < min_mac; }
// the same outside the pseudo-autosomal regions of chromosome X (:3096-3097): mac = sum g (male ? 0.5 : 1) = total - male_total / 2 over the observed
// samples, of which nmales are male; MAC = min(mac, 2 ns - nmales - mac).  Never above the autosomal value.
inline bool below_min_mac_x(double total, double ns, double male_total, double nmales, double min_mac) {
  const double mac = total - 0.5 * male_total;
  return std::min(mac, 2.0 * ns - nmales - mac) < min_mac;
}
// compute_aaf_info (Geno.cpp:3132-3141): IMPUTE info for .bgen (it can be negative for very uncertain dosages), MaCH r2 for .pgen dosages
inline double info_score(bool bgen, double info_num, double ns, double af) {
  if (af == 0.0 || af == 1.0) return 1.0;
  return bgen ? 1.0 - info_num / (2.0 * ns * af * (1.0 - af)) : (info_num / ns - 4.0 * af * af) / (2.0 * af * (1.0 - af));
}
// update_trait_counts (Geno.cpp:2948-2959) as differences: sample k's call v (info term e) leaves the totals of the traits it is masked for
inline void subtract_masked(const uint8_t* Mc, int64_t n, int P, int64_t k, double v, double e, double* af_t, int64_t* ns_t, double* info_t) {
  for (int q = 0; q < P; ++q)
    if (!Mc[(size_t)q * n + k]) { af_t[q] -= v; ns_t[q] -= 1; if (info_t) info_t[q] -= e; }
}
// update_af_cc (Geno.cpp:3069-3075): sample k's observed additive call v joins the sums of the traits it is a case of
inline void add_cases(const uint8_t* Cc, int64_t n, int P, int64_t k, double v, double* af_case, int64_t* ns_case) {
  for (int q = 0; q < P; ++q)
    if (Cc[(size_t)q * n + k]) { af_case[q] += v; ns_case[q] += 1; }
}
// the 2-bit codes of the analysed samples of `bs` rows of the file (bpr bytes each), packed four to a byte; returns the new row length
inline int64_t repack_analysed(const uint8_t* rows, int64_t bpr, int bs, const int64_t* file_idx, int64_t n, int nthreads, std::vector<uint8_t>& packed) {
  const int64_t ld = (n + 3) / 4;
  packed.assign((size_t)bs * ld, 0);
  parallel_for(bs, nthreads, [&](int j) {
    const uint8_t* row = rows + (size_t)j * bpr;
    uint8_t* dst = packed.data() + (size_t)j * ld;
    for (int64_t k = 0; k < n; ++k) {
      const int64_t i = file_idx[k];
      dst[k >> 2] |= (uint8_t)(((row[i >> 2] >> (2 * (i & 3))) & 3) << (2 * (k & 3)));
    }
  });
  return ld;
}

// ---- driver_step2_bgen.cpp
struct BlkRef { int chrom; const std::vector<int64_t>* snps; int64_t j0; int bs; };      // rows [j0, j0 + bs) of a chromosome's variants
// The device decoder works on one stream per wavefront and needs thousands of them in flight: the blocks of a chromosome are prepared in
// groups of >= dev_target variants whatever --bsize is; without a decoder a group is one block.  A group is a BlkRef of its own.
struct Group { BlkRef ref; size_t first_block; int dev_rows; std::vector<int> starts; };       // rows [0, dev_rows) on the device; starts: its blocks' first rows
struct GroupPlan {
  std::vector<Group> groups;
  std::vector<std::pair<size_t, int>> block_group;      // per block: its group, its first row there
};
GroupPlan plan_groups(const std::vector<BlkRef>& blocks, int bsize, int dev_target, double share, bool has_device);

// what the read-ahead hands the block loop: a view of the block's rows in its prepared group (valid until the group after the next is started)
struct PreparedBlock {
  const double *total, *info_num, *af_t, *info_t;       // the *_t: [bs][P], only with S2Common::per_trait
  const double* sum_pos;                                // only with S2Common::coding: the recoded values' sum over the observed samples
  const int64_t *ns1, *ns_t;
  const double* af_case; const int64_t* ns_case;        // [bs][P], only with S2Common::af_cc and rows the host threads walked (on_device == 0)
  const uint8_t* ignored;
  const uint16_t* g16; int64_t ld; int on_device;
  bool integral;                                        // false: prob0 + prob1 > 1 somewhere in the group, the general route reports what the reference would
};
struct BgenTiming {
  int64_t dev_blocks = 0, host_blocks = 0;
  double dev_read = 0, dev_decode = 0, prep_wall = 0, prep_wait = 0, inflate = 0, walk = 0;
};

// 8-bit .bgen blocks (the UK Biobank encoding), one group ahead of the tests: the group's first rows are inflated and walked on the GPU
// (csrc/bgen_inflate.hip; its decoder has its own stream), the others -- or all of them: RG_S2_BGEN_HOST=1, a group the decoder flags --
// by the host threads, which walk the bytes once: 2-byte integer dosages (units of 1 / 255) into a pinned buffer, the allele / info sums of
// parseSnpfromBGEN (Geno.cpp:2186-2330) in the reference's order.  The three double rows per variant of the general route (dosage, info
// term, analysed-sample copy: 12 MB per variant at 500,000 samples) do not exist on this one.
// Lifetime: the workers (prep_ahead_, every slot's rd, the device future inside prepare) use the slots, the groups and the decoder; the
// destructor joins them, then frees the pinned buffers, then destroys the decoder.
class BgenAhead {
 public:
  explicit BgenAhead(const S2Common& cm);
  ~BgenAhead();
  BgenAhead(const BgenAhead&) = delete;
  void start();                                 // the first group, while the first chromosome's predictions are read
  const PreparedBlock* next_block();            // this part's next block; group g + 1 is started when group g's first block is taken
  void report_device() const;                   // the [timing] line of the device decoder
  BgenTiming timing;
 private:
  struct DosPrep {
    uint16_t* g16 = nullptr;                 // pinned, rows of ld16 entries
    std::vector<uint8_t> raw, ignored;
    std::vector<double> total, info_num, af_t, info_t, sum_pos;
    std::vector<int64_t> ns1, ns_t;
    std::vector<double> af_case; std::vector<int64_t> ns_case;      // --af-cc: the host-walked rows' sums among the cases
    bool integral = false;
    double ms_inflate = 0, ms_walk = 0, ms_wall = 0;
    std::string err;
    std::vector<int64_t> vi;                 // the group's variants in the file
    std::vector<double> w_inf, w_walk;       // per host worker
    std::atomic<int> host_bad{0};
    // device route: the stored zlib streams in page-locked memory, the dosage rows left in device memory
    int64_t g16_rows = 0;                    // rows the pinned buffer holds (the host route's; allocated when that route is first taken)
    uint8_t* comp = nullptr; int64_t comp_cap = 0;
    const uint16_t* g16_dev = nullptr; int64_t ld_dev = 0;
    int dev_rows = 0;                        // rows [0, dev_rows) of the group are in device memory (g16_dev), the others in g16 from row host_row0 on
    int host_row0 = 0;
    bool dev_bad = false;
    double ms_read = 0, ms_dev = 0;
    // the stored streams of the group that will be decoded into this slot NEXT, read while the other slot's group is decoded
    std::vector<int64_t> rd_off; std::vector<int32_t> rd_clen, rd_ulen;
    std::future<bool> rd; int64_t rd_group = -1; double rd_ms = 0;
  };
  bool read_streams(const BlkRef& br, DosPrep& d, int rows);
  bool prepare_dev(const BlkRef& br, DosPrep& d, int slot, int64_t gi, int rows);
  void host_rows(const BlkRef& br, DosPrep& d, int lo);
  void prepare(size_t gi);
  const S2Common& cm_;
  rg_bgen_dev* bdev_ = nullptr;
  int64_t block_bytes_ = 0;
  GroupPlan plan_;
  size_t my_next_ = 0;
  PreparedBlock view_{};
  DosPrep preps_[2];
  std::future<void> prep_ahead_;
};

}  // namespace rgdrv
