// regenie-amd, the C++ host driver (see driver.h): what the translation units of `--step 1` share (driver_step1.cpp, driver_step1_plan.cpp,
// driver_step1_ingest.cpp).
#pragma once
#include "driver.h"

namespace rgdrv {

using Clock = std::chrono::steady_clock;
inline long long ms_int(Clock::time_point a, Clock::time_point b) { return (long long)std::chrono::duration_cast<std::chrono::milliseconds>(b - a).count(); }
inline double ms_dbl(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

struct IngestRing;      // driver_step1_ingest.cpp
struct Blk { int chrom; int64_t start; int bs; };      // a SNP block: its chromosome, its first variant among the kept ones, its size

// Everything a Step-1 run decides before a device is touched (plan_step1: no device calls): set_blocks and set_folds of Data.cpp, the ridge
// grids, the level-1 penalties, the columns of W per chromosome and the block / phenotype ranges of the GPUs.
struct Step1Plan {
  std::vector<Blk> blocks;
  int B = 0;                             // blocks
  int64_t M = 0;                         // variants behind lambda: the global count under --run-l0 (Data.cpp:607)
  std::vector<double> h0, h1, lambda;    // heritability grids of the two levels, lambda[i] = M (1 - h0[i]) / h0[i]
  int R0 = 0, R1 = 0, L = 0;             // L = B R0: the columns of W
  bool use_loocv = false;
  std::vector<int32_t> cv_sizes;
  std::vector<double> tau, ct_rate;      // [P][R1] level-1 penalties (a --t2e call writes the ones it used back), [P] mean count of a --ct trait
  std::vector<int32_t> cols_per_chr;     // columns of W per chromosome that has blocks ...
  std::vector<int> chroms;               // ... and those chromosomes
  int nchr = 0, NCS = 5;                 // NCS: rows of a trait's cumsum table
  int G = 1;
  bool use_group = false, pheno_sharded = false;      // pheno_sharded: all-to-all by phenotype; else all-gather + shared level 1
  std::vector<int32_t> bbeg, pbeg;       // [G + 1] block and phenotype ranges of the ranks
};
// logs the " * block size" ... lines; throws the reference's errors (fold checks, grids).  The one thing it changes in the run: under --run-l1 it
// reads the master file (prep_parallel_l1), which needs the block count and fills r.mprefix, r.bstart and r.btot.
Step1Plan plan_step1(Run& r);
int split_l0(const Run& r);              // --split-l0: the master file and the per-job variant lists (Data.cpp:232-309); needs no device

// The outputs of the phenotypes: the per-trait table lines, the .loco / .prs / .firth files (Data::output + write_predictions, Data.cpp:956-1129,
// :1795-1975) and the entries of the lists, written at the end in phenotype order.  No device calls; emit() of different phenotypes may run
// on different threads.
class LocoWriter {
 public:
  LocoWriter(const Run& r, const Step1Plan& pl);
  // cs: the trait's [NCS][R1] cumsum table, pq: its [nchr][N] predictions
  void emit(int q, const double* cs, int bestq, int conv, const double* pq);
  void write_lists();
 private:
  static constexpr int NCK = 16;         // chunks of samples a row is formatted in
  template <class V> void format_rows(int nrows, V&& value, const uint8_t* maskq, std::vector<std::string>& piece) const;
  void write_row(std::ostream& f, const std::string& label, const std::vector<std::string>& piece, int row) const;
  const Run& r;
  const Step1Plan& pl;
  std::string header;
  std::vector<int64_t> kept_order;       // the analysed samples in the writer's order
  int fmt_threads = 1;
  bool timing_on = false;
  std::vector<std::string> ph_log, ph_plist, ph_prslist, ph_firthlist;      // per phenotype, filled by whichever thread emits it
};

// The genotype ingest of Step 1 under one owner: the mapped .bed, its copy in device memory and the ring of host buffers (IngestRing, BedMap,
// BedStage: driver_step1_ingest.cpp), their threads and their teardown.  release() -- also the destructor -- joins the threads and hands back
// the staged device buffer and the slots: it runs BEFORE any rg_destroy, whose contexts the staged buffer belongs to.
class Step1Ingest {
 public:
  Step1Ingest(const Run& r, Clock::time_point t_start);
  ~Step1Ingest();
  // under the parsing of the phenotype and covariate files: maps the .bed, starts its copy to the device or the page-locking of the ring
  void start_early(const std::vector<std::shared_future<rg_ctx*>>& early_ctx);
  // once the problem's sizes are known: a live stage is kept only if `need_bytes` of device memory are still free beside it
  void settle(rg_ctx* ctx0, int64_t need_bytes);
  void map_ready();                      // joins the registration of the mapping, once, before the rank threads start
  // level 0 of blocks [b_lo, b_hi) on one context; in_group: called by a rank thread of a GPU group
  void level0(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg, bool in_group);
  void release();
 private:
  struct State;
  void level0_dosage(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg);
  bool level0_mapped(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg);      // false: not every block is a range of the file
  void level0_ring(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg, IngestRing* pre_ring);      // pre_ring: the ring started early, or null for one of the call's own
  void alive() const;                    // throws after release(): nothing of the ingest can be used then
  const Run& r;
  const Clock::time_point t_start;
  const int64_t ingest_blk_bytes;
  std::unique_ptr<State> s;
};

}  // namespace rgdrv
