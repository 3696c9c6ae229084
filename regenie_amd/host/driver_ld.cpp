// regenie-amd, the C++ host driver (see driver.h): `--step 2 --compute-corr`, the LD matrix of a region (Data::ld_comp, Data.cpp:3807-3848).
//
// The host keeps what the reference's host does around print_ld: which variant takes which column (check_in_map_from_files /
// check_ld_list, Geno.cpp:1343-1380, :1443-1453), the variant lists (write_snplist, Data.cpp:3862-3885), reading the 2-bit rows in
// panels of --bsize (or, for --bgen and .pgen dosages, the exact integer dosages as uint16 rows), the output formats (binary R^2, text,
// and under --skip-scaleG the unscaled text matrix or its --sparse-thr triplets).
// Everything numeric -- the integer Gram of the panels, the covariate projection, the
// diagonal rules, the scaling, the 16-bit quantisation and the sparse threshold -- is the library's (include/rg_ld.h); there is no CPU path.
#include "driver_ld.h"
#include "driver_step2.h"

namespace rgdrv {

// Eigen's operator<< at StreamPrecision (6 significant digits), as print_ld writes the text matrix
static void fmt_sig6(double v, std::string& out) {
  char buf[40];
  if (v == 0) v = 0.0;      // (no "-0")
  const int k = snprintf(buf, sizeof(buf), "%.6g", v);
  out.append(buf, (size_t)k);
}

// with --extract --forcein-vars the lines of the extract file in order; otherwise the kept variants in file order
static LdColumns read_ld_columns(const Run& r) {
  if (!r.p.forcein_vars) return plan_ld_columns(r.snp_ids, nullptr);
  std::vector<std::string> first;
  TextIn f(r.p.extract[0]);
  if (!f) throw std::runtime_error("cannot read file : " + r.p.extract[0]);
  std::string line;
  while (std::getline(f, line)) {
    auto t = split_ws(line);
    if (t.empty()) throw std::runtime_error("incorrectly formatted file.");
    first.push_back(t[0]);
  }
  return plan_ld_columns(r.snp_ids, &first);
}

// What the stages of run_ld share: the column plan, the analysed samples and the library context with its basis and forced columns.
struct LdCommon {
  explicit LdCommon(Run& r_) : r(r_), p(r_.p), sm(r_), lc(read_ld_columns(r_)), M((int64_t)lc.col_ids.size()), out(r_.p.out + ".corr") {
    if (M < 1) throw std::runtime_error("no variant left to include in analysis.");
    sout << std::left << std::setw(20) << " * block size" << ": [" << p.bsize << "]\n";
    const char* runmode = r.dosage_mode ? "in dosage mode" : "in hard-call mode";
    if (p.corr_text) sout << " * computing correlation matrix " << runmode << "\n  + output to text file [" << out << "]\n";      // setup_output, Data.cpp:1986-2004
    else sout << " * computing correlation matrix " << runmode << " (storing R^2 values)\n  + output to binary file [" << out << "]\n";
    sout << "  + list of snps written to [" << out << ".snplist]\n  + n_snps = " << M << "\n\n";
    // the compact, sample-fastest covariate basis (as run_step2)
    const int64_t N = r.N, n = sm.n;
    std::vector<double> Xc((size_t)r.C * n);
    for (int c = 0; c < r.C; ++c) for (int64_t k = 0; k < n; ++k) Xc[(size_t)c * n + k] = r.X[(size_t)c * N + sm.an[k]];
    if (rg_ld_create(&ld, p.device, n, r.C, (int32_t)M) != RG_LD_OK) {
      const std::string m = ld ? rg_ld_last_error(ld) : "rg_ld_create failed";
      throw std::runtime_error(m.find("no HIP device") != std::string::npos ? "no MI355X / HIP device available (rg_ld_create failed)" : m);
    }
    check(rg_ld_set_basis(ld, Xc.data()));
    std::vector<int32_t> forced;
    for (int64_t c = 0; c < M; ++c) if (lc.absent[c]) forced.push_back((int32_t)c);
    if (!forced.empty()) check(rg_ld_force_columns(ld, (int32_t)forced.size(), forced.data()));
    npanels = (int)((lc.present.size() + p.bsize - 1) / p.bsize);      // get_G_svs (Data.cpp:4227-4304): the rows in panels of --bsize
    nthreads = std::max(1, std::min(p.threads > 0 ? p.threads : std::max(1, usable_cpus() - 1), 64));
  }
  void check(int rc) const { if (rc != RG_LD_OK) throw std::runtime_error(rg_ld_last_error(ld)); }
  // panel b: the bs variants from j0 on among those with a column; their place in the file and their columns
  struct Panel { int64_t j0; int bs; std::vector<int64_t> vidx; std::vector<int32_t> cols; };
  Panel panel(int b) const {
    const int64_t j0 = (int64_t)b * p.bsize;
    Panel c{j0, (int)std::min<int64_t>(p.bsize, (int64_t)lc.present.size() - j0), {}, {}};
    for (int j = 0; j < c.bs; ++j) { c.vidx.push_back(r.snp_offset[lc.present[j0 + j]]); c.cols.push_back(lc.col_of_variant[lc.present[j0 + j]]); }
    return c;
  }
  Run& r;
  const Params& p;
  const SampleMap sm;
  const LdColumns lc;
  const int64_t M;
  const std::string out;
  struct Owner { rg_ld_ctx* h = nullptr; ~Owner() { if (h && full_teardown()) rg_ld_destroy(h); } } owner;      // (released when the constructor throws, too)
  rg_ld_ctx*& ld = owner.h;
  int npanels = 0, nthreads = 1;

};

// get_G_svs(int, int) (Data.cpp:4049-4090) for dosages: the block as uint16 rows of exact integers -- 8-bit .bgen probabilities in
// units of 1 / 255 (the inflated blocks walked as the Step-2 read-ahead walks them), .pgen dosages in units of 1 / 16384 -- which the
// library splits into int8 digit planes.  A value that is no such integer is an error: there is no second route.
// zlib .bgen files: the stored streams go to the device decoder (rg_bgen_dev_decode), whose uint16 rows are appended where they lie; a
// block with a variant the decoder turns down (status != 0), zstd and uncompressed files take the host route.
class DosagePanels {
 public:
  explicit DosagePanels(const LdCommon& cm) : cm_(cm), r_(cm.r) {
    sout << "** Computing LD matrix " << (cm.p.skip_scaleG ? "(=GtG) " : "") << "**\n";      // Data.cpp:3919
    if (cm.npanels > 0) sout << "  -> splitting across " << cm.npanels << " SV blocks\n";
    if (!r_.bgenh) return;
    if (rg_bgen_block_bytes(r_.bgenh, &block_bytes_) != RG_BGEN_OK) throw std::runtime_error(rg_bgen_last_error(r_.bgenh));
    block_bytes_ = (block_bytes_ + 63) / 64 * 64;
    int32_t bcomp = 0;
    rg_bgen_info(r_.bgenh, nullptr, nullptr, &bcomp, nullptr);
    if (bcomp == 1 && rg_bgen_dev_create(&bdev_, cm.p.device) == RG_BGEN_OK &&
        rg_bgen_dev_set_samples(bdev_, r_.n_file, cm.sm.n, cm.sm.identity ? nullptr : cm.sm.file_idx.data(), 0, nullptr) != RG_BGEN_OK) {
      rg_bgen_dev_destroy(bdev_);
      bdev_ = nullptr;
    }
  }
  ~DosagePanels() { if (bdev_ && full_teardown()) rg_bgen_dev_destroy(bdev_); }
  DosagePanels(const DosagePanels&) = delete;
  void append_all() {
    int64_t dev_blocks = 0, host_blocks = 0;
    for (int b = 0; b < cm_.npanels; ++b) {
      sout << "     - row " << b + 1 << "\n" << std::flush;
      const LdCommon::Panel pn = cm_.panel(b);
      if (r_.bgenh && device_block(pn)) { ++dev_blocks; continue; }
      host_block(pn), ++host_blocks;
    }
    if (r_.bgenh) sout << "     - " << dev_blocks << " blocks decoded on the device, " << host_blocks << " on the host\n";
  }

 private:
  [[noreturn]] void not_integral(int64_t row, int scale) const {
    throw std::runtime_error("variant '" + r_.snp_ids[cm_.lc.present[row]] + "' has a dosage that is not an integer in [0, " + std::to_string(2 * scale) + "] in units of 1/" +
                             std::to_string(scale) + (r_.bgenh ? " (probabilities that add up to more than 1)" : "") + ": the LD matrix of such dosages is not built.");
  }
  // false: the block is left to the host route
  bool device_block(const LdCommon::Panel& pn) {
    const int bs = pn.bs;
    if (!bdev_) return false;
    int64_t need = 0;
    if (rg_bgen_compressed_bytes(r_.bgenh, bs, pn.vidx.data(), &need) != RG_BGEN_OK) return false;
    if ((int64_t)comp_.size() < need) comp_.resize((size_t)(need + need / 4));
    std::vector<int64_t> off(bs);
    std::vector<int32_t> clen(bs), ulen(bs), status(bs), maxq(bs);
    if (rg_bgen_read_compressed(r_.bgenh, bs, pn.vidx.data(), comp_.data(), (int64_t)comp_.size(), off.data(), clen.data(), ulen.data(), std::min(cm_.nthreads, 32)) != RG_BGEN_OK)
      return false;
    rg_bgen_dev_out o;
    memset(&o, 0, sizeof(o));
    o.max_q = maxq.data(); o.status = status.data();
    if (rg_bgen_dev_decode(bdev_, 0, bs, comp_.data(), off[bs - 1] + clen[bs - 1], off.data(), clen.data(), ulen.data(), cm_.p.ref_first ? 1 : 0, &o) != RG_BGEN_OK) return false;
    for (int j = 0; j < bs; ++j) if (status[j] != 0) return false;
    for (int j = 0; j < bs; ++j) if (!bgen_dosage_integral((unsigned)maxq[j])) not_integral(pn.j0 + j, 255);
    if (!o.g16 || o.ld16 < cm_.sm.n) return false;
    cm_.check(rg_ld_append_int(cm_.ld, o.g16, o.ld16, bs, 1, 255, pn.cols.data()));
    return true;
  }
  void host_block(const LdCommon::Panel& pn) {
    const int bs = pn.bs;
    const int64_t n = cm_.sm.n;
    const int64_t* file_idx = cm_.sm.file_idx.data();
    g16_.resize((size_t)bs * n);
    std::vector<int> bad(bs, 0);
    const int scale = r_.bgenh ? 255 : 16384;
    if (r_.bgenh) {
      raw_.resize((size_t)bs * block_bytes_);
      if (rg_bgen_read_blocks(r_.bgenh, bs, pn.vidx.data(), raw_.data(), block_bytes_, std::min(cm_.nthreads, 32)) != RG_BGEN_OK) throw std::runtime_error(rg_bgen_last_error(r_.bgenh));
    } else {
      dbuf_.resize((size_t)bs * r_.n_file);
      if (rg_pgen_read_dosage_rows(r_.pgen, bs, pn.vidx.data(), dbuf_.data(), r_.n_file) != RG_PGEN_OK) throw std::runtime_error(rg_pgen_last_error(r_.pgen));
    }
    const bool rf = cm_.p.ref_first;
    auto value = [&](int j, int64_t i) -> unsigned {      // sample i of the file in row j
      if (!r_.bgenh) return pgen_dosage_16384(dbuf_[(size_t)j * r_.n_file + i]);
      const uint8_t* blk = raw_.data() + (size_t)j * block_bytes_;      // ploidy bytes from 8 on, then the probability pairs
      if (blk[8 + i] & 0x80) return 0xFFFFu;
      const unsigned q = bgen_dosage_255(blk[10 + r_.n_file + 2 * i], blk[10 + r_.n_file + 2 * i + 1], rf);
      return bgen_dosage_integral(q) ? q : DOSAGE_NOT_INTEGRAL;
    };
    parallel_for(bs, cm_.nthreads, [&](int j) {
      uint16_t* q = g16_.data() + (size_t)j * n;
      for (int64_t k = 0; k < n; ++k) {
        const unsigned qi = value(j, file_idx[k]);
        if (qi == DOSAGE_NOT_INTEGRAL) { bad[j] = 1; break; }
        q[k] = (uint16_t)qi;
      }
    });
    for (int j = 0; j < bs; ++j) if (bad[j]) not_integral(pn.j0 + j, scale);
    cm_.check(rg_ld_append_int(cm_.ld, g16_.data(), n, bs, 0, scale, pn.cols.data()));
  }
  const LdCommon& cm_;
  Run& r_;
  rg_bgen_dev* bdev_ = nullptr;
  int64_t block_bytes_ = 0;
  std::vector<uint8_t> comp_, raw_;
  std::vector<uint16_t> g16_;
  std::vector<double> dbuf_;
};

// the 2-bit rows of the .bed file or of the .pgen hard calls, repacked to the analysed samples
static void append_hard_call_panels(const LdCommon& cm) {
  const Run& r = cm.r;
  sout << "** reading in single variant genotypes **\n  + " << cm.lc.present.size() << " variants in total split across " << cm.npanels << " blocks\n";
  const int fd = r.pgen ? -1 : open((cm.p.bed + ".bed").c_str(), O_RDONLY);
  if (!r.pgen && fd < 0) throw std::runtime_error("cannot read bed file");
  struct FdGuard { int fd; ~FdGuard() { if (fd >= 0) close(fd); } } fdg{fd};
  const int flip = (!r.pgen && cm.p.ref_first) ? 1 : 0;      // .pgen rows always count ALT (as run_step2)
  std::vector<uint8_t> rows, packed;
  for (int b = 0; b < cm.npanels; ++b) {
    sout << "  block [" << b + 1 << "/" << cm.npanels << "] : reading in genotypes..." << std::flush;
    const LdCommon::Panel pn = cm.panel(b);
    rows.resize((size_t)pn.bs * r.bpr);
    if (r.pgen) {
      if (rg_pgen_read_bed_rows(r.pgen, pn.bs, pn.vidx.data(), rows.data(), r.bpr) != RG_PGEN_OK) throw std::runtime_error(rg_pgen_last_error(r.pgen));
    } else {
      std::atomic<int> failed(0);
      parallel_for(pn.bs, std::min(cm.nthreads, 8), [&](int j) {
        int64_t got = 0;
        while (got < r.bpr) {
          const ssize_t k = pread(fd, rows.data() + (size_t)j * r.bpr + got, (size_t)(r.bpr - got), 3 + pn.vidx[j] * r.bpr + got);
          if (k <= 0) { failed = 1; return; }
          got += k;
        }
      });
      if (failed) throw std::runtime_error("cannot read bed file");
    }
    const bool repack = !cm.sm.identity;
    const int64_t ldr = repack ? repack_analysed(rows.data(), r.bpr, pn.bs, cm.sm.file_idx.data(), cm.sm.n, cm.nthreads, packed) : r.bpr;
    cm.check(rg_ld_append(cm.ld, repack ? packed.data() : rows.data(), ldr, pn.bs, 0, flip, pn.cols.data()));
    sout << "done\n";
  }
}

// write_snplist (Data.cpp:3862-3885)
static void write_snplist(const LdCommon& cm) {
  const LdColumns& lc = cm.lc;
  std::ofstream f(cm.out + ".snplist");
  if (!f) throw std::runtime_error("cannot write file : " + cm.out + ".snplist");
  for (auto& id : lc.col_ids) f << id << "\n";
  if (std::find(lc.absent.begin(), lc.absent.end(), (uint8_t)1) == lc.absent.end()) return;
  sout << " WARNING: there were variants not found in the data; these were kept in the LD matrix.\n  + list is written to [" << cm.out << ".forcedIn.snplist]\n";
  std::ofstream ff(cm.out + ".forcedIn.snplist");
  if (!ff) throw std::runtime_error("cannot write file : " + cm.out + ".forcedIn.snplist");
  for (int64_t c = 0; c < cm.M; ++c) if (lc.absent[c]) ff << lc.col_ids[c] << "\n";
}

constexpr double LD_TOL = 1e-8;      // params.tol, Regenie.hpp:226

// the first line of the text file under --skip-scaleG (setup_output, Data.cpp:1992): number of columns, params.n_samples
static std::string gtg_header(const LdCommon& cm) { return std::to_string(cm.M) + " " + std::to_string(cm.r.N) + "\n"; }

// the dense text matrix: correlations, or under --skip-scaleG the header line and the unscaled matrix after the diagonal rules
static void write_corr_text(const LdCommon& cm) {
  const int64_t M = cm.M;
  std::vector<double> R((size_t)M * M);
  cm.check(rg_ld_finish(cm.ld, cm.p.skip_scaleG ? RG_LD_GTG_F64 : RG_LD_CORR_F64, R.data(), 0, LD_TOL, NUMTOL));
  sout << "\n** writing to file **\n";
  std::vector<std::string> lines((size_t)M);
  parallel_for((int)M, cm.nthreads, [&](int i) {
    std::string& s = lines[i];
    s.reserve((size_t)M * 10);
    for (int64_t j = 0; j < M; ++j) { if (j) s.push_back(' '); fmt_sig6(R[(size_t)i * M + j], s); }
  });
  std::ofstream f(cm.out);
  if (!f) throw std::runtime_error("cannot write file : " + cm.out);
  if (cm.p.skip_scaleG) f << gtg_header(cm);
  for (int64_t i = 0; i < M; ++i) { if (i) f << "\n"; f << lines[i]; }      // IOFormat(..., " ", "\n", "", "", "", ""): no newline at the end
  f.flush();
  if (!f) throw std::runtime_error("error while writing file : " + cm.out + " (disk full?)");
}

// --skip-scaleG --sparse-thr t (Data.cpp:4407-4421): the header line, the M standard deviations on one line, then `i j r` (1-based) per
// pair i < j with |r| >= t, in row-major order.  The matrix is thresholded on the device; only the triplets come back.
static void write_corr_sparse(const LdCommon& cm) {
  const int64_t M = cm.M;
  std::vector<double> sd((size_t)M);
  int64_t count = 0;
  cm.check(rg_ld_finish_sparse(cm.ld, cm.p.sparse_thr, LD_TOL, NUMTOL, sd.data(), &count));
  std::vector<int32_t> row((size_t)count), col((size_t)count);
  std::vector<double> val((size_t)count);
  cm.check(rg_ld_sparse_fetch(cm.ld, row.data(), col.data(), val.data()));
  sout << "\n** writing to file **\n";
  std::ofstream f(cm.out);
  if (!f) throw std::runtime_error("cannot write file : " + cm.out);
  std::string s = gtg_header(cm);
  for (int64_t c = 0; c < M; ++c) { if (c) s.push_back(' '); fmt_sig6(sd[c], s); }
  s.push_back('\n');
  f << s;
  char buf[80];
  s.clear();
  for (int64_t k = 0; k < count; ++k) {      // (the stream's default format of a double is %g)
    s.append(buf, (size_t)snprintf(buf, sizeof(buf), "%d %d %g\n", row[k] + 1, col[k] + 1, val[k]));
    if (s.size() > (1u << 20)) { f << s; s.clear(); }
  }
  f << s;
  f.flush();
  if (!f) throw std::runtime_error("error while writing file : " + cm.out + " (disk full?)");
  sout << "  + " << count << " pairs at or above the threshold " << cm.p.sparse_thr << "\n";
}

static void write_corr_binary(const LdCommon& cm) {
  const int64_t M = cm.M;
  std::vector<uint16_t> v((size_t)M * (M - 1) / 2);
  uint16_t dummy = 0;
  cm.check(rg_ld_finish(cm.ld, RG_LD_R2_U16, v.empty() ? &dummy : v.data(), 0, LD_TOL, NUMTOL));
  sout << "\n** writing to file **\n";
  std::ofstream f(cm.out, std::ios::binary);
  if (!f) throw std::runtime_error("cannot write file : " + cm.out);
  const int32_t hdr[2] = {(int32_t)cm.r.N, (int32_t)M};      // params.n_samples (the kept samples of the file), number of columns
  f.write((const char*)hdr, sizeof(hdr));
  f.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(uint16_t)));
  f.flush();
  if (!f) throw std::runtime_error("error while writing file : " + cm.out + " (disk full?)");
}

static int run_ld(Run& r, std::chrono::steady_clock::time_point t_start) {
  const Params& p = r.p;
  if (r.dosage_mode && !p.ld_dosages)
    throw std::runtime_error("--compute-corr with dosage input (a .pgen with a dosage track) is not built into the default mode, which computes the LD matrix from hard calls: add --ld-dosages for the LD matrix of the dosages themselves.");
  if (p.ld_dosages && !r.dosage_mode) throw std::runtime_error("--ld-dosages needs dosage input (--bgen, or a .pgen with a dosage track).");
  {  // set_blocks_for_testing (Data.cpp:2155-2161)
    std::set<int> chrs(r.snp_chrom.begin(), r.snp_chrom.end());
    if (chrs.size() > 1) throw std::runtime_error("can only compute LD matrix for a single chromosome (use --chr/--chrList/--range).");
  }
  LdCommon cm(r);
  if (r.dosage_mode) {      // --bgen, or a .pgen with a dosage track: Data::compute_ld_dosages (Data.cpp:3887-3980)
    DosagePanels(cm).append_all();
  } else {
    append_hard_call_panels(cm);
    sout << "\n** computing LD matrix " << (p.skip_scaleG ? "(=GtG) " : "") << "**\n";      // Data.cpp:4374
  }
  write_snplist(cm);
  if (p.skip_scaleG && p.sparse_thr > 0) write_corr_sparse(cm);      // (--sparse-thr 0: no sparsifying)
  else if (p.corr_text) write_corr_text(cm);
  else write_corr_binary(cm);
  sout << " -> Gram kernel " << rg_ld_last_kernel_ms(cm.ld) << " ms (" << rg_ld_last_tiles(cm.ld) << " tiles of 128 x 128 over " << cm.sm.n << " samples)\n";
  sout << "\nElapsed time : " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() << "s\nEnd of run\n";
  return 0;
}

static const bool ld_registered = (run_ld_entry = &run_ld, true);

}  // namespace rgdrv
