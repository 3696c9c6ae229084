// regenie-amd, the C++ host driver (see driver.h): `--step 2 --compute-corr`, the LD matrix of a region (Data::ld_comp, Data.cpp:3807-3848).
//
// The host keeps what the reference's host does around print_ld: which variant takes which column (check_in_map_from_files /
// check_ld_list, Geno.cpp:1343-1380, :1443-1453), the variant lists (write_snplist, Data.cpp:3862-3885), reading the 2-bit rows in
// panels of --bsize, the two output formats.  Everything numeric -- the integer Gram of the panels, the covariate projection, the
// diagonal rules, the scaling and the 16-bit quantisation -- is the library's (include/rg_ld.h); there is no CPU path.
#include "driver.h"

namespace rgdrv {

// Eigen's operator<< at StreamPrecision (6 significant digits), as print_ld writes the text matrix
static void fmt_sig6(double v, std::string& out) {
  char buf[40];
  if (v == 0) v = 0.0;      // (no "-0")
  const int k = snprintf(buf, sizeof(buf), "%.6g", v);
  out.append(buf, (size_t)k);
}

static int run_ld(Run& r, std::chrono::steady_clock::time_point t_start) {
  const Params& p = r.p;
  if (r.dosage_mode) throw std::runtime_error("--compute-corr with dosage input (a .pgen with a dosage track) is not built: the LD matrix is computed from hard calls.");
  {  // set_blocks_for_testing (Data.cpp:2155-2161)
    std::set<int> chrs(r.snp_chrom.begin(), r.snp_chrom.end());
    if (chrs.size() > 1) throw std::runtime_error("can only compute LD matrix for a single chromosome (use --chr/--chrList/--range).");
  }
  const int64_t N = r.N;
  const int C = r.C;
  // the columns: with --extract --forcein-vars the lines of the extract file in order, duplicates ignored, IDs the genotype file does
  // not have included (zero columns); otherwise the kept variants in file order
  std::vector<std::string> col_ids;
  std::vector<int32_t> col_of_variant(r.snp_ids.size(), -1);
  std::vector<uint8_t> absent;
  if (p.forcein_vars) {
    std::unordered_map<std::string, int32_t> order;
    TextIn f(p.extract[0]);
    if (!f) throw std::runtime_error("cannot read file : " + p.extract[0]);
    std::string line;
    while (std::getline(f, line)) {
      auto t = split_ws(line);
      if (t.empty()) throw std::runtime_error("incorrectly formatted file.");
      if (!t[0].empty() && t[0].back() == '\r') t[0].pop_back();
      if (order.count(t[0])) continue;
      order.emplace(t[0], (int32_t)col_ids.size());
      col_ids.push_back(t[0]);
    }
    absent.assign(col_ids.size(), 1);
    for (size_t j = 0; j < r.snp_ids.size(); ++j) {
      auto it = order.find(r.snp_ids[j]);
      if (it == order.end() || !absent[it->second]) continue;      // (a second variant with the same ID is skipped, Geno.cpp:590-593)
      col_of_variant[j] = it->second;
      absent[it->second] = 0;
    }
  } else {
    std::unordered_set<std::string> seen;
    for (size_t j = 0; j < r.snp_ids.size(); ++j) {
      if (!seen.insert(r.snp_ids[j]).second) continue;
      col_of_variant[j] = (int32_t)col_ids.size();
      col_ids.push_back(r.snp_ids[j]);
    }
    absent.assign(col_ids.size(), 0);
  }
  const int64_t M = (int64_t)col_ids.size();
  if (M < 1) throw std::runtime_error("no variant left to include in analysis.");
  std::vector<int64_t> present;      // variants that take a column, in file order
  for (size_t j = 0; j < r.snp_ids.size(); ++j) if (col_of_variant[j] >= 0) present.push_back((int64_t)j);

  sout << std::left << std::setw(20) << " * block size" << ": [" << p.bsize << "]\n";
  const std::string out = p.out + ".corr";
  if (p.corr_text) sout << " * computing correlation matrix in hard-call mode\n  + output to text file [" << out << "]\n";      // setup_output, Data.cpp:1986-2004
  else sout << " * computing correlation matrix in hard-call mode (storing R^2 values)\n  + output to binary file [" << out << "]\n";
  sout << "  + list of snps written to [" << out << ".snplist]\n  + n_snps = " << M << "\n\n";

  // analysed samples and the compact, sample-fastest covariate basis (as run_step2)
  std::vector<int64_t> an;
  for (int64_t i = 0; i < N; ++i) if (r.ain[i]) an.push_back(i);
  const int64_t n = (int64_t)an.size();
  std::vector<double> Xc((size_t)C * n);
  for (int c = 0; c < C; ++c) for (int64_t k = 0; k < n; ++k) Xc[(size_t)c * n + k] = r.X[(size_t)c * N + an[k]];
  std::vector<int64_t> file_idx(n, 0);
  {
    int64_t kept = 0, k = 0;
    for (int64_t i = 0; i < r.n_file && k < n; ++i) {
      if (r.ind_ignore[i]) continue;
      if (kept == an[k]) file_idx[k++] = i;
      ++kept;
    }
  }
  bool identity = n == r.n_file;
  for (int64_t k = 0; identity && k < n; ++k) identity = file_idx[k] == k;

  rg_ld_ctx* ld = nullptr;
  struct Guard { rg_ld_ctx*& h; ~Guard() { if (h && full_teardown()) rg_ld_destroy(h); } } guard{ld};
  if (rg_ld_create(&ld, p.device, n, C, (int32_t)M) != RG_LD_OK) {
    const std::string m = ld ? rg_ld_last_error(ld) : "rg_ld_create failed";
    throw std::runtime_error(m.find("no HIP device") != std::string::npos ? "no MI355X / HIP device available (rg_ld_create failed)" : m);
  }
  auto ldcheck = [&](int rc) { if (rc != RG_LD_OK) throw std::runtime_error(rg_ld_last_error(ld)); };
  ldcheck(rg_ld_set_basis(ld, Xc.data()));
  {
    std::vector<int32_t> forced;
    for (int64_t c = 0; c < M; ++c) if (absent[c]) forced.push_back((int32_t)c);
    if (!forced.empty()) ldcheck(rg_ld_force_columns(ld, (int32_t)forced.size(), forced.data()));
  }

  // get_G_svs (Data.cpp:4227-4304): the rows in panels of --bsize
  const int nchunks = (int)((present.size() + p.bsize - 1) / p.bsize);
  sout << "** reading in single variant genotypes **\n  + " << present.size() << " variants in total split across " << nchunks << " blocks\n";
  const int fd = r.pgen ? -1 : open((p.bed + ".bed").c_str(), O_RDONLY);
  if (!r.pgen && fd < 0) throw std::runtime_error("cannot read bed file");
  struct FdGuard { int fd; ~FdGuard() { if (fd >= 0) close(fd); } } fdg{fd};
  const int flip = (!r.pgen && p.ref_first) ? 1 : 0;      // .pgen rows always count ALT (as run_step2)
  int nthreads = p.threads > 0 ? p.threads : std::max(1, usable_cpus() - 1);
  nthreads = std::max(1, std::min(nthreads, 64));
  std::vector<uint8_t> rows, packed;
  std::vector<int64_t> vidx;
  std::vector<int32_t> cols;
  for (int b = 0; b < nchunks; ++b) {
    const int64_t j0 = (int64_t)b * p.bsize;
    const int bs = (int)std::min<int64_t>(p.bsize, (int64_t)present.size() - j0);
    sout << "  block [" << b + 1 << "/" << nchunks << "] : reading in genotypes..." << std::flush;
    rows.resize((size_t)bs * r.bpr);
    cols.resize(bs);
    vidx.resize(bs);
    for (int j = 0; j < bs; ++j) { vidx[j] = r.snp_offset[present[j0 + j]]; cols[j] = col_of_variant[present[j0 + j]]; }
    if (r.pgen) {
      if (rg_pgen_read_bed_rows(r.pgen, bs, vidx.data(), rows.data(), r.bpr) != RG_PGEN_OK) throw std::runtime_error(rg_pgen_last_error(r.pgen));
    } else {
      std::atomic<int> failed(0);
      parallel_for(bs, std::min(nthreads, 8), [&](int j) {
        int64_t got = 0;
        while (got < r.bpr) {
          const ssize_t k = pread(fd, rows.data() + (size_t)j * r.bpr + got, (size_t)(r.bpr - got), 3 + vidx[j] * r.bpr + got);
          if (k <= 0) { failed = 1; return; }
          got += k;
        }
      });
      if (failed) throw std::runtime_error("cannot read bed file");
    }
    const uint8_t* src = rows.data();
    int64_t ldr = r.bpr;
    if (!identity) {      // the 2-bit codes of the analysed samples, in their order
      ldr = (n + 3) / 4;
      packed.assign((size_t)bs * ldr, 0);
      parallel_for(bs, nthreads, [&](int j) {
        const uint8_t* row = rows.data() + (size_t)j * r.bpr;
        uint8_t* dst = packed.data() + (size_t)j * ldr;
        for (int64_t k = 0; k < n; ++k) {
          const int64_t i = file_idx[k];
          dst[k >> 2] |= (uint8_t)(((row[i >> 2] >> (2 * (i & 3))) & 3) << (2 * (k & 3)));
        }
      });
      src = packed.data();
    }
    ldcheck(rg_ld_append(ld, src, ldr, bs, 0, flip, cols.data()));
    sout << "done\n";
  }

  sout << "\n** computing LD matrix **\n";
  {  // write_snplist (Data.cpp:3862-3885)
    std::ofstream f(out + ".snplist");
    if (!f) throw std::runtime_error("cannot write file : " + out + ".snplist");
    for (auto& id : col_ids) f << id << "\n";
    if (std::find(absent.begin(), absent.end(), (uint8_t)1) != absent.end()) {
      sout << " WARNING: there were variants not found in the data; these were kept in the LD matrix.\n  + list is written to [" << p.out << ".corr.forcedIn.snplist]\n";
      std::ofstream ff(p.out + ".corr.forcedIn.snplist");
      if (!ff) throw std::runtime_error("cannot write file : " + p.out + ".corr.forcedIn.snplist");
      for (int64_t c = 0; c < M; ++c) if (absent[c]) ff << col_ids[c] << "\n";
    }
  }
  const double tol = 1e-8;      // params.tol, Regenie.hpp:226
  if (p.corr_text) {
    std::vector<double> R((size_t)M * M);
    ldcheck(rg_ld_finish(ld, RG_LD_CORR_F64, R.data(), 0, tol, NUMTOL));
    sout << "\n** writing to file **\n";
    std::vector<std::string> lines((size_t)M);
    parallel_for((int)M, nthreads, [&](int i) {
      std::string& s = lines[i];
      s.reserve((size_t)M * 10);
      for (int64_t j = 0; j < M; ++j) { if (j) s.push_back(' '); fmt_sig6(R[(size_t)i * M + j], s); }
    });
    std::ofstream f(out);
    if (!f) throw std::runtime_error("cannot write file : " + out);
    for (int64_t i = 0; i < M; ++i) { if (i) f << "\n"; f << lines[i]; }      // IOFormat(..., " ", "\n", "", "", "", ""): no newline at the end
    f.flush();
    if (!f) throw std::runtime_error("error while writing file : " + out + " (disk full?)");
  } else {
    std::vector<uint16_t> v((size_t)M * (M - 1) / 2);
    uint16_t dummy = 0;
    ldcheck(rg_ld_finish(ld, RG_LD_R2_U16, v.empty() ? &dummy : v.data(), 0, tol, NUMTOL));
    sout << "\n** writing to file **\n";
    std::ofstream f(out, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write file : " + out);
    const int32_t hdr[2] = {(int32_t)N, (int32_t)M};      // params.n_samples (the kept samples of the file), number of columns
    f.write((const char*)hdr, sizeof(hdr));
    f.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(uint16_t)));
    f.flush();
    if (!f) throw std::runtime_error("error while writing file : " + out + " (disk full?)");
  }
  sout << " -> Gram kernel " << rg_ld_last_kernel_ms(ld) << " ms (" << rg_ld_last_tiles(ld) << " tiles of 128 x 128 over " << n << " samples)\n";
  sout << "\nElapsed time : " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() << "s\nEnd of run\n";
  return 0;
}

static const bool ld_registered = (run_ld_entry = &run_ld, true);

}  // namespace rgdrv
