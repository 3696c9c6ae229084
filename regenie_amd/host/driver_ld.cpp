// regenie-amd, the C++ host driver (see driver.h): `--step 2 --compute-corr`, the LD matrix of a region (Data::ld_comp, Data.cpp:3807-3848).
//
// The host keeps what the reference's host does around print_ld: which variant takes which column (check_in_map_from_files /
// check_ld_list, Geno.cpp:1343-1380, :1443-1453), the variant lists (write_snplist, Data.cpp:3862-3885), reading the 2-bit rows in
// panels of --bsize (or, for --bgen and .pgen dosages, the exact integer dosages as uint16 rows), the two output formats.
// Everything numeric -- the integer Gram of the panels, the covariate projection, the
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
  if (r.dosage_mode && !p.ld_dosages)
    throw std::runtime_error("--compute-corr with dosage input (a .pgen with a dosage track) is not built into the default mode, which computes the LD matrix from hard calls: add --ld-dosages for the LD matrix of the dosages themselves.");
  if (p.ld_dosages && !r.dosage_mode) throw std::runtime_error("--ld-dosages needs dosage input (--bgen, or a .pgen with a dosage track).");
  const bool dos = r.dosage_mode;      // --bgen, or a .pgen with a dosage track: Data::compute_ld_dosages (Data.cpp:3887-3980)
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
  const char* runmode = dos ? "in dosage mode" : "in hard-call mode";
  if (p.corr_text) sout << " * computing correlation matrix " << runmode << "\n  + output to text file [" << out << "]\n";      // setup_output, Data.cpp:1986-2004
  else sout << " * computing correlation matrix " << runmode << " (storing R^2 values)\n  + output to binary file [" << out << "]\n";
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
  if (dos) {
    sout << "** Computing LD matrix **\n";
    if (nchunks > 0) sout << "  -> splitting across " << nchunks << " SV blocks\n";
  } else sout << "** reading in single variant genotypes **\n  + " << present.size() << " variants in total split across " << nchunks << " blocks\n";
  const int fd = (r.pgen || dos) ? -1 : open((p.bed + ".bed").c_str(), O_RDONLY);
  if (!r.pgen && !dos && fd < 0) throw std::runtime_error("cannot read bed file");
  struct FdGuard { int fd; ~FdGuard() { if (fd >= 0) close(fd); } } fdg{fd};
  const int flip = (!r.pgen && p.ref_first) ? 1 : 0;      // .pgen rows always count ALT (as run_step2)
  int nthreads = p.threads > 0 ? p.threads : std::max(1, usable_cpus() - 1);
  nthreads = std::max(1, std::min(nthreads, 64));
  std::vector<uint8_t> rows, packed;
  std::vector<int64_t> vidx;
  std::vector<int32_t> cols;
  // get_G_svs(int, int) (Data.cpp:4049-4090) for dosages: the block as uint16 rows of exact integers -- 8-bit .bgen probabilities in
  // units of 1 / 255 (the inflated blocks walked as the Step-2 read-ahead walks them), .pgen dosages in units of 1 / 16384 -- which the
  // library splits into int8 digit planes.  A value that is no such integer is an error: there is no second route.
  std::vector<uint16_t> g16;
  std::vector<double> dbuf;
  std::vector<uint8_t> raw;
  int64_t block_bytes = 0;
  // zlib files: the stored streams go to the device decoder (rg_bgen_dev_decode), whose uint16 rows are appended where they lie; a
  // block with a variant the decoder turns down (status != 0), zstd and uncompressed files take the host route below
  rg_bgen_dev* bdev = nullptr;
  struct DevGuard { rg_bgen_dev*& d; ~DevGuard() { if (d && full_teardown()) rg_bgen_dev_destroy(d); } } devg{bdev};
  std::vector<uint8_t> comp;
  int64_t dev_blocks = 0, host_blocks = 0;
  if (dos && r.bgenh) {
    if (rg_bgen_block_bytes(r.bgenh, &block_bytes) != RG_BGEN_OK) throw std::runtime_error(rg_bgen_last_error(r.bgenh));
    block_bytes = (block_bytes + 63) / 64 * 64;
    int32_t bcomp = 0;
    rg_bgen_info(r.bgenh, nullptr, nullptr, &bcomp, nullptr);
    if (bcomp == 1 && rg_bgen_dev_create(&bdev, p.device) == RG_BGEN_OK &&
        rg_bgen_dev_set_samples(bdev, r.n_file, n, identity ? nullptr : file_idx.data(), 0, nullptr) != RG_BGEN_OK) {
      rg_bgen_dev_destroy(bdev);
      bdev = nullptr;
    }
  }
  // false: the block is left to the host route
  auto device_block = [&](int64_t j0, int bs) -> bool {
    if (!bdev) return false;
    int64_t need = 0;
    if (rg_bgen_compressed_bytes(r.bgenh, bs, vidx.data(), &need) != RG_BGEN_OK) return false;
    if ((int64_t)comp.size() < need) comp.resize((size_t)(need + need / 4));
    std::vector<int64_t> off(bs);
    std::vector<int32_t> clen(bs), ulen(bs), status(bs), maxq(bs);
    if (rg_bgen_read_compressed(r.bgenh, bs, vidx.data(), comp.data(), (int64_t)comp.size(), off.data(), clen.data(), ulen.data(), std::min(nthreads, 32)) != RG_BGEN_OK)
      return false;
    rg_bgen_dev_out o;
    memset(&o, 0, sizeof(o));
    o.max_q = maxq.data(); o.status = status.data();
    if (rg_bgen_dev_decode(bdev, 0, bs, comp.data(), off[bs - 1] + clen[bs - 1], off.data(), clen.data(), ulen.data(), p.ref_first ? 1 : 0, &o) != RG_BGEN_OK) return false;
    for (int j = 0; j < bs; ++j) if (status[j] != 0) return false;
    for (int j = 0; j < bs; ++j)
      if (maxq[j] > 510)
        throw std::runtime_error("variant '" + r.snp_ids[present[j0 + j]] + "' has a dosage that is not an integer in [0, 510] in units of 1/255 (probabilities that add up to more than 1): the LD matrix of such dosages is not built.");
    if (!o.g16 || o.ld16 < n) return false;
    ldcheck(rg_ld_append_int(ld, o.g16, o.ld16, bs, 1, 255, cols.data()));
    return true;
  };
  for (int b = 0; dos && b < nchunks; ++b) {
    const int64_t j0 = (int64_t)b * p.bsize;
    const int bs = (int)std::min<int64_t>(p.bsize, (int64_t)present.size() - j0);
    sout << "     - row " << b + 1 << "\n" << std::flush;
    cols.resize(bs);
    vidx.resize(bs);
    for (int j = 0; j < bs; ++j) { vidx[j] = r.snp_offset[present[j0 + j]]; cols[j] = col_of_variant[present[j0 + j]]; }
    if (r.bgenh && device_block(j0, bs)) { ++dev_blocks; continue; }
    ++host_blocks;
    g16.resize((size_t)bs * n);
    std::vector<int> bad(bs, 0);
    int scale = 255;
    if (r.bgenh) {
      raw.resize((size_t)bs * block_bytes);
      if (rg_bgen_read_blocks(r.bgenh, bs, vidx.data(), raw.data(), block_bytes, std::min(nthreads, 32)) != RG_BGEN_OK) throw std::runtime_error(rg_bgen_last_error(r.bgenh));
      const bool rf = p.ref_first;
      parallel_for(bs, nthreads, [&](int j) {
        const uint8_t* blk = raw.data() + (size_t)j * block_bytes;
        const uint8_t* ploidy = blk + 8;
        const uint8_t* pr = blk + 10 + r.n_file;
        uint16_t* q = g16.data() + (size_t)j * n;
        for (int64_t k = 0; k < n; ++k) {
          const int64_t i = file_idx[k];
          if (ploidy[i] & 0x80) { q[k] = 0xFFFFu; continue; }
          const unsigned b0 = pr[2 * i], b1 = pr[2 * i + 1];
          // G * 255 = prob1 + 2 prob0, or with --ref-first prob1 + 2 max(1 - prob0 - prob1, 0) (Geno.cpp:2286-2290)
          const unsigned qi = rf ? b1 + 2u * (b0 + b1 < 255u ? 255u - b0 - b1 : 0u) : b1 + 2u * b0;
          if (qi > 510u) { bad[j] = 1; break; }      // prob0 + prob1 > 1 in the file: max_q > 510
          q[k] = (uint16_t)qi;
        }
      });
    } else {
      scale = 16384;
      dbuf.resize((size_t)bs * r.n_file);
      if (rg_pgen_read_dosage_rows(r.pgen, bs, vidx.data(), dbuf.data(), r.n_file) != RG_PGEN_OK) throw std::runtime_error(rg_pgen_last_error(r.pgen));
      parallel_for(bs, nthreads, [&](int j) {
        const double* d = dbuf.data() + (size_t)j * r.n_file;
        uint16_t* q = g16.data() + (size_t)j * n;
        for (int64_t k = 0; k < n; ++k) {
          const double g = d[file_idx[k]];
          if (g == -3.0) { q[k] = 0xFFFFu; continue; }
          const double v = g * 16384.0, rv = std::nearbyint(v);
          if (std::fabs(v - rv) > 1e-6 || rv < 0 || rv > 2.0 * 16384.0) { bad[j] = 1; break; }
          q[k] = (uint16_t)rv;
        }
      });
    }
    for (int j = 0; j < bs; ++j)
      if (bad[j])
        throw std::runtime_error("variant '" + r.snp_ids[present[j0 + j]] + "' has a dosage that is not an integer in [0, " + std::to_string(2 * scale) + "] in units of 1/" +
                                 std::to_string(scale) + (r.bgenh ? " (probabilities that add up to more than 1)" : "") + ": the LD matrix of such dosages is not built.");
    ldcheck(rg_ld_append_int(ld, g16.data(), n, bs, 0, scale, cols.data()));
  }
  if (dos && r.bgenh) sout << "     - " << dev_blocks << " blocks decoded on the device, " << host_blocks << " on the host\n";
  for (int b = 0; !dos && b < nchunks; ++b) {
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

  if (!dos) sout << "\n** computing LD matrix **\n";
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
