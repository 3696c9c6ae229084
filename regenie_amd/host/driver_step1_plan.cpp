// regenie-amd, the C++ host driver (see driver.h): the parts of `--step 1` that make no device call (driver_step1.h) -- the plan of a run,
// the `--split-l0` exit and the writer of the per-phenotype outputs.
#include "driver_step1.h"
#include "fmt_g6.h"

namespace rgdrv {

// set_parallel_l0 / write_l0_master (Data.cpp:232-309): master + per-job variant lists
int split_l0(const Run& r) {
  const Params& p = r.p;
  std::map<int, int> cn;
  for (int c : r.snp_chrom) cn[c]++;
  std::vector<int> bsizes;     // block sizes in traversal order
  for (int c : r.chr_read) {
    const int n = cn.count(c) ? cn[c] : 0;
    const int nbc = (n + p.bsize - 1) / p.bsize;
    for (int bb = 0; bb < nbc; ++bb) bsizes.push_back(std::min(p.bsize, n - bb * p.bsize));
  }
  const int total = (int)bsizes.size();
  int njobs = p.njobs;
  sout << " * running level 0 in parallel across " << total << " genotype blocks\n";
  if (njobs <= 1) throw std::runtime_error("number of jobs must be >1.");
  if (njobs > total) { sout << "   -WARNING: Number of jobs cannot be greater than number of blocks.\n"; njobs = total; }
  sout << "   -using " << njobs << " jobs\n   -master file written to [" << p.split_file << ".master]\n";
  sout << "   -variant list files written to [" << p.split_file << "_job*.snplist]\n";
  std::ofstream mf(p.split_file + ".master");
  if (!mf) throw std::runtime_error("cannot write file : " + p.split_file + ".master");
  mf << r.snp_chrom.size() << " " << p.bsize << std::endl;
  const int nall = total / njobs, rem = total - nall * njobs;
  int b = 0; size_t scount = 0;
  for (int j = 0; j < njobs; ++j) {
    const int bt = nall + (j < rem ? 1 : 0);
    int ns = 0;
    for (int t = 0; t < bt; ++t) ns += bsizes[b++];
    const std::string fname = p.split_file + "_job" + std::to_string(j + 1);
    mf << fname << " " << bt << " " << ns << std::endl;
    std::ofstream sf(fname + ".snplist");
    if (!sf) throw std::runtime_error("cannot write file : " + fname + ".snplist");
    for (int t = 0; t < ns; ++t) sf << r.snp_ids[scount + t] << "\n";
    scount += ns;
  }
  sout << "\nEnd of run\n";
  return 0;
}

// --setl0 / --setl1 (get_unit_params, Regenie.cpp:1477-1495): sorted, duplicates removed, every value inside (0, 1)
static std::vector<double> unit_params(std::vector<double> v, const char* opt) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  for (double x : v) if (!(x > 0.0 && x < 1.0)) throw std::runtime_error(std::string("must specify values for ") + opt + " in (0,1).");
  return v;
}
static std::vector<double> ridge_grid(int n) {  // set_ridge_params (Regenie.cpp:1497-1508)
  if (n < 2) throw std::runtime_error("number of ridge parameters must be at least 2 (=" + std::to_string(n) + ")");
  std::vector<double> v(n);
  for (int i = 0; i < n; ++i) v[i] = (double)i / (n - 1);
  v[0] = 0.01; v[n - 1] = 0.99;
  return v;
}

Step1Plan plan_step1(Run& r) {
  const Params& p = r.p;
  const int64_t N = r.N;
  const int P = r.P;
  Step1Plan pl;
  std::vector<Blk>& blocks = pl.blocks;
  // set_blocks (Data.cpp:311-398)
  std::map<int, int> chr_nsnp;
  for (int c : r.snp_chrom) chr_nsnp[c]++;
  {
    int64_t pos = 0;
    int left = p.n_block;      // --nb: at most that many blocks, taken chromosome by chromosome; the variants past them are not analysed
    for (int c : r.chr_read) {
      const int n = chr_nsnp.count(c) ? chr_nsnp[c] : 0;
      int nb = (n + p.bsize - 1) / p.bsize;
      if (p.n_block > 0) { nb = std::min(nb, left); left -= nb; }
      for (int bb = 0; bb < nb; ++bb) blocks.push_back({c, pos + (int64_t)bb * p.bsize, std::min(p.bsize, n - bb * p.bsize)});
      pos += n;
    }
  }
  const int B = pl.B = (int)blocks.size();
  if (B == 0) throw std::runtime_error("total number of blocks must be > 0.");
  const int64_t M = pl.M = p.run_l0 ? r.parallel_nGeno : (int64_t)r.snp_chrom.size();   // --run-l0: global count (Data.cpp:607)
  if (p.run_l0 && (B != r.parallel_nBlocks || (int)r.snp_chrom.size() != r.parallel_nSnps))
    throw std::runtime_error("number of blocks/variants in the job's snplist doesn't match the master file.");
  if (p.run_l1) prep_parallel_l1(r, B, (int64_t)r.snp_chrom.size());
  std::vector<double>&h0 = pl.h0, &h1 = pl.h1, &lambda = pl.lambda;
  h0 = unit_params(p.setl0, "--l0"); h1 = unit_params(p.setl1, "--l1");
  if (h0.empty()) h0 = ridge_grid(p.n_ridge_l0);
  if (h1.empty()) h1 = ridge_grid(p.n_ridge_l1);
  const int R0 = pl.R0 = (int)h0.size(), R1 = pl.R1 = (int)h1.size(), L = pl.L = B * R0;
  lambda.resize(R0);
  for (int i = 0; i < R0; ++i) lambda[i] = (double)M * (1 - h0[i]) / h0[i];  // Data.cpp:607
  sout << std::left << std::setw(20) << " * block size" << ": [" << p.bsize << "]\n";
  sout << std::left << std::setw(20) << " * # blocks" << ": [" << B << "] for " << M << " variants\n";
  sout << std::left << std::setw(20) << " * # CV folds" << ": [" << p.cv_folds << "]\n";
  if (p.loocv) sout << std::left << std::setw(20) << " * LOOCV" << ": [enabled]\n";
  sout << std::left << std::setw(20) << " * ridge data_l0" << ": [ " << R0 << " : ";
  for (double h : h0) sout << h << " ";
  sout << "]\n" << std::left << std::setw(20) << " * ridge data_l1" << ": [ " << R1 << " : ";
  for (double h : h1) sout << h << " ";
  sout << "]\n";

  bool& use_loocv = pl.use_loocv = p.loocv;
  if (p.bt && !use_loocv && r.n_analyzed < 5000) {  // Data.cpp:353-356
    sout << "   -WARNING: Sample size is less than 5,000 so using LOOCV instead of " << p.cv_folds << "-fold CV.\n";
    use_loocv = true;
  }
  // set_folds (Data.cpp:401-426)
  std::vector<int32_t>& cv_sizes = pl.cv_sizes;
  cv_sizes.assign(p.cv_folds, 1);
  if (!use_loocv) {
    const int64_t target = r.n_analyzed / p.cv_folds;
    if (target < 1) throw std::runtime_error("not enough samples are present for " + std::to_string(p.cv_folds) + "-fold CV.");
    int64_t cnt = 0, cum = 0;
    int cur = 0;
    for (int64_t i = 0; i < N; ++i) {
      if (r.ain[i]) cnt++;
      if (cnt == target) { cv_sizes[cur] = (int32_t)(i - cum + 1); cum += cv_sizes[cur]; cnt = 0; cur++; }
      else if (cur == p.cv_folds - 1) { cv_sizes[cur] = (int32_t)(N - i); break; }
    }
  }

  if (!use_loocv && (p.bt || p.ct)) {  // Data.cpp:436-466: every fold needs both classes / at least one count
    int64_t start = 0;
    for (int f = 0; f < p.cv_folds; ++f) {
      for (int q = 0; q < r.P; ++q) {
        if (!r.pheno_pass[q]) continue;
        double sum = 0.0, n = 0.0;
        for (int64_t i = start; i < start + cv_sizes[f]; ++i)
          if (r.mask[(size_t)q * N + i]) { sum += r.Yraw[(size_t)q * N + i]; n += 1.0; }
        if (p.bt && (sum / n) * (1 - sum / n) < NUMTOL)
          throw std::runtime_error("one of the folds has only cases/controls for phenotype '" + r.pheno_names[q] +
                                   "'. Either use smaller #folds (option --cv) or use LOOCV (option --loocv).");
        if (p.ct && sum == 0)
          throw std::runtime_error("one of the folds has only zero counts for phenotype '" + r.pheno_names[q] +
                                   "'. Either use smaller #folds (option --cv) or use LOOCV (option --loocv).");
      }
      start += cv_sizes[f];
    }
  }

  // level-1 inputs shared by the ranks
  std::vector<double>&tau = pl.tau, &ct_rate = pl.ct_rate;
  tau.resize((size_t)P * R1);
  for (int q = 0; q < P; ++q)
    for (int j = 0; j < R1; ++j)   // check_l0, Step1_Models.cpp:2115-2117
      tau[(size_t)q * R1 + j] = (double)L * (1 - h1[j]) / h1[j] * (p.bt ? 3.0 / (M_PI * M_PI) : p.t2e && p.t2e_l1_pi6 ? 6.0 / (M_PI * M_PI) : 1.0);
  ct_rate.assign(P, 0.0);
  if (p.ct)  // Step1_Models.cpp:2101-2104: tau_j = L / log(1 + h_j / (rate (1 - h_j))); rate sums the raw column as it is
    for (int q = 0; q < P; ++q) {
      double sum = 0.0;
      for (int64_t i = 0; i < N; ++i) sum += r.Yraw[(size_t)q * N + i];
      ct_rate[q] = sum / r.neff[q];
      for (int j = 0; j < R1; ++j) tau[(size_t)q * R1 + j] = (double)L / std::log(1.0 + h1[j] / (ct_rate[q] * (1 - h1[j])));
    }
  for (int c : r.chr_read) {
    int nb = 0;
    for (auto& bl : blocks) nb += bl.chrom == c;
    if (nb > 0) { pl.cols_per_chr.push_back(nb * R0); pl.chroms.push_back(c); }
  }
  pl.nchr = (int)pl.chroms.size();
  pl.NCS = (p.bt || p.ct || p.t2e) ? 6 : 5;

  // block ranges of the ranks: floor(B/G) blocks each, the first B mod G one more (write_l0_master, Data.cpp:270-302)
  const int G = pl.G = p.gpus;
  pl.use_group = G > 1 || p.force_collectives;
  pl.bbeg.assign(G + 1, 0); pl.pbeg.assign(G + 1, 0);
  for (int g = 0; g < G; ++g) pl.bbeg[g + 1] = pl.bbeg[g] + B / G + (g < B % G ? 1 : 0);
  pl.pheno_sharded = pl.use_group && P >= G && !p.l1_shared;      // all-to-all by phenotype; else all-gather + shared level 1
  for (int g = 0; g < G; ++g) pl.pbeg[g + 1] = pl.pheno_sharded ? pl.pbeg[g] + P / G + (g < P % G ? 1 : 0) : P;
  if (!pl.pheno_sharded) pl.pbeg[0] = 0;
  return pl;
}

LocoWriter::LocoWriter(const Run& run, const Step1Plan& plan) : r(run), pl(plan), ph_log(run.P), ph_plist(run.P), ph_prslist(run.P), ph_firthlist(run.P) {
  const int64_t N = r.N;
  std::vector<int64_t> order(N);  // std::map<string,...> iteration order (Data.cpp:1934)
  for (int64_t i = 0; i < N; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return r.ids[a] < r.ids[b]; });
  header = "FID_IID ";
  for (int64_t i : order) if (r.ain[i]) { header += r.ids[i] + " "; kept_order.push_back(i); }
  header += "\n";
  fmt_threads = std::max(1, std::min(32, r.p.threads > 0 ? r.p.threads : usable_cpus() - 1));
  timing_on = getenv("RG_TIMING") != nullptr;
}

// one row of a .loco / .prs file (write_chr_row, Data.cpp:1951-1975): `<chr> v1 v2 ... \n`, NA where the phenotype is missing.
// The values are formatted by several threads over chunks of samples, in the default stream format of a double (%g, six
// significant digits: rgfmt::fmt_g6, a third of the time of std::to_chars(general, 6) and the same text); the pieces go to the
// file in order, without being joined first (115 MB per .loco file at 500,000 samples).
template <class V>
void LocoWriter::format_rows(int nrows, V&& value, const uint8_t* maskq, std::vector<std::string>& piece) const {
  const int64_t nk = (int64_t)kept_order.size();
  piece.assign((size_t)nrows * NCK, std::string());
  parallel_for(nrows * NCK, fmt_threads, [&](int t) {
    const int row = t / NCK, ck = t % NCK;
    const int64_t k0 = nk * ck / NCK, k1 = nk * (ck + 1) / NCK;
    std::string& o = piece[t];
    o.resize((size_t)(k1 - k0) * 14 + 32);          // a value is at most 13 characters ("-1.23456e-308") and a blank
    char* w = &o[0];
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t i = kept_order[k];
      if (maskq[i]) w = rgfmt::fmt_g6(value(row, i), w);
      else { w[0] = 'N'; w[1] = 'A'; w += 2; }
      *w++ = ' ';
    }
    o.resize((size_t)(w - &o[0]));
  });
}
void LocoWriter::write_row(std::ostream& f, const std::string& label, const std::vector<std::string>& piece, int row) const {
  f << label << " ";
  for (int ck = 0; ck < NCK; ++ck) f.write(piece[(size_t)row * NCK + ck].data(), (std::streamsize)piece[(size_t)row * NCK + ck].size());
  f << "\n";
}

// output of one phenotype (Data::output + write_predictions, Data.cpp:956-1129, :1795-1975)
void LocoWriter::emit(int q, const double* cs, int bestq, int conv, const double* pq /* [nchr][N] */) {
  const Params& p = r.p;
  const int64_t N = r.N;
  const int R1 = pl.R1, L = pl.L, nchr = pl.nchr;
  const std::vector<double>&tau = pl.tau, &ct_rate = pl.ct_rate;
  const std::vector<int>& chroms = pl.chroms;
  if (!r.pheno_pass[q]) return;   // null model did not converge: the trait is ignored, no table, no file, no list entry (Data.cpp:984)
  std::ostringstream lo;
  lo << "phenotype " << r.outnum(q) << " (" << r.pheno_names[q] << ") : ";
  if (!conv) {  // Data.cpp:1009-1014: on the header's own line
    lo << "Level 1 model did not converge. LOCO predictions calculations are skipped.\n\n";
    ph_log[q] = lo.str();
    return;
  }
  lo << "\n";
  for (int j = 0; j < R1 && p.t2e; ++j)   // Data.cpp:1043-1049: the penalty and the held-out deviance summed over the folds
    lo << " " << std::right << std::setw(5) << tau[(size_t)q * R1 + j] << " : Deviance = " << cs[5 * R1 + j] << (j == bestq ? "<- min value" : "") << "\n";
  for (int j = 0; j < R1 && !p.t2e; ++j) {
    const double neff = r.neff[q];
    double num = cs[4 * R1 + j] - cs[0 * R1 + j] * cs[1 * R1 + j] / neff;
    const double rsq = num * num / ((cs[2 * R1 + j] - cs[0 * R1 + j] * cs[0 * R1 + j] / neff) * (cs[3 * R1 + j] - cs[1 * R1 + j] * cs[1 * R1 + j] / neff));
    const double sse = cs[2 * R1 + j] + cs[3 * R1 + j] - 2 * cs[4 * R1 + j];
    double label = (double)L / (L + (p.bt ? M_PI * M_PI / 3.0 : 1.0) * tau[(size_t)q * R1 + j]);
    if (p.ct) {  // Data.cpp:1039-1054
      const double zv = std::exp((double)L / tau[(size_t)q * R1 + j]) - 1;
      label = ct_rate[q] * zv / (1 + ct_rate[q] * zv);
    }
    lo << "  " << std::right << std::setw(5) << label << " : Rsq = " << rsq;
    if (!p.ct) lo << ", MSE = " << sse / neff;
    if (p.bt || p.ct) lo << ", -logLik/N = " << cs[5 * R1 + j] / neff;
    if (j == bestq) lo << "<- min value";
    lo << "\n";
  }
  lo << "  * making predictions...writing LOCO predictions...";
  const std::string loco_fn = p.out + "_" + std::to_string(r.outnum(q)) + ".loco" + (p.gz ? ".gz" : "");  // Data.cpp:987
  std::vector<double> tot(N, 0.0);
  for (int c = 0; c < nchr; ++c)
    for (int64_t i = 0; i < N; ++i) tot[i] += pq[(size_t)c * N + i];
  std::vector<const double*> sub(p.nchrom, nullptr);
  for (int c = 0; c < nchr; ++c) if (chroms[c] >= 1 && chroms[c] <= p.nchrom) sub[chroms[c] - 1] = pq + (size_t)c * N;
  {
    const auto te0 = Clock::now();
    TextOut lf(loco_fn, p.gz);
    if (!lf) throw std::runtime_error("cannot write file : " + loco_fn);
    lf << header;
    std::vector<std::string> rows;
    format_rows(p.nchrom, [&](int row, int64_t i) { return tot[i] - (sub[row] ? sub[row][i] : 0.0); }, r.mask.data() + (size_t)q * N, rows);
    const auto te1 = Clock::now();
    for (int chr = 1; chr <= p.nchrom; ++chr) write_row(lf, std::to_string(chr), rows, chr - 1);
    if (timing_on) {
      const auto te2 = Clock::now();
      fprintf(stderr, "[timing] .loco of phenotype %d: totals + header + formatting %.0f ms, writing %.0f ms (%d formatting threads)\n", q + 1,
              ms_dbl(te0, te1), ms_dbl(te1, te2), fmt_threads);
    }
  }
  ph_plist[q] = r.pheno_names[q] + " " + (p.use_rel_path ? loco_fn : get_fullpath(loco_fn)) + "\n";
  if (p.print_prs) {
    const std::string prs_fn = p.out + "_" + std::to_string(r.outnum(q)) + ".prs" + (p.gz ? ".gz" : "");
    TextOut pf(prs_fn, p.gz);
    pf << header;
    std::vector<std::string> rows;
    format_rows(1, [&](int, int64_t i) { return tot[i]; }, r.mask.data() + (size_t)q * N, rows);
    write_row(pf, "0", rows, 0);
    ph_prslist[q] = r.pheno_names[q] + " " + (p.use_rel_path ? prs_fn : get_fullpath(prs_fn)) + "\n";
  }
  if (p.write_null_firth) {   // Data.cpp:1873-1902: the null approximate-Firth estimates of every chromosome (offset = its LOCO prediction),
                              // warm-started along the chromosomes from the null logistic estimates; read back by `--step 2 --use-null-firth`
    const std::string ffn = p.out + "_" + std::to_string(q + 1) + ".firth" + (p.gz ? ".gz" : "");
    lo << "writing null approximate Firth estimates...";
    const int Cn = r.C;
    std::vector<double> bh(r.bhat_start.begin() + (size_t)q * Cn, r.bhat_start.begin() + (size_t)(q + 1) * Cn), off(N);
    std::ostringstream body;
    bool conv = true;
    for (int chr = 1; chr <= p.nchrom && conv; ++chr) {
      for (int64_t i = 0; i < N; ++i) off[i] = tot[i] - (sub[chr - 1] ? sub[chr - 1][i] : 0.0);
      conv = firth_null_fit(r.Yraw.data() + (size_t)q * N, r.X.data(), r.mask.data() + (size_t)q * N, off.data(), N, Cn, bh);
      if (!conv) break;
      body << chr << " ";
      for (int c = 0; c < Cn; ++c) body << bh[c] << (c + 1 < Cn ? " " : "");
      body << "\n";
    }
    if (!conv) lo << "WARNING: Firth failed to converge";
    else {
      TextOut ff(ffn, p.gz);
      if (!ff) throw std::runtime_error("cannot write file : " + ffn);
      ff << body.str();
      ph_firthlist[q] = r.pheno_names[q] + " " + (p.use_rel_path ? ffn : get_fullpath(ffn)) + "\n";
    }
  }
  lo << "done\n\n";
  ph_log[q] = lo.str();
}

// output (Data.cpp:956-1129): the per-phenotype tables and file lists in phenotype order
void LocoWriter::write_lists() {
  const Params& p = r.p;
  const int P = r.P;
  sout << "Output\n------\n";
  std::ofstream plist(p.out + "_pred.list"), prslist;
  if (p.print_prs) prslist.open(p.out + "_prs.list");
  for (int q = 0; q < P; ++q) {
    sout << ph_log[q];
    plist << ph_plist[q];
    if (p.print_prs) prslist << ph_prslist[q];
  }
  sout << "List of blup files written to: [" << p.out << "_pred.list]\n";
  if (p.write_null_firth) {   // Data.cpp:1102-1121
    std::ofstream fl(p.out + "_firth.list");
    for (int q = 0; q < P; ++q) fl << ph_firthlist[q];
    sout << "List of files with null Firth estimates written to: [" << p.out << "_firth.list]\n";
  }
  if (p.print_prs) sout << "List of files with whole genome PRS written to: [" << p.out << "_prs.list]\n";
}

}  // namespace rgdrv
