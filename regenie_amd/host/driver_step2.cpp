// regenie-amd, the C++ host driver (see driver.h): `--step 2`.
#include "driver_step2.h"

namespace rgdrv {

// The per-variant corrections -- fit_firth_logistic_snp_fast (Step2_Models.cpp:1158-1253) and run_SPA_test_snp (:2072-2297) -- run on the
// device behind the C ABI (rg_s2_bt_correct, regenie_amd/csrc/step2_bt.hip).

// buildLookupTable (Geno.cpp:2833-2856): 00 -> 2, 01 -> missing (-3), 10 -> 1, 11 -> 0 copies of the first .bim allele
static const double lut[4] = {2.0, -3.0, 1.0, 0.0};

S2Common::S2Common(Run& r_, const S2Part& part_) : SampleMap(r_), r(r_), p(r_.p), part(part_), N(r_.N), P(r_.P), C(r_.C) {
  has_missing.assign(n, 0);
  for (int64_t k = 0; k < n; ++k)
    for (int q = 0; q < P; ++q)
      if (!r.mask[(size_t)q * N + an[k]]) { has_missing[k] = 1; any_missing = true; }
  glm = p.bt || p.ct;                                 // binary / count traits: the score test of a generalised linear null model
  mcc = r.mcc_test && !glm;                           // --mcc: quantitative traits only (the reference ignores it elsewhere, apart from the log line)
  rerint = glm ? 0 : p.rerint ? RG_S2_RERINT : p.rerintcov ? RG_S2_RERINT_COV : 0;      // compute_res alone reads the flags (Data.cpp:2393)
  Xc.resize((size_t)C * n); Yc.resize((size_t)P * n); Mc.resize((size_t)P * n);
  for (int c = 0; c < C; ++c) for (int64_t k = 0; k < n; ++k) Xc[(size_t)c * n + k] = r.X[(size_t)c * N + an[k]];
  for (int q = 0; q < P; ++q)
    for (int64_t k = 0; k < n; ++k) { Yc[(size_t)q * n + k] = (glm ? r.Yraw : r.Y)[(size_t)q * N + an[k]]; Mc[(size_t)q * n + k] = r.mask[(size_t)q * N + an[k]]; }
  firth = p.bt && p.firth; spa = p.bt && p.spa; correct = firth || spa;
  z_thr = correct ? norm_quantile(1.0 - 0.5 * p.pthresh) : 0.0;   // sqrt of the chi-square(1) quantile at 1 - pThresh (Data.cpp:2119-2120)
  per_trait = any_missing || glm;
  in = r.dosage_mode ? In::Dosage : (r.pgen ? In::PgenHard : In::Bed);
  show_info = r.dosage_mode;                            // params.dosage_mode: the INFO column
  flip = (in == In::Bed && p.ref_first) ? 1 : 0;        // .pgen rows always count ALT (PgenReader::Read / ReadHardcalls)
  dscale = r.bgenh ? 255 : 16384;
  coding = p.test_type;
  test_name = coding == 1 ? "DOM" : coding == 2 ? "REC" : "ADD";
  multi = part.nparts > 1;                              // parts write plain part files; run_step2_all concatenates (and compresses) them
  for (size_t j = 0; j < r.snp_chrom.size(); ++j) chr_snps[r.snp_chrom[j]].push_back((int64_t)j);
  for (auto& kv : chr_snps) total_blocks += (int)((kv.second.size() + p.bsize - 1) / p.bsize);
  nthreads = p.threads > 0 ? p.threads : std::max(1, usable_cpus() - 1);   // Regenie.cpp:1104-1106
  nthreads = std::max(1, std::min(nthreads, 64) / part.nparts);
  // host threads of the BGEN read-ahead: inflate is the bound of this input (about 10 ms per 1.5 MB block and thread with zlib), so it takes
  // --threads as given, or every hardware thread but two, shared by the parts of a multi-GPU run
  nt_prep = env.prep_threads ? env.prep_threads : std::max(1, std::min(p.threads > 0 ? p.threads : usable_cpus(), 256) / part.nparts);
  ld16 = (n + 7) / 8 * 8;
  // chromosome X with males under --par-region: the analysed samples' sex (without --par-region run_step2 refuses)
  if (chr_snps.count(p.nchrom) && r.has_male && p.par_set) {
    sex_aware = true;
    male.assign(n, 0);
    for (int64_t k = 0; k < n; ++k) male[k] = (r.sex.size() == (size_t)r.n_file && r.sex[file_idx[k]] == 1) ? 1 : 0;
  }
  // (the device decoder's rows hold the CODED probabilities under --test dominant | recessive: the males' additive sums then come from the general rows)
  af_cc = p.af_cc && p.bt;
  if (af_cc) {
    Cc.assign((size_t)P * n, 0); any_case.assign(n, 0);
    for (int q = 0; q < P; ++q)
      for (int64_t k = 0; k < n; ++k)
        if (Mc[(size_t)q * n + k] && Yc[(size_t)q * n + k] == 1.0) { Cc[(size_t)q * n + k] = 1; any_case[k] = 1; }
  }
  // (the same for the cases' additive sums of --af-cc)
  fast_bgen = in == In::Dosage && r.bgenh && (!env.dense || glm) && !(correct && !spa && !p.firth_approx) && !env.bgen_rows && !((sex_aware || af_cc) && coding);
}

// .bed rows of a block: runs of consecutive variants are cut into pieces read by several threads (the page-cache copy of one pread is a
// single core's memcpy), and the NEXT block of the chromosome is read while the current one is tested
class BedAhead {
 public:
  explicit BedAhead(const S2Common& cm) : cm_(cm), fd_(open((cm.p.bed + ".bed").c_str(), O_RDONLY)) { if (fd_ < 0) throw std::runtime_error("cannot read bed file"); }
  ~BedAhead() { if (ahead_.valid()) ahead_.wait(); close(fd_); }
  // the block's rows: read ahead by the previous call when it could be (same chromosome), else read now; then (bn > 0) the next block is started
  const uint8_t* take(const std::vector<int64_t>& snps, int64_t j0, int bs, int bn) {
    if (ahead_.valid()) { ahead_.get(); rows_.swap(rows_ahead_); }
    else read_bed(snps, j0, bs, rows_);
    if (bn > 0) ahead_ = std::async(std::launch::async, [this, &snps, jn = j0 + bs, bn]() { read_bed(snps, jn, bn, rows_ahead_); });
    return rows_.data();
  }
 private:
  void read_bed(const std::vector<int64_t>& snps, int64_t j0, int bs, std::vector<uint8_t>& buf) {
    const Run& r = cm_.r;
    buf.resize((size_t)bs * r.bpr);
    struct Piece { int64_t file_off, buf_off, len; };
    std::vector<Piece> pieces;
    const int64_t chunk = 16 << 20;
    for (int j = 0; j < bs;) {
      int e = j + 1;
      while (e < bs && r.snp_offset[snps[j0 + e]] == r.snp_offset[snps[j0 + e - 1]] + 1) ++e;
      const int64_t want = (int64_t)(e - j) * r.bpr, off = 3 + r.snp_offset[snps[j0 + j]] * r.bpr;
      for (int64_t o = 0; o < want; o += chunk) pieces.push_back({off + o, (int64_t)j * r.bpr + o, std::min(chunk, want - o)});
      j = e;
    }
    std::atomic<int> failed(0);
    parallel_for((int)pieces.size(), std::min(cm_.nthreads, 8), [&](int t) {
      int64_t got = 0;
      while (got < pieces[t].len) {
        const ssize_t k = pread(fd_, buf.data() + pieces[t].buf_off + got, (size_t)(pieces[t].len - got), pieces[t].file_off + got);
        if (k <= 0) { failed = 1; return; }
        got += k;
      }
    });
    if (failed) throw std::runtime_error("cannot read bed file");
  }
  const S2Common& cm_;
  const int fd_;
  std::vector<uint8_t> rows_, rows_ahead_;
  std::future<void> ahead_;
};

// The null models of a chromosome.  Binary traits (compute_res_bin, Data.cpp:2439-2445; compute_score_bt, Step2_Models.cpp:471-552): the
// null logistic model with the LOCO offset gives p^, w = p^ (1 - p^); the score test of a variant needs, per trait, sum w g~^2, X^T W g~
// and g~ . (y - p^) -- contractions of the hard-call row with fixed columns, which rg_s2_contract_packed evaluates on the i8 matrix cores.
struct ChromNull {
  const S2Common& cm;
  std::vector<double> bt_fit, resc, scf;
  std::vector<uint8_t> bt_pass;
  std::vector<double> firth_off;                      // [P][n] cov_blup_offset: X beta_nullFirth + LOCO prediction (fit_null_firth, Step2_Models.cpp:1011-1013)
  std::vector<double> firth_bnull, blup_off;          // exact Firth: the covariate-only estimates (start values), the LOCO offsets
  std::vector<MccTrait> mcc_traits;                   // --mcc: setup_y's per-trait sums of the chromosome's residuals
  std::vector<std::string> null_firth_files, firth_file_body;       // --use-null-firth: per-trait files of the list; --write-null-firth: what goes out
  double ms_chr = 0;

  explicit ChromNull(const S2Common& cm_) : cm(cm_), resc((size_t)cm_.P * cm_.n), scf(cm_.P), bt_pass(cm_.P, 1), firth_bnull((size_t)cm_.P * cm_.C, 0.0), firth_file_body(cm_.P) {
    const Params& p = cm.p;
    const int P = cm.P;
    if (cm.firth) firth_off.assign((size_t)P * cm.n, 0.0);
    if (!p.use_null_firth.empty()) {      // check_firth_file / the list reader (Step2_Models.cpp:1871-1934): `<phenotype> <file>` per line
      sout << " * reading null Firth estimates using file : [" << p.use_null_firth << "]\n";
      null_firth_files.assign(P, "");
      TextIn lf(p.use_null_firth);
      if (!lf) throw std::runtime_error("cannot read file : " + p.use_null_firth);
      std::string ln;
      while (std::getline(lf, ln)) {
        const auto t = split_ws(ln);
        if (t.empty()) continue;
        if (t.size() != 2) throw std::runtime_error("incorrectly formatted file specified by --use-null-firth.");
        for (int q = 0; q < P; ++q) if (cm.r.pheno_names[q] == t[0]) null_firth_files[q] = t[1];
      }
    }
    if (p.write_null_firth) sout << " * writing null Firth estimates to file\n";
    if (cm.firth && !p.firth_approx) blup_off.assign((size_t)P * cm.n, 0.0);
    if (cm.glm) bt_fit.assign((size_t)P * cm.n, 0.5);
  }

  // the chromosome's row of every phenotype's .loco file (500,000 numbers each at UK Biobank size): read and converted by one host thread
  // per phenotype, the checks reported in phenotype order
  std::vector<std::vector<double>> read_loco(int chrom) const {
    const Run& r = cm.r;
    const int P = cm.P;
    std::vector<std::vector<double>> blup_q(P);
    std::vector<std::string> blup_err(P);
    parallel_for(P, cm.nthreads, [&](int q) {
      const Run::Blup& bl = r.blups[q];
      if (chrom < 1 || chrom > (int)bl.line_off.size()) { blup_err[q] = "blup file for phenotype '" + r.pheno_names[q] + "' has no line for chromosome " + std::to_string(chrom) + "."; return; }
      std::string line;
      if (!bl.lines.empty()) line = bl.lines[chrom - 1];
      else {
        std::ifstream f(bl.file, std::ios::binary);
        f.seekg(bl.line_off[chrom - 1]);
        std::getline(f, line);
      }
      std::vector<Tok> t(bl.col_sample.size() + 1);
      const int nt = tokenize(line.data(), line.data() + line.size(), t.data(), (int)t.size());
      if ((size_t)nt != bl.col_sample.size()) {
        blup_err[q] = "blup file for phenotype '" + r.pheno_names[q] + "' has different number of entries on line " + std::to_string(chrom + 1) + " compared to the header (=" + std::to_string(nt) + " vs " + std::to_string(bl.col_sample.size()) + ").";
        return;
      }
      if (chr_str_to_int(std::string(t[0].b, t[0].e), cm.p.nchrom) != chrom) {
        blup_err[q] = "blup file for phenotype '" + r.pheno_names[q] + "' starts with `" + std::string(t[0].b, t[0].e) + "`instead of chromosome number=" + std::to_string(chrom) + ".";
        return;
      }
      std::vector<double>& blup = blup_q[q];
      blup.assign(cm.N, 0.0);
      for (int c = 1; c < nt; ++c) {
        const int64_t i = bl.col_sample[c];
        if (i < 0 || !r.ain[i] || !r.mask[(size_t)q * cm.N + i]) continue;
        const double v = convert_double_tok(t[c].b, t[c].e);
        if (v == MISSING) { blup_err[q] = "individual has missing predictions (chr=" + std::to_string(chrom) + ";phenotype=" + r.pheno_names[q] + ")."; return; }
        blup[i] = v;
      }
    });
    for (int q = 0; q < P; ++q)
      if (!blup_err[q].empty()) throw std::runtime_error(blup_err[q]);
    return blup_q;
  }

  // fit_null_logistic / fit_null_poisson, test-mode branch (Step1_Models.cpp:54-140, :225-288): offset = the LOCO prediction of the
  // analysed, unmasked samples
  void fit_glm(int chrom, int q, const std::vector<double>& blup) {
    const Params& p = cm.p;
    const int C = cm.C;
    const int64_t n = cm.n;
    const std::vector<int64_t>& an = cm.an;
    const std::vector<double>& Xc = cm.Xc;
    std::vector<double> off(n), eta, pv;
    for (int64_t k = 0; k < n; ++k) off[k] = blup[an[k]] * cm.Mc[(size_t)q * n + k];
    const double* yq = cm.Yc.data() + (size_t)q * n;
    const uint8_t* mq = cm.Mc.data() + (size_t)q * n;
    bool ok;
    std::vector<double> bnull;
    if (p.ct) ok = fit_poisson(yq, Xc.data(), mq, n, C, p, eta, off.data(), &pv);
    else {
      LogisticState lst;
      ok = fit_logistic(yq, Xc.data(), mq, n, C, p, true, eta, off.data(), &pv, &bnull, &lst);
      if (!ok) ok = fit_logistic(yq, Xc.data(), mq, n, C, p, false, eta, off.data(), &pv, &bnull, &lst);
    }
    if (ok && cm.firth) {   // fit_null_firth (Step2_Models.cpp:985-1060): penalised fit of the covariates, start = the unpenalised estimate
      if (!null_firth_files.empty() && !null_firth_files[q].empty()) {   // --use-null-firth: the stored estimates of this chromosome as start
        TextIn nf(null_firth_files[q]);                                   // (get_beta_start_firth, Step2_Models.cpp:1936-1981)
        if (!nf) throw std::runtime_error("cannot read file : " + null_firth_files[q]);
        std::string ln;
        while (std::getline(nf, ln)) {
          const auto t = split_ws(ln);
          if (t.empty()) throw std::runtime_error("error reading null firth estimates file");
          if (chr_str_to_int(t[0], p.nchrom) != chrom) continue;
          if ((int)t.size() - 1 > C) throw std::runtime_error("file has more predictors than included in analysis (=" + std::to_string(t.size()) + " vs " + std::to_string(C) + ")");
          for (size_t c = 1; c < t.size(); ++c) {
            const double v = convert_double(t[c]);
            if (v == MISSING) throw std::runtime_error("no missing values allowed in file");
            bnull[c - 1] = v;
          }
          break;
        }
      }
      ok = firth_null_fit(yq, Xc.data(), mq, off.data(), n, C, bnull);
      if (ok && p.write_null_firth) {     // (*firth_est_files[i]) << chrom << " " << bvec (Step2_Models.cpp:1019-1020)
        std::ostringstream ln;
        ln << chrom << " ";
        for (int c = 0; c < C; ++c) ln << bnull[c] << (c + 1 < C ? " " : "");
        firth_file_body[q] += ln.str() + "\n";
      }
      if (!ok) sout << "\n     WARNING: null Firth failed for phenotype '" << cm.r.pheno_names[q] << "' (it will be skipped).";
      for (int64_t k = 0; ok && k < n; ++k) {
        double e = blup[an[k]];
        for (int c = 0; c < C; ++c) e += Xc[(size_t)c * n + k] * bnull[c];
        firth_off[(size_t)q * n + k] = e;
        if (!p.firth_approx) blup_off[(size_t)q * n + k] = blup[an[k]];
      }
      for (int c = 0; ok && c < C; ++c) firth_bnull[(size_t)q * C + c] = bnull[c];
    }
    bt_pass[q] = ok ? 1 : 0;
    if (!ok) { if (!(cm.firth && !bnull.empty())) sout << "\n     WARNING: " << (p.ct ? "poisson" : "logistic") << " regression did not converge for phenotype '" << cm.r.pheno_names[q] << "'."; return; }
    // the fitted mean of the null model: the library forms Gamma_sqrt^2, the weighted covariates and (X^T W X)^-1 from it (rg_s2_bt_set_null)
    for (int64_t k = 0; k < n; ++k) bt_fit[(size_t)q * n + k] = pv[k];
  }

  // blup_read_chr (Step2_Models.cpp:51-140) + compute_res (Data.cpp:2386-2400)
  void set_up(int chrom, rg_s2_ctx* s2) {
    const Params& p = cm.p;
    const int64_t n = cm.n;
    sout << (p.bt ? "   -reading loco predictions for the chromosome and fitting null logistic regression on binary phenotypes..."
                  : p.ct ? "   -reading loco predictions for the chromosome and fitting null poisson regression..." : "   -reading loco predictions for the chromosome...");
    auto tb = std::chrono::steady_clock::now();
    const std::vector<std::vector<double>> blup_q = read_loco(chrom);
    const auto tb1 = std::chrono::steady_clock::now();
    for (int q = 0; q < cm.P; ++q) {
      const std::vector<double>& blup = blup_q[q];
      if (cm.glm) { fit_glm(chrom, q, blup); continue; }
      if (cm.rerint) {      // residualize_res and the scaling run on the device below, on the masked residuals as they are
        for (int64_t k = 0; k < n; ++k) resc[(size_t)q * n + k] = (cm.Yc[(size_t)q * n + k] - blup[cm.an[k]]) * cm.Mc[(size_t)q * n + k];
        continue;
      }
      double ss = 0.0;
      for (int64_t k = 0; k < n; ++k) {
        const double v = (cm.Yc[(size_t)q * n + k] - blup[cm.an[k]]) * cm.Mc[(size_t)q * n + k];
        resc[(size_t)q * n + k] = v;
        ss += v * v;
      }
      const double sd = std::sqrt(ss) / std::sqrt(cm.r.neff[q] - cm.C);
      for (int64_t k = 0; k < n; ++k) resc[(size_t)q * n + k] /= sd;
      scf[q] = cm.r.scale_Y[q] * sd;
    }
    const auto tb2 = std::chrono::steady_clock::now();
    int rc;
    if (cm.glm) {   // compute_res_bin / compute_res_count (Data.cpp:2439-2455): the null models of the chromosome go to the device
      rg_s2_bt_null nm;
      memset(&nm, 0, sizeof(nm));
      nm.family = p.ct ? 1 : 0; nm.niter_max = p.niter_max; nm.X = cm.Xc.data(); nm.y = cm.Yc.data(); nm.mask = cm.Mc.data(); nm.fitted = bt_fit.data();
      nm.firth_offset = (cm.firth && p.firth_approx) ? firth_off.data() : nullptr; nm.pass = bt_pass.data();
      rc = rg_s2_bt_set_null(s2, &nm);
    } else {
      rc = rg_s2_set_null(s2, cm.Xc.data(), resc.data(), cm.Mc.data(), scf.data());
      if (rc == RG_S2_OK && cm.rerint) {      // residualize_res (Data.cpp:2407-2436) + the scaling of compute_res: the residuals come back as the tests read them
        rg_s2_rerint_out ro;                  // (every part of a --gpus N run: its own context), scale_Y * p_sd_yres replaces scf_sv
        memset(&ro, 0, sizeof(ro));
        ro.scf_sv = scf.data(); ro.res = cm.mcc ? resc.data() : nullptr;
        rc = rg_s2_qt_rerint(s2, cm.rerint, cm.r.pheno_pass.size() == (size_t)cm.P ? cm.r.pheno_pass.data() : nullptr, 1e-6, &ro);
      }
      if (rc == RG_S2_OK && cm.mcc) {
        mcc_traits.resize(cm.P);
        for (int q = 0; q < cm.P; ++q) mcc_traits[q] = mcc_setup_trait(resc.data() + (size_t)q * n, cm.Mc.data() + (size_t)q * n, n, cm.C);
      }
    }
    if (rc != RG_S2_OK) throw std::runtime_error(rg_s2_last_error(s2));
    sout << "done (" << std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - tb).count() << "ms) \n";
    ms_chr += ms_since(tb);
    if (cm.env.timing)
      fprintf(stderr, "[timing] chromosome %d set-up: predictions read + converted %.0f ms, null models / residuals %.0f ms, to the device %.0f ms\n", chrom,
              std::chrono::duration<double, std::milli>(tb1 - tb).count(), std::chrono::duration<double, std::milli>(tb2 - tb1).count(), ms_since(tb2));
  }
};

// what every input route of a block fills: allele totals, observed samples, the info-score numerator, and per trait [bs][P] their
// DIFFERENCES from those for the samples the trait masks (only filled with S2Common::per_trait)
struct BlockCounts {
  std::vector<double> total, info_num, af_t, info_t;
  std::vector<int64_t> ns1, ns_t;
  std::vector<uint8_t> variant_ignored;
  std::vector<double> sum_pos;      // --test dominant | recessive: the recoded vector's sum over the observed samples (the counts above stay additive)
  // non-PAR variants of chromosome X (S2Common::sex_aware): the MALES' allele total and observed count, [bs][1 + P] = overall, then among the samples
  // observed for trait q (update_trait_counts' mac / nmales, Geno.cpp:2948-2959) -- filled by the input route (host loops) or fetch_group (device)
  std::vector<uint8_t> nonpar, het_male;
  bool any_nonpar = false;
  int P1 = 1;
  std::vector<double> msum;
  std::vector<int64_t> mobs;
  // --af-cc: the allele total and the observed count among the cases of each trait, [bs][P] (update_af_cc, Geno.cpp:3069-3075)
  std::vector<double> af_case;
  std::vector<int64_t> ns_case;
  explicit BlockCounts(int bs) : total(bs, 0.0), ns1(bs, 0), variant_ignored(bs, 0), sum_pos(bs, 0.0), nonpar(bs, 0), het_male(bs, 0) {}
  void mark_non_par(const S2Common& cm, const std::vector<int64_t>& snps, int64_t j0) {
    if (!cm.sex_aware) return;
    P1 = 1 + cm.P;
    for (size_t j = 0; j < nonpar.size(); ++j) if ((nonpar[j] = cm.non_par(snps[j0 + (int64_t)j]) ? 1 : 0)) any_nonpar = true;
    if (any_nonpar) { msum.assign(nonpar.size() * P1, 0.0); mobs.assign(nonpar.size() * P1, 0); }
  }
  // a male's observed call v of a non-PAR variant j, sample k (host routes)
  void add_male(const S2Common& cm, int j, int64_t k, double v) {
    double* ms = &msum[(size_t)j * P1]; int64_t* mo = &mobs[(size_t)j * P1];
    ms[0] += v; mo[0] += 1;
    for (int q = 0; q < cm.P; ++q) if (cm.Mc[(size_t)q * cm.n + k]) { ms[1 + q] += v; mo[1 + q] += 1; }
  }
  // compute_mac (Geno.cpp:3077-3108) for the variant (all samples) and for a trait's samples: allele total tq over nsq observed samples
  bool low_mac(int j, double min_mac) const {
    return nonpar[j] ? below_min_mac_x(total[j], (double)ns1[j], msum[(size_t)j * P1], (double)mobs[(size_t)j * P1], min_mac) : below_min_mac(total[j], (double)ns1[j], min_mac);
  }
  bool low_mac_t(int j, int q, double tq, double nsq, double min_mac) const {
    return nonpar[j] ? below_min_mac_x(tq, nsq, msum[(size_t)j * P1 + 1 + q], (double)mobs[(size_t)j * P1 + 1 + q], min_mac) : below_min_mac(tq, nsq, min_mac);
  }
};

// One block through the tests: an input route leaves the counts and the genotype source, the scorer the statistics, correct() the
// Firth / saddlepoint results, format() the result lines.  The buffers are kept from block to block.
struct S2Block {
  const S2Common& cm;
  const ChromNull& null;
  rg_s2_ctx* s2;
  S2Block(const S2Common& cm_, const ChromNull& null_, rg_s2_ctx* s2_) : cm(cm_), null(null_), s2(s2_) {}
  void check(int rc) const { if (rc != RG_S2_OK) throw std::runtime_error(rg_s2_last_error(s2)); }

  int bs = 0;
  std::vector<int64_t> vidx;                        // the block's variants in the file
  std::vector<uint8_t> rows_buf, packed;
  std::vector<double> dbuf, ibuf, cbuf, G;
  std::vector<uint16_t> G16;
  // the source an input route leaves for the scorer: 2-bit rows (hard calls), uint16 rows (integral) or the doubles of G
  const uint8_t* rows = nullptr; int64_t ld = 0;
  bool integral = false;
  const uint16_t* g16p = nullptr; int64_t g16ld = 0; int g16_on_device = 0;
  // statistics and corrections per (variant, trait)
  std::vector<double> stats, bhat, sfac, denum_v, mu_v, corr_beta, corr_se, corr_chisq, corr_logp;
  std::vector<int32_t> ign;
  std::vector<uint8_t> test_ignored, sparse_v, corrected, corr_fail;
  std::vector<double> mcc_logp, mcc_se_mult;        // --mcc, per (variant, trait): -log10 p of the test (NaN: the score test stands), factor on SE
  std::vector<uint8_t> mcc_fail;

  void begin(int bs_) {
    bs = bs_;
    stats.resize((size_t)bs * cm.P); bhat.resize((size_t)bs * cm.P); sfac.resize(bs); ign.resize(bs);
    test_ignored.assign((size_t)bs * cm.P, 0);
    integral = false; g16p = nullptr; g16ld = cm.n; g16_on_device = 0;
  }

  // reads of the routes that go through a reader handle (the caller holds the reader's lock in a multi-GPU run)
  void read_pgen_hard() {   // ReadHardcalls per variant (Geno.cpp:2570-2573), as .bed-coded rows (00 = two ALT copies)
    rows_buf.resize((size_t)bs * cm.r.bpr);
    if (rg_pgen_read_bed_rows(cm.r.pgen, bs, vidx.data(), rows_buf.data(), cm.r.bpr) != RG_PGEN_OK) throw std::runtime_error(rg_pgen_last_error(cm.r.pgen));
    rows = rows_buf.data();
  }
  void read_dosage_rows() {
    const Run& r = cm.r;
    dbuf.resize((size_t)bs * r.n_file);
    if (r.bgenh) {            // parseSnpfromBGEN (Geno.cpp:2186-2330): dosages and the terms of the IMPUTE info score
      ibuf.resize((size_t)bs * r.n_file);
      if (cm.coding) {        // its second pass too (Geno.cpp:2362-2392): the coded probabilities the test takes
        cbuf.resize((size_t)bs * r.n_file);
        if (rg_bgen_read_dosages_coded(r.bgenh, bs, vidx.data(), cm.p.ref_first ? 1 : 0, cm.coding, dbuf.data(), ibuf.data(), cbuf.data(), r.n_file) != RG_BGEN_OK)
          throw std::runtime_error(rg_bgen_last_error(r.bgenh));
      } else if (rg_bgen_read_dosages_info(r.bgenh, bs, vidx.data(), cm.p.ref_first ? 1 : 0, dbuf.data(), ibuf.data(), r.n_file) != RG_BGEN_OK)
        throw std::runtime_error(rg_bgen_last_error(r.bgenh));
    } else if (rg_pgen_read_dosage_rows(r.pgen, bs, vidx.data(), dbuf.data(), r.n_file) != RG_PGEN_OK)   // Read() (Geno.cpp:2570-2571)
      throw std::runtime_error(rg_pgen_last_error(r.pgen));
  }

  // route 1: the block the BGEN read-ahead prepared
  void from_prepared(const PreparedBlock& pb, BlockCounts& bc) {
    const size_t P = (size_t)cm.P;
    bc.total.assign(pb.total, pb.total + bs); bc.ns1.assign(pb.ns1, pb.ns1 + bs);
    bc.info_num.assign(pb.info_num, pb.info_num + bs);
    bc.variant_ignored.assign(pb.ignored, pb.ignored + bs);
    if (cm.coding) bc.sum_pos.assign(pb.sum_pos, pb.sum_pos + bs);
    if (cm.per_trait) { bc.af_t.assign(pb.af_t, pb.af_t + bs * P); bc.ns_t.assign(pb.ns_t, pb.ns_t + bs * P); bc.info_t.assign(pb.info_t, pb.info_t + bs * P); }
    integral = true; g16p = pb.g16; g16ld = pb.ld; g16_on_device = pb.on_device;
    // --af-cc: rows the host threads walked come with their sums among the cases; device-decoded rows never leave the GPU, the library sums them there
    // (exact integers in units of 1 / scale) -- in the launch that serves the males' planes when the block has a non-PAR variant
    const bool cases_dev = cm.af_cc && pb.on_device;
    if (cm.af_cc && !cases_dev) { bc.af_case.assign(pb.af_case, pb.af_case + bs * P); bc.ns_case.assign(pb.ns_case, pb.ns_case + bs * P); }
    if (cases_dev) fetch_case_sums(bc);
    if (!bc.any_nonpar) return;
    // the males' sums of the prepared rows
    std::vector<int64_t> gs((size_t)bs * bc.P1 * 2);
    check(cases_dev ? rg_s2_group_sums_last(s2, bs, gs.data()) : rg_s2_group_sums_int(s2, g16p, g16ld, bs, g16_on_device, gs.data()));
    for (int j = 0; j < bs; ++j) {
      if (!bc.nonpar[j]) continue;
      for (int q = 0; q < bc.P1; ++q) { bc.msum[(size_t)j * bc.P1 + q] = (double)gs[((size_t)j * bc.P1 + q) * 2] / cm.dscale; bc.mobs[(size_t)j * bc.P1 + q] = gs[((size_t)j * bc.P1 + q) * 2 + 1]; }
      bc.variant_ignored[j] = bc.low_mac(j, cm.p.min_mac) ? 1 : 0;      // (the read-ahead applied the autosomal rule, which never drops what this one keeps)
    }
  }

  // --af-cc on integer rows: the sums among the cases of each trait from the library (rg_s2_case_sums_int reads the rows the score entry will be given)
  void fetch_case_sums(BlockCounts& bc) {
    const size_t P = (size_t)cm.P;
    std::vector<int64_t> cs((size_t)bs * P * 2);
    check(rg_s2_case_sums_int(s2, g16p, g16ld, bs, g16_on_device, cs.data()));
    bc.af_case.resize((size_t)bs * P); bc.ns_case.resize((size_t)bs * P);
    for (size_t e = 0; e < (size_t)bs * P; ++e) { bc.af_case[e] = (double)cs[2 * e] / cm.dscale; bc.ns_case[e] = cs[2 * e + 1]; }
  }

  // route 2, general dosage rows: the analysed samples' doubles, allele totals, the info-score numerator and the per-trait corrections on the
  // host (parseSnpfromBGEN / readChunkFromPGENFileToG with update_trait_counts, Geno.cpp:2948-2959)
  void from_dosage_rows(BlockCounts& bc) {
    const Run& r = cm.r;
    const int P = cm.P, dscale = cm.dscale;
    const int64_t n = cm.n;
    G.assign((size_t)bs * n, 0.0);
    bc.info_num.assign(bs, 0.0);
    if (cm.per_trait) { bc.af_t.assign((size_t)bs * P, 0.0); bc.ns_t.assign((size_t)bs * P, 0); bc.info_t.assign((size_t)bs * P, 0.0); }
    // --af-cc: .bgen rows in this loop (their doubles are no integers, the sums are regenie's own in its order; under a coding the uint16 rows hold
    // the coded values); .pgen dosages -- exact in units of 1 / 16384 -- from the library below
    const bool cases_here = cm.af_cc && r.bgenh;
    if (cases_here) { bc.af_case.assign((size_t)bs * P, 0.0); bc.ns_case.assign((size_t)bs * P, 0); }
    parallel_for(bs, cm.nthreads, [&](int j) {
      const double* d = dbuf.data() + (size_t)j * r.n_file;
      const double* iv = r.bgenh ? ibuf.data() + (size_t)j * r.n_file : nullptr;
      const double* cv = (cm.coding && r.bgenh) ? cbuf.data() + (size_t)j * r.n_file : nullptr;
      double* g = G.data() + (size_t)j * n;
      double tot = 0.0, inf = 0.0, pos = 0.0; int64_t ns = 0;
      for (int64_t k = 0; k < n; ++k) {
        const int64_t i = cm.file_idx[k];
        const double v = d[i];
        g[k] = v;
        if (v == -3.0) continue;
        if (cm.coding) {      // the vector the test takes: the coded BGEN probabilities (.pgen dosage tracks are refused in run_step2)
          g[k] = cv[i];
          pos += g[k];
        }
        const double e = iv ? iv[i] : v * v;
        tot += v; inf += e; ++ns;
        if (bc.nonpar[j] && cm.male[k]) bc.add_male(cm, j, k, v);
        if (cm.per_trait && cm.has_missing[k]) subtract_masked(cm.Mc.data(), n, P, k, v, e, &bc.af_t[(size_t)j * P], &bc.ns_t[(size_t)j * P], &bc.info_t[(size_t)j * P]);
        if (cases_here && cm.any_case[k]) add_cases(cm.Cc.data(), n, P, k, v, &bc.af_case[(size_t)j * P], &bc.ns_case[(size_t)j * P]);
      }
      bc.total[j] = tot; bc.ns1[j] = ns; bc.info_num[j] = inf; bc.sum_pos[j] = pos;
      if (bc.low_mac(j, cm.p.min_mac)) bc.variant_ignored[j] = 1;
    });
    // 8-bit .bgen probabilities and .pgen dosages are integers in units of 1 / 255 and 1 / 16384: as uint16 rows they take the
    // integer route of the library (digit planes on the i8 matrix cores, 2 B per genotype over PCIe); anything else, or
    // RG_S2_DENSE=1, the fp64 route
    integral = !cm.env.dense || cm.glm;
    if (!integral) return;
    G16.resize((size_t)bs * n);
    std::vector<uint8_t> bad(bs, 0);
    parallel_for(bs, cm.nthreads, [&](int j) {
      const double* g = G.data() + (size_t)j * n;
      uint16_t* q = G16.data() + (size_t)j * n;
      for (int64_t k = 0; k < n; ++k) {
        if (g[k] == -3.0) { q[k] = 0xFFFFu; continue; }
        const double v = g[k] * dscale, rv = std::nearbyint(v);
        if (std::fabs(v - rv) > 1e-6 || rv < 0 || rv > 2.0 * dscale) { bad[j] = 1; break; }
        q[k] = (uint16_t)rv;
      }
    });
    for (int j = 0; j < bs; ++j) if (bad[j]) integral = false;
    g16p = G16.data();
    if (cm.af_cc && !cases_here && integral) {      // the case entry uploads the rows; the score entry reads that device copy in place
      fetch_case_sums(bc);
      const void* d = nullptr;
      check(rg_s2_case_rows_staged(s2, &d, &g16ld));
      g16p = (const uint16_t*)d; g16_on_device = 1;
    }
  }

  // route 3, hard calls stay packed: the 2-bit codes of the analysed samples go to the device as they are (the rows of the file itself
  // when no sample was dropped), the library counts the calls and contracts them on the i8 matrix cores; the counts come with the scores
  void from_packed() {
    ld = cm.r.bpr;
    if (cm.identity) return;
    ld = repack_analysed(rows, cm.r.bpr, bs, cm.file_idx.data(), cm.n, cm.nthreads, packed);
    rows = packed.data();
  }

  // route 4 (RG_S2_DENSE=1), parseSnpfromBed: decode the analysed samples, allele counts
  void from_dense_bed(BlockCounts& bc) {
    const int P = cm.P, flip = cm.flip;
    const int64_t n = cm.n;
    G.assign((size_t)bs * n, 0.0);
    if (cm.any_missing) { bc.af_t.assign((size_t)bs * P, 0.0); bc.ns_t.assign((size_t)bs * P, 0); }
    parallel_for(bs, cm.nthreads, [&](int j) {
      const uint8_t* row = rows + (size_t)j * cm.r.bpr;
      double* g = G.data() + (size_t)j * n;
      double tot = 0.0, pos = 0.0; int64_t ns = 0;
      for (int64_t k = 0; k < n; ++k) {
        const int64_t i = cm.file_idx[k];
        double hc = lut[(row[i >> 2] >> (2 * (i & 3))) & 3];
        if (flip && hc != -3.0) hc = 2.0 - hc;
        g[k] = hc;
        if (hc != -3.0) {
          if (cm.coding) { g[k] = recode_hard_call(hc, cm.coding); pos += g[k]; }
          tot += hc; ++ns;
          if (bc.nonpar[j] && cm.male[k]) { bc.add_male(cm, j, k, hc); if (hc == 1.0) bc.het_male[j] = 1; }
          if (cm.any_missing && cm.has_missing[k]) subtract_masked(cm.Mc.data(), n, P, k, hc, 0.0, &bc.af_t[(size_t)j * P], &bc.ns_t[(size_t)j * P], nullptr);
        }
      }
      bc.total[j] = tot; bc.ns1[j] = ns; bc.sum_pos[j] = pos;
      if (bc.low_mac(j, cm.p.min_mac)) bc.variant_ignored[j] = 1;
    });
  }

  // --test dominant | recessive, after the additive filters (parseSnpfromBed, Geno.cpp:2517-2527, and its like in every reader): the recessive test
  // ignores a variant with fewer than --minHOMs homALT carriers (the recoded sum), both a variant whose recoded mean is below numtol
  void coding_filters(BlockCounts& bc) const {
    if (!cm.coding) return;
    for (int j = 0; j < bs; ++j) {
      if (cm.coding == 2 && bc.sum_pos[j] < cm.p.min_homs) bc.variant_ignored[j] = 1;
      if (bc.ns1[j] > 0 && bc.sum_pos[j] / (double)bc.ns1[j] < NUMTOL) bc.variant_ignored[j] = 1;
    }
  }

  // hard calls that stayed packed, a block with a non-PAR variant of chromosome X: the males' calls equal to 1, equal to 2 and observed, overall
  // and among each trait's samples, from the library (rg_s2_group_counts_packed reads the rows the score entry was given; additive under every coding)
  // --af-cc: the same among the cases of each trait (rg_s2_case_counts_packed), first: with a group set its launch covers the males' planes too, the
  // rows are read once and the males' counts are taken from it
  void fetch_group(BlockCounts& bc) {
    if (cm.af_cc) {
      const size_t P = (size_t)cm.P;
      std::vector<int32_t> cc((size_t)bs * P * 3);
      check(rg_s2_case_counts_packed(s2, rows, ld, bs, 0, cm.flip, cc.data()));
      bc.af_case.resize((size_t)bs * P); bc.ns_case.resize((size_t)bs * P);
      for (size_t e = 0; e < (size_t)bs * P; ++e) { bc.af_case[e] = (double)cc[3 * e] + 2.0 * cc[3 * e + 1]; bc.ns_case[e] = cc[3 * e + 2]; }
    }
    if (!bc.any_nonpar) return;
    std::vector<int32_t> gc((size_t)bs * bc.P1 * 3);
    check(cm.af_cc ? rg_s2_group_counts_last(s2, bs, gc.data()) : rg_s2_group_counts_packed(s2, rows, ld, bs, 0, cm.flip, gc.data()));
    for (int j = 0; j < bs; ++j) {
      if (!bc.nonpar[j]) continue;
      for (int q = 0; q < bc.P1; ++q) {
        const int32_t* c = &gc[((size_t)j * bc.P1 + q) * 3];
        bc.msum[(size_t)j * bc.P1 + q] = (double)c[0] + 2.0 * c[1]; bc.mobs[(size_t)j * bc.P1 + q] = c[2];
      }
      if (gc[(size_t)j * bc.P1 * 3] > 0) bc.het_male[j] = 1;
    }
  }

  // quantitative traits: the block's statistics from whatever source the route left
  void score_qt(BlockCounts& bc) {
    const int P = cm.P;
    rg_s2_qt_out o;
    memset(&o, 0, sizeof(o));
    o.stats = stats.data(); o.bhat = bhat.data(); o.scale_fac = sfac.data(); o.ignored = ign.data();
    if (cm.in == In::Dosage) {
      std::vector<double> mean_c(cm.coding ? bs : 0);
      std::vector<int32_t> nobs_c(cm.coding ? bs : 0);
      if (cm.coding && integral) { o.mean = mean_c.data(); o.n_obs = nobs_c.data(); }
      if (!integral) { check(rg_s2_qt_block(s2, G.data(), cm.n, bs, 0, NUMTOL, &o)); return; }
      check(rg_s2_qt_block_int(s2, g16p, g16ld, bs, g16_on_device, cm.dscale, NUMTOL, &o));
      // rows the device decoder coded: their sum is an integer in units of 1 / scale, recovered exactly from the mean the entry returns
      for (int j = 0; cm.coding && j < bs; ++j) {
        if (std::isnan(bc.sum_pos[j])) bc.sum_pos[j] = std::nearbyint(mean_c[j] * (double)nobs_c[j] * cm.dscale) / cm.dscale;
      }
      return;
    }
    if (cm.env.dense) { check(rg_s2_qt_block(s2, G.data(), cm.n, bs, 0, NUMTOL, &o)); return; }
    std::vector<double> mean_v(bs), totp_v;
    std::vector<int32_t> nobs_v(bs), nobsp_v;
    o.mean = mean_v.data(); o.n_obs = nobs_v.data();
    if (cm.any_missing) {
      totp_v.resize((size_t)bs * P); nobsp_v.resize((size_t)bs * P);
      o.total_p = totp_v.data(); o.n_obs_p = nobsp_v.data();
    }
    check(rg_s2_qt_block_packed(s2, rows, ld, bs, 0, cm.flip, NUMTOL, &o));
    fetch_group(bc);
    std::vector<int32_t> cnt_v;      // --test dominant | recessive: the mean is the recoded vector's, the additive counts come on their own
    if (cm.coding) { cnt_v.resize((size_t)bs * 4); check(rg_s2_packed_counts(s2, cnt_v.data())); }
    if (cm.any_missing) { bc.af_t.assign((size_t)bs * P, 0.0); bc.ns_t.assign((size_t)bs * P, 0); }
    for (int j = 0; j < bs; ++j) {
      bc.ns1[j] = nobs_v[j];
      if (cm.coding) {
        const double n1 = cnt_v[(size_t)j * 4], n2 = cnt_v[(size_t)j * 4 + 1];
        bc.total[j] = n1 + 2.0 * n2; bc.sum_pos[j] = cm.coding == 1 ? n1 + n2 : n2;
      } else
      bc.total[j] = std::nearbyint(mean_v[j] * (double)nobs_v[j]);       // the allele count is an integer: mean = total / n_obs
      if (bc.low_mac(j, cm.p.min_mac)) bc.variant_ignored[j] = 1;
      if (cm.any_missing)                                                  // update_trait_counts (Geno.cpp:2948-2959) as differences from the totals
        for (int q = 0; q < P; ++q) {
          bc.af_t[(size_t)j * P + q] = std::nearbyint(totp_v[(size_t)j * P + q]) - bc.total[j];
          bc.ns_t[(size_t)j * P + q] = (int64_t)nobsp_v[(size_t)j * P + q] - bc.ns1[j];
        }
    }
  }

  // --mcc (compute_score_qt_mcc, Step2_Models.cpp:237-341): the rows that need the test -- with --mcc-thr 1 every kept row, else the rows with a
  // qualifying trait whose score test passes the threshold, and every kept SPARSE row: the reference forms the statistic of this mode from the
  // vector the MCC sees, which for a sparse variant is the raw genotype (sum mask g^2 as denominator, not the residualised one of the plain
  // score test), so its BETA / SE / CHISQ come from the same sums -- one rg_s2_qt_moments call, then the closed form per (row, trait)
  void mcc(const BlockCounts& bc) {
    const Params& p = cm.p;
    const int P = cm.P;
    const bool every = !(p.mcc_thr < 1.0);
    const double thr_nlog10 = -std::log10(p.mcc_thr);
    mcc_logp.assign((size_t)bs * P, NAN); mcc_se_mult.assign((size_t)bs * P, 1.0); mcc_fail.assign((size_t)bs * P, 0);
    std::vector<int32_t> todo;
    for (int j = 0; j < bs; ++j) {
      if (bc.variant_ignored[j] || ign[j]) continue;
      bool need = every || sfac[j] == 1.0;       // scale_fac = 1: check_sparse_G's verdict as the score entries return it
      for (int q = 0; q < P && !need; ++q) {
        const double st = stats[(size_t)j * P + q];
        need = cm.r.mcc_Y[q] && get_logp(st * st) > thr_nlog10;
      }
      if (need) todo.push_back(j);
    }
    if (todo.empty()) return;
    std::vector<double> sums(todo.size() * (size_t)P * 7);
    rg_s2_mcc_out mo;
    mo.sums = sums.data();
    check(rg_s2_qt_moments(s2, (int32_t)todo.size(), todo.data(), &mo));
    parallel_for((int)todo.size(), cm.nthreads, [&](int t) {
      const int j = todo[t];
      for (int q = 0; q < P; ++q) {
        const size_t e = (size_t)j * P + q;
        const double* S = sums.data() + ((size_t)t * P + q) * 7;
        if (sfac[j] == 1.0) {      // the non-strict statistic on the vector as it is (gsc = 1)
          const double sd = std::sqrt(S[1]);
          stats[e] = S[6] / sd;
          bhat[e] = stats[e] * null.scf[q] / sd;
        }
        const double chisq = stats[e] * stats[e];
        if (!every && !(cm.r.mcc_Y[q] && get_logp(chisq) > thr_nlog10)) continue;
        bool ok = false;
        const double pv = mcc_pvalue(null.mcc_traits[q], S, &ok);
        if (!ok) { mcc_fail[e] = 1; mcc_logp[e] = -1.0; continue; }
        mcc_logp[e] = -std::log10(pv);
        mcc_se_mult[e] = std::sqrt(chisq / chisq1_upper_quantile(pv));
      }
    });
  }

  // binary / count traits: the score test of the block through the C ABI (rg_s2_bt_score_*: contractions on the i8 matrix cores, C x C
  // algebra in the library): hard calls as packed rows, dosages as integer rows
  void score_glm(BlockCounts& bc) {
    const int P = cm.P;
    std::vector<int32_t> bt_counts((size_t)bs * 4), nobsp((size_t)bs * P, 0);
    std::vector<double> bt_vstat((size_t)bs * 4), totp((size_t)bs * P, 0.0);
    denum_v.assign((size_t)bs * P, 0.0);
    mu_v.assign(bs, 0.0); sparse_v.assign(bs, 0);
    rg_s2_bt_out bo;
    memset(&bo, 0, sizeof(bo));
    bo.stats = stats.data(); bo.bhat = bhat.data(); bo.denum = denum_v.data(); bo.test_ignored = test_ignored.data(); bo.mean = mu_v.data();
    bo.ignored = ign.data(); bo.sparse = sparse_v.data();
    const bool dosage = cm.in == In::Dosage;
    if (dosage) {
      if (!integral) throw std::runtime_error("--step 2 --bt / --ct on dosages that are not integer multiples of 1/" + std::to_string(cm.dscale) + " is not built.");
      bo.vstat = bt_vstat.data();
      check(rg_s2_bt_score_int(s2, g16p, g16ld, bs, g16_on_device, cm.dscale, NUMTOL, &bo));
      for (int j = 0; cm.coding && j < bs; ++j)      // rows the device decoder coded: vstat[0] is their exact integer sum
        if (std::isnan(bc.sum_pos[j])) bc.sum_pos[j] = bt_vstat[(size_t)j * 4] / cm.dscale;
    } else {
      bo.counts = bt_counts.data(); bo.total_p = totp.data(); bo.n_obs_p = nobsp.data();
      // --af-cc: the case entry goes first and uploads the block; the score entry takes that device copy, so the rows cross PCIe once
      const void* drows = nullptr; int64_t dld = 0;
      if (cm.af_cc) { fetch_group(bc); check(rg_s2_case_rows_staged(s2, &drows, &dld)); }
      if (drows) check(rg_s2_bt_score_packed(s2, (const uint8_t*)drows, dld, bs, 1, cm.flip, NUMTOL, &bo));
      else { check(rg_s2_bt_score_packed(s2, rows, ld, bs, 0, cm.flip, NUMTOL, &bo)); fetch_group(bc); }
      bc.af_t.assign(totp.begin(), totp.end());      // per-trait allele and sample counts (dosages: the route has them, summed as the reference sums)
      bc.ns_t.assign(nobsp.begin(), nobsp.end());
    }
    for (int j = 0; j < bs; ++j) {
      if (!dosage) {
        const double n1 = bt_counts[(size_t)j * 4], n2 = bt_counts[(size_t)j * 4 + 1], nm = bt_counts[(size_t)j * 4 + 2];
        bc.ns1[j] = (int64_t)((double)cm.n - nm); bc.total[j] = n1 + 2.0 * n2;      // (the counts are additive under every coding)
        if (cm.coding) bc.sum_pos[j] = cm.coding == 1 ? n1 + n2 : n2;
      }
      sfac[j] = 1.0;
      if (bc.low_mac(j, cm.p.min_mac)) bc.variant_ignored[j] = 1;
    }
  }

  // check_pval_snp (Step2_Models.cpp:1987-2029): |z| above the threshold -> run_SPA_test (--spa) or fit_firth_logistic_snp_fast on Gres / Gamma_sqrt
  // with the null Firth model's covariate effects in the offset.  The flagged (variant, trait) pairs are re-tested on the device, one
  // workgroup per pair (rg_s2_bt_correct); the exact Firth test (--firth without --approx: a C + 1 parameter fit) stays on the host threads.
  void correct(const BlockCounts& bc) {
    const Params& p = cm.p;
    const int P = cm.P, C = cm.C;
    const int64_t n = cm.n;
    corrected.assign((size_t)bs * P, 0); corr_fail.assign((size_t)bs * P, 0);
    corr_beta.assign((size_t)bs * P, 0.0); corr_se.assign((size_t)bs * P, 0.0); corr_chisq.assign((size_t)bs * P, 0.0); corr_logp.assign((size_t)bs * P, -1.0);
    std::vector<int> todo;
    for (int j = 0; j < bs; ++j)
      for (int q = 0; q < P; ++q)
        if (!bc.variant_ignored[j] && !ign[j] && !test_ignored[(size_t)j * P + q] && std::fabs(stats[(size_t)j * P + q]) > cm.z_thr) todo.push_back(j * P + q);
    if (cm.spa || p.firth_approx) {
      std::vector<int32_t> pv_(todo.size()), pt_(todo.size());
      std::vector<uint8_t> pf_(todo.size());
      for (size_t t = 0; t < todo.size(); ++t) {
        const int j = todo[t] / P, q = todo[t] % P;
        pv_[t] = j; pt_[t] = q;
        if (cm.spa) pf_[t] = sparse_v[j];                                                            // fastSPA (Step2_Models.cpp:2087-2097)
        else {
          const double tq = bc.total[j] + bc.af_t[(size_t)j * P + q];
          const double nsq = (double)(bc.ns1[j] + bc.ns_t[(size_t)j * P + q]);
          pf_[t] = sparse_v[j] && bc.low_mac_t(j, q, tq, nsq, 50.0);                                       // fit_firth_logistic_snp_fast :1173-1185: carriers only
        }
      }
      std::vector<rg_s2_bt_corr> cr(todo.size());
      check(rg_s2_bt_correct(s2, cm.spa ? RG_S2_BT_SPA : RG_S2_BT_FIRTH_APPROX, (int32_t)todo.size(), pv_.data(), pt_.data(), pf_.data(), p.firth_se ? 1 : 0, cr.data()));
      for (size_t t = 0; t < todo.size(); ++t) {
        const size_t e = (size_t)todo[t];
        corrected[e] = 1;
        if (cr[t].fail) { corr_fail[e] = 1; continue; }
        corr_beta[e] = cr[t].beta; corr_se[e] = cr[t].se; corr_chisq[e] = cr[t].chisq; corr_logp[e] = cr[t].logp;
      }
      return;
    }
    parallel_for((int)todo.size(), cm.nthreads, [&](int t) {
      const int j = todo[t] / P, q = todo[t] % P;
      const double mu = mu_v[j];
      std::vector<double> gt(n);                // the mean-imputed genotype of the analysed samples
      if (cm.in == In::Dosage) { const double* g = G.data() + (size_t)j * n; for (int64_t k = 0; k < n; ++k) gt[k] = g[k] == -3.0 ? mu : g[k]; }
      else {
        const uint8_t* row = rows + (size_t)j * ld;
        for (int64_t k = 0; k < n; ++k) {
          double hc = lut[(row[k >> 2] >> (2 * (k & 3))) & 3];
          if (cm.flip && hc != -3.0) hc = 2.0 - hc;
          gt[k] = hc == -3.0 ? mu : recode_hard_call(hc, cm.coding);      // (mu: the recoded vector's mean under --test dominant | recessive)
        }
      }
      // the exact test (fit_firth_logistic_snp, Step2_Models.cpp:1062-1156): design [covariates | g~ on its raw scale], offset = the LOCO
      // prediction; null fit = the variant's coefficient held at 0 under the same penalty, then every coefficient free
      const uint8_t* mq = cm.Mc.data() + (size_t)q * n;
      const double *yq = cm.Yc.data() + (size_t)q * n, *oq = null.blup_off.data() + (size_t)q * n;
      std::vector<const double*> cols(C + 1);
      for (int c = 0; c < C; ++c) cols[c] = cm.Xc.data() + (size_t)c * n;
      cols[C] = gt.data();
      std::vector<double> bf(C + 1, 0.0), inv;
      for (int c = 0; c < C; ++c) bf[c] = null.firth_bnull[(size_t)q * C + c];
      double dev0 = 0.0, dev1 = 0.0;
      corrected[(size_t)j * P + q] = 1;
      const bool okx = firth_fit_cols(yq, cols, mq, oq, n, C, 25.0, bf, &dev0) && firth_fit_cols(yq, cols, mq, oq, n, C + 1, 5.0, bf, &dev1, &inv);
      const double lrt = dev0 - dev1;
      if (!okx || lrt < 0) { corr_fail[(size_t)j * P + q] = 1; return; }
      corr_beta[(size_t)j * P + q] = bf[C];
      corr_chisq[(size_t)j * P + q] = lrt;
      corr_se[(size_t)j * P + q] = (p.firth_se && lrt > 0) ? std::fabs(bf[C]) / std::sqrt(lrt) : std::sqrt(inv[(size_t)C * (C + 1) + C]);
    });
  }

  // the result lines (compute_score_qt after the statistic, Step2_Models.cpp:440-466; print_sum_stats_single): formatted by the host threads
  // in contiguous chunks of variants, appended to the files in order; n_ign[3] += ignored variants, ignored tests, tests
  void format(BlockCounts& bc, const std::vector<int64_t>& snps, int64_t j0, std::vector<std::unique_ptr<TextOut>>& ofs, int64_t* n_ign) {
    const Run& r = cm.r;
    const Params& p = cm.p;
    const int P = cm.P;
    const bool show_info = cm.show_info, bgen = r.bgenh != nullptr;
    const int nchunk = std::max(1, std::min(cm.nthreads, bs / 64));
    std::vector<std::string> chunk_out((size_t)nchunk * P);
    std::vector<int64_t> c_snps(nchunk, 0), c_tests(nchunk, 0), c_tested(nchunk, 0);
    parallel_for(nchunk, nchunk, [&](int t) {
      for (int j = (int)((int64_t)bs * t / nchunk), je = (int)((int64_t)bs * (t + 1) / nchunk); j < je; ++j) {
        const double total = bc.total[j];
        const int64_t ns1 = bc.ns1[j];
        if (!bc.variant_ignored[j] && show_info && p.set_min_info && ns1 > 0)    // the all-sample info score below --minINFO drops the variant (Geno.cpp:2349-2353)
          if (info_score(bgen, bc.info_num[j], (double)ns1, total / (2.0 * ns1)) < p.min_info) bc.variant_ignored[j] = 1;
        if (bc.variant_ignored[j] || ign[j]) { ++c_snps[t]; continue; }
        const int64_t sj = snps[j0 + j];
        std::ostringstream head;
        head << r.snp_chrom[sj] << " " << r.snp_pos[sj] << " " << r.snp_ids[sj] << " " << r.snp_a0[sj] << " " << r.snp_a1[sj] << " ";
        for (int q = 0; q < P; ++q) {
          const size_t e = (size_t)j * P + q;
          double af = total / (2.0 * ns1);
          int64_t nsq = ns1;
          double infq = show_info ? bc.info_num[j] : 0.0;
          double af_case = 0.0, af_control = 0.0;
          int64_t ns_case = 0, ns_control = 0;
          if (test_ignored[e]) continue;
          if (cm.per_trait) {   // compute_mac / compute_aaf_info per trait
            const double tq = total + bc.af_t[e];
            nsq = ns1 + bc.ns_t[e];
            if (bc.low_mac_t(j, q, tq, (double)nsq, p.min_mac)) { ++c_tests[t]; continue; }
            af = tq / (2.0 * nsq);
            if (show_info) infq += bc.info_t[e];
            if (cm.af_cc) {      // compute_aaf_info (Geno.cpp:3119-3126)
              ns_case = bc.ns_case[e]; ns_control = nsq - ns_case;
              af_control = (tq - bc.af_case[e]) / (2.0 * nsq - 2.0 * ns_case);
              af_case = bc.af_case[e] / (2.0 * ns_case);
            }
          }
          const double info = show_info ? info_score(bgen, infq, (double)nsq, af) : 1.0;
          if (show_info && p.set_min_info && info < p.min_info) { ++c_tests[t]; continue; }     // ignored_trait (Geno.cpp:3143-3144)
          const double st = stats[e];
          double bh = bhat[e], se = bh / st, chisq = st * st;
          bool test_fail = false;
          double logp_spa = -1.0;
          if (cm.correct && corrected[e]) {
            if (corr_fail[e]) test_fail = true;                    // get_sumstats(true, ...): the score test's BETA / SE, no p-value
            else { bh = corr_beta[e]; se = corr_se[e]; chisq = corr_chisq[e]; logp_spa = corr_logp[e]; }
          }
          double logp_mcc = NAN;
          if (cm.mcc && !std::isnan(mcc_logp[e])) {      // LOG10P of the moment-matched test, SE scaled to it; BETA and CHISQ stay
            if (mcc_fail[e]) test_fail = true;
            else { logp_mcc = mcc_logp[e]; se *= mcc_se_mult[e]; }
          }
          const double logp = !std::isnan(logp_mcc) ? logp_mcc : logp_spa >= 0 ? logp_spa : get_logp(chisq);       // --spa prints the p-value it computed, the chi-square is derived from it
          std::ostringstream ln;
          if (af >= 0) ln << head.str() << af << " ";            // print_sum_stats_single (Step2_Models.cpp:2505-2518): a negative value is "NA"
          else ln << head.str() << "NA ";
          if (cm.af_cc) { if (af >= 0) ln << af_case << " " << af_control << " "; else ln << "NA NA "; }
          if (show_info) { if (info >= 0) ln << info << " "; else ln << "NA "; }      // (the IMPUTE score of very uncertain dosages can be negative)
          ln << nsq;
          if (cm.af_cc) ln << ' ' << ns_case << ' ' << ns_control;
          ln << ' ' << cm.test_name << ' ';
          if (se >= 0 && !std::isnan(se)) ln << bh << ' ' << se;
          else ln << "NA NA";
          if (chisq >= 0 && !std::isnan(logp) && !test_fail) ln << ' ' << chisq << ' ' << logp;
          else ln << " NA NA";
          ln << (test_fail ? " TEST_FAIL\n" : " NA\n");
          chunk_out[(size_t)t * P + q] += ln.str();
          ++c_tested[t];
        }
      }
    });
    for (int t = 0; t < nchunk; ++t) {
      for (int q = 0; q < P; ++q) *ofs[q] << chunk_out[(size_t)t * P + q];
      n_ign[0] += c_snps[t]; n_ign[1] += c_tests[t]; n_ign[2] += c_tested[t];
    }
  }
};

int run_step2(Run& r, std::chrono::steady_clock::time_point t_start, S2Part& part) {
  const S2Common cm(r, part);
  const Params& p = cm.p;
  const int P = cm.P;
  // The reference rounds a .pgen dosage track to hard calls under a coding (Geno.cpp:2669-2679) but keeps check_sparse_G's zero count of the ADDITIVE
  // dosages (:2594); the integer-dosage entries count the zeros of the row they are given, so that combination is not built
  if (cm.coding && cm.in == In::Dosage && !r.bgenh)
    throw std::runtime_error("--test dominant / recessive on a .pgen file with dosages is not built: use hard calls (a .pgen without a dosage track, or --bed).");
  ChromNull null(cm);
  rg_s2_ctx* s2 = nullptr;
  if (rg_s2_create(&s2, part.device, cm.n, cm.C, P) != RG_S2_OK || !s2) throw std::runtime_error("no MI355X / HIP device available (rg_s2_create failed)");
  S2Block blk(cm, null, s2);
  // check_sparse_G: params.n_samples, params.prop_zero_thr (Regenie.hpp:311); the .pgen reader counts the observed zeros itself
  blk.check(rg_s2_set_sparse_rule(s2, cm.N, 0.5, r.pgen ? 1 : 0));
  if (cm.coding) blk.check(rg_s2_set_coding(s2, cm.coding));      // (an additive run never calls it)
  // in_non_par (Geno.cpp:2419, :2251): outside the pseudo-autosomal regions of chromosome X the reference halves the males' calls in the
  // MAC (and, with the default dosage compensation off, nothing else) -- with no male in the sample file that is the autosomal rule
  if (cm.chr_snps.count(p.nchrom) && r.has_male && !p.par_set)
    throw std::runtime_error("--step 2 on chromosome " + std::to_string(p.nchrom) + " (X) with male samples: the sex-aware allele counts of the non-PAR region "
                             "need the bounds of the pseudo-autosomal regions; give --par-region hg38|hg19|hg18|b37|b36|<end_par1>,<start_par2> "
                             "(or test the autosomes, or supply a sample file without sex codes of 1).");
  if (cm.sex_aware) {
    std::vector<uint8_t> grp(cm.male);
    blk.check(rg_s2_set_group(s2, grp.data(), cm.Mc.data()));      // (every part of a --gpus N run: its own context)
    if (part.part == 0) {
      int64_t nm = 0;
      for (uint8_t m : cm.male) nm += m;
      sout << " * chromosome " << p.nchrom << " (X): non-PAR region is (" << p.par1_max << ", " << p.par2_min << ") [--par-region " << p.build_code << "]; "
           << nm << " analysed males count half in the MAC there\n";
    }
  }
  if (cm.af_cc) blk.check(rg_s2_set_cases(s2, cm.Cc.data(), cm.Mc.data()));      // (every part of a --gpus N run: its own context)
  sout << std::left << std::setw(20) << " * block size" << ": [" << p.bsize << "]\n";
  sout << std::left << std::setw(20) << " * # blocks" << ": [" << cm.total_blocks << "]\n";
  sout << " * approximate memory usage : n/a (genotype blocks are tested on the GPU)\n";
  sout << " * using minimum MAC of " << p.min_mac << " (variants with lower MAC are ignored)\n";
  if (cm.coding == 2 && p.min_homs > 0) sout << " * ignoring variants (masks for gene-based tests) with fewer than " << p.min_homs << " homALT carriers\n";      // Data.cpp:2059-2060

  // output files, one per phenotype (split_by_pheno is the default; print_header_output_single, Step2_Models.cpp:2386-2398)
  std::vector<std::unique_ptr<TextOut>> ofs;
  for (int q = 0; q < P; ++q) {
    part.files.push_back(p.out + "_" + r.pheno_names[q] + ".regenie" + (cm.multi ? ".part" + std::to_string(part.part) : (p.gz ? ".gz" : "")));
    ofs.emplace_back(new TextOut(part.files.back(), cm.multi ? false : p.gz));
    if (!*ofs.back()) throw std::runtime_error("cannot write file : " + part.files.back());
    if (part.part == 0) *ofs.back() << "CHROM GENPOS ID ALLELE0 ALLELE1 A1FREQ " << (cm.af_cc ? "A1FREQ_CASES A1FREQ_CONTROLS " : "") << (cm.show_info ? "INFO " : "")
                                          << "N " << (cm.af_cc ? "N_CASES N_CONTROLS " : "") << "TEST BETA SE CHISQ LOG10P EXTRA\n";
  }
  std::unique_ptr<BedAhead> bed(cm.in == In::Bed ? new BedAhead(cm) : nullptr);
  std::unique_ptr<BgenAhead> bgen(cm.fast_bgen ? new BgenAhead(cm) : nullptr);
  if (bgen) bgen->start();
  int64_t n_ign[3] = {0, 0, 0};      // ignored variants, ignored tests, tests
  double ms_device = 0, ms_format = 0;
  int block = 0;
  for (int chrom : r.chr_read) {
    if (!cm.chr_snps.count(chrom)) continue;
    const std::vector<int64_t>& snps = cm.chr_snps.at(chrom);
    const int nb_chr = (int)((snps.size() + p.bsize - 1) / p.bsize);
    if (block + nb_chr <= part.blk_lo || block >= part.blk_hi) { block += nb_chr; continue; }     // none of the chromosome's blocks is this part's
    sout << "Chromosome " << chrom << " [" << nb_chr << " blocks in total]\n";
    null.set_up(chrom, s2);
    for (int bb = 0; bb < nb_chr; ++bb, ++block) {
      if (block < part.blk_lo || block >= part.blk_hi) continue;
      const int64_t j0 = (int64_t)bb * p.bsize;
      const int bs = (int)std::min<int64_t>(p.bsize, (int64_t)snps.size() - j0);
      sout << " block [" << block + 1 << "/" << cm.total_blocks << "] : ";
      auto t1 = std::chrono::steady_clock::now();
      blk.begin(bs);
      blk.vidx.resize(bs);
      for (int j = 0; j < bs; ++j) blk.vidx[j] = r.snp_offset[snps[j0 + j]];
      // fetch the genotypes
      const PreparedBlock* pb = nullptr;
      {
        std::unique_lock<std::mutex> rlk(g_reader_mu, std::defer_lock);
        if (cm.multi && cm.in != In::Bed && !bgen) rlk.lock();      // (the read-ahead's calls only read the handle)
        if (bgen && !(pb = bgen->next_block())->integral) pb = nullptr;
        if (cm.in == In::PgenHard) blk.read_pgen_hard();
        else if (cm.in == In::Dosage && !pb) blk.read_dosage_rows();
      }
      if (bed) {
        const int64_t jn = j0 + bs;
        blk.rows = bed->take(snps, j0, bs, (bb + 1 < nb_chr && block + 1 < part.blk_hi) ? (int)std::min<int64_t>(p.bsize, (int64_t)snps.size() - jn) : 0);
      }
      auto t_dev = std::chrono::steady_clock::now();
      BlockCounts bc(bs);
      bc.mark_non_par(cm, snps, j0);
      if (pb) blk.from_prepared(*pb, bc);
      else if (cm.in == In::Dosage) blk.from_dosage_rows(bc);
      else if (cm.glm || !cm.env.dense) blk.from_packed();
      else blk.from_dense_bed(bc);
      // score, correct, format
      if (cm.glm) blk.score_glm(bc); else blk.score_qt(bc);
      if (bc.any_nonpar) {     // the reference's warning (Geno.cpp:2453, :2705-2711): a hard call of 1 for a male counts 0.5
        std::vector<std::string> het;
        for (int j = 0; j < bs; ++j) if (bc.het_male[j]) het.push_back(r.snp_ids[snps[j0 + j]]);
        if (!het.empty()) {
          std::string msg = "WARNING: genotype is 1 for a male on chrX (males should coded as diploid) at variants [";
          for (size_t h = 0; h < het.size(); ++h) msg += (h ? ";" : "") + het[h];
          std::cerr << msg + "].\n";
        }
      }
      blk.coding_filters(bc);
      if (cm.glm && cm.correct) blk.correct(bc);
      if (cm.mcc) blk.mcc(bc);
      auto t_fmt = std::chrono::steady_clock::now();
      ms_device += std::chrono::duration<double, std::milli>(t_fmt - t_dev).count();
      blk.format(bc, snps, j0, ofs, n_ign);
      ms_format += ms_since(t_fmt);
      sout << "done (" << std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t1).count() << "ms) \n";
    }
  }
  BgenTiming bt;
  if (bgen) { bgen->report_device(); bt = bgen->timing; bgen.reset(); }
  if (cm.env.timing)
    fprintf(stderr, "[timing] step 2 part %d: host threads %d (read-ahead %d) | chromosome set-up %.0f ms | waiting for the prepared block %.0f ms (preparing: %.0f ms wall, overlapped; %.0f thread-ms inflate + %.0f thread-ms byte walk) | "
            "upload + device + results %.0f ms | formatting + writing %.0f ms\n", part.part, cm.nthreads, cm.nt_prep, null.ms_chr, bt.prep_wait, bt.prep_wall, bt.inflate, bt.walk, ms_device, ms_format);
  rg_s2_destroy(s2);
  part.n_ignored_snps = n_ign[0]; part.n_ignored_tests = n_ign[1];
  part.firth_body = null.firth_file_body;
  return 0;
}

// `--step 2` on G GPUs (G = 1: the calling thread): contiguous block ranges per GPU, floor(B / G) blocks each and the first B mod G one more
// (the split of write_l0_master, Data.cpp:270-302), one host thread and one library context per GPU, no collective on the data path.
int run_step2_all(Run& r, std::chrono::steady_clock::time_point t_start) {
  const Params& p = r.p;
  const int P = r.P, G = p.gpus;
  std::map<int, int64_t> cn;
  for (int c : r.snp_chrom) cn[c]++;
  int B = 0;
  for (auto& kv : cn) B += (int)((kv.second + p.bsize - 1) / p.bsize);
  std::vector<S2Part> parts(G);
  int b0 = 0;
  for (int g = 0; g < G; ++g) {
    parts[g].part = g; parts[g].nparts = G; parts[g].device = p.single_device ? p.device : p.device + g;
    parts[g].blk_lo = b0; b0 += B / G + (g < B % G ? 1 : 0); parts[g].blk_hi = b0;
  }
  if (G == 1) { parts[0].blk_hi = INT_MAX; run_step2(r, t_start, parts[0]); }
  else {
    sout << std::left << std::setw(20) << " * # GPUs" << ": [" << G << "] (blocks [1.." << B << "] in contiguous ranges)\n";
    std::vector<std::ostringstream> logs(G);
    std::vector<std::exception_ptr> errs(G, nullptr);
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g)
      th.emplace_back([&, g]() {
        tl_log = &logs[g];
        try { run_step2(r, t_start, parts[g]); } catch (...) { errs[g] = std::current_exception(); }
        tl_log = nullptr;
      });
    for (auto& t : th) t.join();
    for (int g = 0; g < G; ++g) {
      sout << " GPU " << g << " : blocks [" << parts[g].blk_lo + 1 << ".." << parts[g].blk_hi << "]\n";
      if (g == 0) sout << logs[g].str();
      else {   // the run-wide header lines were logged by part 0
        const std::string lg = logs[g].str();
        const size_t at = lg.find("Chromosome ");
        if (at != std::string::npos) sout << lg.substr(at);
      }
    }
    for (int g = 0; g < G; ++g)
      if (errs[g]) {   // a part failed: no partial result files are left behind
        for (int h = 0; h < G; ++h) for (auto& f : parts[h].files) if (!f.empty()) std::remove(f.c_str());
        std::rethrow_exception(errs[g]);
      }
    // the parts' result files in block order -> PFX_<trait>.regenie[.gz]
    for (int q = 0; q < P; ++q) {
      const std::string fn = p.out + "_" + r.pheno_names[q] + ".regenie" + (p.gz ? ".gz" : "");
      TextOut of(fn, p.gz);
      if (!of) throw std::runtime_error("cannot write file : " + fn);
      std::vector<char> buf(8 << 20);
      for (int g = 0; g < G; ++g) {
        std::ifstream in(parts[g].files[q], std::ios::binary);
        if (!in) throw std::runtime_error("cannot read the results of GPU " + std::to_string(g) + " : " + parts[g].files[q]);
        while (in) { in.read(buf.data(), (std::streamsize)buf.size()); of.write(buf.data(), in.gcount()); }
        if (in.bad() || !of) throw std::runtime_error("error while merging " + parts[g].files[q] + " into " + fn + " (disk full?)");
        in.close();
      }
      of.flush();
      if (!of) throw std::runtime_error("error while writing file : " + fn + " (disk full?)");
      for (int g = 0; g < G; ++g) std::remove(parts[g].files[q].c_str());    // only once the merged file is complete
      parts[0].files[q] = fn;
    }
  }
  if (p.write_null_firth) {   // print_null_firth_info (Step2_Models.cpp:1871-1900): PFX_<k>.firth per trait + PFX_firth.list
    std::ofstream fl(p.out + "_firth.list");
    for (int q = 0; q < P; ++q) {
      std::string body;
      std::set<std::string> seen;     // a chromosome that spans two parts was fitted by both: one line
      for (int g = 0; g < G; ++g) {
        std::istringstream is(parts[g].firth_body.empty() ? std::string() : parts[g].firth_body[q]);
        std::string ln;
        while (std::getline(is, ln)) { const std::string chr = ln.substr(0, ln.find(' ')); if (seen.insert(chr).second) body += ln + "\n"; }
      }
      if (body.empty()) continue;
      const std::string ffn = p.out + "_" + std::to_string(q + 1) + ".firth" + (p.gz ? ".gz" : "");
      TextOut ff(ffn, p.gz);
      if (!ff) throw std::runtime_error("cannot write file : " + ffn);
      ff << body;
      fl << r.pheno_names[q] << " " << (p.use_rel_path ? ffn : get_fullpath(ffn)) << "\n";
    }
    sout << "List of files with null Firth estimates written to: [" << p.out << "_firth.list]\n";
  }
  int64_t n_ignored = 0;
  for (auto& pt : parts) n_ignored += pt.n_ignored_snps * P + pt.n_ignored_tests;
  sout << "\nAssociation results stored separately for each trait in files : \n";
  for (auto& fn : parts[0].files) sout << "* [" << fn << "]\n";
  sout << "\nNumber of ignored tests due to low MAC" << (p.set_min_info ? " or info score" : "") << " : " << n_ignored << "\n";
  sout << "\nElapsed time : " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() << "s\nEnd of run\n";
  return 0;
}

}  // namespace rgdrv
