// regenie-amd, the C++ host driver (see driver.h): `--step 1` on the devices -- contexts, level 0 and level 1 on one GPU or a group -- and run().
#include "driver_step1.h"

namespace rgdrv {

struct Devices {                       // one context per GPU; torn down by teardown() only, never by unwinding
  std::vector<rg_ctx*> ctxs;
  rg_group* grp = nullptr;
};

// The HIP runtime and the device contexts come up on their own threads while the main one parses the text files (bringing the
// runtime up costs 150 - 200 ms, as much as the parsing)
static std::vector<std::shared_future<rg_ctx*>> start_contexts(const Params& p) {
  std::vector<std::shared_future<rg_ctx*>> early_ctx;
  if (p.step == 1 && !p.split_l0)
    for (int g = 0; g < p.gpus; ++g)
      early_ctx.push_back(std::async(std::launch::async, [&p, g]() -> rg_ctx* {
        rg_ctx* c = nullptr;
        if (rg_create(&c, p.single_device ? p.device : p.device + g, nullptr) != 0) return nullptr;
        return c;
      }).share());
  return early_ctx;
}

// ---- devices: one context per GPU, the problem on each, the group
static Devices bring_up_devices(const Run& r, const Step1Plan& pl, const std::vector<std::shared_future<rg_ctx*>>& early_ctx, Step1Ingest& ingest, Clock::time_point t_start) {
  const Params& p = r.p;
  const int G = pl.G, B = pl.B;
  Devices dev;
  dev.ctxs.assign(G, nullptr);
  rg_problem pr;
  memset(&pr, 0, sizeof(pr));
  pr.n_samples = r.N; pr.n_file = r.n_file; pr.n_pheno = r.P; pr.n_cov = r.C; pr.cv_folds = pl.use_loocv ? 0 : p.cv_folds;
  pr.n_ridge_l0 = pl.R0; pr.ref_first = p.ref_first; pr.n_analyzed = r.n_analyzed; pr.cv_sizes = pl.cv_sizes.data();
  pr.lambda = pl.lambda.data(); pr.X = r.X.data(); pr.Y = r.Y.data(); pr.mask = r.mask.data();
  pr.ind_in_analysis = r.ain.data(); pr.ind_ignore = (r.N != r.n_file) ? r.ind_ignore.data() : nullptr;
  pr.neff = r.neff.data(); pr.n_blocks_total = B; pr.max_block_size = p.bsize;
  for (int g = 0; g < G; ++g) dev.ctxs[g] = early_ctx[g].get();
  for (int g = 0; g < G; ++g) {
    rg_ctx* cx = dev.ctxs[g];
    if (!cx)
      throw std::runtime_error("no MI355X / HIP device available (rg_create failed for device " + std::to_string(p.single_device ? p.device : p.device + g) + ")");
    // level-0 workspaces in proportion to what this GPU will ingest: a run over a small file asks for small batches (the
    // bytes a process allocates are set-up time, for it and for the next process on the device), a large one gets the
    // library's default of 64 GB
    const int64_t bed_bytes = (int64_t)(B / G + 1) * p.bsize * r.bpr;
    const int64_t ws_bytes = std::max<int64_t>(6000000000LL, std::min<int64_t>(64000000000LL, 8 * bed_bytes));
    check(cx, rg_set_l0_workspace(cx, 0, 0, ws_bytes));
    // W ([B R0][P][Np] doubles), the level-0 workspaces and an allowance for level 1 beside a .bed kept in device memory
    if (g == 0) ingest.settle(cx, (int64_t)((double)B * pl.R0 * r.P * (double)(r.N + 4096) * 8.0 + (double)ws_bytes + 24e9));
    const auto tsp = Clock::now();
    check(cx, rg_set_problem(cx, &pr));
    if (getenv("RG_TIMING"))
      fprintf(stderr, "[timing] rg_set_problem (GPU %d): %.0f ms (entered %lld ms since start)\n", g, ms_dbl(tsp, Clock::now()), ms_int(t_start, tsp));
  }
  sout << "   -GPU context" << (G > 1 ? "s" : "") << " ready (" << ms_int(t_start, Clock::now()) << "ms since start)\n";
  if (pl.use_group) {
    if (rg_group_create(&dev.grp, G, dev.ctxs.data(), p.transport) != 0 || !dev.grp) throw std::runtime_error(std::string("cannot set up the GPU group: ") + rg_last_error(dev.ctxs[0]));
    sout << std::left << std::setw(20) << " * # GPUs" << ": [" << G << "] (" << (p.transport == RG_TRANSPORT_RCCL ? "RCCL" : "peer copies") << ")\n";
  }
  return dev;
}

// Every output file is written: the contexts' device memory (tens of GB of workspaces and W) and the runtime are left to process exit -- main()
// leaves through _exit -- instead of being freed buffer by buffer (80 - 100 ms of a 0.4 s run at BASELINE configs[1]); RG_TEARDOWN=1 frees them.
// INVARIANT the fast exit rests on: every output stream of the run (.loco / .prs / .firth / lists) is a local of a scope that has ended by
// here, so it is flushed and closed; main() flushes the log and stdout itself.  A tool that finalises at exit (rocprofv3, sanitizers,
// coverage) would lose its output, so the fast exit is off whenever one is detected, and RG_TEARDOWN=1 (the test suite sets it) always
// takes the full path: the ingest first -- its staged buffer belongs to a context -- then contexts, RCCL communicators and the runtime are
// torn down in order, which is also what surfaces leaks.
static void teardown(Step1Ingest& ingest, Devices& dev) {
  if (!full_teardown()) { fast_exit = true; return; }
  ingest.release();
  if (dev.grp) rg_group_destroy(dev.grp);
  for (rg_ctx* cx : dev.ctxs) rg_destroy(cx);
}

// --run-l1: read_l0 (Step1_Models.cpp:1921-1987): every job file holds N x (blocks_k * R0) raw doubles, column-major,
// block-major then ridge index; its columns go to W at block offset bstart_k
static void read_l0_files(rg_ctx* ctx, const Run& r, const Step1Plan& pl) {
  const int64_t N = r.N;
  std::vector<double> slab((size_t)N * pl.R0);
  for (size_t k = 0; k < r.mprefix.size(); ++k)
    for (int q = 0; q < r.P; ++q) {
      const std::string fn = r.mprefix[k] + "_l0_Y" + std::to_string(q + 1);
      std::ifstream lf(fn, std::ios::binary | std::ios::ate);
      if (!lf) throw std::runtime_error("cannot read file : " + fn);
      const int64_t want = (int64_t)sizeof(double) * N * r.btot[k] * pl.R0;
      if ((int64_t)lf.tellg() != want) throw std::runtime_error("file " + fn + " is not the right size.");   // Step1_Models.cpp:1962
      lf.seekg(0);
      for (int bb = 0; bb < r.btot[k]; ++bb) {
        lf.read((char*)slab.data(), sizeof(double) * slab.size());
        if (!lf) throw std::runtime_error("cannot read file : " + fn);
        check(ctx, rg_l0_set_w(ctx, r.bstart[k] + bb, q, slab.data()));
      }
    }
  sout << "   -level 0 predictors read from the job files\n";
}

// --run-l0: write_l0_file (Step1_Models.cpp:728-734): PFX_job<k>_l0_Y<ph>
static void write_l0_files(rg_ctx* ctx, const Run& r, const Step1Plan& pl) {
  std::vector<double> slab((size_t)r.N * pl.R0);
  for (int q = 0; q < r.P; ++q) {
    const std::string fn = r.job_prefix + "_l0_Y" + std::to_string(q + 1);
    std::ofstream lf(fn, std::ios::binary);
    if (!lf) throw std::runtime_error("cannot write file : " + fn);
    for (int bb = 0; bb < pl.B; ++bb) {
      check(ctx, rg_l0_get_w(ctx, bb, q, slab.data()));
      lf.write((const char*)slab.data(), sizeof(double) * slab.size());
    }
  }
  sout << "   -level 0 predictions written to [" << r.job_prefix << "_l0_Y*]\n";
}

// Level 1 of phenotypes [q0, q0 + nq) on one context whose view holds exactly them: cumsum [nq][NCS][R1], converged / best [nq], pred [nq][nchr][N].
static void level1_call(rg_ctx* cx, const Run& r, Step1Plan& pl, int q0, int nq, double* cumsum, int32_t* converged, int32_t* best, double* pred) {
  const Params& p = r.p;
  const int64_t N = r.N;
  const int R1 = pl.R1, nchr = pl.nchr;
  const int32_t* cols = pl.cols_per_chr.data();
  double* tq = pl.tau.data() + (size_t)q0 * R1;
  if (p.t2e) {   // one call per trait: the library derives the penalties from the score at beta = 0 and returns them
    rg_cox_options co{};
    co.niter_max = p.niter_max; co.niter_max_line_search = p.niter_max_line_search; co.niter_max_ridge = p.niter_max_ridge;
    co.niter_max_line_search_ridge = 100; co.numtol_cox = 2.5e-4; co.l1_ridge_tol = 1e-4;
    const std::vector<double> tau_in(tq, tq + (size_t)nq * R1);   // --t2e-l1-pi6: the grid of the caller's (the call writes the penalties it used back into tau)
    for (int q = 0; q < nq; ++q) {
      co.tau = p.t2e_l1_pi6 ? tau_in.data() + (size_t)q * R1 : nullptr;
      double* cq = cumsum + (size_t)q * pl.NCS * R1;
      std::fill(cq, cq + (size_t)pl.NCS * R1, 0.0);
      if (!r.pheno_pass[q0 + q]) { converged[q] = 0; best[q] = 0; continue; }   // no offset to fit against: skipped like the other trait modes
      check(cx, rg_l1_cox(cx, q0 + q, R1, r.Yraw.data() + (size_t)(q0 + q) * N, r.Yevent.data() + (size_t)(q0 + q) * N, r.offset.data() + (size_t)(q0 + q) * N, &co,
                          nchr, cols, tq + (size_t)q * R1, cq + 5 * R1, &converged[q], &best[q], pred + (size_t)q * nchr * N));
    }
  } else if (p.bt || p.ct) {
    rg_bt_options bo{};  // Regenie.hpp:287-290 defaults; family picks ridge_logistic_level_1* or ridge_poisson_level_1*
    bo.niter_max_ridge = p.niter_max_ridge; bo.niter_max_line_search_ridge = 100; bo.niter_max_line_search = p.niter_max_line_search;
    bo.family = p.ct ? 1 : 0; bo.l1_ridge_tol = 1e-4; bo.tol = 1e-8;
    check(cx, rg_l1_bt(cx, R1, tq, r.Yraw.data() + (size_t)q0 * N, r.offset.data() + (size_t)q0 * N, &bo, nchr, cols, cumsum, converged, best, pred));
    for (int q = 0; q < nq; ++q) if (!r.pheno_pass[q0 + q]) converged[q] = 0;
  } else if (pl.use_loocv)
    check(cx, rg_l1_qt_loocv(cx, R1, tq, nchr, cols, cumsum, best, pred));
  else
    check(cx, rg_l1_qt(cx, R1, tq, nchr, cols, cumsum, best, pred));
}

// One context, no exchanged view (the usual single-GPU run): the phenotypes are taken ONE AT A TIME (rg_set_l1_view with a sub-range on
// the context's own W) and each one's tables and files are written on a thread of their own while the next phenotype is on the GPU --
// at 500,000 samples a .loco file is 115 MB of text, formatting and writing ten of them took as long as level 1 itself.
// The predictions of a phenotype ([nchr][N] doubles, 92 MB at BASELINE configs[2]) land in one of three page-locked slots -- the GPU fills one
// while the writers of the two phenotypes before it read theirs.  The slots are allocated on a thread of their own while level 0 streams
// (l1_slots_start): page-locking all ten phenotypes' 920 MB at the head of level 1 cost 0.25 s of its 0.96 s (RG_TIMING=1).
constexpr int L1_SLOTS = 3;
static std::future<double*> l1_slots_start(const Run& r, const Step1Plan& pl) {
  const int64_t bytes = (int64_t)sizeof(double) * pl.nchr * r.N * std::min(r.P, L1_SLOTS);
  return std::async(std::launch::async, [bytes]() { return (double*)rg_host_alloc(bytes); });
}
static void level1_pipelined(rg_ctx* cx, const Run& r, Step1Plan& pl, LocoWriter& out, std::future<double*> l1_slots) {
  const Params& p = r.p;
  const int P = r.P, R1 = pl.R1, NCS = pl.NCS;
  const bool timing_on = getenv("RG_TIMING") != nullptr;
  const size_t per = (size_t)pl.nchr * r.N;
  const int nslot = std::min(P, L1_SLOTS);
  const auto ta0 = Clock::now();
  double* pred = l1_slots.get();             // page-locked if the runtime grants it (device -> host at the PCIe rate, no first-touch faults),
  std::unique_ptr<double[]> pred_own;        // uninitialised either way -- every entry is written by the library
  const bool pinned = pred != nullptr;
  if (!pinned) { pred_own.reset(new double[per * nslot]); pred = pred_own.get(); }
  if (timing_on)
    fprintf(stderr, "[timing] level 1: waited %.0f ms for the %d prediction slots (%s)\n", ms_dbl(ta0, Clock::now()), nslot, pinned ? "page-locked" : "pageable");
  std::vector<double> cumsum((size_t)P * NCS * R1, 0.0);
  std::vector<int32_t> best(P, 0), converged(P, 1);
  std::vector<std::future<void>> writers;
  std::exception_ptr err = nullptr;
  try {
    for (int q = 0; q < P; ++q) {
      double* cq = cumsum.data() + (size_t)q * NCS * R1;
      double* pq = pred + (size_t)(q % nslot) * per;
      const auto tw0 = Clock::now();
      if (q >= nslot) writers[q - nslot].wait();      // the slot's previous phenotype is on disk (at most nslot - 1 writers in flight behind the GPU)
      const auto tq0 = Clock::now();
      if (!p.t2e) check(cx, rg_set_l1_view(cx, nullptr, q, 1));
      level1_call(cx, r, pl, q, 1, cq, &converged[q], &best[q], pq);
      const int bq = best[q], cv = converged[q];
      if (timing_on)
        fprintf(stderr, "[timing] level 1 of phenotype %d: waited %.0f ms for its slot, on the GPU %.0f ms\n", q + 1, ms_dbl(tw0, tq0), ms_dbl(tq0, Clock::now()));
      writers.push_back(std::async(std::launch::async, [&out, q, cq, bq, cv, pq]() { out.emit(q, cq, bq, cv, pq); }));
    }
  } catch (...) { err = std::current_exception(); }
  if (!p.t2e) rg_set_l1_view(cx, nullptr, 0, P);
  for (auto& w : writers) { try { w.get(); } catch (...) { if (!err) err = std::current_exception(); } }
  if (pinned) rg_host_free(pred);
  if (err) std::rethrow_exception(err);
}

// level 1 of phenotypes [q0, q0 + nq) on one context (its view already set for a phenotype-sharded run)
static void level1_range(rg_ctx* cx, const Run& r, Step1Plan& pl, LocoWriter& out, int q0, int nq, bool write_out) {
  const size_t ncs = (size_t)pl.NCS * pl.R1, per = (size_t)pl.nchr * r.N;
  std::vector<double> cumsum(nq * ncs), pred(nq * per);
  std::vector<int32_t> best(nq), converged(nq, 1);
  level1_call(cx, r, pl, q0, nq, cumsum.data(), converged.data(), best.data(), pred.data());
  for (int q = 0; q < nq && write_out; ++q) out.emit(q0 + q, cumsum.data() + q * ncs, best[q], converged[q], pred.data() + q * per);
}

static void level0_logged(Step1Ingest& ingest, rg_ctx* ctx, const Step1Plan& pl) {
  std::ostringstream lg;
  ingest.level0(ctx, pl.blocks, 0, pl.B, lg, false);
  sout << lg.str();
}

// one GPU without the exchange: level 0 (unless --run-l1 read it), then the pipelined level 1; returns when level 1 started
static Clock::time_point levels_single(rg_ctx* ctx, const Run& r, Step1Plan& pl, Step1Ingest& ingest, LocoWriter& out) {
  std::future<double*> l1_slots = l1_slots_start(r, pl);
  if (!r.p.run_l1) level0_logged(ingest, ctx, pl);
  sout << "\n Level 1 ridge...\n";
  if (r.p.ct) sout << " Level 1 ridge with poisson regression...\n";
  if (r.p.t2e) sout << " Level 1 ridge with cox regression...\n";
  const auto tl0 = Clock::now();
  level1_pipelined(ctx, r, pl, out, std::move(l1_slots));
  return tl0;
}

// one rank of a group: level 0 of the rank's blocks, the exchange, level 1 of the rank's phenotypes (phenotype-sharded) or of all
// phenotypes with the heavy steps shared (all-gather form; level-1 models other than the K-fold ridge run on rank 0 alone there)
static void rank_levels(int g, Devices& dev, const Run& r, Step1Plan& pl, Step1Ingest& ingest, LocoWriter& out, std::string& rank_log) {
  rg_ctx* cx = dev.ctxs[g];
  const int32_t* pbeg = pl.pheno_sharded ? pl.pbeg.data() : nullptr;
  const bool shared_l1 = !pl.pheno_sharded && !(r.p.bt || r.p.ct || r.p.t2e) && !pl.use_loocv;
  std::ostringstream lg;
  // the exchange buffers of this rank (phenotype view, packed send buffer) are allocated before level 0 starts
  check(cx, rg_group_prepare(dev.grp, g, pl.bbeg.data(), pbeg));
  ingest.level0(cx, pl.blocks, pl.bbeg[g], pl.bbeg[g + 1], lg, true);
  rank_log = lg.str();
  check(cx, rg_l0_finish(dev.grp, g, pl.bbeg.data(), pbeg));
  if (pl.pheno_sharded) level1_range(cx, r, pl, out, pl.pbeg[g], pl.pbeg[g + 1] - pl.pbeg[g], true);
  else if (shared_l1 || g == 0) level1_range(cx, r, pl, out, 0, r.P, g == 0);
}

// one host thread per GPU
static void levels_group(Devices& dev, const Run& r, Step1Plan& pl, Step1Ingest& ingest, LocoWriter& out) {
  const int G = pl.G;
  std::vector<std::string> rank_log(G);
  std::vector<std::exception_ptr> errs(G, nullptr);
  std::vector<std::thread> th;
  for (int g = 0; g < G; ++g)
    th.emplace_back([&, g]() {
      try { rank_levels(g, dev, r, pl, ingest, out, rank_log[g]); }
      catch (...) {
        // whatever failed here (reader, file, level 0, level 1): the group is broken, so that the other ranks -- waiting in
        // the exchange or in a shared level-1 all-reduce, now or later -- fail too instead of waiting for this one
        errs[g] = std::current_exception();
        rg_group_abort(dev.grp, g);
      }
    });
  for (auto& t : th) t.join();
  for (int g = 0; g < G; ++g) {
    sout << " GPU " << g << " : blocks [" << pl.bbeg[g] + 1 << ".." << pl.bbeg[g + 1] << "]"
         << (pl.pheno_sharded ? ", level 1 of phenotypes [" + std::to_string(pl.pbeg[g] + 1) + ".." + std::to_string(pl.pbeg[g + 1]) + "]" : std::string()) << "\n" << rank_log[g];
  }
  // report the rank that failed first-hand, not a peer that only noticed it
  std::exception_ptr any = nullptr;
  for (int g = 0; g < G; ++g) {
    if (!errs[g]) continue;
    if (!any) any = errs[g];
    try { std::rethrow_exception(errs[g]); }
    catch (const std::exception& e) { if (!strstr(e.what(), "another GPU")) std::rethrow_exception(errs[g]); }
    catch (...) { std::rethrow_exception(errs[g]); }
  }
  if (any) std::rethrow_exception(any);
  sout << "\n Level 1 ridge...\n";
}

static void log_banner(const Params& p, int argc, char** argv) {
  sout << "              |=============================|\n              |   REGENIE-AMD (step 1, HIP)  |\n              |=============================|\n\n";
  sout << "Log of output saved in file : " << p.out << ".log\n\nOptions in effect:\n";
  for (int i = 1; i < argc; ++i) sout << (argv[i][0] == '-' && argv[i][1] == '-' ? "  " : " ") << argv[i] << (i + 1 < argc && argv[i + 1][0] == '-' ? " \\\n" : "");
  sout << "\n\nFitting null model\n";
}

int run(int argc, char** argv) {
  Run r;
  r.p = parse_args(argc, argv);
  const Params& p = r.p;
  sout.f.open(p.out + ".log");
  const auto t_start = Clock::now();
  auto since_start = [&]() { return ms_int(t_start, Clock::now()); };
  auto elapsed = [&]() { return std::chrono::duration<double>(Clock::now() - t_start).count(); };
  log_banner(p, argc, argv);
  const auto early_ctx = start_contexts(p);
  if (p.run_l0) prep_parallel_l0(r);
  read_bim_fam(r);
  if (p.split_l0) return split_l0(r);
  sout << "   -genotype metadata read (" << since_start() << "ms since start)\n";
  Step1Ingest ingest(r, t_start);
  ingest.start_early(early_ctx);
  read_pheno_cov(r);
  sout << "   -phenotypes and covariates ready (" << since_start() << "ms since start)\n";
  if (p.compute_corr) {
    if (!run_ld_entry) throw std::runtime_error("--compute-corr is not part of this build of the driver.");
    return run_ld_entry(r, t_start);
  }
  if (p.step == 2) return run_step2_all(r, t_start);

  Step1Plan pl = plan_step1(r);
  Devices dev = bring_up_devices(r, pl, early_ctx, ingest, t_start);
  rg_ctx* ctx = dev.ctxs[0];
  ingest.map_ready();
  if (p.run_l1) read_l0_files(ctx, r, pl);
  if (p.run_l0) {  // level 0 of this job, its predictions to the job's files, and stop (Data.cpp:113-117)
    level0_logged(ingest, ctx, pl);
    write_l0_files(ctx, r, pl);
    ingest.release();
    rg_destroy(ctx);
    sout << "\nElapsed time : " << elapsed() << "s\nEnd of run\n";
    return 0;
  }
  LocoWriter out(r, pl);
  auto tl0 = Clock::now();
  if (!pl.use_group) tl0 = levels_single(ctx, r, pl, ingest, out);
  else levels_group(dev, r, pl, ingest, out);
  sout << "   -level 1 for " << r.P << " phenotype(s) done (" << ms_int(tl0, Clock::now()) << "ms)\n\n";
  sout << "   -predictions written (" << since_start() << "ms since start)\n";
  out.write_lists();
  if (p.run_l1 && !p.keep_l0)   // rm_l0_files (Data.cpp:1131-1147)
    for (auto& pre : r.mprefix)
      for (int q = 0; q < r.P; ++q) std::remove((pre + "_l0_Y" + std::to_string(q + 1)).c_str());
  teardown(ingest, dev);
  sout << "\nElapsed time : " << elapsed() << "s\nEnd of run\n";
  return 0;
}

}  // namespace rgdrv
