// regenie-amd, the C++ host driver (see driver.h): the genotype ingest of `--step 1` (Step1Ingest of driver_step1.h) -- the three sources of
// level 0's rows and the one owner of their threads, buffers and teardown.
#include "driver_step1.h"
#include <sys/mman.h>

namespace rgdrv {

// Ring of host buffers between the .bed / .pgen reader thread and rg_l0_blocks (the block loop of Data.cpp:636-678 with the file
// read taken off the critical path).  The buffers are page-locked -- copies to the device are then asynchronous and run at the
// PCIe rate -- on a thread of their own: page-locking costs ~0.2 s per GB, so a run on one GPU starts it while the phenotype and
// covariate files are still being parsed and the reader takes each buffer as it becomes ready.
struct IngestRing {
  static constexpr int NBUF = 3;
  int per = 1;                       // SNP blocks per buffer
  bool pinned = true, failed = false;
  uint8_t* mem[NBUF] = {nullptr, nullptr, nullptr};
  std::mutex mu; std::condition_variable cv; std::deque<int> free_q;
  std::thread th;
  // total_bytes: the rows this ring will carry; blk_bytes: one block; max_per: most blocks per buffer (the library's batch size) or
  // <= 0 when not known yet; pin: 1 / 0 forces page-locked / pageable buffers, -1 page-locks only when the input is several rings long
  void start(int64_t total_bytes, int64_t blk_bytes, int max_per, int pin) {
    int64_t slot = std::max<int64_t>(16LL << 20, std::min<int64_t>(total_bytes / 8, 4LL << 30));
    if (const char* e = getenv("RG_INGEST_MB")) slot = (int64_t)std::max(1, atoi(e)) << 20;
    per = (int)std::max<int64_t>(1, slot / std::max<int64_t>(1, blk_bytes));
    if (max_per > 0) per = std::min(per, max_per);
    const int64_t bytes = (int64_t)per * blk_bytes;
    pinned = pin >= 0 ? pin != 0 : total_bytes >= 4 * NBUF * bytes;
    if (const char* e = getenv("RG_INGEST_PINNED")) pinned = atoi(e) != 0;
    th = std::thread([this, bytes]() {
      for (int i = 0; i < NBUF; ++i) {
        uint8_t* m = pinned ? (uint8_t*)rg_host_alloc(bytes) : (uint8_t*)aligned_alloc(4096, (size_t)(bytes + 4095) / 4096 * 4096);
        std::lock_guard<std::mutex> lk(mu);
        if (!m) { failed = true; cv.notify_all(); return; }
        mem[i] = m;
        free_q.push_back(i);
        cv.notify_all();
      }
    });
  }
  // Un-pinning costs what pinning did (0.1 - 0.15 s per GB: 1.4 s for the three 4.2 GB buffers of BASELINE configs[2], measured between the
  // end of level 0 and the start of level 1 -- round 6, gpurun_out/r6_ingest): a run that leaves through _exit (the default, see the end of
  // run_step1) hands the buffers back to the system with the process instead.
  void release() {
    if (th.joinable()) th.join();
    for (auto& m : mem) { if (m && full_teardown()) { if (pinned) rg_host_free(m); else free(m); } m = nullptr; }
  }
  ~IngestRing() { release(); }
};

// The .bed itself as the source of the host -> device copies: the file is mapped and the mapping registered (read-only) with the runtime on a
// thread of its own while the text files are parsed; the pages of the page cache are then what the DMA engines read -- no pread, no host
// buffer, no page-locking of 4 GB slots (which, at 5 GB/s, also slowed the parsing it ran beside).  tools/ingest_probe.cpp: registering an
// 8 GB mapping takes 0.08 s and copies from it run at 57 GB/s.  Used for one GPU when every block's variants are consecutive in the file
// (no --extract / --exclude gaps inside a block); RG_INGEST_MAP=0, a mapping or a registration that fails, fall back on the ring.
struct BedMap {
  int fd = -1;
  uint8_t* base = nullptr;
  size_t bytes = 0;
  int state = 0;                       // 0 not started / unusable, 1 registering, 2 registered
  std::thread th;
  void start(const std::string& path, bool want_registered) {
    fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return;
    const off_t sz = lseek(fd, 0, SEEK_END);
    if (sz <= 3) return;
    void* m = mmap(nullptr, (size_t)sz, PROT_READ, MAP_SHARED, fd, 0);
    if (m == MAP_FAILED) return;
    base = (uint8_t*)m; bytes = (size_t)sz; state = 1;
    // RG_INGEST_MAP=2: the mapping is NOT registered -- the copies then go through the runtime's own staging of pageable memory
    registered = getenv("RG_INGEST_MAP") ? atoi(getenv("RG_INGEST_MAP")) != 2 : want_registered;
    if (!registered) { state = 2; return; }
    th = std::thread([this]() { if (rg_host_register(base, (int64_t)bytes, 1) != 0) state = -1; else state = 2; });
  }
  bool registered = true;
  bool ready() { if (th.joinable()) th.join(); return state == 2; }
  ~BedMap() {
    if (th.joinable()) th.join();
    if (fast_exit) return;                 // the process is about to leave through _exit: the mapping goes with it
    if (state == 2 && registered) rg_host_unregister(base);
    if (base) munmap(base, bytes);
    if (fd >= 0) close(fd);
  }
};

// The whole .bed staged in HBM (rg_stage_*, include/rg_step1.h): from the moment the runtime is up -- under the parsing of the phenotype and
// covariate files and under rg_set_problem -- the file is copied to the device, and level 0 reads the rows in place.  A few threads pread
// 32 MB pieces of the file into a small ring of page-locked slots (8 x 32 MB: page-locking them costs 50 ms, not the 1.4 s of the 12.6 GB
// ring of round 5), one thread sends the pieces in file order (DMA from page-locked memory: the PCIe rate, where the runtime's staging of
// pageable memory gave 36 - 38 GB/s).  At BASELINE configs[2] (62.5 GB) the copy starts 0.3 s earlier than the first batch of the
// streamed form did and the level-0 thread queues kernels only.  One GPU, a file of at least 4 GB and at most a quarter of the free device memory whose kept
// variants are one range covering at least 80 % of it; RG_INGEST_STAGE=0 streams the file batch by batch as before, =2 copies from the
// mapping instead of the slots.  A copy that fails leaves the bytes behind `done` unusable: level 0 takes the rest from the mapping.
struct BedStage {
  static constexpr int NS = 8;
  rg_ctx* ctx = nullptr;
  uint8_t* dev = nullptr;
  int64_t bytes = 0, piece = 32LL << 20, npieces = 0;
  std::atomic<int64_t> done{0}, next_piece{0};
  std::atomic<int> state{0};           // 0 not used, 1 copying, 2 complete, -1 failed / refused
  std::atomic<bool> stop{false};
  std::mutex mu;
  std::condition_variable cv;
  std::thread th;
  std::vector<std::thread> fillers;
  uint8_t* slot[NS] = {};
  int64_t filled[NS] = {};             // (mu) piece number + 1 held by the slot, 0 = free
  int64_t sent = 0;                    // (mu) pieces in device memory
  int fd = -1;
  int nfill = 0;
  std::chrono::steady_clock::time_point t_first, t_last;
  void fail() { { std::lock_guard<std::mutex> lk(mu); state = -1; } cv.notify_all(); }
  void fill_loop() {
    for (;;) {
      const int64_t k = next_piece++;
      if (k >= npieces) return;
      const int si = (int)(k % NS);
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return sent + NS > k || state < 0 || stop; });      // piece k - NS has left the slot
        if (state < 0 || stop) return;
      }
      if (!slot[si] && !(slot[si] = (uint8_t*)rg_host_alloc(piece))) return fail();
      const int64_t off = k * piece, n = std::min(piece, bytes - off);
      for (int64_t got = 0; got < n;) {
        const ssize_t rd = pread(fd, slot[si] + got, (size_t)(n - got), (off_t)(off + got));
        if (rd <= 0) return fail();
        got += rd;
      }
      { std::lock_guard<std::mutex> lk(mu); filled[si] = k + 1; }
      cv.notify_all();
    }
  }
  void start(std::shared_future<rg_ctx*> fctx, const std::string& path, const uint8_t* mapped, int64_t nbytes, int mode, int threads) {
    bytes = nbytes;
    npieces = (bytes + piece - 1) / piece;
    nfill = threads;
    state = 1;
    if (mode != 2) fd = open(path.c_str(), O_RDONLY);
    const bool from_map = fd < 0;
    th = std::thread([this, fctx, mapped, from_map]() {
      ctx = fctx.get();
      if (!ctx) return fail();
      dev = (uint8_t*)rg_stage_alloc(ctx, bytes, 0.25);
      if (!dev) return fail();
      t_first = std::chrono::steady_clock::now();
      if (!from_map)
        for (int t = 0; t < nfill; ++t) fillers.emplace_back([this]() { fill_loop(); });
      for (int64_t k = 0; k < npieces; ++k) {
        const int64_t off = k * piece, n = std::min(piece, bytes - off);
        const int si = (int)(k % NS);
        const uint8_t* src = mapped + off;
        if (!from_map) {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return filled[si] == k + 1 || state < 0 || stop; });
          if (filled[si] != k + 1) { lk.unlock(); return fail(); }
          src = slot[si];
        }
        if (stop || rg_stage_copy(ctx, dev + off, src, n) != 0) return fail();
        { std::lock_guard<std::mutex> lk(mu); filled[si] = 0; sent = k + 1; done = off + n; }
        cv.notify_all();
      }
      t_last = std::chrono::steady_clock::now();
      { std::lock_guard<std::mutex> lk(mu); state = 2; }
      cv.notify_all();
    });
  }
  // the stage is given up (W, the workspaces and level 1 would not fit beside it): the copy stops, the buffer goes back, level 0 streams the file
  void cancel() {
    if (state == 0) return;
    stop = true;
    cv.notify_all();
    if (th.joinable()) th.join();
    for (auto& f : fillers) if (f.joinable()) f.join();
    fillers.clear();
    { std::lock_guard<std::mutex> lk(mu); state = -1; done = 0; }      // (nothing of the buffer counts as arrived any more)
    if (dev) { rg_stage_free(ctx, dev); dev = nullptr; }
  }
  bool live() const { return state > 0; }      // a copy is under way or complete: not refused its buffer, failed or given up
  // true once bytes [0, upto) are in device memory; false when the copy failed (or was never started)
  bool wait(int64_t upto) {
    if (state == 0) return false;
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done >= upto || state < 0; });
    return done >= upto;
  }
  ~BedStage() {
    stop = true;                        // (a run that failed before level 0 was through does not wait for the rest of the file)
    cv.notify_all();
    if (th.joinable()) th.join();
    for (auto& f : fillers) if (f.joinable()) f.join();
    if (fd >= 0) close(fd);
    if (full_teardown()) {
      for (auto& m : slot) if (m) rg_host_free(m);
      if (dev) rg_stage_free(ctx, dev);
    }
  }
};

struct Step1Ingest::State {
  IngestRing pre_ring;
  IngestRing* pre_ring_ptr = nullptr;  // the ring whose page-locking start_early began, if it did
  BedMap bed_map;
  BedStage bed_stage;                  // declared after bed_map: its thread reads the mapping and is joined first
  bool mapped_ok = false;              // the mapping is usable (map_ready: the rank threads only read the flag)
  std::mutex io_mu;                    // the .pgen / .bgen readers keep per-handle state: one block read at a time
};

Step1Ingest::Step1Ingest(const Run& run, Clock::time_point t0) : r(run), t_start(t0), ingest_blk_bytes((int64_t)run.p.bsize * run.bpr), s(new State) {}
Step1Ingest::~Step1Ingest() { release(); }

// The threads are joined and the staged device buffer, the slots and the mapping handed back (~BedStage, ~BedMap, ~IngestRing) here and nowhere
// else; nothing of the ingest can be used afterwards.
void Step1Ingest::release() { s.reset(); }
void Step1Ingest::alive() const { if (!s) throw std::logic_error("the genotype ingest was used after its release()"); }

void Step1Ingest::start_early(const std::vector<std::shared_future<rg_ctx*>>& early_ctx) {
  alive();
  const Params& p = r.p;
  if (!(p.step == 1 && !p.run_l1 && !r.dosage_mode && r.bpr > 0)) return;   // the host side of the ingest is set up under the parsing of the text files
  IngestRing& pre_ring = s->pre_ring; BedMap& bed_map = s->bed_map; BedStage& bed_stage = s->bed_stage;
  // The mapped .bed is the source of the copies (rounds 3 - 5: registered with the runtime, and only for files up to 16 GB -- for the 62.5 GB
  // file of configs[2] the registered mapping and the ring of page-locked buffers traded places from box to box: DESIGN_HISTORY.md).
  // Round 6: ONE GPU takes the mapping UNREGISTERED, whatever the file's size -- the copies then go through the runtime's staging of pageable
  // memory, and nothing is page-locked: at configs[2] the page-locking of the ring (12.6 GB, on a thread beside the parsing) delayed the
  // runtime's start-up by 1.4 s and cost 1.4 s again when it was released; measured on a device whose memory was clean: ring 5.6 - 6.1 s,
  // registered mapping 4.4 s, unregistered mapping 3.55 s (level 0 of the 62.5 GB file queued in 1.63 s = 38 GB/s, context ready after
  // 0.42 s); configs[1]: predictions written after 0.17 - 0.19 s instead of 0.26 - 0.31 s (gpurun_out/r6_ingest, tools/r6_ingest_small.sh).
  // RG_INGEST_MAP=1 registers the mapping (several GPUs: the ranks share it and their copies are asynchronous), =0 takes the ring.
  const char* em = getenv("RG_INGEST_MAP");
  const bool want_map = em ? atoi(em) != 0 : true;
  if (!r.pgen && want_map) bed_map.start(p.bed + ".bed", p.gpus > 1);           // the mapped file, registered on its own thread (shared by the ranks)
  {
    const char* es = getenv("RG_INGEST_STAGE");
    const int64_t kept_bytes = (int64_t)r.snp_chrom.size() * r.bpr;
    if (p.gpus == 1 && !p.force_collectives && bed_map.state == 2 && !bed_map.registered && !(es && atoi(es) == 0) && !early_ctx.empty() &&
        (int64_t)bed_map.bytes >= ((es && atoi(es) != 0) ? 4 : (4LL << 30)) && 5 * kept_bytes >= 4 * ((int64_t)bed_map.bytes - 3) && !r.snp_offset.empty() &&      // (a file of a few GB is in HBM before the ring's slots are page-locked: configs[1], 1.25 GB, 0.20 s without the stage, 0.24 s with it; RG_INGEST_STAGE=1 forces it)
        r.snp_offset.back() - r.snp_offset.front() + 1 == (int64_t)r.snp_offset.size())      // the kept variants: one range of the file
      bed_stage.start(early_ctx[0], p.bed + ".bed", bed_map.base, (int64_t)bed_map.bytes, es ? atoi(es) : 1,
                      getenv("RG_STAGE_THREADS") ? std::max(1, atoi(getenv("RG_STAGE_THREADS"))) : std::max(2, std::min(6, usable_cpus() / 3)));     // 2 threads fed 24 GB/s, 4 and 8 the 50 GB/s the DMA takes (gpurun_out/r6_ingest)
  }
  if (bed_map.state == 0 && p.gpus == 1) {                                         // else, one GPU: the ring of page-locked buffers
    pre_ring.start((int64_t)r.snp_chrom.size() * r.bpr, ingest_blk_bytes, -1, 1);
    s->pre_ring_ptr = &pre_ring;
  }
}

void Step1Ingest::settle(rg_ctx* ctx0, int64_t need_bytes) {
  // W ([B R0][P][Np] doubles), the level-0 workspaces and an allowance for level 1 must still fit beside the staged file -- known only now
  // that the phenotypes are parsed; if they do not, the stage is given up and the file streams batch by batch.  A stage that was refused
  // its buffer or failed is not live: there is nothing to give up and nothing to report.
  // REMAINING RACE, left on purpose: the question is asked while the stage thread may still be on its way to rg_stage_alloc (state 1 counts
  // as live), so the stage's own bytes may or may not be taken yet, and a stage that is about to be refused can still be "given up" with
  // its log line.  Waiting here until the stage thread has its buffer or has failed was built and measured: on a device that is still
  // scrubbing the memory of the process before, rg_stage_fits then says no where it said yes before, the stage is given up, and the 62.5 GB
  // run from files took 3.26 - 3.34 s instead of 2.80 - 2.91 s.  Which route is taken when is not this function's to change.
  alive();
  if (!s->bed_stage.live()) return;
  if (!rg_stage_fits(ctx0, need_bytes) || getenv("RG_STAGE_FORCE_CANCEL")) {      // (the switch: for the test of this path)
    s->bed_stage.cancel();
    sout << "   -the genotype file is not kept in device memory (" << (int64_t)((double)need_bytes / 1e9) << " GB of predictors and workspaces take the room)\n";
  }
}

void Step1Ingest::map_ready() { alive(); s->mapped_ok = s->bed_map.state != 0 && s->bed_map.ready(); }

// get_G + the block loop of level_0_calculations (Data.cpp:636-678) with the file read taken off the critical path: a
// reader thread fills page-locked buffers (one pread per block when its variants are contiguous in the file, Geno.cpp:
// 1702-1769 reads them one by one), the calling thread hands each buffer to rg_l0_blocks -- asynchronous copies, kernels
// queued behind the previous batch on the other pipeline -- and recycles it once its copy has completed (rg_ingest_fence).
void Step1Ingest::level0(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg, bool in_group) {
  alive();
  if (b_lo >= b_hi) return;
  IngestRing* pre_ring = in_group ? nullptr : s->pre_ring_ptr;      // a rank of a group takes a ring of its own
  if (r.dosage_mode) return level0_dosage(cx, blocks, b_lo, b_hi, lg);
  if (!pre_ring && s->mapped_ok && level0_mapped(cx, blocks, b_lo, b_hi, lg)) return;
  level0_ring(cx, blocks, b_lo, b_hi, lg, pre_ring);
}

// a block of dosages is bs x N_file doubles on the host: one block at a time, synchronous
void Step1Ingest::level0_dosage(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg) {
  const Params& p = r.p;
  std::mutex& io_mu = s->io_mu;
  std::vector<double> dbuf;
  for (int b = b_lo; b < b_hi; ++b) {
    const Blk& bl = blocks[b];
    auto t0 = Clock::now();
    dbuf.resize((size_t)bl.bs * r.n_file);
    {
      std::lock_guard<std::mutex> lk(io_mu);
      if (r.bgenh) {  // readChunkFromBGENFileToG_fast (Geno.cpp:1574-1699): inflate + probabilities -> dosages
        if (rg_bgen_read_dosages(r.bgenh, bl.bs, &r.snp_offset[bl.start], p.ref_first ? 1 : 0, dbuf.data(), r.n_file) != RG_BGEN_OK)
          throw std::runtime_error(rg_bgen_last_error(r.bgenh));
      } else {        // Read() per kept variant (Geno.cpp:1795-1796): ALT dosages, -3 = missing
        if (rg_pgen_read_dosage_rows(r.pgen, bl.bs, &r.snp_offset[bl.start], dbuf.data(), r.n_file) != RG_PGEN_OK)
          throw std::runtime_error(rg_pgen_last_error(r.pgen));
      }
    }
    auto t1 = Clock::now();
    const int32_t id = b, bsv = bl.bs;
    const double* dp = dbuf.data();
    check(cx, rg_l0_blocks_f64(cx, 1, &id, &bsv, &dp, r.n_file, RG_MEM_HOST));
    check(cx, rg_sync(cx));
    auto t2 = Clock::now();
    lg << " block [" << b + 1 << "] (chromosome " << bl.chrom << ") : " << bl.bs << " snps  (read "
       << ms_int(t0, t1) << "ms, level 0 ridge on GPU "
       << ms_int(t1, t2) << "ms)\n";
  }
}

// the mapped .bed: every block is a range of the file
bool Step1Ingest::level0_mapped(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg) {
  BedMap& bed_map = s->bed_map; BedStage& bed_stage = s->bed_stage;
  bool consecutive = true;
  for (int b = b_lo; b < b_hi && consecutive; ++b)
    for (int j = 1; j < blocks[b].bs; ++j)
      if (r.snp_offset[blocks[b].start + j] != r.snp_offset[blocks[b].start + j - 1] + 1) { consecutive = false; break; }
  const int64_t last = r.snp_offset[blocks[b_hi - 1].start + blocks[b_hi - 1].bs - 1];
  if (consecutive && 3 + (last + 1) * r.bpr <= (int64_t)bed_map.bytes) {
    const int nb = b_hi - b_lo;
    std::vector<int32_t> ids(nb), bss(nb);
    std::vector<const uint8_t*> ptrs(nb);
    int64_t nsnp = 0;
    for (int b = 0; b < nb; ++b) {
      ids[b] = b_lo + b; bss[b] = blocks[b_lo + b].bs; nsnp += bss[b];
      ptrs[b] = bed_map.base + 3 + r.snp_offset[blocks[b_lo + b].start] * r.bpr;
    }
    auto t1 = Clock::now();
    int b_staged = 0;          // blocks taken from the copy of the file in device memory: one library batch at a time, as the copy reaches them
    if (bed_stage.state != 0) {
      const int per = std::max(1, (int)rg_l0_batch_blocks(cx));
      std::vector<const uint8_t*> dptrs(nb);
      for (int b0 = 0; b0 < nb; b0 += per) {
        const int n = std::min(per, nb - b0);
        const int64_t end = (int64_t)(ptrs[b0 + n - 1] - bed_map.base) + (int64_t)bss[b0 + n - 1] * r.bpr;
        if (!bed_stage.wait(end)) break;
        for (int b = b0; b < b0 + n; ++b) dptrs[b] = bed_stage.dev + (ptrs[b] - bed_map.base);
        check(cx, rg_l0_blocks(cx, n, ids.data() + b0, bss.data() + b0, dptrs.data() + b0, r.bpr, RG_MEM_DEVICE));
        b_staged = b0 + n;
      }
    }
    if (b_staged < nb)
      check(cx, rg_l0_blocks(cx, nb - b_staged, ids.data() + b_staged, bss.data() + b_staged, ptrs.data() + b_staged, r.bpr, RG_MEM_HOST));
    auto t2 = Clock::now();
    lg << " blocks [" << b_lo + 1 << ".." << b_hi << "] (chromosomes " << blocks[b_lo].chrom << ".." << blocks[b_hi - 1].chrom << ") : " << nsnp
       << " snps  (" << (b_staged == nb ? "read from the copy of the file in device memory" : b_staged ? "partly read from the copy of the file in device memory" : "copied to the GPU from the mapped file")
       << ", queued after " << ms_int(t1, t2) << "ms)\n";
    if (b_staged && bed_stage.state == 2 && getenv("RG_TIMING"))
      fprintf(stderr, "[timing] the .bed in device memory: first piece requested %.0f ms, last piece arrived %.0f ms since start (%.1f GB/s)\n",
              ms_dbl(t_start, bed_stage.t_first), ms_dbl(t_start, bed_stage.t_last),
              bed_stage.bytes / 1e9 / std::max(1e-9, std::chrono::duration<double>(bed_stage.t_last - bed_stage.t_first).count()));
    check(cx, rg_sync(cx));
    lg << "   -level 0 ridge of blocks [" << b_lo + 1 << ".." << b_hi << "] complete (" <<
        ms_int(t2, Clock::now()) << "ms after the last batch was queued)\n";
    return true;
  }
  return false;
}

void Step1Ingest::level0_ring(rg_ctx* cx, const std::vector<Blk>& blocks, int b_lo, int b_hi, std::ostringstream& lg, IngestRing* pre_ring) {
  const Params& p = r.p;
  std::mutex& io_mu = s->io_mu;
  const int64_t blk_bytes = ingest_blk_bytes;
  // the ring of host buffers: the one whose page-locking was started while the text files were parsed (one GPU), or a
  // ring of this rank's own
  IngestRing own;
  IngestRing& ring = pre_ring ? *pre_ring : own;
  if (!pre_ring) own.start((int64_t)(b_hi - b_lo) * blk_bytes, blk_bytes, rg_l0_batch_blocks(cx), -1);
  const int per = ring.per;
  const int NBUF = IngestRing::NBUF;
  struct Slot { int b0 = 0, nb = 0; double read_ms = 0; };
  std::vector<Slot> slots(NBUF);
  std::mutex& mu = ring.mu; std::condition_variable& cv = ring.cv;
  std::deque<int>& free_q = ring.free_q;
  std::deque<int> ready_q;
  std::exception_ptr rd_err = nullptr;
  bool rd_done = false;
  // preads of one buffer in flight (page-cache copies scale with threads; a disk queue likes depth): half the CPUs this process may use
  // (affinity mask and cgroup quota), between 4 and 16, shared by the ranks of a multi-GPU run
  int rd_threads = std::max(4, std::min(16, usable_cpus() / 2 / std::max(1, p.gpus)));
  if (const char* e = getenv("RG_READ_THREADS")) rd_threads = std::max(1, atoi(e));
  std::thread reader([&]() {
    int fd = -1;
    try {
      if (!r.pgen) {
        fd = open((p.bed + ".bed").c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error("cannot read bed file");
      }
      for (int b0 = b_lo; b0 < b_hi; b0 += per) {
        int si;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return !free_q.empty() || ring.failed; });
          if (ring.failed) throw std::runtime_error("cannot allocate memory for the genotype buffers");
          si = free_q.front(); free_q.pop_front();
        }
        Slot& sl = slots[si];
        uint8_t* slmem = ring.mem[si];
        sl.b0 = b0; sl.nb = std::min(per, b_hi - b0);
        auto t0 = Clock::now();
        struct Piece { uint8_t* dst; int64_t off, want; };
        std::vector<Piece> pieces;
        for (int b = 0; b < sl.nb; ++b) {
          const Blk& bl = blocks[b0 + b];
          uint8_t* dst = slmem + (int64_t)b * blk_bytes;
          if (r.pgen) {  // ReadHardcalls per kept variant (Geno.cpp:1781-1798), as .bed-coded rows
            std::lock_guard<std::mutex> lk(io_mu);
            if (rg_pgen_read_bed_rows(r.pgen, bl.bs, &r.snp_offset[bl.start], dst, r.bpr) != RG_PGEN_OK)
              throw std::runtime_error(rg_pgen_last_error(r.pgen));
            continue;
          }
          int j = 0;
          while (j < bl.bs) {   // runs of variants that are consecutive in the file: one pread each (jumpto_bed, Geno.cpp:2828-2830)
            int e = j + 1;
            while (e < bl.bs && r.snp_offset[bl.start + e] == r.snp_offset[bl.start + e - 1] + 1) ++e;
            const int64_t want = (int64_t)(e - j) * r.bpr, off = 3 + r.snp_offset[bl.start + j] * r.bpr, chunk = 8 << 20;
            for (int64_t o = 0; o < want; o += chunk) pieces.push_back({dst + (int64_t)j * r.bpr + o, off + o, std::min(chunk, want - o)});
            j = e;
          }
        }
        if (!pieces.empty()) {
          std::atomic<int> bad{0};
          parallel_for((int)pieces.size(), rd_threads, [&](int t) {
            const Piece& pc = pieces[t];
            int64_t got = 0;
            while (got < pc.want) {
              const ssize_t k = pread(fd, pc.dst + got, (size_t)(pc.want - got), pc.off + got);
              if (k <= 0) { bad = 1; return; }
              got += k;
            }
          });
          if (bad) throw std::runtime_error("cannot read bed file");
        }
        sl.read_ms = ms_dbl(t0, Clock::now());
        {
          std::lock_guard<std::mutex> lk(mu);
          ready_q.push_back(si);
        }
        cv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      rd_err = std::current_exception();
    }
    if (fd >= 0) close(fd);
    {
      std::lock_guard<std::mutex> lk(mu);
      rd_done = true;
    }
    cv.notify_all();
  });
  std::exception_ptr main_err = nullptr;
  try {
    for (;;) {
      int si = -1;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !ready_q.empty() || rd_done; });
        if (!ready_q.empty()) { si = ready_q.front(); ready_q.pop_front(); }
        else if (rd_err) std::rethrow_exception(rd_err);
        else break;
      }
      Slot& sl = slots[si];
      std::vector<int32_t> ids(sl.nb), bss(sl.nb);
      std::vector<const uint8_t*> ptrs(sl.nb);
      int64_t nsnp = 0;
      for (int b = 0; b < sl.nb; ++b) {
        ids[b] = sl.b0 + b; bss[b] = blocks[sl.b0 + b].bs; ptrs[b] = ring.mem[si] + (int64_t)b * blk_bytes;
        nsnp += bss[b];
      }
      auto t1 = Clock::now();
      check(cx, rg_l0_blocks(cx, sl.nb, ids.data(), bss.data(), ptrs.data(), r.bpr, RG_MEM_HOST));
      check(cx, rg_ingest_fence(cx));     // the rows have crossed PCIe: the buffer goes back to the reader
      auto t2 = Clock::now();
      lg << " blocks [" << sl.b0 + 1 << ".." << sl.b0 + sl.nb << "] (chromosomes " << blocks[sl.b0].chrom << ".." << blocks[sl.b0 + sl.nb - 1].chrom
         << ") : " << nsnp << " snps  (read " << (int64_t)sl.read_ms << "ms in the reader thread, queued on the GPU after "
         << ms_int(t1, t2) << "ms)\n";
      {
        std::lock_guard<std::mutex> lk(mu);
        free_q.push_back(si);
      }
      cv.notify_all();
    }
  } catch (...) {
    main_err = std::current_exception();
    {   // let the reader come to its end
      std::lock_guard<std::mutex> lk(mu);
      ring.failed = true;
    }
    cv.notify_all();
  }
  reader.join();
  if (!main_err) {
    auto t1 = Clock::now();
    try { check(cx, rg_sync(cx)); } catch (...) { main_err = std::current_exception(); }
    lg << "   -level 0 ridge of blocks [" << b_lo + 1 << ".." << b_hi << "] complete (" <<
        ms_int(t1, Clock::now()) << "ms after the last batch was queued)\n";
  }
  ring.release();
  if (main_err) std::rethrow_exception(main_err);
}

}  // namespace rgdrv
