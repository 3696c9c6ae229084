// regenie-amd, the C++ host driver (see driver.h): the BGEN read-ahead of `--step 2` (BgenAhead, driver_step2.h).
#include "driver_step2.h"

namespace rgdrv {

static const struct T255 { double v[256]; T255() { for (int b = 0; b < 256; ++b) v[b] = b / 255.0; } } t255;   // the reader's prob = byte / 255.0

// share = f: the host threads take the share f of every group beside the device (whole blocks from the group's end; their route gives the
// same result lines -- both are held to regenie's).  The device's part keeps its size -- a launch takes as long for 2,000 streams as for
// 3,072, every stream being a chain of its own -- and the host's blocks come on top.  Off by default: on a box that gives the job 16 CPUs
// the workers take those from the reads, the chromosome set-ups and the uploads (36,864 variants at 500,000 samples: 4.3 s without, 4.7 s
// with f = 0.25, 5.4 s with 0.38, 6.9 s with 0.5); it is for hosts with idle cores.  The share is fixed for a run, so that the split does
// not depend on timing.
GroupPlan plan_groups(const std::vector<BlkRef>& blocks, int bsize, int dev_target, double share, bool has_device) {
  GroupPlan pl;
  if (!has_device) share = 0.0;
  const int target = has_device ? (int)std::min(65536.0, std::max(bsize, dev_target) / (1.0 - share)) : bsize;
  for (size_t b = 0; b < blocks.size(); ++b) {
    const BlkRef& br = blocks[b];
    if (!pl.groups.empty()) {
      Group& g = pl.groups.back();
      if (g.ref.chrom == br.chrom && g.ref.j0 + g.ref.bs == br.j0 && g.ref.bs + br.bs <= target) {
        pl.block_group.push_back({pl.groups.size() - 1, g.ref.bs});
        g.starts.push_back(g.ref.bs);
        g.ref.bs += br.bs;
        continue;
      }
    }
    pl.groups.push_back({br, b, 0, {0}});
    pl.block_group.push_back({pl.groups.size() - 1, 0});
  }
  for (Group& g : pl.groups) {
    g.dev_rows = has_device ? g.ref.bs : 0;
    if (share > 0.0) {      // the block boundary nearest to the device's share; a group of one block stays whole
      const double want = (1.0 - share) * g.ref.bs;
      int best = g.ref.bs;
      for (int st : g.starts) if (st > 0 && std::fabs(st - want) < std::fabs(best - want)) best = st;
      g.dev_rows = best;
    }
  }
  return pl;
}

BgenAhead::BgenAhead(const S2Common& cm) : cm_(cm) {
  const Run& r = cm.r;
  const Params& p = cm.p;
  if (rg_bgen_block_bytes(r.bgenh, &block_bytes_) != RG_BGEN_OK) throw std::runtime_error(rg_bgen_last_error(r.bgenh));
  block_bytes_ = (block_bytes_ + 63) / 64 * 64;
  int32_t bcomp = 0;
  rg_bgen_info(r.bgenh, nullptr, nullptr, &bcomp, nullptr);
  // the device decoder: default for zlib files (under --test dominant | recessive its rows hold the coded probabilities, its sums stay additive)
  if (bcomp == 1 && !cm.env.bgen_host && rg_bgen_dev_create(&bdev_, cm.part.device) == RG_BGEN_OK) {
    if (rg_bgen_dev_set_samples(bdev_, r.n_file, cm.n, cm.identity ? nullptr : cm.file_idx.data(), cm.per_trait ? cm.P : 0, cm.per_trait ? cm.Mc.data() : nullptr) != RG_BGEN_OK) {
      rg_bgen_dev_destroy(bdev_);
      bdev_ = nullptr;
    }
    if (bdev_ && cm.coding && rg_bgen_dev_set_coding(bdev_, cm.coding) != RG_BGEN_OK) { rg_bgen_dev_destroy(bdev_); bdev_ = nullptr; }
  }
  std::vector<BlkRef> my_blocks;             // this part's blocks in the order they are tested
  int b = 0;
  for (int chrom : r.chr_read) {
    if (!cm.chr_snps.count(chrom)) continue;
    const std::vector<int64_t>& sn = cm.chr_snps.at(chrom);
    const int nbc = (int)((sn.size() + p.bsize - 1) / p.bsize);
    for (int bb = 0; bb < nbc; ++bb, ++b)
      if (b >= cm.part.blk_lo && b < cm.part.blk_hi)
        my_blocks.push_back({chrom, &sn, (int64_t)bb * p.bsize, (int)std::min<int64_t>(p.bsize, (int64_t)sn.size() - (int64_t)bb * p.bsize)});
  }
  plan_ = plan_groups(my_blocks, p.bsize, cm.env.bgen_group, cm.env.bgen_host_share, bdev_ != nullptr);
}

BgenAhead::~BgenAhead() {
  if (prep_ahead_.valid()) prep_ahead_.wait();
  for (auto& d : preps_) if (d.rd.valid()) d.rd.wait();
  for (auto& d : preps_) { if (d.g16) rg_host_free(d.g16); if (d.comp) rg_host_free(d.comp); }
  if (bdev_) rg_bgen_dev_destroy(bdev_);
}

void BgenAhead::start() {
  if (!plan_.groups.empty()) prep_ahead_ = std::async(std::launch::async, [this]() { prepare(0); });
}

void BgenAhead::report_device() const {
  if (bdev_ && cm_.env.timing)
    fprintf(stderr, "[timing] step 2 part %d: BGEN on the device: %lld blocks (%lld on the host route) | reading the stored streams %.0f ms | copy + inflate + walk on the GPU %.0f ms (both overlapped with the tests of the previous block)\n",
            cm_.part.part, (long long)timing.dev_blocks, (long long)timing.host_blocks, timing.dev_read, timing.dev_decode);
}

const PreparedBlock* BgenAhead::next_block() {
  auto tw = std::chrono::steady_clock::now();
  const size_t gi = plan_.block_group[my_next_].first;
  const Group& g = plan_.groups[gi];
  const size_t r0 = (size_t)plan_.block_group[my_next_].second;      // the block's first row in its prepared group
  DosPrep& d = preps_[gi & 1];
  if (g.first_block == my_next_) {      // first block of its group: the group has to be ready, the next one is started
    if (prep_ahead_.valid()) prep_ahead_.get();
    else prepare(gi);
    if (gi + 1 < plan_.groups.size()) prep_ahead_ = std::async(std::launch::async, [this, nx = gi + 1]() { prepare(nx); });
    if (!d.err.empty()) { if (prep_ahead_.valid()) prep_ahead_.wait(); throw std::runtime_error(d.err); }
    timing.inflate += d.ms_inflate; timing.walk += d.ms_walk; timing.prep_wall += d.ms_wall;
    if (d.dev_rows > 0) { timing.dev_read += d.ms_read; timing.dev_decode += d.ms_dev; }
  }
  ++my_next_;
  timing.prep_wait += ms_since(tw);
  const bool on_dev = (int)r0 < d.dev_rows;      // (a group is split at a block boundary)
  if (on_dev) ++timing.dev_blocks; else ++timing.host_blocks;
  const size_t P = (size_t)cm_.P;
  PreparedBlock& v = view_;
  v.integral = d.integral;
  if (!d.integral) return &v;
  v.total = d.total.data() + r0; v.ns1 = d.ns1.data() + r0; v.info_num = d.info_num.data() + r0; v.ignored = d.ignored.data() + r0;
  v.sum_pos = cm_.coding ? d.sum_pos.data() + r0 : nullptr;
  if (cm_.per_trait) { v.af_t = d.af_t.data() + r0 * P; v.ns_t = d.ns_t.data() + r0 * P; v.info_t = d.info_t.data() + r0 * P; }
  if (cm_.af_cc) { v.af_case = d.af_case.data() + r0 * P; v.ns_case = d.ns_case.data() + r0 * P; }
  v.ld = on_dev ? d.ld_dev : cm_.ld16;
  v.g16 = on_dev ? d.g16_dev + r0 * (size_t)v.ld : d.g16 + (r0 - (size_t)d.host_row0) * (size_t)v.ld;
  v.on_device = on_dev ? 1 : 0;
  return &v;
}

// reads the stored streams of a group into a slot's page-locked buffer (any thread; the handle is only read)
bool BgenAhead::read_streams(const BlkRef& br, DosPrep& d, int rows) {
  const Run& r = cm_.r;
  auto t0 = std::chrono::steady_clock::now();
  const int bs = rows;
  std::vector<int64_t> vi(bs);
  for (int j = 0; j < bs; ++j) vi[j] = r.snp_offset[(*br.snps)[br.j0 + j]];
  int64_t need = 0;
  if (rg_bgen_compressed_bytes(r.bgenh, bs, vi.data(), &need) != RG_BGEN_OK) return false;
  if (d.comp_cap < need) {
    if (d.comp) rg_host_free(d.comp);
    d.comp_cap = need + need / 4;
    d.comp = (uint8_t*)rg_host_alloc((size_t)d.comp_cap);
    if (!d.comp) { d.comp_cap = 0; return false; }
  }
  d.rd_off.resize(bs); d.rd_clen.resize(bs); d.rd_ulen.resize(bs);
  const bool ok = rg_bgen_read_compressed(r.bgenh, bs, vi.data(), d.comp, d.comp_cap, d.rd_off.data(), d.rd_clen.data(), d.rd_ulen.data(), std::min(cm_.nt_prep, 32)) == RG_BGEN_OK;
  d.rd_ms = ms_since(t0);
  return ok;
}

// The device route of a group: false = not taken (no decoder, or a variant the decoder flagged: the host route then gives the reference's
// verdict).  The first `rows` variants of the group on the device: their sums into d.total ... (sized by the caller), their dosage rows
// left in device memory.
bool BgenAhead::prepare_dev(const BlkRef& br, DosPrep& d, int slot, int64_t gi, int rows) {
  const Params& p = cm_.p;
  const int P = cm_.P;
  if (!bdev_ || rows < 1) return false;
  const int bs = rows;
  // this group's streams: read ahead (while the previous group was decoded), or now
  bool have = false;
  if (d.rd.valid()) { const bool ok = d.rd.get(); have = ok && d.rd_group == gi; }
  if (!have && !read_streams(br, d, rows)) return false;
  d.rd_group = -1;
  // the NEXT group's streams go into the other slot's buffer while this one is decoded (that slot's decode is long done; the main thread
  // only reads its sums and its device rows)
  if (gi >= 0 && (size_t)gi + 1 < plan_.groups.size() && plan_.groups[gi + 1].dev_rows > 0) {
    DosPrep& dn = preps_[(gi + 1) & 1];
    if (dn.rd.valid()) dn.rd.wait();
    dn.rd_group = gi + 1;
    dn.rd = std::async(std::launch::async, [this, gn = gi + 1]() { return read_streams(plan_.groups[gn].ref, preps_[gn & 1], plan_.groups[gn].dev_rows); });
  }
  const std::vector<int64_t>& off = d.rd_off;
  const std::vector<int32_t>&clen = d.rd_clen, &ulen = d.rd_ulen;
  std::vector<int32_t> status(bs), maxq(bs);
  auto t1 = std::chrono::steady_clock::now();
  const bool per_trait = cm_.per_trait;
  std::vector<int64_t> sq(bs), si(bs), no(bs), sqt, sit, nt;
  if (per_trait) { sqt.resize((size_t)bs * P); sit.resize((size_t)bs * P); nt.resize((size_t)bs * P); }
  rg_bgen_dev_out o;
  memset(&o, 0, sizeof(o));
  o.sum_q = sq.data(); o.sum_info = si.data(); o.n_obs = no.data(); o.max_q = maxq.data(); o.status = status.data();
  if (per_trait) { o.sum_q_t = sqt.data(); o.sum_info_t = sit.data(); o.n_obs_t = nt.data(); }
  if (rg_bgen_dev_decode(bdev_, slot, bs, d.comp, off[bs - 1] + clen[bs - 1], off.data(), clen.data(), ulen.data(), p.ref_first ? 1 : 0, &o) != RG_BGEN_OK) return false;
  for (int j = 0; j < bs; ++j) if (status[j] != 0) return false;
  bool bad = false;
  for (int j = 0; j < bs; ++j) {
    // the walk's exact integer sums in the units the host route accumulates as doubles: dosages in 1 / 255, info terms in 1 / 65025
    d.total[j] = (double)sq[j] / 255.0; d.info_num[j] = (double)si[j] / 65025.0; d.ns1[j] = no[j];
    if (cm_.coding) d.sum_pos[j] = NAN;      // the coded rows' sum comes back with their scores (S2Block::score_*)
    if (maxq[j] > 510) bad = true;
    const double mac = std::min(d.total[j], 2.0 * d.ns1[j] - d.total[j]);
    // The sum here is the exact integer sum / 255; the host route and regenie add the samples' doubles in order.  A count that lands on
    // --minMAC to within that summation's rounding could fall on the other side of the `<` there: such a group goes to the host route as a
    // whole (its verdict is the reference's), so that the filter does not depend on which route a variant took.  (si == 0: every call is a
    // hard call, the doubles are integers and their sum is exact whatever the order -- the common case of a count that EQUALS --minMAC.)
    if (si[j] != 0 && std::fabs(mac - p.min_mac) <= 1e-9 * std::max(1.0, mac)) return false;
    if (mac < p.min_mac) d.ignored[j] = 1;      // below_min_mac
    if (per_trait)
      for (int q = 0; q < P; ++q) {      // the host route SUBTRACTS what the samples missing for trait q contribute
        d.af_t[(size_t)j * P + q] = -(double)sqt[(size_t)j * P + q] / 255.0;
        d.ns_t[(size_t)j * P + q] = -nt[(size_t)j * P + q];
        d.info_t[(size_t)j * P + q] = -(double)sit[(size_t)j * P + q] / 65025.0;
      }
  }
  d.dev_bad = bad;
  d.g16_dev = o.g16; d.ld_dev = o.ld16;
  d.ms_read = have ? 0.0 : d.rd_ms;      // what the read cost THIS group's preparation (read ahead: nothing)
  d.ms_dev = ms_since(t1);
  return true;
}

// rows [lo, bs) of the group on the host threads, into the pinned buffer from its first row on
void BgenAhead::host_rows(const BlkRef& br, DosPrep& d, int lo) {
  const Run& r = cm_.r;
  const int P = cm_.P, bs = br.bs, nt_prep = cm_.nt_prep;
  const int64_t n = cm_.n, ld16 = cm_.ld16, block_bytes = block_bytes_;
  const bool per_trait = cm_.per_trait, identity = cm_.identity, rf = cm_.p.ref_first;
  const double min_mac = cm_.p.min_mac;
  const int coding = cm_.coding;
  const int64_t* file_idx = cm_.file_idx.data();
  const uint8_t *has_missing = cm_.has_missing.data(), *Mc = cm_.Mc.data();
  const bool af_cc = cm_.af_cc;
  const uint8_t *any_case = cm_.any_case.data(), *Cc = cm_.Cc.data();
  if (lo >= bs) return;
  if (d.g16_rows < bs - lo) {
    if (d.g16) rg_host_free(d.g16);
    d.g16 = (uint16_t*)rg_host_alloc((size_t)(bs - lo) * ld16 * sizeof(uint16_t));
    d.g16_rows = d.g16 ? bs - lo : 0;
    if (!d.g16) throw std::runtime_error("cannot allocate the pinned dosage buffers");
  }
  d.host_row0 = lo;
  d.raw.resize((size_t)nt_prep * block_bytes);        // one inflated block per worker: walked while it is still in that core's cache
  std::vector<std::string> werr(nt_prep);
  std::atomic<int> next(lo);
  // (no reader lock: the read call only reads the handle, so the parts of a --gpus N run inflate at the same time)
  parallel_for(nt_prep, nt_prep, [&](int w) {
    uint8_t* blk = d.raw.data() + (size_t)w * block_bytes;
    for (int j; (j = next.fetch_add(1)) < bs;) {
      auto t0 = std::chrono::steady_clock::now();
      if (rg_bgen_read_blocks(r.bgenh, 1, &d.vi[j], blk, block_bytes, 1) != RG_BGEN_OK) { werr[w] = rg_bgen_last_error(r.bgenh); next = bs; return; }
      auto t1 = std::chrono::steady_clock::now();
      const uint8_t* ploidy = blk + 8;
      const uint8_t* pr = blk + 10 + r.n_file;
      uint16_t* q16 = d.g16 + (size_t)(j - lo) * ld16;
      double tot = 0.0, inf = 0.0, pos = 0.0; int64_t ns = 0;
      unsigned worst = 0;
      double* af_t = nullptr; int64_t* ns_t = nullptr; double* info_t = nullptr;
      if (per_trait) {
        af_t = d.af_t.data() + (size_t)j * P; ns_t = d.ns_t.data() + (size_t)j * P; info_t = d.info_t.data() + (size_t)j * P;
        for (int q = 0; q < P; ++q) { af_t[q] = 0.0; ns_t[q] = 0; info_t[q] = 0.0; }
      }
      double* af_case = af_cc ? d.af_case.data() + (size_t)j * P : nullptr;
      int64_t* ns_case = af_cc ? d.ns_case.data() + (size_t)j * P : nullptr;
      for (int64_t k = 0; k < n; ++k) {
        const int64_t i = identity ? k : file_idx[k];
        if (ploidy[i] & 0x80) { q16[k] = 0xFFFFu; continue; }
        const unsigned b0 = pr[2 * i], b1 = pr[2 * i + 1];
        const double p0 = t255.v[b0], p1 = t255.v[b1];
        double v, e;
        unsigned qi;
        if (rf) {     // G = prob1 + 2 prob2, prob2 = max(1 - prob0 - prob1, 0) (Geno.cpp:2286-2290)
          const double p2 = std::max(1.0 - p0 - p1, 0.0);
          v = p1 + 2.0 * p2; e = (4.0 * p2 + p1) - v * v;
          qi = bgen_dosage_255(b0, b1, true);
        } else {
          v = p1 + 2.0 * p0; e = (4.0 * p0 + p1) - v * v;
          qi = bgen_dosage_255(b0, b1, false);
        }
        worst = std::max(worst, qi);
        if (coding) {      // the row the test takes: the coded probability (the sums stay those of the additive dosage)
          q16[k] = (uint16_t)bgen_coded_255(b0, b1, rf, coding);
          const double p2 = rf ? std::max(1.0 - p0 - p1, 0.0) : 0.0;
          pos += coding == 1 ? (rf ? p1 + p2 : p0 + p1) : (rf ? p2 : p0);
        } else q16[k] = (uint16_t)qi;
        tot += v; inf += e; ++ns;
        if (per_trait && has_missing[k]) subtract_masked(Mc, n, P, k, v, e, af_t, ns_t, info_t);
        if (af_cc && any_case[k]) add_cases(Cc, n, P, k, v, af_case, ns_case);
      }
      for (int64_t k = n; k < ld16; ++k) q16[k] = 0;
      if (!bgen_dosage_integral(worst)) d.host_bad = 1;          // prob0 + prob1 > 1 in the file: not a dosage in [0, 2], the general route reports what the reference would
      d.total[j] = tot; d.ns1[j] = ns; d.info_num[j] = inf;
      if (coding) d.sum_pos[j] = pos;
      d.ignored[j] = below_min_mac(tot, (double)ns, min_mac) ? 1 : 0;
      auto t2 = std::chrono::steady_clock::now();
      d.w_inf[w] += std::chrono::duration<double, std::milli>(t1 - t0).count();
      d.w_walk[w] += std::chrono::duration<double, std::milli>(t2 - t1).count();
    }
  });
  for (const auto& e : werr) if (!e.empty()) throw std::runtime_error(e);
}

// group gi into its slot (a worker of its own, or the main thread when nothing was started ahead); an error is left in the slot's `err`
void BgenAhead::prepare(size_t gi) {
  const BlkRef& br = plan_.groups[gi].ref;
  const int slot = (int)(gi & 1), P = cm_.P, nt_prep = cm_.nt_prep;
  DosPrep& d = preps_[slot];
  try {
    const int bs = br.bs;
    auto ta = std::chrono::steady_clock::now();
    d.vi.resize(bs);
    for (int j = 0; j < bs; ++j) d.vi[j] = cm_.r.snp_offset[(*br.snps)[br.j0 + j]];
    d.g16_dev = nullptr; d.ms_read = d.ms_dev = 0; d.dev_rows = 0; d.host_row0 = 0; d.dev_bad = false; d.host_bad = 0;
    if (cm_.coding) d.sum_pos.assign(bs, 0.0);
    d.total.assign(bs, 0.0); d.info_num.assign(bs, 0.0); d.ns1.assign(bs, 0); d.ignored.assign(bs, 0);
    if (cm_.per_trait) { d.af_t.assign((size_t)bs * P, 0.0); d.ns_t.assign((size_t)bs * P, 0); d.info_t.assign((size_t)bs * P, 0.0); }
    if (cm_.af_cc) { d.af_case.assign((size_t)bs * P, 0.0); d.ns_case.assign((size_t)bs * P, 0); }
    d.w_inf.assign(nt_prep, 0.0); d.w_walk.assign(nt_prep, 0.0);
    // the group's first rows on the device and, beside them, its last blocks on the host threads; a group the decoder turns down goes to
    // the host threads as a whole (a damaged stream, another encoding: their messages are the reference's)
    const int split = bdev_ ? plan_.groups[gi].dev_rows : 0;
    bool dev_ok = false;
    if (split > 0) {
      std::future<bool> fdev = std::async(std::launch::async, [&]() { return prepare_dev(br, d, slot, (int64_t)gi, split); });
      try { host_rows(br, d, split); } catch (...) { fdev.wait(); throw; }
      dev_ok = fdev.get();
    }
    if (dev_ok) d.dev_rows = split;
    else { d.g16_dev = nullptr; d.dev_bad = false; host_rows(br, d, 0); }
    d.integral = !d.host_bad && !d.dev_bad;
    // thread-milliseconds of the two halves, and the wall time of the group's preparation
    d.ms_inflate = 0; d.ms_walk = 0;
    for (int w = 0; w < nt_prep; ++w) { d.ms_inflate += d.w_inf[w]; d.ms_walk += d.w_walk[w]; }
    d.ms_wall = ms_since(ta);
  } catch (const std::exception& e) { d.err = e.what(); if (d.err.empty()) d.err = "bgen read failed"; }
}

}  // namespace rgdrv
