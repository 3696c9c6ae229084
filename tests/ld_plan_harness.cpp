// The pure pieces of the LD driver behind a C interface (tests/test_ld_plan_cpu.py loads it as a shared object), and, with
// -DLD_PLAN_MAIN, a program of its own that runs them on small inputs (for a build with -fsanitize=address,undefined).
#include "driver_ld.h"
#include "driver_step2.h"
using namespace rgdrv;

// Run's destructor names the readers' close calls; no reader is opened here
extern "C" void rg_pgen_close(rg_pgen*) {}
extern "C" void rg_bgen_close(rg_bgen*) {}

static std::vector<std::string> lines_of(const char* blob, int n) {      // n strings, each ended by '\n'
  std::vector<std::string> v;
  for (int k = 0; k < n; ++k) { const char* e = strchr(blob, '\n'); v.emplace_back(blob, e); blob = e + 1; }
  return v;
}

// n_forced < 0: default mode.  Returns the number of columns; col_ids: the IDs, each ended by '\n' (at most cap bytes, else -1).
extern "C" int ld_plan(const char* ids, int n_ids, const char* forced, int n_forced, int32_t* col_of_variant, uint8_t* absent, int64_t* present, int32_t* n_present,
                       char* col_ids, int cap) {
  const std::vector<std::string> snp = lines_of(ids, n_ids), fr = n_forced < 0 ? std::vector<std::string>() : lines_of(forced, n_forced);
  const LdColumns lc = plan_ld_columns(snp, n_forced < 0 ? nullptr : &fr);
  if (lc.col_of_variant.size() != snp.size() || lc.absent.size() != lc.col_ids.size()) return -1;
  std::copy(lc.col_of_variant.begin(), lc.col_of_variant.end(), col_of_variant);
  std::copy(lc.absent.begin(), lc.absent.end(), absent);
  std::copy(lc.present.begin(), lc.present.end(), present);
  *n_present = (int32_t)lc.present.size();
  std::string all;
  for (auto& id : lc.col_ids) all += id + "\n";
  if ((int)all.size() > cap) return -1;
  memcpy(col_ids, all.data(), all.size());
  return (int)lc.col_ids.size();
}

// ind_ignore [n_file]; ain [N], N = the samples of the file that are not ignored.  Returns n; an, file_idx [n].
extern "C" int64_t sample_map(const uint8_t* ind_ignore, int64_t n_file, const uint8_t* ain, int64_t N, int64_t* an, int64_t* file_idx, int32_t* identity) {
  Run r;
  r.n_file = n_file; r.N = N;
  r.ind_ignore.assign(ind_ignore, ind_ignore + n_file);
  r.ain.assign(ain, ain + N);
  const SampleMap sm(r);
  if ((int64_t)sm.an.size() != sm.n || (int64_t)sm.file_idx.size() != sm.n) return -1;
  std::copy(sm.an.begin(), sm.an.end(), an);
  std::copy(sm.file_idx.begin(), sm.file_idx.end(), file_idx);
  *identity = sm.identity ? 1 : 0;
  return sm.n;
}

// every byte pair: q [256][256] (b0 major), integral likewise
extern "C" void bgen_rule(int ref_first, uint32_t* q, uint8_t* integral) {
  for (unsigned b0 = 0; b0 < 256; ++b0)
    for (unsigned b1 = 0; b1 < 256; ++b1) {
      q[b0 * 256 + b1] = bgen_dosage_255(b0, b1, ref_first != 0);
      integral[b0 * 256 + b1] = bgen_dosage_integral(q[b0 * 256 + b1]) ? 1 : 0;
    }
}
extern "C" uint32_t pgen_rule(double g) { return pgen_dosage_16384(g); }
extern "C" uint32_t not_integral() { return DOSAGE_NOT_INTEGRAL; }

#ifdef LD_PLAN_MAIN
#define EXPECT(x) do { if (!(x)) { fprintf(stderr, "failed: %s\n", #x); return 1; } } while (0)
int main() {
  {  // the column plan, both modes
    const char* ids = "a\nb\na\nc\n";
    int32_t cov[4], np = 0; uint8_t absent[8]; int64_t present[4]; char out[64];
    EXPECT(ld_plan(ids, 4, nullptr, -1, cov, absent, present, &np, out, sizeof(out)) == 3 && np == 3 && cov[2] == -1 && cov[3] == 2);
    EXPECT(ld_plan(ids, 4, "c\r\nzz\nc\na\n", 4, cov, absent, present, &np, out, sizeof(out)) == 3 && np == 2);
    EXPECT(cov[0] == 2 && cov[1] == -1 && cov[2] == -1 && cov[3] == 0 && absent[0] == 0 && absent[1] == 1 && absent[2] == 0 && !memcmp(out, "c\nzz\na\n", 7));
  }
  std::vector<int64_t> file_idx(7);
  int64_t n = 0;
  {  // the sample map: file sample 2 ignored, kept sample 0 not analysed
    const uint8_t ign[8] = {0, 0, 1, 0, 0, 0, 0, 0}, ain[7] = {0, 1, 1, 1, 1, 1, 1};
    int64_t an[7]; int32_t identity = 1;
    n = sample_map(ign, 8, ain, 7, an, file_idx.data(), &identity);
    EXPECT(n == 6 && !identity && an[0] == 1 && file_idx[0] == 1 && file_idx[1] == 3 && file_idx[5] == 7);
    const uint8_t none[3] = {0, 0, 0}, all[3] = {1, 1, 1};
    int64_t fi[3];
    EXPECT(sample_map(none, 3, all, 3, an, fi, &identity) == 3 && identity && fi[2] == 2);
  }
  {  // the repack to the analysed samples: 3 rows of 8 samples (2 bytes), on one and on two threads
    const uint8_t rows[6] = {0x1B, 0xE4, 0xFF, 0x00, 0x6C, 0x93};
    for (int nt = 1; nt <= 2; ++nt) {
      std::vector<uint8_t> packed;
      EXPECT(repack_analysed(rows, 2, 3, file_idx.data(), n, nt, packed) == 2 && packed.size() == 6);
      for (int j = 0; j < 3; ++j)
        for (int64_t k = 0; k < n; ++k) {
          const int64_t i = file_idx[k];
          EXPECT(((packed[j * 2 + (k >> 2)] >> (2 * (k & 3))) & 3) == ((rows[j * 2 + (i >> 2)] >> (2 * (i & 3))) & 3));
        }
    }
  }
  {  // the dosage rules
    std::vector<uint32_t> q(65536); std::vector<uint8_t> ok(65536);
    for (int rf = 0; rf < 2; ++rf) {
      bgen_rule(rf, q.data(), ok.data());
      EXPECT(q[255 * 256 + 0] == (rf ? 0u : 510u) && q[0] == (rf ? 510u : 0u) && q[0 * 256 + 255] == 255u);
      EXPECT(ok[255 * 256 + 0] && (ok[255 * 256 + 1] != 0) == (rf != 0) && q[255 * 256 + 255] == (rf ? 255u : 765u));
    }
    EXPECT(pgen_rule(-3.0) == 0xFFFFu && pgen_rule(0.0) == 0 && pgen_rule(2.0) == 32768u && pgen_rule(1.0 / 16384.0) == 1u);
    EXPECT(pgen_rule(0.5 + 1e-5) == not_integral() && pgen_rule(-0.5) == not_integral() && pgen_rule(2.0 + 1.0 / 16384.0) == not_integral());
  }
  printf("ok\n");
  return 0;
}
#endif
