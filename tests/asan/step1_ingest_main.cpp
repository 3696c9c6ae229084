// TEST SCAFFOLDING: a stand-alone program (its own main, host code only) that drives Step1Ingest (regenie_amd/host/driver_step1_ingest.cpp) over
// a .bed of a few KB with the device library replaced by malloc-backed stand-ins, built with -fsanitize=address,undefined by
// tests/test_step1_ingest_asan_cpu.py.  The stand-in rg_stage_free reads its context, as the library's does: an ingest that outlives its
// context is a use-after-free here.  Four orders of events: start -> level 0 from the staged copy -> release -> destroy; start -> given up ->
// release; start -> release while the copy is under way; never started.
#include "driver_step1.h"
using namespace rgdrv;

struct rg_ctx { int device; int64_t staged; };
static std::vector<uint8_t> g_file;      // the .bed as written
static int64_t g_rows_checked = 0;
extern "C" {
const char* rg_last_error(const rg_ctx*) { return "stand-in"; }
void* rg_host_alloc(int64_t b) { return malloc(b > 0 ? b : 1); }
void rg_host_free(void* p) { free(p); }
int rg_host_register(void*, int64_t, int) { return 0; }
int rg_host_unregister(void*) { return 0; }
void* rg_stage_alloc(rg_ctx* c, int64_t bytes, double) { c->staged += bytes; return malloc(bytes); }
int rg_stage_copy(rg_ctx* c, void* dst, const void* src, int64_t bytes) {
  std::this_thread::sleep_for(std::chrono::milliseconds(30));      // long enough for a release to arrive while the copy is under way
  if (c->device != 7) return 1;
  memcpy(dst, src, bytes);
  return 0;
}
void rg_stage_free(rg_ctx* c, void* p) { if (c->device != 7) abort(); c->staged = 0; free(p); }
int rg_stage_fits(rg_ctx* c, int64_t bytes) { return c->device == 7 && bytes < (1LL << 40); }
int32_t rg_l0_batch_blocks(const rg_ctx*) { return 3; }
int rg_l0_blocks(rg_ctx*, int32_t n, const int32_t*, const int32_t* bs, const uint8_t* const* rows, int64_t pitch, int) {
  for (int b = 0; b < n; ++b) {      // the rows handed over are the file's, wherever they come from
    const uint8_t* at = (const uint8_t*)memmem(g_file.data(), g_file.size(), rows[b], (size_t)(bs[b] * pitch));
    if (!at) return 1;
    g_rows_checked += bs[b];
  }
  return 0;
}
int rg_l0_blocks_f64(rg_ctx*, int32_t, const int32_t*, const int32_t*, const double* const*, int64_t, int) { return 1; }
int rg_sync(rg_ctx*) { return 0; }
int rg_ingest_fence(rg_ctx*) { return 0; }
void rg_destroy(rg_ctx* c) { c->device = -1; delete c; }
}

static std::vector<std::shared_future<rg_ctx*>> ready(rg_ctx* c) {
  std::promise<rg_ctx*> pr;
  pr.set_value(c);
  return {pr.get_future().share()};
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  setenv("RG_TEARDOWN", "1", 1);
  setenv("RG_INGEST_STAGE", "1", 1);
  const std::string pfx = std::string(argv[1]) + "/tiny";
  Run r;
  r.p.step = 1; r.p.gpus = 1; r.p.bsize = 8; r.p.bed = pfx;
  r.n_file = 200; r.bpr = 50;
  const int M = 61;
  g_file.assign(3 + (size_t)M * r.bpr, 0);
  g_file[0] = 0x6c; g_file[1] = 0x1b; g_file[2] = 1;
  for (size_t i = 3; i < g_file.size(); ++i) g_file[i] = (uint8_t)(i * 2654435761u >> 13);
  { std::ofstream f(pfx + ".bed", std::ios::binary); f.write((const char*)g_file.data(), (std::streamsize)g_file.size()); }
  std::vector<Blk> blocks;
  for (int v = 0; v < M; ++v) { r.snp_chrom.push_back(1); r.snp_offset.push_back(v); }
  for (int v = 0; v < M; v += 8) blocks.push_back({1, v, std::min(8, M - v)});
  const int B = (int)blocks.size();
  const auto t0 = Clock::now();

  {  // 1: the whole file staged, level 0 reads the copy, release, then the context goes
    rg_ctx* c = new rg_ctx{7, 0};
    Step1Ingest ing(r, t0);
    ing.start_early(ready(c));
    ing.settle(c, 1 << 20);
    ing.map_ready();
    std::ostringstream lg;
    ing.level0(c, blocks, 0, B, lg, false);
    if (lg.str().find("read from the copy of the file in device memory") == std::string::npos || g_rows_checked != M) { fprintf(stderr, "1: %s", lg.str().c_str()); return 1; }
    ing.release();
    if (c->staged != 0) return 1;
    rg_destroy(c);
  }
  {  // 2: the stage is given up (no room beside it), level 0 copies from the mapping
    rg_ctx* c = new rg_ctx{7, 0};
    Step1Ingest ing(r, t0);
    ing.start_early(ready(c));
    ing.settle(c, 1LL << 41);
    if (c->staged != 0) return 1;
    ing.map_ready();
    std::ostringstream lg;
    ing.level0(c, blocks, 0, B, lg, false);
    if (lg.str().find("copied to the GPU from the mapped file") == std::string::npos) { fprintf(stderr, "2: %s", lg.str().c_str()); return 1; }
    ing.release();
    rg_destroy(c);
  }
  {  // 3: release while the copy is under way
    rg_ctx* c = new rg_ctx{7, 0};
    Step1Ingest ing(r, t0);
    ing.start_early(ready(c));
    ing.release();
    if (c->staged != 0) return 1;
    rg_destroy(c);
  }
  {  // 4: never started; and the ring of host buffers for the same blocks (RG_INGEST_MAP=0), released by the destructor
    rg_ctx* c = new rg_ctx{7, 0};
    {
      Step1Ingest ing(r, t0);
      ing.release();
      bool threw = false;
      try { ing.map_ready(); } catch (const std::logic_error&) { threw = true; }      // a released ingest says so
      if (!threw) return 1;
    }
    setenv("RG_INGEST_MAP", "0", 1);
    g_rows_checked = 0;
    {
      Step1Ingest ing(r, t0);
      ing.start_early(ready(c));
      ing.settle(c, 1LL << 41);      // no room, and no stage to give up: nothing is cancelled, nothing logged
      ing.map_ready();
      std::ostringstream lg;
      ing.level0(c, blocks, 0, B, lg, false);
      if (lg.str().find("in the reader thread") == std::string::npos || g_rows_checked != M) { fprintf(stderr, "4: %s", lg.str().c_str()); return 1; }
    }
    rg_destroy(c);
  }
  printf("step1 ingest: four sequences clean\n");
  return 0;
}
