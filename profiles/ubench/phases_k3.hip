// Diagnostic: where do the cycles of the chunk kernel (acm_chunk) go?  Builds the real kernel source with ACM_STAMPS (s_memtime stamps per
// phase, per wavefront) on synthetic byte-plane data and prints the phase shares, and when the wavefronts of the launch begin and end their
// share of the chunk table (both clocks, every wavefront).  Timing only (the PCM is not looked at).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include -I libacm_amd/csrc -o profiles/ubench/phases_k3.bin profiles/ubench/phases_k3.hip \
//         libacm_amd/csrc/acm_kernels_f32.hip libacm_amd/csrc/acm_kernel_geo.cpp    (the launchers name their float32 twins and ask for the launch geometry)
//   ./phases_k3 <level> [rows per block = 16] [percent of the blocks at 16 bits = 56] [percent at 12 bits = 0]
//               [chunks per claimed run = -1: the level's default; 0: the static split] [static share in thousandths = -1: the default]
#ifndef NO_STAMPS
#define ACM_STAMPS 1              /* (-DNO_STAMPS: the plain kernel, for counter collections and timing) */
#endif
#include "../../libacm_amd/csrc/acm_kernels.hip"
#include <algorithm>
#include <cstdio>
#include <vector>
int main(int argc, char **argv) {
  const int level = argc > 1 ? atoi(argv[1]) : 9;
  const uint32_t rows = argc > 2 ? atoi(argv[2]) : 16, pct16 = argc > 3 ? atoi(argv[3]) : 56, pct12 = argc > 4 ? atoi(argv[4]) : 0;
  const int run_chunks = argc > 5 ? atoi(argv[5]) : -1, static_permille = argc > 6 ? atoi(argv[6]) : -1;
  acmk_tile2m_claim_config(run_chunks, static_permille, nullptr, nullptr);
  const uint32_t nstreams = 1024, nrows = (uint32_t)((1u << 21) >> level), nblocks = (nrows + rows - 1) / rows;
  const uint64_t cols = 1ull << level, per = (uint64_t)nrows * cols;
  const uint32_t TR = (uint32_t)acmk_tile2m_rows(level);
  if (acmk_tile2m_stages(level) != 6) { printf("level %d has no chunk kernel\n", level); return 1; }
  std::vector<AcmTile2> tiles; std::vector<uint32_t> pairs; uint64_t at = 0; uint32_t seed = 12345;
  for (uint32_t i = 0; i < nstreams; i++) {
    const uint32_t p0 = (uint32_t)pairs.size();
    pairs.push_back((uint32_t)((at >> 6) << 2 | ACMHIP_BP_BYTE)); at += 2 * cols;            /* the pair of zeros in front */
    uint32_t cls = ACMHIP_BP_WORD;
    for (uint32_t p = 0; p < nrows / 2; p++) {
      if ((2 * p) % rows < 2) { seed = seed * 1664525u + 1013904223u; const uint32_t d100 = (seed >> 16) % 100; cls = d100 < pct16 ? ACMHIP_BP_WORD : d100 < pct16 + pct12 ? ACMHIP_BP_NIB12 : ACMHIP_BP_BYTE; }
      pairs.push_back((uint32_t)((at >> 6) << 2 | cls)); at += (cls == ACMHIP_BP_WORD ? 4 : cls == ACMHIP_BP_NIB12 ? 3 : 2) * cols;
    }
    for (uint32_t r = 0; r + TR <= nrows; r += TR) {
      const uint64_t rh = r >= 2 ? r - 2 : 0;
      tiles.push_back(AcmTile2{ p0 + r / 2, i * per + r * cols, (uint32_t)(i * nblocks + rh / rows), (uint32_t)(rh % rows),
                                (uint32_t)(((1ull << 32) + rows - 1) / rows), (r == 0 ? ACM_TILE_FRESH : 0u) | (r == 1 ? ACM_TILE_ROW1 : 0u) | ((r & 1) ? ACM_TILE_ODD : 0u) |
                                ((rh % rows) + (r + TR - 1 - rh) < rows ? ACM_TILE_ONEBLOCK : 0u) });
    }
  }
  for (int k = 0; k < 64; k++) pairs.push_back(0);
  uint8_t *d_blob; int16_t *d_pcm, *d_sink; acmhip_blkhdr *d_hdr; AcmTile2 *d_t; uint32_t *d_pairs, *d_claim;
  (void)hipMalloc(&d_claim, 256); (void)hipMemset(d_claim, 0, 256);
  uint32_t static_per = 0, run_len = 0, nclaimed = 0;
  (void)hipMalloc(&d_sink, ACM_K2_SINK_BYTES); (void)hipMalloc(&d_blob, at + 4096); (void)hipMalloc(&d_pcm, per * nstreams * 2);
  (void)hipMalloc(&d_hdr, (size_t)nstreams * nblocks * 8); (void)hipMalloc(&d_t, tiles.size() * sizeof(AcmTile2)); (void)hipMalloc(&d_pairs, pairs.size() * 4);
  (void)hipMemset(d_blob, 3, at + 4096);
  std::vector<acmhip_blkhdr> hdr((size_t)nstreams * nblocks); for (size_t k = 0; k < hdr.size(); k++) { hdr[k].val = 1 + (uint32_t)(k * 7919u) % 255; hdr[k].pwr = 8; }
  (void)hipMemcpy(d_hdr, hdr.data(), hdr.size() * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(d_t, tiles.data(), tiles.size() * sizeof(AcmTile2), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice);
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  float ms = 0, best = 1e9;
  for (int rep = 0; rep < 8; rep++) {
    (void)hipEventRecord(e0);
    int rc = acmk_launch_tile2m(level, 256, d_t, (uint32_t)tiles.size(), d_blob, d_pairs, d_hdr, d_pcm, d_sink, 0, d_claim, nullptr);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    if (rc) { printf("launch failed %d\n", rc); return 1; }
    (void)hipEventElapsedTime(&ms, e0, e1); if (ms < best) best = ms;
  }
  (void)acmk_tile2m_split(level, 256, (uint32_t)tiles.size(), &static_per, &run_len, &nclaimed);
  uint32_t claim_left = 0; (void)hipMemcpy(&claim_left, d_claim, 4, hipMemcpyDeviceToHost);
  printf("split of %zu chunks over %d wavefronts: static runs of %u, %u claimed runs of %u; the claim word after 8 launches: %u\n", tiles.size(),
         acmk_tile2m_run_waves(level, 256), static_per, nclaimed, run_len, claim_left);
#ifdef NO_STAMPS
  printf("acm_chunk level %d, %u rows per block, %u %% / %u %% of the blocks at 16 / 12 bits (staged %.2f B/sample), %zu chunks, no stamps: %.3f ms per launch (best of 8; %.3f of the 8 TB/s roofline at 4 B/sample)\n",
         level, rows, pct16, pct12, (double)at / (per * nstreams), tiles.size(), best, per * nstreams * 4.0 / best / 8e9);
  return 0;
#else
  static unsigned long long h[2048][8];
  (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_acm_stamps), sizeof(h));
  double sum[8] = {0}; int n = 0;
  for (int w = 0; w < 2048; w++) { if (!h[w][1]) continue; n++; for (int k = 0; k < 8; k++) sum[k] += (double)h[w][k]; }
  double tot = 0; for (int k = 0; k < 7; k++) tot += sum[k];
  const char *names[7] = {"carry reset + row values", "first pass (matrix passes, scaling, LDS store)", "issue of the next chunk's loads", "LDS passes",
                          "start of a run (its first loads, waited for; a claimed run: + the replayed chunk's share of the rest)",
                          "write-out (LDS gather + PCM stores)", "end-of-iteration wait for the prefetched loads"};
  const double chunks_per_wave = tiles.size() / 4096.0;
  printf("acm_chunk level %d, %u rows per block, %u %% of the blocks at 16 bits: %.3f ms per launch with stamps (best of 8; %.3f of the 8 TB/s roofline at 4 B/sample), "
         "%zu chunks, %d waves sampled, ticks per chunk %.0f (staged %.2f B/sample)\n", level, rows, pct16, best, per * nstreams * 4.0 / best / 8e9, tiles.size(), n,
         tot / n / chunks_per_wave, (double)at / (per * nstreams));
  for (int k = 0; k < 7; k++) printf("  %-62s %5.1f %%  %8.0f ticks per chunk\n", names[k], 100.0 * sum[k] / tot, sum[k] / n / chunks_per_wave);

  /* when the wavefronts of the LAST launch begin and end (g_acm_wave_stamps): s_memtime and the constant-rate counter at both ends */
  const int NWV = acmk_tile2m_run_waves(level, 256);
  static unsigned long long w[ACM_WAVE_STAMPS_MAX][8];
  (void)hipMemcpyFromSymbol(w, HIP_SYMBOL(g_acm_wave_stamps), sizeof(w));
  struct Wave { double r0, r1, c; unsigned chunks, runs, slot, simd, cu, se, xcc, age; };
  std::vector<Wave> ws;
  unsigned long long rmin = ~0ull, rmax = 0;
  for (int v = 0; v < NWV && v < ACM_WAVE_STAMPS_MAX; v++) {
    if (!w[v][4]) continue;
    rmin = std::min(rmin, w[v][1]); rmax = std::max(rmax, w[v][3]);
  }
  for (int v = 0; v < NWV && v < ACM_WAVE_STAMPS_MAX; v++) {
    if (!w[v][4]) continue;
    const unsigned hw = (unsigned)w[v][5], xcc = (unsigned)(w[v][5] >> 32) & 15u;
    /* HW_ID: wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13 (gfx9) */
    ws.push_back(Wave{ (double)(w[v][1] - rmin), (double)(w[v][3] - rmin), (double)(w[v][2] - w[v][0]), (unsigned)w[v][4], (unsigned)w[v][6], (unsigned)v % 16u,
                       (hw >> 4) & 3u, (hw >> 8) & 15u, (hw >> 13) & 7u, xcc, 0u });
  }
  if (ws.empty()) { printf("no wavefront stamps\n"); return 0; }
  /* age on a SIMD: the rank of a wavefront's start among the wavefronts of its workgroup (= its CU) on the same SIMD */
  for (size_t a = 0; a < ws.size(); a++)
    for (size_t b = a - a % 16; b < ws.size() && b < a - a % 16 + 16; b++)
      if (b != a && ws[b].simd == ws[a].simd && (ws[b].r0 < ws[a].r0 || (ws[b].r0 == ws[a].r0 && b < a))) ws[a].age++;
  const double span = (double)(rmax - rmin);                       /* ticks of the constant-rate counter from the first start to the last end */
  const double tick_ns = 10.0;                                     /* 100 MHz */
  double busy = 0, chunks = 0, runs = 0, ratio = 0, start_max = 0; std::vector<double> ends;
  for (const Wave &x : ws) { busy += x.r1 - x.r0; chunks += x.chunks; runs += x.runs; ends.push_back(x.r1 / span); ratio += x.c / (x.r1 - x.r0); start_max = std::max(start_max, x.r0); }
  std::sort(ends.begin(), ends.end());
  auto pct = [&](double p) { return ends[std::min(ends.size() - 1, (size_t)(p * (ends.size() - 1) + 0.5))]; };
  printf("wavefronts: %zu stamped, %.0f chunk executions (%.1f per wavefront, %.2f runs per wavefront; the table has %zu), first start to last end %.4f ms "
         "(the launch by events, with stamps: %.4f ms best of 8), latest start %.4f ms\n", ws.size(), chunks, chunks / ws.size(), runs / ws.size(), tiles.size(),
         span * tick_ns * 1e-6, best, start_max * tick_ns * 1e-6);
  printf("  s_memtime ticks per tick of the constant-rate counter (100 MHz), mean over wavefronts: %.3f\n", ratio / ws.size());
  printf("  end of a wavefront as a share of the span, percentile 1 / 10 / 50 / 90 / 99 / 100: %.3f %.3f %.3f %.3f %.3f %.3f\n", pct(0.01), pct(0.10), pct(0.50), pct(0.90), pct(0.99), pct(1.0));
  printf("  mean busy share (end - start over the span): %.4f, mean idle share %.4f\n", busy / ws.size() / span, 1.0 - busy / ws.size() / span);
  auto split = [&](const char *what, int nkeys, auto key) {
    printf("  by %s: mean end share (mean chunks) ", what);
    for (int k = 0; k < nkeys; k++) {
      double e = 0, c = 0; int m = 0;
      for (const Wave &x : ws) if ((int)key(x) == k) { e += x.r1 / span; c += x.chunks; m++; }
      if (m) printf(" %d: %.3f (%.1f)", k, e / m, c / m);
    }
    printf("\n");
  };
  split("wavefront slot in the workgroup", 16, [](const Wave &x) { return x.slot; });
  split("age on its SIMD (0 = started first)", 4, [](const Wave &x) { return x.age; });
  split("SIMD", 4, [](const Wave &x) { return x.simd; });
  split("XCD", 8, [](const Wave &x) { return x.xcc; });
  return 0;
#endif
}
