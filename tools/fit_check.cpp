// Host check of the device similarity fit's arithmetic: runs align_fit.h's fit_similarity5 and
// invert_affine5 (the code one GPU lane runs, here compiled for the CPU) against align_host.cpp's
// fit_similarity and invert_affine on landmark sets and compares the doubles bit for bit.  A
// stand-alone program, so that it can be built with the host sanitizers:
//
//   python tests/_fit_sets.py 112 /tmp/sets112.f32
//   hipcc --cuda-host-only -x hip -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude \
//       -Ifacerecognitionpipeline_amd/csrc tools/fit_check.cpp \
//       facerecognitionpipeline_amd/csrc/align_host.cpp -o /tmp/fit_check
//   /tmp/fit_check 112 /tmp/sets112.f32
//
// Prints the number of sets the host fits and refuses, the mismatches (exit status 1 if any) and
// the longest run of redraws of the second RANSAC index (align_fit.h bounds that loop).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "align_fit.h"
#include "runtime.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: fit_check OUT_SIZE SETS.f32\n");
    return 2;
  }
  const int S = atoi(argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    perror(argv[2]);
    return 2;
  }
  std::vector<float> lm;
  float buf[10];
  while (fread(buf, sizeof(float), 10, f) == 10) lm.insert(lm.end(), buf, buf + 10);
  fclose(f);
  const int n = (int)(lm.size() / 10);

  float tmpl[10];
  frhip_rt::reference_template(S, tmpl);
  frhip::FitLogs lg;
  frhip_rt::fit_logs(&lg);
  int fitted = 0, refused = 0, bad = 0;
  for (int i = 0; i < n; ++i) {
    double Mh[6], Md[6];
    const bool oh = frhip_rt::fit_similarity(&lm[(size_t)i * 10], tmpl, 5, Mh);
    const bool od = frhip::fit_similarity5(&lm[(size_t)i * 10], tmpl, lg, Md);
    (oh ? fitted : refused)++;
    bool same = oh == od && memcmp(Mh, Md, sizeof(Mh)) == 0;
    if (oh && od) {
      double Ih[6], Id[6];
      frhip_rt::invert_affine(Mh, Ih);
      frhip::invert_affine5(Md, Id);
      same = same && memcmp(Ih, Id, sizeof(Ih)) == 0;
    }
    if (!same) {
      ++bad;
      printf("set %d differs: host ok %d [%a %a %a %a] device ok %d [%a %a %a %a]\n", i, oh, Mh[0], Mh[1], Mh[2],
             Mh[5], od, Md[0], Md[1], Md[2], Md[5]);
    }
  }
  // the index stream of the RANSAC loop (it does not depend on the data)
  uint64_t st = ~0ull;
  int longest = 0;
  for (int it = 0; it < frhip::fit::kMaxIters; ++it) {
    const unsigned i0 = frhip::fit::rng_next(st) % 5u;
    unsigned i1 = frhip::fit::rng_next(st) % 5u;
    int run = 0;
    while (i1 == i0) {
      i1 = frhip::fit::rng_next(st) % 5u;
      ++run;
    }
    if (run > longest) longest = run;
  }
  printf("out_size %d: %d sets, host fits %d and refuses %d, %d differ; longest redraw run %d (bound %d)\n", S, n,
         fitted, refused, bad, longest, frhip::fit::kRedrawMax);
  return bad || longest >= frhip::fit::kRedrawMax ? 1 : 0;
}
