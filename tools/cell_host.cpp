// The periodic cell and the chain that makes a wrapped molecule whole by the text of csrc/cvf_cell.hpp -
// the very source the kernels of csrc/cv_bias.hip inline - as a stand-alone host program, for tests/test_cell_host.py and
// tests/test_cv_bias_cell_gpu.py: plain C++, no GPU, no HIP; it may be built with -fsanitize=address,undefined.
//
// stdin:   n_atoms n_frames n_triples
//          per frame   9 cell floats, then 3 n_atoms wrapped coordinates            (floats as %a or %.9g; nan and inf are read)
//          n_triples lines  nx ny nz                                                 image triples for the packed word
// stdout:  per frame   N and the 3 n_atoms summed image counts (nx ny nz per atom, as the packed word returns them)
//                      W and the 3 n_atoms whole coordinates as the hex of their fp32 bits
//          per triple  S, the packed word in hex, and the triple it unpacks to
// The chain runs sequentially here: n_j from the wrapped x_j - x_{j-1}, N_j = N_{j-1} + n_j in ints - what the kernels' scans sum.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cvf_cell.hpp"

int main() {
  int n_atoms, n_frames, n_triples;
  if (scanf("%d %d %d", &n_atoms, &n_frames, &n_triples) != 3 || n_atoms < 1 || n_frames < 0 || n_triples < 0) return 2;
  std::vector<float> x((size_t)3 * n_atoms);
  for (int f = 0; f < n_frames; ++f) {
    float cell[9];
    for (int i = 0; i < 9; ++i)
      if (scanf("%f", &cell[i]) != 1) return 2;
    for (size_t i = 0; i < x.size(); ++i)
      if (scanf("%f", &x[i]) != 1) return 2;
    const CvfCell c = cvf_cell_load(cell);
    std::vector<uint32_t> word(n_atoms);
    int N[3] = {0, 0, 0};
    for (int a = 0; a < n_atoms; ++a) {
      if (a > 0) {
        int n[3];
        cvf_cell_image(c, x[3 * a] - x[3 * a - 3], x[3 * a + 1] - x[3 * a - 2], x[3 * a + 2] - x[3 * a - 1], &n[0], &n[1], &n[2]);
        for (int i = 0; i < 3; ++i) N[i] += n[i];
      }
      word[a] = cvf_cell_pack(N[0], N[1], N[2]);
    }
    printf("N");
    for (int a = 0; a < n_atoms; ++a) {
      int u[3];
      cvf_cell_unpack(word[a], &u[0], &u[1], &u[2]);
      printf(" %d %d %d", u[0], u[1], u[2]);
    }
    printf("\nW");
    for (int a = 0; a < n_atoms; ++a) {
      float w[3];
      cvf_cell_whole(c, word[a], &x[3 * (size_t)a], w);
      for (int i = 0; i < 3; ++i) {
        uint32_t bits;
        memcpy(&bits, &w[i], 4);
        printf(" %08x", bits);
      }
    }
    printf("\n");
  }
  for (int t = 0; t < n_triples; ++t) {
    int n[3], u[3];
    if (scanf("%d %d %d", &n[0], &n[1], &n[2]) != 3) return 2;
    const uint32_t w = cvf_cell_pack(n[0], n[1], n[2]);
    cvf_cell_unpack(w, &u[0], &u[1], &u[2]);
    printf("S %08x %d %d %d\n", w, u[0], u[1], u[2]);
  }
  return 0;
}
