// The bias term formulas of csrc/cvf_bias.hpp - the very source the one-launch kernels inline (csrc/cv_bias.hip) - as a stand-alone
// host program, for tests/test_cv_bias_host.py: plain C++, no GPU, no HIP; it may be built with -fsanitize=address,undefined.
//
// stdin:   k n_terms n_table n_points
//          n_terms lines  kind cv kappa center tab_off n_nodes lo inv_h
//          n_table floats
//          n_points lines of k floats (xi)
// stdout:  per point one line  U du_0 .. du_{k-1}   (%.9g: fp32 round trip), U = sum_i u_i in index order as the kernels take it
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "cvf_bias.hpp"

int main() {
  int k, n_terms, n_table, n_points;
  if (scanf("%d %d %d %d", &k, &n_terms, &n_table, &n_points) != 4 || k < 1 || n_table < 0 || n_points < 0) return 2;
  cvf_bias_desc b = {};
  b.n_terms = n_terms;
  b.n_table = n_table;
  for (int t = 0; t < n_terms && t < CVF_BIAS_MAX_TERMS; ++t) {
    cvf_bias_term& e = b.term[t];
    if (scanf("%d %d %f %f %d %d %f %f", &e.kind, &e.cv, &e.kappa, &e.center, &e.tab_off, &e.n_nodes, &e.lo, &e.inv_h) != 8) return 2;
  }
  std::vector<float> table(n_table);
  for (int i = 0; i < n_table; ++i)
    if (scanf("%f", &table[i]) != 1) return 2;
  b.table = n_table > 0 ? table.data() : nullptr;
  char buf[200];
  const char* why = cvf_bias_why(&b, k, buf, sizeof buf);
  if (why != nullptr) {
    fprintf(stderr, "%s\n", why);
    return 3;
  }
  std::vector<float> xi(k);
  for (int p = 0; p < n_points; ++p) {
    for (int i = 0; i < k; ++i)
      if (scanf("%f", &xi[i]) != 1) return 2;
    float U = 0.0f;
    std::vector<float> du(k);
    for (int i = 0; i < k; ++i) {
      float u;
      cvf_bias_cv_eval(b, i, xi[i], &u, &du[i]);
      U += u;
    }
    printf("%.9g", (double)U);
    for (int i = 0; i < k; ++i) printf(" %.9g", (double)du[i]);
    printf("\n");
  }
  return 0;
}
