// Joint 2-D grid terms and hill deposition by the formulas of csrc/cvf_bias.hpp - the very source the
// one-launch kernels (csrc/cv_bias.hip) and the deposit kernels (csrc/cv_bias_hills.hip) inline - as a stand-alone host program, for
// tests/test_cv_bias2_host.py and tests/test_cv_bias2_gpu.py: plain C++, no GPU, no HIP; it may be built with
// -fsanitize=address,undefined.
//
// stdin:   k n_terms n_table n_points n_deposits
//          n_terms lines     kind cv kappa center tab_off n_nodes lo inv_h cv2 n_nodes2 lo2 inv_h2
//          n_table floats
//          n_points lines of k floats (xi), evaluated on the table as given
//          n_deposits times  term height sigma sigma2 inv_kdt B   and B lines of k floats (the hills' xi rows); the calls run in order,
//                            each as cvf_cv_bias_deposit does: all heights from the table before the call, then every node once
// stdout:  per point     P U du_0 .. du_{k-1} and, per 2-D term in term order, the mixed derivative of its interpolant there
//          per hill      H c1 c2 w V
//          at the end    T and the n_table floats                                      (%.9g: fp32 round trip)
// U = sum_i u_i in index order, as the kernels take it.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "cvf_bias.hpp"

int main() {
  int k, n_terms, n_table, n_points, n_dep;
  if (scanf("%d %d %d %d %d", &k, &n_terms, &n_table, &n_points, &n_dep) != 5 || k < 1 || n_table < 0 || n_points < 0 || n_dep < 0) return 2;
  cvf_bias_desc b = {};
  b.n_terms = n_terms;
  b.n_table = n_table;
  for (int t = 0; t < n_terms && t < CVF_BIAS_MAX_TERMS; ++t) {
    cvf_bias_term& e = b.term[t];
    if (scanf("%d %d %f %f %d %d %f %f %d %d %f %f", &e.kind, &e.cv, &e.kappa, &e.center, &e.tab_off, &e.n_nodes, &e.lo, &e.inv_h, &e.cv2,
              &e.n_nodes2, &e.lo2, &e.inv_h2) != 12)
      return 2;
  }
  float* table = nullptr;   // (16-byte aligned, as a 2-D term asks)
  if (n_table > 0) {
    table = (float*)aligned_alloc(16, ((size_t)n_table * sizeof(float) + 15) / 16 * 16);
    if (table == nullptr) return 2;
  }
  for (int i = 0; i < n_table; ++i)
    if (scanf("%f", &table[i]) != 1) return 2;
  b.table = table;
  char buf[240];
  const char* why = cvf_bias_why(&b, k, buf, sizeof buf);
  if (why != nullptr) {
    fprintf(stderr, "%s\n", why);
    return 3;
  }
  std::vector<float> xi(k), du(k);
  for (int p = 0; p < n_points; ++p) {
    for (int i = 0; i < k; ++i)
      if (scanf("%f", &xi[i]) != 1) return 2;
    float U = 0.0f;
    for (int i = 0; i < k; ++i) {
      float u;
      cvf_bias_cv_eval(b, i, xi.data(), &u, &du[i]);
      U += u;
    }
    printf("P %.9g", (double)U);
    for (int i = 0; i < k; ++i) printf(" %.9g", (double)du[i]);
    for (int t = 0; t < b.n_terms; ++t) {
      const cvf_bias_term& e = b.term[t];
      if (e.kind != CVF_BIAS_TABLE || e.n_nodes2 == 0) continue;
      float u, d1, d2, d12;
      cvf_bias_term2_eval(e, table, xi[e.cv], xi[e.cv2], &u, &d1, &d2, &d12);
      printf(" %.9g", (double)d12);
    }
    printf("\n");
  }
  for (int c = 0; c < n_dep; ++c) {
    cvf_hill_desc h = {};
    int B;
    if (scanf("%d %f %f %f %f %d", &h.term, &h.height, &h.sigma, &h.sigma2, &h.inv_kdt, &B) != 6 || B < 0) return 2;
    why = cvf_hill_why(&b, &h, buf, sizeof buf);
    if (why != nullptr) {
      fprintf(stderr, "%s\n", why);
      return 3;
    }
    const cvf_bias_term& e = b.term[h.term];
    std::vector<float> rows((size_t)4 * B);
    for (int r = 0; r < B; ++r) {   // every height from the table before the call
      for (int i = 0; i < k; ++i)
        if (scanf("%f", &xi[i]) != 1) return 2;
      cvf_hill_row(e, table, h, xi.data(), &rows[(size_t)4 * r]);
      printf("H %.9g %.9g %.9g %.9g\n", (double)rows[4 * r], (double)rows[4 * r + 1], (double)rows[4 * r + 2], (double)rows[4 * r + 3]);
    }
    const bool two_d = e.n_nodes2 != 0;
    const int n2 = two_d ? e.n_nodes2 : 1, w = two_d ? 4 : 2;
    for (int node = 0; node < e.n_nodes * n2; ++node) {   // every node once, the hills in order
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      float* p = table + e.tab_off + (size_t)w * node;
      for (int i = 0; i < w; ++i) acc[i] = p[i];
      const int j1 = node / n2, j2 = node - j1 * n2;
      const float x1 = cvf_bias_node_pos(e.lo, e.inv_h, j1), x2 = two_d ? cvf_bias_node_pos(e.lo2, e.inv_h2, j2) : 0.0f;
      for (int r = 0; r < B; ++r) {
        if (two_d)
          cvf_hill_node_add<true>(h, &rows[(size_t)4 * r], x1, x2, acc);
        else
          cvf_hill_node_add<false>(h, &rows[(size_t)4 * r], x1, x2, acc);
      }
      for (int i = 0; i < w; ++i) p[i] = acc[i];
    }
  }
  printf("T");
  for (int i = 0; i < n_table; ++i) printf(" %.9g", (double)table[i]);
  printf("\n");
  free(table);
  return 0;
}
