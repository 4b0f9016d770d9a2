// The bias potential along a CV (include/cvf.h: cvf_bias_desc, cvf_cv_*_bias_*): the term formulas ONCE,
// for the two one-launch kernels (csrc/cv_bias.hip) and for the host (cvf_cv_bias_check; tools/bias_host.cpp compiles this file
// into a stand-alone program that tests/test_cv_bias_host.py checks against fp64).  No HIP include: plain C++ on either side.
//
//   U(xi) = sum_t U_t(xi[cv_t]),  du[i] = sum_{t: cv_t = i} U_t'(xi[i])       both sums in term order
//
// CVF_BIAS_TABLE: nodes j = 0 .. n_nodes - 1 at lo + j / inv_h carry (U_j, U'_j) at table[tab_off + 2 j]; on interval j, with
// s = (xi - lo) inv_h, t = s - j in [0, 1] and h = 1 / inv_h, U is the cubic Hermite interpolant
//   U  = h00(t) U_j + h01(t) U_{j+1} + h (h10(t) U'_j + h11(t) U'_{j+1})
//   U' = inv_h (h00'(t) U_j + h01'(t) U_{j+1}) + h10'(t) U'_j + h11'(t) U'_{j+1}        (the derivative of that polynomial)
// so U is C1 across the nodes.  xi on the last node belongs to the last interval (t = 1: U = U_last, U' = U'_last exactly).  Below
// lo and above the last node U continues linearly with the end node's value and slope.
//
// A CVF_BIAS_TABLE term with n_nodes2 >= 2 is a joint grid U(xi[cv], xi[cv2]) with four floats per node (cvf_bias_term2_eval), and
// the hills of metadynamics are added to either kind of table by cvf_hill_row and cvf_hill_node_add (DESIGN.md section 4.19;
// tools/bias2_host.cpp is the stand-alone program of these).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "cvf.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CVF_BIAS_HD __host__ __device__ inline
#else
#define CVF_BIAS_HD inline
#endif

// U_t(xi) and U_t'(xi) of one term.  The node index stays within 0 .. n_nodes - 2 for every xi, NaN included (cvf_bias_why has
// checked that the table holds tab_off + 2 n_nodes floats).
CVF_BIAS_HD void cvf_bias_term_eval(const cvf_bias_term& t, const float* table, float xi, float* u, float* du) {
  const float d = xi - t.center;
  switch (t.kind) {
    case CVF_BIAS_HARMONIC:
      *du = t.kappa * d;
      *u = 0.5f * t.kappa * d * d;
      return;
    case CVF_BIAS_UPPER_WALL:
      *du = xi > t.center ? t.kappa * d : 0.0f;
      *u = xi > t.center ? 0.5f * t.kappa * d * d : 0.0f;
      return;
    case CVF_BIAS_LOWER_WALL:
      *du = xi < t.center ? t.kappa * d : 0.0f;
      *u = xi < t.center ? 0.5f * t.kappa * d * d : 0.0f;
      return;
    case CVF_BIAS_LINEAR:
      *du = t.kappa;
      *u = t.kappa * xi;
      return;
    case CVF_BIAS_TABLE: {
      const float* nodes = table + t.tab_off;
      const float h = 1.0f / t.inv_h, s = (xi - t.lo) * t.inv_h;
      const int last = t.n_nodes - 1;
      if (!(s >= 0.0f)) {   // below lo (and NaN): the first node's line
        *du = nodes[1];
        *u = nodes[0] + nodes[1] * (xi - t.lo);
        return;
      }
      if (s > (float)last) {   // above the last node: its line
        *du = nodes[2 * last + 1];
        *u = nodes[2 * last] + nodes[2 * last + 1] * ((s - (float)last) * h);
        return;
      }
      int j = (int)s;   // 0 <= s <= last
      j = j > last - 1 ? last - 1 : j;
      const float x = s - (float)j, x2 = x * x, x3 = x2 * x;
      const float u0 = nodes[2 * j], d0 = nodes[2 * j + 1], u1 = nodes[2 * j + 2], d1 = nodes[2 * j + 3];
      const float h00 = 2.0f * x3 - 3.0f * x2 + 1.0f, h10 = x3 - 2.0f * x2 + x, h01 = 3.0f * x2 - 2.0f * x3, h11 = x3 - x2;
      const float g00 = 6.0f * (x2 - x), g10 = 3.0f * x2 - 4.0f * x + 1.0f, g11 = 3.0f * x2 - 2.0f * x;   // (h01' = -h00')
      *u = h00 * u0 + h01 * u1 + h * (h10 * d0 + h11 * d1);
      *du = t.inv_h * (g00 * (u0 - u1)) + g10 * d0 + g11 * d1;   // (the difference first: inv_h magnifies what it loses)
      return;
    }
    default:   // (refused by cvf_bias_why)
      *du = 0.0f;
      *u = 0.0f;
  }
}

// One axis of a joint grid (below): the node line j of the cell, the cell coordinate x in [0, 1], and d - how far xi lies outside the
// grid (0 inside).  The 1-D rules: NaN goes below, xi on the last node belongs to the last cell (x = 1).
CVF_BIAS_HD void cvf_bias_axis(float xi, float lo, float inv_h, int n_nodes, int* j, float* x, float* d) {
  const float s = (xi - lo) * inv_h;
  const int last = n_nodes - 1;
  if (!(s >= 0.0f)) {
    *j = 0, *x = 0.0f, *d = xi - lo;
    return;
  }
  if (s > (float)last) {
    *j = last - 1, *x = 1.0f, *d = (s - (float)last) * (1.0f / inv_h);
    return;
  }
  int c = (int)s;
  c = c > last - 1 ? last - 1 : c;
  *j = c, *x = s - (float)c, *d = 0.0f;
}

// The cubic Hermite interpolant of (u0, d0) at x = 0 and (u1, d1) at x = 1 on a cell of width h = 1 / inv_h, and its derivative in
// the units of xi: the formulas of CVF_BIAS_TABLE above.  diff = u0 - u1 comes from the caller, who takes it where it is exact -
// between neighbouring nodes - because inv_h magnifies what it has lost.
CVF_BIAS_HD void cvf_bias_hermite(float x, float h, float inv_h, float u0, float d0, float u1, float d1, float diff, float* v, float* dv) {
  const float x2 = x * x, x3 = x2 * x;
  const float h00 = 2.0f * x3 - 3.0f * x2 + 1.0f, h10 = x3 - 2.0f * x2 + x, h01 = 3.0f * x2 - 2.0f * x3, h11 = x3 - x2;
  const float g00 = 6.0f * (x2 - x), g10 = 3.0f * x2 - 4.0f * x + 1.0f, g11 = 3.0f * x2 - 2.0f * x;
  *v = h00 * u0 + h01 * u1 + h * (h10 * d0 + h11 * d1);
  *dv = inv_h * (g00 * diff) + g10 * d0 + g11 * d1;
}

// A node of a joint grid: (U, d1 U, d2 U, d12 U) in one 16-byte access (cvf_bias_why has checked table and tab_off).
struct cvf_bias_node2 {
  float u, d1, d2, d12;
};
CVF_BIAS_HD cvf_bias_node2 cvf_bias_load2(const float* nodes, int j1, int j2, int n2) {
  cvf_bias_node2 n;
  __builtin_memcpy(&n, __builtin_assume_aligned(nodes + 4 * (j1 * n2 + j2), 16), sizeof n);
  return n;
}

// A joint grid term (CVF_BIAS_TABLE with n_nodes2 >= 2) at (xi_cv, xi_cv2) = (a, b): U, its two derivatives and (d12 != NULL) the
// mixed one.  Inside the grid the bicubic Hermite interpolant of the cell - along cv2 on the cell's two node lines, where (U, d2 U)
// give U and d2 U and (d1 U, d12 U) give d1 U and d12 U, then along cv - so the tensor product of the 1-D basis, and the derivatives
// are those of that polynomial.  Outside, with P = xi clamped per axis and d = xi - P (include/cvf.h):
//   U = U(P) + d1U(P) d_1 + d2U(P) d_2 + d12U(P) d_1 d_2,  d1 U = d1U(P) + d12U(P) d_2,  d2 U = d2U(P) + d12U(P) d_1
// The node indices stay within the grid for every xi, NaN included.
CVF_BIAS_HD void cvf_bias_term2_eval(const cvf_bias_term& t, const float* table, float a, float b, float* u, float* d1, float* d2,
                                     float* d12 = nullptr) {
  int j1, j2;
  float x, y, e1, e2;
  cvf_bias_axis(a, t.lo, t.inv_h, t.n_nodes, &j1, &x, &e1);
  cvf_bias_axis(b, t.lo2, t.inv_h2, t.n_nodes2, &j2, &y, &e2);
  const float* nodes = table + t.tab_off;
  const float h1 = 1.0f / t.inv_h, h2 = 1.0f / t.inv_h2;
  cvf_bias_node2 n[2][2];         // the cell's corners (j1 + i, j2 + j)
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) n[i][j] = cvf_bias_load2(nodes, j1 + i, j2 + j, t.n_nodes2);
  float p[2], q[2], r[2], s[2];   // on node line j1 + i: U, d2 U, d1 U, d12 U at y
  for (int i = 0; i < 2; ++i) {
    cvf_bias_hermite(y, h2, t.inv_h2, n[i][0].u, n[i][0].d2, n[i][1].u, n[i][1].d2, n[i][0].u - n[i][1].u, &p[i], &q[i]);
    cvf_bias_hermite(y, h2, t.inv_h2, n[i][0].d1, n[i][0].d12, n[i][1].d1, n[i][1].d12, n[i][0].d1 - n[i][1].d1, &r[i], &s[i]);
  }
  // p[0] - p[1] and q[0] - q[1] as the interpolant of the corner differences: the x-derivatives below multiply them by inv_h
  float pd, qd;
  cvf_bias_hermite(y, h2, t.inv_h2, n[0][0].u - n[1][0].u, n[0][0].d2 - n[1][0].d2, n[0][1].u - n[1][1].u, n[0][1].d2 - n[1][1].d2,
                   (n[0][0].u - n[1][0].u) - (n[0][1].u - n[1][1].u), &pd, &qd);
  float U, U1, U2, U12;
  cvf_bias_hermite(x, h1, t.inv_h, p[0], r[0], p[1], r[1], pd, &U, &U1);
  cvf_bias_hermite(x, h1, t.inv_h, q[0], s[0], q[1], s[1], qd, &U2, &U12);
  if (e1 != 0.0f || e2 != 0.0f) {   // outside (and NaN)
    U = U + U1 * e1 + U2 * e2 + U12 * (e1 * e2);
    U1 = U1 + U12 * e2;
    U2 = U2 + U12 * e1;
  }
  *u = U, *d1 = U1, *d2 = U2;
  if (d12 != nullptr) *d12 = U12;
}

// CV i's share of the bias from the whole xi row: in term order, the 1-D terms with cv_t = i as below; of a joint grid term its U and
// dU/dxi_cv where cv_t = i, and dU/dxi_cv2 alone where cv2_t = i.
CVF_BIAS_HD void cvf_bias_cv_eval(const cvf_bias_desc& b, int i, const float* xi_row, float* u, float* du) {
  float us = 0.0f, ds = 0.0f;
  const float xi = xi_row[i];   // (read once, ahead of the loop: the row lies in LDS on the device)
  for (int t = 0; t < b.n_terms; ++t) {
    const cvf_bias_term& e = b.term[t];
    // (the four fields read together, no short circuit: on the device each dependent read of the description is a round trip)
    const int kind = e.kind, cv = e.cv, cv2 = e.cv2, n_nodes2 = e.n_nodes2;
    if ((kind == CVF_BIAS_TABLE) & (n_nodes2 != 0)) {
      if ((cv != i) & (cv2 != i)) continue;
      float ut, d1, d2;
      cvf_bias_term2_eval(e, b.table, xi_row[cv], xi_row[cv2], &ut, &d1, &d2);
      if (cv == i) {
        us += ut;
        ds += d1;
      } else {
        ds += d2;
      }
      continue;
    }
    if (cv != i) continue;
    float ut, dt;
    cvf_bias_term_eval(e, b.table, xi, &ut, &dt);
    us += ut;
    ds += dt;
  }
  *u = us;
  *du = ds;
}

// The same from xi_i alone: the 1-D terms (a joint grid term needs the row and is passed over).
CVF_BIAS_HD void cvf_bias_cv_eval(const cvf_bias_desc& b, int i, float xi, float* u, float* du) {
  float us = 0.0f, ds = 0.0f;
  for (int t = 0; t < b.n_terms; ++t) {
    if (b.term[t].cv != i) continue;
    if (b.term[t].kind == CVF_BIAS_TABLE && b.term[t].n_nodes2 != 0) continue;
    float ut, dt;
    cvf_bias_term_eval(b.term[t], b.table, xi, &ut, &dt);
    us += ut;
    ds += dt;
  }
  *u = us;
  *du = ds;
}

// NULL, or why `b` is no bias on k CVs (in buf, the field named).  Host arithmetic: `table` is only compared with NULL.
inline const char* cvf_bias_why(const cvf_bias_desc* b, int k, char* buf, size_t n_buf) {
  if (b == nullptr) return "no bias description";
  if (b->n_terms < 0 || b->n_terms > CVF_BIAS_MAX_TERMS) {
    snprintf(buf, n_buf, "n_terms = %d: 0 to %d (CVF_BIAS_MAX_TERMS) are supported", b->n_terms, CVF_BIAS_MAX_TERMS);
    return buf;
  }
  if (b->n_table < 0) {
    snprintf(buf, n_buf, "n_table = %d is negative", b->n_table);
    return buf;
  }
  for (int i = 0; i < b->n_terms; ++i) {
    const cvf_bias_term& t = b->term[i];
#define CVF_BIAS_NO(...)                  \
  do {                                    \
    snprintf(buf, n_buf, __VA_ARGS__);    \
    return buf;                           \
  } while (0)
    if (t.kind < CVF_BIAS_HARMONIC || t.kind > CVF_BIAS_TABLE) CVF_BIAS_NO("term[%d].kind = %d is no CVF_BIAS_* kind", i, t.kind);
    if (t.cv < 0 || t.cv >= k) CVF_BIAS_NO("term[%d].cv = %d: the model has CVs 0 to %d", i, t.cv, k - 1);
    if (!isfinite(t.kappa)) CVF_BIAS_NO("term[%d].kappa is not finite", i);   // (every kind: unused fields are 0)
    if (!isfinite(t.center)) CVF_BIAS_NO("term[%d].center is not finite", i);
    if (!isfinite(t.lo)) CVF_BIAS_NO("term[%d].lo is not finite", i);
    if (t.kind != CVF_BIAS_TABLE) continue;
    if (!(t.inv_h > 0.0f) || !isfinite(t.inv_h)) CVF_BIAS_NO("term[%d].inv_h = %g: the node spacing 1 / inv_h must be positive and finite", i, (double)t.inv_h);
    if (t.n_nodes < 2) CVF_BIAS_NO("term[%d].n_nodes = %d: a table has at least 2 nodes", i, t.n_nodes);
    if (t.n_nodes2 != 0) {   // a joint grid on (cv, cv2)
      if (t.n_nodes2 < 2) CVF_BIAS_NO("term[%d].n_nodes2 = %d: 0 (a 1-D table) or at least 2 nodes along cv2", i, t.n_nodes2);
      if (t.cv2 < 0 || t.cv2 >= k) CVF_BIAS_NO("term[%d].cv2 = %d: the model has CVs 0 to %d", i, t.cv2, k - 1);
      if (t.cv2 == t.cv) CVF_BIAS_NO("term[%d].cv2 = %d is the term's cv: a joint grid needs two CVs", i, t.cv2);
      if (!isfinite(t.lo2)) CVF_BIAS_NO("term[%d].lo2 is not finite", i);
      if (!(t.inv_h2 > 0.0f) || !isfinite(t.inv_h2))
        CVF_BIAS_NO("term[%d].inv_h2 = %g: the node spacing 1 / inv_h2 must be positive and finite", i, (double)t.inv_h2);
      if (t.tab_off < 0 || t.tab_off % 4 != 0)
        CVF_BIAS_NO("term[%d].tab_off = %d: a multiple of 4 >= 0 (a 2-D node holds four floats)", i, t.tab_off);
      const int64_t end = (int64_t)t.tab_off + 4 * (int64_t)t.n_nodes * (int64_t)t.n_nodes2;
      if (end > (int64_t)b->n_table) CVF_BIAS_NO("term[%d]: tab_off + 4 n_nodes n_nodes2 = %lld floats, n_table = %d", i, (long long)end, b->n_table);
      if (b->table == nullptr) CVF_BIAS_NO("term[%d] is a table and table is NULL", i);
      if (((uintptr_t)b->table & 15) != 0) CVF_BIAS_NO("table = %p is not 16-byte aligned (term[%d] is a 2-D grid)", (const void*)b->table, i);
      continue;
    }
    if (t.tab_off < 0 || t.tab_off % 2 != 0) CVF_BIAS_NO("term[%d].tab_off = %d: an even offset >= 0 (the table holds pairs)", i, t.tab_off);
    if ((int64_t)t.tab_off + 2 * (int64_t)t.n_nodes > (int64_t)b->n_table)
      CVF_BIAS_NO("term[%d]: tab_off + 2 n_nodes = %lld floats, n_table = %d", i, (long long)t.tab_off + 2 * (long long)t.n_nodes, b->n_table);
    if (b->table == nullptr) CVF_BIAS_NO("term[%d] is a table and table is NULL", i);
#undef CVF_BIAS_NO
  }
  return nullptr;
}

// ---- hill deposition (cvf_cv_bias_deposit: csrc/cv_bias_hills.hip; tools/bias2_host.cpp) ----

// the position of node j of an axis, in fp32 - what a hill's delta is measured from
CVF_BIAS_HD float cvf_bias_node_pos(float lo, float inv_h, int j) { return lo + (float)j / inv_h; }

// hills[b] = (c1, c2, w, V) of a hill on table term `t` centred on the xi row: V = the term's own U there on the table as it is,
// w = height exp(-V inv_kdt) (plain metadynamics, inv_kdt == 0: the height itself); a non-finite centre gives w = 0, and so does a
// weight that is not finite (a V so negative that the exponential overflows, a NaN in the table): such a hill is skipped.
CVF_BIAS_HD void cvf_hill_row(const cvf_bias_term& t, const float* table, const cvf_hill_desc& h, const float* xi_row, float* row) {
  const bool two_d = t.n_nodes2 != 0;
  const float c1 = xi_row[t.cv], c2 = two_d ? xi_row[t.cv2] : 0.0f;
  float v, d1, d2;
  if (two_d)
    cvf_bias_term2_eval(t, table, c1, c2, &v, &d1, &d2);
  else
    cvf_bias_term_eval(t, table, c1, &v, &d1);
  float w = h.inv_kdt == 0.0f ? h.height : h.height * expf(-v * h.inv_kdt);
  if (!(fabsf(c1) <= 3.402823466e+38f && fabsf(c2) <= 3.402823466e+38f) || !(w <= 3.402823466e+38f)) w = 0.0f;
  row[0] = c1, row[1] = c2, row[2] = w, row[3] = v;
}

// One hill's share of the node at (x1, x2), added to acc = (U, d1 U, d2 U, d12 U) (1-D: (U, U')): with delta = x - c and
// G = exp(-(delta_1^2 / sigma^2 + delta_2^2 / sigma2^2) / 2) the Gaussian w G and its exact derivatives.  A hill without a positive,
// finite height (w = 0 from cvf_hill_row, an underflown weight, a row the caller filled with NaN or infinity) adds nothing;
// 1 / sigma^2 is finite (cvf_hill_why), so a node on the centre takes w and zero slopes.
template <bool TWO_D>
CVF_BIAS_HD void cvf_hill_node_add(const cvf_hill_desc& h, const float* row, float x1, float x2, float* acc) {
  const float w = row[2];
  if (!(w > 0.0f && w <= 3.402823466e+38f)) return;
  const float delta1 = x1 - row[0], a1 = delta1 * (1.0f / (h.sigma * h.sigma));   // delta_1 / sigma^2
  if (TWO_D) {
    const float delta2 = x2 - row[1], a2 = delta2 * (1.0f / (h.sigma2 * h.sigma2));
    const float g = w * expf(-0.5f * (delta1 * a1 + delta2 * a2));
    acc[0] += g;
    acc[1] += -g * a1;
    acc[2] += -g * a2;
    acc[3] += g * (a1 * a2);
  } else {
    const float g = w * expf(-0.5f * (delta1 * a1));
    acc[0] += g;
    acc[1] += -g * a1;
  }
}

// NULL, or why `h` is no deposit into the checked bias `b` (in buf, the field named).
inline const char* cvf_hill_why(const cvf_bias_desc* b, const cvf_hill_desc* h, char* buf, size_t n_buf) {
  if (h == nullptr) return "no hill description";
#define CVF_HILL_NO(...)               \
  do {                                 \
    snprintf(buf, n_buf, __VA_ARGS__); \
    return buf;                        \
  } while (0)
  if (h->term < 0 || h->term >= b->n_terms) CVF_HILL_NO("hill.term = %d: the bias has terms 0 to %d", h->term, b->n_terms - 1);
  const cvf_bias_term& t = b->term[h->term];
  if (t.kind != CVF_BIAS_TABLE) CVF_HILL_NO("hill.term = %d is no CVF_BIAS_TABLE term (kind %d)", h->term, t.kind);
  if (!(h->height > 0.0f) || !isfinite(h->height)) CVF_HILL_NO("hill.height = %g must be positive and finite", (double)h->height);
  if (!(h->sigma > 0.0f) || !isfinite(h->sigma)) CVF_HILL_NO("hill.sigma = %g must be positive and finite", (double)h->sigma);
  if (!isfinite(1.0f / (h->sigma * h->sigma))) CVF_HILL_NO("hill.sigma = %g: 1 / sigma^2 is not finite in fp32", (double)h->sigma);
  if (t.n_nodes2 != 0 && (!(h->sigma2 > 0.0f) || !isfinite(h->sigma2)))
    CVF_HILL_NO("hill.sigma2 = %g must be positive and finite (term %d is a 2-D grid)", (double)h->sigma2, h->term);
  if (t.n_nodes2 != 0 && !isfinite(1.0f / (h->sigma2 * h->sigma2)))
    CVF_HILL_NO("hill.sigma2 = %g: 1 / sigma2^2 is not finite in fp32", (double)h->sigma2);
  if (!(h->inv_kdt >= 0.0f) || !isfinite(h->inv_kdt)) CVF_HILL_NO("hill.inv_kdt = %g must be finite and >= 0", (double)h->inv_kdt);
#undef CVF_HILL_NO
  return nullptr;
}
