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
#pragma once
#include <math.h>
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

// CV i's share of the bias: du_i = sum_{t: cv_t = i} U_t'(xi_i) and u_i = sum_{t: cv_t = i} U_t(xi_i), in term order.
CVF_BIAS_HD void cvf_bias_cv_eval(const cvf_bias_desc& b, int i, float xi, float* u, float* du) {
  float us = 0.0f, ds = 0.0f;
  for (int t = 0; t < b.n_terms; ++t) {
    if (b.term[t].cv != i) continue;
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
    if (t.tab_off < 0 || t.tab_off % 2 != 0) CVF_BIAS_NO("term[%d].tab_off = %d: an even offset >= 0 (the table holds pairs)", i, t.tab_off);
    if ((int64_t)t.tab_off + 2 * (int64_t)t.n_nodes > (int64_t)b->n_table)
      CVF_BIAS_NO("term[%d]: tab_off + 2 n_nodes = %lld floats, n_table = %d", i, (long long)t.tab_off + 2 * (long long)t.n_nodes, b->n_table);
    if (b->table == nullptr) CVF_BIAS_NO("term[%d] is a table and table is NULL", i);
#undef CVF_BIAS_NO
  }
  return nullptr;
}
