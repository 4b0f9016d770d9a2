// The feature map of the alignment layer and its chain rule, written once for every kernel that evaluates it:
// values (k1_align.hip, k1_large.hip, k1_features.hip), J^T g (k1_align.hip, k1_vjp.hip, metric_large.hip, k1_features.hip) and
// J u (k1_align.hip, metric_large.hip, k1_features.hip).  What differs between the kernels comes in as callables: where atom k of a record is read from (an LDS
// tile, HBM, a captured slot), where the upstream value of output out + j is read from, and where a value or an atom's
// gradient row goes.  Everything is __forceinline__: each kernel keeps its own layout, registers and arithmetic.
#pragma once
#include "cvf_common.hpp"

// The launch plans of the derivative entry points (cvf_align_feature_deriv_route, include/cvf.h): each file plans its own kernels -
// csrc/k1_vjp.hip (vjp, vjp_rows), k1_jvp.hip, k1_hvp.hip, and k1_features.hip for every CVF_PP_FEATURES launch.
int cvf_vjp_plan(const cvf_pp_desc* pp, int64_t B, int which, int k, int out_aligned16, cvf_deriv_plan* P);
int cvf_jvp_plan(const cvf_pp_desc* pp, int64_t B, cvf_deriv_plan* P);
int cvf_hvp_plan(const cvf_pp_desc* pp, int64_t B, int out_aligned16, cvf_deriv_plan* P);
int cvf_features_deriv_plan(const cvf_pp_desc* pp, int64_t B, int which, int k, cvf_deriv_plan* P);

// One entry of cvf_pp_desc.rec / rec_slot (include/cvf.h): type, four atoms (or slots), first output.
struct Rec {
  int type, a[4], out;
};
__device__ __forceinline__ Rec load_rec(const int32_t* rec, int r) {
  const int32_t* p = rec + 6 * r;
  return Rec{p[0], {p[1], p[2], p[3], p[4]}, p[5]};
}
// atom a of a frame stored as [atom][3] floats
__device__ __forceinline__ V3 atom_xyz(const float* x, int a) { return V3{x[3 * a], x[3 * a + 1], x[3 * a + 2]}; }

// ------------------------------------------------------------------------------------
// Invariant features on raw coordinates.  The gradient vectors are those of the *scalar* each evaluation returns
// (bond length, cos of the angle, dihedral angle phi); the outputs' chain rule is applied by the functions further down.
// ------------------------------------------------------------------------------------
struct BondG {
  float val;
  V3 ga, gb;
};
__device__ __forceinline__ BondG bond_eval(V3 xa, V3 xb) {
  V3 r = xb - xa;
  float d = sqrtf(dot(r, r));
  float inv = 1.0f / d;
  BondG o;
  o.val = d;
  o.gb = inv * r;
  o.ga = (-inv) * r;
  return o;
}

struct AngleG {
  float cs;  // cos of the angle at b
  float sn;  // sin of the angle, from |r1 x r2|: no cancellation where the angle is nearly straight (1 - cs^2 loses its digits there)
  V3 ga, gb, gc;  // gradient of cos
};
__device__ __forceinline__ AngleG angle_eval(V3 xa, V3 xb, V3 xc) {
  V3 r1 = xa - xb, r2 = xc - xb;
  float l1 = sqrtf(dot(r1, r1)), l2 = sqrtf(dot(r2, r2));
  float inv12 = 1.0f / (l1 * l2);
  float cs = dot(r1, r2) * inv12;
  AngleG o;
  o.cs = cs;
  const V3 n = cross(r1, r2);
  o.sn = sqrtf(dot(n, n)) * inv12;
  o.ga = inv12 * r2 - (cs / (l1 * l1)) * r1;
  o.gc = inv12 * r1 - (cs / (l2 * l2)) * r2;
  o.gb = (-1.0f) * (o.ga + o.gc);
  return o;
}

struct DihedralG {
  float cs, sn;
  V3 g1, g2, g3, g4;  // gradient of phi
  float p, q;         // g2 = (-1 - p) g1 + q g4,  g3 = p g1 + (-1 - q) g4
};
// The two normals n1 = b1 x b2, n2 = b2 x b3 are where a dihedral loses digits in fp32: when two bonds are close to parallel
// (kappa = |b||b'| / |b x b'| large) the rounding of the differences b = x' - x and of the products of the cross product is
// amplified kappa times, in the values and - divided by |n|^2 - in the gradient.  EXACT evaluates the normals as if the
// differences and the products were exact: the rounding error of every difference is recovered (two_diff), every component
// a b - c d is taken with the fma error-free product (Kahan), and the first-order terms e x b' + b x e' are added.  Everything
// downstream of the normals is as before (no amplification there).  Off by default: the kernels that predate it keep their bits.
__device__ __forceinline__ float two_diff(float a, float b, float& err) {   // a - b = s + err exactly
  const float s = a - b;
  const float bb = s - a;
  err = (a - (s - bb)) - (b + bb);
  return s;
}
__device__ __forceinline__ V3 two_diff(V3 a, V3 b, V3& err) {
  return V3{two_diff(a.x, b.x, err.x), two_diff(a.y, b.y, err.y), two_diff(a.z, b.z, err.z)};
}
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {   // a b - c d, one rounding of the result
  const float w = c * d;
  const float e = fmaf(-c, d, w);
  const float f = fmaf(a, b, -w);
  return f + e;
}
__device__ __forceinline__ V3 cross_exact(V3 a, V3 b) {
  return V3{diff_of_products(a.y, b.z, a.z, b.y), diff_of_products(a.z, b.x, a.x, b.z), diff_of_products(a.x, b.y, a.y, b.x)};
}
template <bool EXACT = false>
__device__ __forceinline__ DihedralG dihedral_eval(V3 x1, V3 x2, V3 x3, V3 x4) {
  V3 b1, b2, b3, n1, n2;
  if constexpr (EXACT) {
    V3 e1, e2, e3;
    b1 = two_diff(x2, x1, e1);
    b2 = two_diff(x3, x2, e2);
    b3 = two_diff(x4, x3, e3);
    n1 = cross_exact(b1, b2) + (cross(e1, b2) + cross(b1, e2));
    n2 = cross_exact(b2, b3) + (cross(e2, b3) + cross(b2, e3));
  } else {
    b1 = x2 - x1, b2 = x3 - x2, b3 = x4 - x3;
    n1 = cross(b1, b2), n2 = cross(b2, b3);
  }
  float n1sq = dot(n1, n1), n2sq = dot(n2, n2), b2sq = dot(b2, b2);
  float l2 = sqrtf(b2sq);
  float inv = 1.0f / sqrtf(n1sq * n2sq);
  DihedralG o;
  o.cs = dot(n1, n2) * inv;
  o.sn = dot(n1, b3) * l2 * inv;
  o.g1 = (-l2 / n1sq) * n1;
  o.g4 = (l2 / n2sq) * n2;
  float p = dot(b1, b2) / b2sq, q = dot(b3, b2) / b2sq;
  o.g2 = (-1.0f - p) * o.g1 + q * o.g4;
  o.g3 = p * o.g1 + (-1.0f - q) * o.g4;
  o.p = p;
  o.q = q;
  return o;
}

// ------------------------------------------------------------------------------------
// The outputs' chain rule.  An angle record emits cos or, with use_angle_value, the angle: d acos(cs) = -d cs / acos_den(cs).
// A dihedral record emits (cos phi, sin phi) or, with use_angle_value, phi: d cos = -sin dphi, d sin = cos dphi.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ float acos_den(float cs) { return sqrtf(fmaxf(1.0f - cs * cs, 1e-30f)); }
// ... of an evaluated angle: its sine as angle_eval formed it (the same clamp)
__device__ __forceinline__ float acos_den(const AngleG& e) { return fmaxf(e.sn, 1e-15f); }
// the adjoint of phi from the upstream values g(j) of the record's outputs (g(1) is read only when it exists)
template <class G>
__device__ __forceinline__ float dihedral_adjoint(bool angle_value, float cs, float sn, G g) {
  return angle_value ? g(0) : (g(1) * cs - g(0) * sn);
}
// the tangent of the record's outputs from dphi: put(j, v) writes output out + j
template <class Put>
__device__ __forceinline__ void dihedral_tangent(bool angle_value, float cs, float sn, float dphi, Put put) {
  if (angle_value) {
    put(0, dphi);
  } else {
    put(0, -sn * dphi);
    put(1, cs * dphi);
  }
}

// In the three functions below the record is a bond, an angle or a dihedral (the callers take positions and padding apart),
// and at(k) returns its atom k (k < 4).

// Values of a bond, angle or dihedral record: emit(j, v) writes output out + j.
template <bool EXACT = false, class At, class Emit>
__device__ __forceinline__ void invariant_values(int type, bool angle_value, At at, Emit emit) {
  if (type == CVF_FEAT_BOND) {
    emit(0, bond_eval(at(0), at(1)).val);
  } else if (type == CVF_FEAT_ANGLE) {
    const float cs = angle_eval(at(0), at(1), at(2)).cs;
    emit(0, angle_value ? acosf(cs) : cs);
  } else {
    const DihedralG dg = dihedral_eval<EXACT>(at(0), at(1), at(2), at(3));
    if (angle_value) {
      emit(0, atan2f(dg.sn, dg.cs));
    } else {
      emit(0, dg.cs);
      emit(1, dg.sn);
    }
  }
}

// J^T g of a bond, angle or dihedral record for n upstream rows that share the record's geometry: g(i, j) is row i's
// upstream value of output out + j, add(i, k, v) adds v to the gradient of atom k in row i.
template <bool EXACT = false, class At, class G, class Add>
__device__ __forceinline__ void invariant_vjp(int type, bool angle_value, int n, At at, G g, Add add) {
  if (type == CVF_FEAT_BOND) {
    const BondG e = bond_eval(at(0), at(1));
    for (int i = 0; i < n; ++i) {
      const float gs = g(i, 0);
      add(i, 0, gs * e.ga);
      add(i, 1, gs * e.gb);
    }
  } else if (type == CVF_FEAT_ANGLE) {
    const AngleG e = angle_eval(at(0), at(1), at(2));
    for (int i = 0; i < n; ++i) {
      float gs = g(i, 0);
      if (angle_value) gs = -gs / acos_den(e);
      add(i, 0, gs * e.ga);
      add(i, 1, gs * e.gb);
      add(i, 2, gs * e.gc);
    }
  } else {
    const DihedralG e = dihedral_eval<EXACT>(at(0), at(1), at(2), at(3));
    for (int i = 0; i < n; ++i) {
      const float gs = dihedral_adjoint(angle_value, e.cs, e.sn, [&](int j) { return g(i, j); });
      add(i, 0, gs * e.g1);
      add(i, 1, gs * e.g2);
      add(i, 2, gs * e.g3);
      add(i, 3, gs * e.g4);
    }
  }
}

// J u of a bond, angle or dihedral record: u(k) is the tangent of atom k, put(j, v) writes output out + j.
template <bool EXACT = false, class At, class U, class Put>
__device__ __forceinline__ void invariant_jvp(int type, bool angle_value, At at, U u, Put put) {
  if (type == CVF_FEAT_BOND) {
    const BondG e = bond_eval(at(0), at(1));
    put(0, dot(e.ga, u(0)) + dot(e.gb, u(1)));
  } else if (type == CVF_FEAT_ANGLE) {
    const AngleG e = angle_eval(at(0), at(1), at(2));
    float dv = dot(e.ga, u(0)) + dot(e.gb, u(1)) + dot(e.gc, u(2));
    if (angle_value) dv = -dv / acos_den(e);
    put(0, dv);
  } else {
    const DihedralG e = dihedral_eval<EXACT>(at(0), at(1), at(2), at(3));
    const float dphi = dot(e.g1, u(0)) + dot(e.g2, u(1)) + dot(e.g3, u(2)) + dot(e.g4, u(3));
    dihedral_tangent(angle_value, e.cs, e.sn, dphi, put);
  }
}

// ------------------------------------------------------------------------------------
// Position records: output = xc R, xc = x - c (row vector).  Their J^T g is R g on the atom plus, through the rotation
// and the centroid, terms on the align atoms that need M = sum_p xc_p (x) g_p; their J u is (u - ubar) R + xc dR.
// ------------------------------------------------------------------------------------
// M += a (x) b, row-major 3x3 with entry (i, j) at M[S * (3 i + j)]
template <int S = 1>
__device__ __forceinline__ void outer_add(float* M, V3 a, V3 b) {
  M[0 * S] += a.x * b.x; M[1 * S] += a.x * b.y; M[2 * S] += a.x * b.z;
  M[3 * S] += a.y * b.x; M[4 * S] += a.y * b.y; M[5 * S] += a.y * b.z;
  M[6 * S] += a.z * b.x; M[7 * S] += a.z * b.y; M[8 * S] += a.z * b.z;
}
// Z = R [Kinv ax(R^T M)]x   ([s]x rows: (0,-sz,sy), (sz,0,-sx), (-sy,sx,0)).  With M = sum_p xc_p (x) g_p this is the
// rotation's adjoint (J^T g: G_b += Z ref_b on the align atoms); with M = dH, the tangent of the covariance, it is the
// rotation's tangent dR (J u).
__device__ __forceinline__ void rotation_term(const float* R, const float* Kinv, const float* M, float* Z) {
  float T[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[3 * i + j] = R[i] * M[j] + R[3 + i] * M[3 + j] + R[6 + i] * M[6 + j];
  const V3 s = sym_times(Kinv, v3(T[7] - T[5], T[2] - T[6], T[3] - T[1]));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Z[3 * i + 0] = R[3 * i + 1] * s.z - R[3 * i + 2] * s.y;
    Z[3 * i + 1] = -R[3 * i + 0] * s.z + R[3 * i + 2] * s.x;
    Z[3 * i + 2] = R[3 * i + 0] * s.y - R[3 * i + 1] * s.x;
  }
}
// J u of a position record: du = u - ubar of its atom, xc its centred coordinates
__device__ __forceinline__ V3 position_jvp(const float* R, const float* dR, V3 du, V3 xc) {
  return row_times(du, R) + row_times(xc, dR);
}
