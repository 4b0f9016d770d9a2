// Second derivatives of the alignment + feature map for the Hessian-vector product h = (sum_i g_i Hess r_i(x)) u
// (csrc/k1_hvp.hip, cvf_align_feature_hvp): the derivative along u of what the VJP (csrc/k1_vjp.hip) adds to every atom.
//
// Invariant records (bond, angle, dihedral): forward-mode duals - a value and ONE tangent - that mirror bond_eval / angle_eval /
// dihedral_eval<EXACT> of cvf_features.hpp expression for expression, so the primal half of every dual is the number the VJP
// forms.  With EXACT the primal normals of a dihedral keep their error-free form and their tangents are plain cross products
// (the tangent of a rounding error is not a quantity).  The 1e-30 clamp of acos_den is taken as inactive in the tangent.
//
// Position records: the derivative along u of  Z = R [Kinv ax(R^T M)]x  and of  R g  (rigid_curvature_*), in the notation of
// the header of csrc/k1_hvp.hip.
#pragma once
#include "cvf_features.hpp"

// ------------------------------------------------------------------------------------
// duals: v + e d, e^2 = 0
// ------------------------------------------------------------------------------------
struct Du {
  float v, d;
};
__device__ __forceinline__ Du du(float v, float d = 0.0f) { return Du{v, d}; }
__device__ __forceinline__ Du operator+(Du a, Du b) { return Du{a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Du operator-(Du a, Du b) { return Du{a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Du operator-(Du a) { return Du{-a.v, -a.d}; }
__device__ __forceinline__ Du operator*(Du a, Du b) { return Du{a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Du operator/(Du a, Du b) {
  const float q = a.v / b.v;
  return Du{q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Du dsqrt(Du a) {
  const float s = sqrtf(a.v);
  return Du{s, a.d / (2.0f * s)};
}
// acos_den(cs) = sqrt(max(1 - cs^2, 1e-30)) with the tangent of sqrt(1 - cs^2)
__device__ __forceinline__ Du dacos_den(Du cs) {
  const float den = acos_den(cs.v);
  return Du{den, -cs.v * cs.d / den};
}

struct Du3 {
  V3 v, d;
};
__device__ __forceinline__ Du3 operator+(Du3 a, Du3 b) { return Du3{a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Du3 operator-(Du3 a, Du3 b) { return Du3{a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Du3 operator*(Du s, Du3 a) { return Du3{s.v * a.v, s.d * a.v + s.v * a.d}; }
__device__ __forceinline__ Du ddot(Du3 a, Du3 b) { return Du{dot(a.v, b.v), dot(a.d, b.v) + dot(a.v, b.d)}; }
__device__ __forceinline__ Du3 dcross(Du3 a, Du3 b) { return Du3{cross(a.v, b.v), cross(a.d, b.v) + cross(a.v, b.d)}; }

// ------------------------------------------------------------------------------------
// bond_eval / angle_eval / dihedral_eval<EXACT> on duals: the same scalars and gradient vectors, each with its tangent along u
// ------------------------------------------------------------------------------------
struct BondG2 {
  Du3 ga, gb;
};
__device__ __forceinline__ BondG2 bond_eval2(Du3 xa, Du3 xb) {
  const Du3 r = xb - xa;
  const Du d = dsqrt(ddot(r, r));
  const Du inv = du(1.0f) / d;
  BondG2 o;
  o.gb = inv * r;
  o.ga = (-inv) * r;
  return o;
}

struct AngleG2 {
  Du cs;
  Du3 ga, gb, gc;
};
__device__ __forceinline__ AngleG2 angle_eval2(Du3 xa, Du3 xb, Du3 xc) {
  const Du3 r1 = xa - xb, r2 = xc - xb;
  const Du l1 = dsqrt(ddot(r1, r1)), l2 = dsqrt(ddot(r2, r2));
  const Du inv12 = du(1.0f) / (l1 * l2);
  const Du cs = ddot(r1, r2) * inv12;
  AngleG2 o;
  o.cs = cs;
  o.ga = inv12 * r2 - (cs / (l1 * l1)) * r1;
  o.gc = inv12 * r1 - (cs / (l2 * l2)) * r2;
  o.gb = du(-1.0f) * (o.ga + o.gc);
  return o;
}

struct DihedralG2 {
  Du cs, sn;
  Du3 g1, g2, g3, g4;
};
template <bool EXACT = false>
__device__ __forceinline__ DihedralG2 dihedral_eval2(Du3 x1, Du3 x2, Du3 x3, Du3 x4) {
  Du3 b1, b2, b3, n1, n2;
  if constexpr (EXACT) {
    V3 e1, e2, e3;
    b1 = Du3{two_diff(x2.v, x1.v, e1), x2.d - x1.d};
    b2 = Du3{two_diff(x3.v, x2.v, e2), x3.d - x2.d};
    b3 = Du3{two_diff(x4.v, x3.v, e3), x4.d - x3.d};
    n1 = Du3{cross_exact(b1.v, b2.v) + (cross(e1, b2.v) + cross(b1.v, e2)), cross(b1.d, b2.v) + cross(b1.v, b2.d)};
    n2 = Du3{cross_exact(b2.v, b3.v) + (cross(e2, b3.v) + cross(b2.v, e3)), cross(b2.d, b3.v) + cross(b2.v, b3.d)};
  } else {
    b1 = x2 - x1, b2 = x3 - x2, b3 = x4 - x3;
    n1 = dcross(b1, b2), n2 = dcross(b2, b3);
  }
  const Du n1sq = ddot(n1, n1), n2sq = ddot(n2, n2), b2sq = ddot(b2, b2);
  const Du l2 = dsqrt(b2sq);
  const Du inv = du(1.0f) / dsqrt(n1sq * n2sq);
  DihedralG2 o;
  o.cs = ddot(n1, n2) * inv;
  o.sn = ddot(n1, b3) * l2 * inv;
  o.g1 = ((-l2) / n1sq) * n1;
  o.g4 = (l2 / n2sq) * n2;
  const Du p = ddot(b1, b2) / b2sq, q = ddot(b3, b2) / b2sq;
  o.g2 = (du(-1.0f) - p) * o.g1 + q * o.g4;
  o.g3 = p * o.g1 + (du(-1.0f) - q) * o.g4;
  return o;
}

// d/de [gs . grad_k] at x + e u of a bond, angle or dihedral record - the derivative of what invariant_vjp adds to atom k.
// at(k), ut(k): atom k and its tangent; g(j): the upstream value of output out + j; add(k, v) adds v to the row of atom k.
// gs depends on x where the output's chain rule does (an angle in value mode, a (cos, sin) dihedral) and carries its own tangent.
template <bool EXACT = false, class At, class U, class G, class Add>
__device__ __forceinline__ void invariant_hvp(int type, bool angle_value, At at, U ut, G g, Add add) {
  auto dual = [&](int k) { return Du3{at(k), ut(k)}; };
  if (type == CVF_FEAT_BOND) {
    const BondG2 e = bond_eval2(dual(0), dual(1));
    const float gs = g(0);
    add(0, gs * e.ga.d);
    add(1, gs * e.gb.d);
  } else if (type == CVF_FEAT_ANGLE) {
    const AngleG2 e = angle_eval2(dual(0), dual(1), dual(2));
    Du gs = du(g(0));
    if (angle_value) gs = (-gs) / dacos_den(e.cs);
    add(0, (gs * e.ga).d);
    add(1, (gs * e.gb).d);
    add(2, (gs * e.gc).d);
  } else {
    const DihedralG2 e = dihedral_eval2<EXACT>(dual(0), dual(1), dual(2), dual(3));
    const Du gs = angle_value ? du(g(0)) : (du(g(1)) * e.cs - du(g(0)) * e.sn);
    add(0, (gs * e.g1).d);
    add(1, (gs * e.g2).d);
    add(2, (gs * e.g3).d);
    add(3, (gs * e.g4).d);
  }
}

// ------------------------------------------------------------------------------------
// Position records.  With H = sum_b xc_b (x) ref_b, dH its tangent, M = sum_p xc_p (x) g_p and dM its tangent:
//   dR = R [Kinv ax(R^T dH)]x                         dS = dR^T H + R^T dH  (symmetric: S = R^T H is)
//   dK = tr(dS) I - dS                                s  = Kinv ax(R^T M)
//   ds = Kinv (ax(dR^T M + R^T dM) - dK s)            (= dKinv ax(R^T M) + Kinv ax(..), dKinv = -Kinv dK Kinv)
//   dZ = dR [s]x + R [ds]x
// Two steps, so that H and dH are dead before the records are visited: _rotation needs the align atoms' sums, _adjoint the
// records'.  Row-major 3x3 in 9 floats; dK symmetric in 6 (00 01 02 11 12 22), as Kinv.
// ------------------------------------------------------------------------------------
// T = A^T B
__device__ __forceinline__ void transpose_times(const float* A, const float* B, float* T) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ V3 axial(const float* T) { return v3(T[7] - T[5], T[2] - T[6], T[3] - T[1]); }
// Z (+)= A [s]x
template <bool ACC>
__device__ __forceinline__ void times_skew(const float* A, V3 s, float* Z) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float z0 = A[3 * i + 1] * s.z - A[3 * i + 2] * s.y;
    const float z1 = -A[3 * i + 0] * s.z + A[3 * i + 2] * s.x;
    const float z2 = A[3 * i + 0] * s.y - A[3 * i + 1] * s.x;
    Z[3 * i + 0] = ACC ? Z[3 * i + 0] + z0 : z0;
    Z[3 * i + 1] = ACC ? Z[3 * i + 1] + z1 : z1;
    Z[3 * i + 2] = ACC ? Z[3 * i + 2] + z2 : z2;
  }
}
__device__ __forceinline__ void rigid_curvature_rotation(const float* R, const float* Kinv, const float* H, const float* dH,
                                                         float* dR, float* dK) {
  rotation_term(R, Kinv, dH, dR);
  float A[9], C[9];
  transpose_times(dR, H, A);
  transpose_times(R, dH, C);
#pragma unroll
  for (int i = 0; i < 9; ++i) A[i] += C[i];
  const float tr = A[0] + A[4] + A[8];
  dK[0] = tr - A[0];
  dK[1] = -0.5f * (A[1] + A[3]);
  dK[2] = -0.5f * (A[2] + A[6]);
  dK[3] = tr - A[4];
  dK[4] = -0.5f * (A[5] + A[7]);
  dK[5] = tr - A[8];
}
__device__ __forceinline__ void rigid_curvature_adjoint(const float* R, const float* Kinv, const float* dR, const float* dK,
                                                        const float* M, const float* dM, float* dZ) {
  float T[9], C[9];
  transpose_times(R, M, T);
  const V3 s = sym_times(Kinv, axial(T));
  transpose_times(dR, M, T);
  transpose_times(R, dM, C);
#pragma unroll
  for (int i = 0; i < 9; ++i) T[i] += C[i];
  const V3 ds = sym_times(Kinv, axial(T) - sym_times(dK, s));
  times_skew<false>(dR, s, dZ);
  times_skew<true>(R, ds, dZ);
}
