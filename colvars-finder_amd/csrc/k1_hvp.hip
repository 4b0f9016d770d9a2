// Hessian-vector product of K1: h = d/dx <g, J(x) u> = (sum_i g_i Hess r_i(x)) u per frame (cvf_align_feature_hvp), r(x) the
// alignment + feature map, J its Jacobian.  The derivative along u of csrc/k1_vjp.hip on the same aux rows (R, centroid, Kinv of
// the forward); symmetric in u.  What a double backward through the layer needs for the coordinates.
//
// Position records (the rigid-body part), the derivative along u of the VJP's  G_a += R g_a,  G_b += Z ref_b - w_b shift:
//   H    = sum_b (x_b - c) (x) ref_b                       recomputed over the align atoms (ref_c holds w_b ref_b already)
//   ubar = (1 / n_align) sum_b w_b u_b,  dH = sum_b (u_b - ubar) (x) ref_b,  dR = R [Kinv ax(R^T dH)]x     exactly the JVP's
//   dS   = dR^T H + R^T dH   (symmetric)          dK = tr(dS) I - dS
//   M    = sum_p (x_p - c) (x) g_p                dM = sum_p (u_p - ubar) (x) g_p          over the position records p
//   s    = Kinv ax(R^T M)                         ds = Kinv (ax(dR^T M + R^T dM) - dK s)
//   dZ   = dR [s]x + R [ds]x
//   h_a += dR g_a                                          on each position record's atom
//   h_b += dZ ref_b - w_b (1 / n_align) sum_p dR g_p       on the align atoms (w_b = 1 without align_w)
// Bond / angle / dihedral records do not see the alignment: atom k of a record receives d/de [gs . grad_k] at x + e u, the
// forward-mode duals of cvf_features2.hpp (invariant_hvp).
//
// Frames of at most 192 coordinates: one lane = one frame; the 64-frame tiles of x and of u and the image of h in LDS, every sum
// sequential per lane.  Larger frames: one workgroup per frame, the align atoms and then the records over the threads, each
// (record, atom) pair writing its own contribution row, each slot summing its rows in order (the tables of csrc/k1_vjp.hip).
// No alignment (CVF_PP_FEATURES): the group decomposition of csrc/k1_features.hip.  Of x and u only the align atoms and the
// atoms some feature reads reach the arithmetic; every other atom of h is exactly 0.  No atomics: two calls give the same bits.
#include "cvf_features2.hpp"
#include "cvf_metric.hpp"

namespace {

constexpr int kLanePerFrameMaxCoord = 192;   // as cvf_align_feature_fwd / _vjp / _jvp: the aux rows are the same on every path
constexpr int kLargeThreads = 256;
constexpr int kAlignSums = 24;    // sum_b w_b u_b (3), sum_b u_b (x) ref_b (9), sum_b ref_b (3), sum_b (x_b - c) (x) ref_b (9)
constexpr int kRecordSums = 24;   // M (9), sum_p u_p (x) g_p (9), sum_p dR g_p (3), sum_p g_p (3)
constexpr size_t kLdsLimit = 160 * 1024;

// ------------------------------------------------------------------------------------
// small frames: one lane per frame.  LDS: x tile [64][stride] | u tile [64][stride] | h [64][stride] | (TABLES_LDS) rec, align_idx,
// ref_c.  The three images share the x tile's row stride: the per-lane reads and accumulation (lane = frame) and the coalesced
// copy-out (consecutive lanes = consecutive coordinates of one frame) are free of bank conflicts, as in vjp_align_kernel.
// Two passes over the records: M and dM of the position records first, then every record's own terms.
// ------------------------------------------------------------------------------------
template <bool TABLES_LDS>
__global__ __launch_bounds__(64) void hvp_align_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B,
                                                        const float* __restrict__ aux_tiled, const float* __restrict__ g_rows,
                                                        const float* __restrict__ u_rows, float* __restrict__ h_rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int nc = pp.n_coord, stride = x_tile_stride(nc);
  float* Ut = lds + CVF_TILE * stride;
  float* Ht = Ut + CVF_TILE * stride;
  load_x_tile(x, B, nc, tile, lds, lane);
  load_x_tile(u_rows, B, nc, tile, Ut, lane);
  for (int j = lane; j < CVF_TILE * stride; j += CVF_WAVE) Ht[j] = 0.0f;
  const int32_t* rec = pp.rec;
  const int32_t* al_idx = pp.align_idx;
  const float* ref = pp.ref_c;
  if (TABLES_LDS) {
    int32_t* L = reinterpret_cast<int32_t*>(Ht + CVF_TILE * stride);
    const int n1 = 6 * pp.n_rec, n2 = n1 + pp.n_align, n3 = n2 + 3 * pp.n_align;
    for (int i = lane; i < n3; i += CVF_WAVE)
      L[i] = i < n1 ? pp.rec[i] : (i < n2 ? pp.align_idx[i - n1] : reinterpret_cast<const int32_t*>(pp.ref_c)[i - n2]);
    rec = L;
    al_idx = L + n1;
    ref = reinterpret_cast<const float*>(L + n2);
  }
  __syncthreads();
  const float* my = lds + lane * stride;
  const float* mu = Ut + lane * stride;
  float* Hl = Ht + lane * stride;
  const int64_t frame = tile * CVF_TILE + lane;
  const float* gr = g_rows + (frame < B ? frame : B - 1) * pp.d_r;   // tail lanes repeat the last frame; only valid rows leave
  const float* ax = aux_tiled + tile * CVF_AUX_ROWS * CVF_TILE + lane;
  float R[9], Kinv[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const Centre c = centre_of(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
#pragma unroll
  for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
  auto addH = [&](int atm, V3 v) {
    Hl[3 * atm] += v.x;
    Hl[3 * atm + 1] += v.y;
    Hl[3 * atm + 2] += v.z;
  };
  V3 ubar = v3(0, 0, 0);
  float dR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dZ[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (pp.has_position) {
    // (weighted alignment: atom b's share of the centroid is align_w[b] / n_align, and ref_c holds align_w[b] * ref_b)
    for (int b = 0; b < pp.n_align; ++b) ubar = ubar + (pp.align_w ? pp.align_w[b] : 1.0f) * atom_xyz(mu, al_idx[b]);
    ubar = (1.0f / (float)pp.n_align) * ubar;
    float dK[6];
    {
      float H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dH[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int b = 0; b < pp.n_align; ++b) {
        const V3 rf = v3(ref[3 * b], ref[3 * b + 1], ref[3 * b + 2]);
        outer_add(H, centred(my, al_idx[b], c), rf);
        outer_add(dH, atom_xyz(mu, al_idx[b]) - ubar, rf);
      }
      rigid_curvature_rotation(R, Kinv, H, dH, dR, dK);
    }
    float M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dM[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < pp.n_rec; ++r) {
      const int32_t* p = rec + 6 * r;   // (type, atoms 0..3, out) as Rec, read field by field
      if (p[0] != CVF_FEAT_POSITION) continue;
      const V3 g = v3(gr[p[5]], gr[p[5] + 1], gr[p[5] + 2]);
      outer_add(M, centred(my, p[1], c), g);
      outer_add(dM, atom_xyz(mu, p[1]) - ubar, g);
    }
    rigid_curvature_adjoint(R, Kinv, dR, dK, M, dM, dZ);
  }
  V3 sump = v3(0, 0, 0);
  for (int r = 0; r < pp.n_rec; ++r) {
    const int32_t* p = rec + 6 * r;
    const int type = p[0], out = p[5];
    if (type == CVF_FEAT_POSITION) {
      const V3 pr = mat_times(dR, v3(gr[out], gr[out + 1], gr[out + 2]));
      addH(p[1], pr);
      sump = sump + pr;
    } else {
      invariant_hvp(type, pp.use_angle_value != 0, [&](int k) { return atom_xyz(my, p[1 + k]); },
                    [&](int k) { return atom_xyz(mu, p[1 + k]); }, [&](int j) { return gr[out + j]; },
                    [&](int k, V3 v) { addH(p[1 + k], v); });
    }
  }
  if (pp.has_position) {
    const V3 shift = (1.0f / (float)pp.n_align) * sump;
    for (int b = 0; b < pp.n_align; ++b) {
      const V3 rf = v3(ref[3 * b], ref[3 * b + 1], ref[3 * b + 2]);
      const float wb = pp.align_w ? pp.align_w[b] : 1.0f;
      addH(al_idx[b], mat_times(dZ, rf) - wb * shift);
    }
  }
  lds_barrier();
  // copy-out: the tile's valid frames are one contiguous run of h_rows
  const int64_t f0 = tile * CVF_TILE;
  const int nvalid = (int)(B - f0 < CVF_TILE ? B - f0 : CVF_TILE);
  float* dst = h_rows + f0 * nc;
  const int total = nvalid * nc, dfr = CVF_WAVE / nc, dj = CVF_WAVE - dfr * nc;
  int fr = lane / nc, j = lane - fr * nc;
  for (int e = lane; e < total; e += CVF_WAVE) {
    dst[e] = Ht[fr * stride + j];
    fr += dfr;
    j += dj;
    if (j >= nc) { j -= nc; ++fr; }
  }
}

// one entry of cvf_pp_desc.mrec: type, first output, the slots of its atoms and the contribution row of each atom
struct MRec {
  int type, out, s[4], row[4];
};
__device__ __forceinline__ MRec load_mrec(const int32_t* mrec, int r) {
  const int4 m0 = reinterpret_cast<const int4*>(mrec)[2 * r];
  const int4 m1 = reinterpret_cast<const int4*>(mrec)[2 * r + 1];
  MRec m;
  m.type = (m0.x & 7) - 1;
  m.out = (int)((unsigned)m0.x >> 3);
  m.s[0] = m0.y & 0xffff; m.s[1] = (int)((unsigned)m0.y >> 16); m.s[2] = m0.z & 0xffff; m.s[3] = (int)((unsigned)m0.z >> 16);
  const int off = m1.y;
  m.row[0] = (m0.w & 0xffff) + (off & 0xff); m.row[1] = (int)((unsigned)m0.w >> 16) + ((off >> 8) & 0xff);
  m.row[2] = (m1.x & 0xffff) + ((off >> 16) & 0xff); m.row[3] = (int)((unsigned)m1.x >> 16) + (int)((unsigned)off >> 24);
  return m;
}

// ------------------------------------------------------------------------------------
// large frames: one workgroup per frame.  LDS: the contribution rows [n_ref][3] (after phase B the first row of every slot holds
// the slot's sum) and the partial sums of the two reductions per wave.
// Phase 1, align atom b = tid, tid + 256, ...: sum_b w_b u_b, sum_b u_b (x) ref_b, sum_b ref_b (dH = sum_b u_b (x) ref_b - ubar (x)
//   sum_b ref_b, as jvp_large_kernel) and H = sum_b (x_b - c) (x) ref_b in one pass; DPP sums inside each wave, the waves in order.
// Phase A, record r = tid, tid + 256, ... of mrec: its (record, atom) rows - dR g_p of a position record, invariant_hvp of the
//   others - and M, sum_p u_p (x) g_p, sum_p g_p (dM = sum_p u_p (x) g_p - ubar (x) sum_p g_p), sum_p dR g_p.
// Phase B: slot t sums its rows in order.  Phase 2: the dense row, dZ ref_b - w_b shift on the align atoms plus the slot's sum on
//   the feature atoms, 0 elsewhere; 16-byte stores when `vec4` (n_coord % 4 == 0 and an aligned h_rows).
// WEIGHTED: per-atom alignment weights (cvf_pp_desc.align_w).
// ------------------------------------------------------------------------------------
template <bool WEIGHTED>
__global__ __launch_bounds__(kLargeThreads) void hvp_large_kernel(cvf_pp_desc pp, const float* __restrict__ x,
                                                                   const float* __restrict__ aux_tiled,
                                                                   const float* __restrict__ g_rows, const float* __restrict__ u_rows,
                                                                   float* __restrict__ h_rows, int vec4) {
  constexpr int kWaves = kLargeThreads / CVF_WAVE;
  extern __shared__ __attribute__((aligned(16))) float rows[];
  __shared__ float red1[kWaves][kAlignSums];
  __shared__ float red2[kWaves][kRecordSums];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t frame = blockIdx.x;
  const int nc = pp.n_coord;
  const float* xf = x + frame * nc;
  const float* uf = u_rows + frame * nc;
  const float* gf = g_rows + frame * pp.d_r;
  const float* ax = aux_tiled + (frame / CVF_TILE) * CVF_AUX_ROWS * CVF_TILE + (frame % CVF_TILE);
  float R[9], Kinv[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const V3 c = v3(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
#pragma unroll
  for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
  auto put = [&](int row, V3 v) {
    rows[3 * row] = v.x;
    rows[3 * row + 1] = v.y;
    rows[3 * row + 2] = v.z;
  };
  V3 ubar = v3(0, 0, 0);
  float dR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dK[6] = {0, 0, 0, 0, 0, 0};
  if (pp.has_position) {   // (uniform over the workgroup: the barrier below is taken by all threads or by none)
    // ---- phase 1
    float acc[kAlignSums];
#pragma unroll
    for (int i = 0; i < kAlignSums; ++i) acc[i] = 0.0f;
    for (int b = tid; b < pp.n_align; b += kLargeThreads) {
      const int a = pp.align_idx[b];
      const V3 u = atom_xyz(uf, a);
      const V3 rf = v3(pp.ref_c[3 * b], pp.ref_c[3 * b + 1], pp.ref_c[3 * b + 2]);
      const V3 wu = WEIGHTED ? pp.align_w[b] * u : u;
      acc[0] += wu.x; acc[1] += wu.y; acc[2] += wu.z;
      outer_add(acc + 3, u, rf);
      acc[12] += rf.x; acc[13] += rf.y; acc[14] += rf.z;
      outer_add(acc + 15, atom_xyz(xf, a) - c, rf);
    }
    // (each wave sum is stored as soon as it is formed, so that the uniform sums do not pile up in the scalar registers)
#pragma unroll
    for (int i = 0; i < kAlignSums; ++i) {
      const float v = wave_sumf(acc[i]);
      if (lane == 0) red1[wave][i] = v;
    }
    __syncthreads();
    float tot[kAlignSums];
#pragma unroll
    for (int i = 0; i < kAlignSums; ++i) {
      float v = red1[0][i];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += red1[w][i];
      tot[i] = v;
    }
    ubar = (1.0f / (float)pp.n_align) * v3(tot[0], tot[1], tot[2]);
    float dH[9];
    const float ub[3] = {ubar.x, ubar.y, ubar.z};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) dH[3 * i + j] = tot[3 + 3 * i + j] - ub[i] * tot[12 + j];
    rigid_curvature_rotation(R, Kinv, tot + 15, dH, dR, dK);
  }
  // ---- phase A: one record per thread; atom p of the record writes its row
  float acc[kRecordSums];   // M (9), sum_p u_p (x) g_p (9), sum_p dR g_p (3), sum_p g_p (3)
#pragma unroll
  for (int i = 0; i < kRecordSums; ++i) acc[i] = 0.0f;
  for (int r = tid; r < pp.n_mrec; r += kLargeThreads) {
    const MRec m = load_mrec(pp.mrec, r);
    if (m.type == CVF_FEAT_POSITION) {
      const int a = pp.slot_atom[m.s[0]];
      const V3 g = v3(gf[m.out], gf[m.out + 1], gf[m.out + 2]);
      const V3 pr = mat_times(dR, g);
      put(m.row[0], pr);
      outer_add(acc, atom_xyz(xf, a) - c, g);
      outer_add(acc + 9, atom_xyz(uf, a), g);
      acc[18] += pr.x; acc[19] += pr.y; acc[20] += pr.z;
      acc[21] += g.x; acc[22] += g.y; acc[23] += g.z;
    } else if (m.type >= 0) {
      invariant_hvp(m.type, pp.use_angle_value != 0, [&](int k) { return atom_xyz(xf, pp.slot_atom[m.s[k]]); },
                    [&](int k) { return atom_xyz(uf, pp.slot_atom[m.s[k]]); }, [&](int j) { return gf[m.out + j]; },
                    [&](int k, V3 v) { put(m.row[k], v); });
    }
  }
#pragma unroll
  for (int i = 0; i < kRecordSums; ++i) {
    const float v = wave_sumf(acc[i]);
    if (lane == 0) red2[wave][i] = v;
  }
  __syncthreads();
  // ---- phase B: slot t sums its rows slot_row[t] .. slot_row[t+1]-1 in order into its first row
  for (int t = tid; t < pp.n_slot; t += kLargeThreads) {
    const int q0 = pp.slot_row[t], q1 = pp.slot_row[t + 1];
    V3 s = v3(rows[3 * q0], rows[3 * q0 + 1], rows[3 * q0 + 2]);
    for (int q = q0 + 1; q < q1; ++q) s = s + v3(rows[3 * q], rows[3 * q + 1], rows[3 * q + 2]);
    put(q0, s);
  }
  float dZ[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  V3 shift = v3(0, 0, 0);
  if (pp.has_position) {
    float tot[kRecordSums];
#pragma unroll
    for (int i = 0; i < kRecordSums; ++i) {
      float v = red2[0][i];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += red2[w][i];
      tot[i] = v;
    }
    float dM[9];
    const float ub[3] = {ubar.x, ubar.y, ubar.z};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) dM[3 * i + j] = tot[9 + 3 * i + j] - ub[i] * tot[21 + j];
    rigid_curvature_adjoint(R, Kinv, dR, dK, tot, dM, dZ);
    shift = (1.0f / (float)pp.n_align) * v3(tot[18], tot[19], tot[20]);
  }
  __syncthreads();
  // ---- phase 2: the dense row
  auto row_of = [&](int a) {
    V3 v = v3(0, 0, 0);
    const int b = pp.atom_align[a];
    if (b >= 0) {
      const V3 zr = mat_times(dZ, v3(pp.ref_c[3 * b], pp.ref_c[3 * b + 1], pp.ref_c[3 * b + 2]));
      v = WEIGHTED ? zr - pp.align_w[b] * shift : zr - shift;
    }
    const int t = pp.atom_slot[a];
    if (t >= 0) {
      const int q = pp.slot_row[t];
      v = v + v3(rows[3 * q], rows[3 * q + 1], rows[3 * q + 2]);
    }
    return v;
  };
  float* hf = h_rows + frame * nc;
  if (vec4) {   // nc % 4 == 0 and 16-byte rows: coordinates 4v..4v+3 lie in atoms A = 4v/3 and A + 1
    for (int v = tid; v < nc / 4; v += kLargeThreads) {
      const int j0 = 4 * v, A = j0 / 3, k0 = j0 - 3 * A;
      const V3 p = row_of(A), w = row_of(A + 1);
      float4 o;
      o.x = k0 == 0 ? p.x : (k0 == 1 ? p.y : p.z);
      o.y = k0 == 0 ? p.y : (k0 == 1 ? p.z : w.x);
      o.z = k0 == 0 ? p.z : (k0 == 1 ? w.x : w.y);
      o.w = k0 == 0 ? w.x : (k0 == 1 ? w.y : w.z);
      reinterpret_cast<float4*>(hf)[v] = o;
    }
  } else {
    for (int j = tid; j < nc; j += kLargeThreads) {
      const int A = j / 3, k = j - 3 * A;
      const V3 p = row_of(A);
      hf[j] = k == 0 ? p.x : (k == 1 ? p.y : p.z);
    }
  }
}

// ------------------------------------------------------------------------------------
// no alignment (CVF_PP_FEATURES): the decomposition of csrc/k1_features.hip - a workgroup of 256 threads owns G = 1 << lg
// consecutive frames of one 64-frame tile, work items are (entry, frame) pairs with the frame fastest, every LDS image is
// [entry][G].  Step 0 copies the feature atoms of x and (U_LDS) of u through slot_atom; phase A, one (record, frame) per item,
// writes the record's contribution rows - invariant_hvp with the dihedrals' normals in their EXACT form, 0 for a position record
// (a copy has no curvature); phase B sums every slot's rows in order; then the dense rows.  Without U_LDS (a feature list at
// the limits of include/cvf.h, whose two atom images and rows exceed the LDS) the tangents are read where they lie.
// ------------------------------------------------------------------------------------
constexpr int kFeatThreads = 256;

__device__ __forceinline__ V3 img_get(const float* img, int e, int f, int G) {
  return V3{img[(3 * e) * G + f], img[(3 * e + 1) * G + f], img[(3 * e + 2) * G + f]};
}
__device__ __forceinline__ void img_put(float* img, int e, int f, int G, V3 v) {
  img[(3 * e) * G + f] = v.x;
  img[(3 * e + 1) * G + f] = v.y;
  img[(3 * e + 2) * G + f] = v.z;
}

__global__ __launch_bounds__(kFeatThreads) void features_hvp_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B, int lg,
                                                                     int u_lds, const float* __restrict__ g_rows,
                                                                     const float* __restrict__ u_rows, float* __restrict__ h_rows) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const int G = 1 << lg, per_tile = CVF_TILE >> lg;
  const int64_t f0 = (int64_t)(blockIdx.x / per_tile) * CVF_TILE + ((int)(blockIdx.x % per_tile) << lg);
  if (f0 >= B) return;
  const int nc = pp.n_coord;
  float* us = xs + 3 * (pp.n_slot << lg);
  float* rows = us + (u_lds ? 3 * (pp.n_slot << lg) : 0);
  auto frame_of = [&](int f) { return f0 + f < B ? f0 + f : B - 1; };   // frames past B: copies of the last one
  for (int e = threadIdx.x; e < (pp.n_slot << lg); e += kFeatThreads) {
    const int t = e >> lg, f = e & (G - 1), a = pp.slot_atom[t];
    img_put(xs, t, f, G, atom_xyz(x + frame_of(f) * nc, a));
    if (u_lds) img_put(us, t, f, G, atom_xyz(u_rows + frame_of(f) * nc, a));
  }
  __syncthreads();
  for (int e = threadIdx.x; e < (pp.n_mrec << lg); e += kFeatThreads) {   // phase A
    const int r = e >> lg, f = e & (G - 1);
    const MRec m = load_mrec(pp.mrec, r);
    if (m.type == CVF_FEAT_POSITION) {
      img_put(rows, m.row[0], f, G, v3(0, 0, 0));
    } else if (m.type >= 0) {
      const float* gr = g_rows + frame_of(f) * pp.d_r + m.out;
      const float* uf = u_rows + frame_of(f) * nc;
      invariant_hvp<true>(m.type, pp.use_angle_value != 0, [&](int k) { return img_get(xs, m.s[k], f, G); },
                          [&](int k) { return u_lds ? img_get(us, m.s[k], f, G) : atom_xyz(uf, pp.slot_atom[m.s[k]]); },
                          [&](int j) { return gr[j]; }, [&](int k, V3 v) { img_put(rows, m.row[k], f, G, v); });
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < (pp.n_slot << lg); e += kFeatThreads) {   // phase B: every slot sums its rows in order
    const int t = e >> lg, f = e & (G - 1);
    const int q0 = pp.slot_row[t], q1 = pp.slot_row[t + 1];
    V3 s = img_get(rows, q0, f, G);
    for (int q = q0 + 1; q < q1; ++q) s = s + img_get(rows, q, f, G);
    img_put(rows, q0, f, G, s);
  }
  __syncthreads();
  for (int f = 0; f < G && f0 + f < B; ++f) {   // the dense rows: the slot's sum on a feature atom, 0 elsewhere
    float* dst = h_rows + (f0 + f) * nc;
    for (int c = threadIdx.x; c < nc; c += kFeatThreads) {
      const int a = c / 3, t = pp.atom_slot[a];
      dst[c] = t >= 0 ? rows[(3 * pp.slot_row[t] + (c - 3 * a)) * G + f] : 0.0f;
    }
  }
}

// (P: cvf_features_deriv_plan, csrc/k1_features.hip - counts, limits, lg, u_lds)
int features_hvp_launch(const cvf_deriv_plan& P, const cvf_pp_desc* pp, const float* x, int64_t B, const float* g_rows, const float* u_rows,
                        float* h_rows, hipStream_t s) {
  const char* who = "cvf_align_feature_hvp";
  CVF_REQUIRE(pp->slot_atom, "%s: CVF_PP_FEATURES needs n_coord = 3 N, the records and the slot tables (slot_atom)", who);
  CVF_REQUIRE(pp->mrec && pp->slot_row && pp->atom_slot,
              "%s: CVF_PP_FEATURES derivatives need the contribution-row tables (atom_slot, mrec, slot_row)", who);
  CVF_REQUIRE(((uintptr_t)pp->mrec & 15) == 0, "%s: mrec must be 16-byte aligned", who);
  CVF_REQUIRE(x, "%s: CVF_PP_FEATURES needs x", who);
  if (P.lds_bytes > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)features_hvp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_bytes);
  hipLaunchKernelGGL(features_hvp_kernel, dim3((unsigned)P.grid), dim3(kFeatThreads), (size_t)P.lds_bytes, s, *pp, x, B, P.lg, P.u_lds,
                     g_rows, u_rows, h_rows);
  return cvf_check_launch("features_hvp_kernel");
}

}  // namespace

// Which kernel cvf_align_feature_hvp launches, with its LDS and grid (cvf_align_feature_deriv_route answers with it, the entry point
// launches by it): host arithmetic on the descriptor's counts and flags - no pointer of the descriptor is read but align_w, for NULL.
int cvf_hvp_plan(const cvf_pp_desc* pp, int64_t B, int out_aligned16, cvf_deriv_plan* P) {
  *P = cvf_deriv_plan{};
  CVF_REQUIRE(pp && B > 0, "cvf_align_feature_hvp: null descriptor or empty batch (B=%lld)", (long long)B);
  P->rows_per_launch = P->launches = 1;
  if (pp->mode == CVF_PP_IDENTITY) return P->family = CVF_DERIV_ROUTE_IDENTITY, 0;   // r(x) = x: the Hessian is 0, a zero fill
  CVF_REQUIRE(pp->mode != CVF_PP_FACTORED,
              "cvf_align_feature_hvp: CVF_PP_FACTORED records come from a torch module, which is differentiated by its own autograd");
  if (pp->mode == CVF_PP_FEATURES) return cvf_features_deriv_plan(pp, B, CVF_DERIV_HVP, 1, P);
  CVF_REQUIRE(pp->mode == CVF_PP_ALIGN, "unknown pp mode %d", pp->mode);
  CVF_REQUIRE(pp->n_coord % 3 == 0 && pp->n_align >= 3 && pp->d_r >= 1,
              "cvf_align_feature_hvp: malformed descriptor (n_coord=%d n_align=%d d_r=%d)", pp->n_coord, pp->n_align, pp->d_r);
  CVF_REQUIRE(!pp->align_w || pp->flags == 0 || pp->n_coord > kLanePerFrameMaxCoord,
              "cvf_align_feature_hvp: per-atom alignment weights on frames of at most %d coordinates need flags == 0",
              kLanePerFrameMaxCoord);
  P->weighted = pp->align_w != nullptr;
  if (pp->n_coord <= kLanePerFrameMaxCoord) {
    // 192 coordinates: 3 * 64 * 193 * 4 = 148 224 B of the 160 KiB; the tables join them while they still fit
    const size_t base = (size_t)3 * CVF_TILE * x_tile_stride(pp->n_coord) * sizeof(float);
    const size_t tables = ((size_t)6 * pp->n_rec + 4 * (size_t)pp->n_align) * sizeof(float);
    CVF_REQUIRE(base <= kLdsLimit, "cvf_align_feature_hvp: frames of %d coordinates do not fit the LDS", pp->n_coord);
    P->family = CVF_DERIV_ROUTE_SMALL;
    P->tables_lds = base + tables <= kLdsLimit;
    P->lds_bytes = (int64_t)(base + (P->tables_lds ? tables : 0));
    P->grid = cvf_ntiles(B);
    return 0;
  }
  CVF_REQUIRE(pp->n_slot > 0 && pp->n_ref > 0,
              "cvf_align_feature_hvp: frames of more than %d coordinates need the slot and contribution-row tables "
              "(atom_align, atom_slot, slot_atom, mrec, slot_row)", kLanePerFrameMaxCoord);
  CVF_REQUIRE(B <= 0x7fffffff, "cvf_align_feature_hvp: at most 2^31 - 1 frames per call");
  const size_t lds = (size_t)pp->n_ref * 3 * sizeof(float);
  CVF_REQUIRE(lds + sizeof(float) * (kAlignSums + kRecordSums) * (kLargeThreads / CVF_WAVE) <= kLdsLimit,
              "cvf_align_feature_hvp: %d contribution rows (atoms summed over the features) do not fit the LDS", pp->n_ref);
  P->family = CVF_DERIV_ROUTE_LARGE;
  P->vec4 = pp->n_coord % 4 == 0 && out_aligned16;
  P->lds_bytes = (int64_t)lds;
  P->grid = B;
  return 0;
}

extern "C" int cvf_align_feature_hvp(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled, const float* g_rows,
                                     const float* u_rows, float* h_rows, void* stream) {
  CVF_REQUIRE(pp && B >= 0, "cvf_align_feature_hvp: null descriptor or negative batch (B=%lld)", (long long)B);
  if (B == 0) return 0;
  CVF_REQUIRE(h_rows, "cvf_align_feature_hvp: null h_rows");
  hipStream_t s = (hipStream_t)stream;
  cvf_deriv_plan P;
  if (const int rc = cvf_hvp_plan(pp, B, ((uintptr_t)h_rows & 15) == 0, &P)) return rc;
  if (P.family == CVF_DERIV_ROUTE_IDENTITY) {
    const hipError_t e = hipMemsetAsync(h_rows, 0, (size_t)B * pp->n_coord * sizeof(float), s);
    CVF_REQUIRE(e == hipSuccess, "cvf_align_feature_hvp: identity zero fill: %s", hipGetErrorString(e));
    return 0;
  }
  CVF_REQUIRE(g_rows && u_rows, "cvf_align_feature_hvp: null g_rows or u_rows");
  if (P.family == CVF_DERIV_ROUTE_FEATURES) return features_hvp_launch(P, pp, x, B, g_rows, u_rows, h_rows, s);
  CVF_REQUIRE(x && aux_tiled, "cvf_align_feature_hvp: align mode needs x and the forward's aux rows");
  CVF_REQUIRE(pp->align_idx && pp->ref_c && pp->rec,
              "cvf_align_feature_hvp: malformed descriptor (n_coord=%d n_align=%d d_r=%d)", pp->n_coord, pp->n_align, pp->d_r);
  const size_t lds = (size_t)P.lds_bytes;
  if (P.family == CVF_DERIV_ROUTE_SMALL) {
    auto launch = [&](auto kernel) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(64), lds, s, *pp, x, B, aux_tiled, g_rows, u_rows, h_rows);
    };
    if (P.tables_lds) launch(hvp_align_kernel<true>);
    else launch(hvp_align_kernel<false>);
    return cvf_check_launch("hvp_align_kernel");
  }
  CVF_REQUIRE(pp->mrec && pp->slot_row && pp->slot_atom && pp->atom_align && pp->atom_slot,
              "cvf_align_feature_hvp: frames of more than %d coordinates need the slot and contribution-row tables "
              "(atom_align, atom_slot, slot_atom, mrec, slot_row)", kLanePerFrameMaxCoord);
  CVF_REQUIRE(((uintptr_t)pp->mrec & 15) == 0, "cvf_align_feature_hvp: mrec must be 16-byte aligned");
  auto launch = [&](auto kernel) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(kLargeThreads), lds, s, *pp, x, aux_tiled, g_rows, u_rows, h_rows, P.vec4);
  };
  if (P.weighted) launch(hvp_large_kernel<true>);
  else launch(hvp_large_kernel<false>);
  return cvf_check_launch("hvp_large_kernel");
}
