// JVP of K1: q = J(x) u per frame, J the Jacobian of the alignment + feature map r(x) (cvf_align_feature_jvp) - the transpose of
// csrc/k1_vjp.hip on the same aux rows (R, centroid, Kinv of the forward) and the same gradient code (cvf_features.hpp).
//
//   ubar = (1 / n_align) sum_b w_b u_b                     the centroid's tangent (w_b = 1 without align_w)
//   dH   = sum_b (u_b - ubar) (x) ref_b                    the covariance's tangent (ref_c holds w_b ref_b already)
//   dR   = R [Kinv ax(R^T dH)]x                            the rotation's tangent (rotation_term)
//   position record of atom a:   q = (u_a - ubar) R + (x_a - c) dR          (position_jvp)
//   bond / angle / dihedral:     q = sum_k grad_k . u_k, then the output's chain rule   (invariant_jvp)
// (this is the last pass of metric_align_kernel, csrc/k1_align.hip "JVP: q = J u", for a tangent the caller brings.)
//
// Frames of at most 192 coordinates: one lane = one frame, the 64-frame tiles of x and of u and the [64][d_r] result in LDS, every
// sum sequential per lane, the result leaves as one contiguous run.  Larger frames: one workgroup per frame; the align atoms over
// the threads for ubar and dH (per-thread sums in atom order, DPP sums inside each wave, the waves in order), then the records
// over the threads, each writing its own outputs.  Of x and u only the align atoms (align_idx) and the feature atoms (slot_atom)
// are read.  No atomics anywhere: two calls give the same bits.
#include "cvf_features.hpp"
#include "cvf_metric.hpp"

int cvf_features_jvp_launch(const cvf_pp_desc* pp, const float* x, int64_t B, const float* u_rows, float* q_rows, hipStream_t s);

namespace {

constexpr int kLanePerFrameMaxCoord = 192;   // as cvf_align_feature_fwd / _vjp: the aux rows are the same on both paths
constexpr int kLargeThreads = 256;
constexpr int kLargeSums = 15;               // sum_b w_b u_b (3), sum_b u_b (x) ref_b (9), sum_b ref_b (3)

// ------------------------------------------------------------------------------------
// small frames: one lane per frame.  LDS: x tile [64][stride] | u tile [64][stride] | (Q_LDS) q [64][d_r | 1] | (TABLES_LDS) rec,
// align_idx, ref_c.  The q image has an odd row stride: the per-lane writes (lane = frame) and the copy-out (consecutive lanes =
// consecutive outputs of one frame) are both free of bank conflicts.  Without Q_LDS (a feature list whose image does not fit)
// every lane writes its own row.
// ------------------------------------------------------------------------------------
template <bool TABLES_LDS, bool Q_LDS>
__global__ __launch_bounds__(64) void jvp_align_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B,
                                                        const float* __restrict__ aux_tiled, const float* __restrict__ u_rows,
                                                        float* __restrict__ q_rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int nc = pp.n_coord, stride = x_tile_stride(nc), dr = pp.d_r, qstride = dr | 1;
  float* Ut = lds + CVF_TILE * stride;
  float* Qt = Ut + CVF_TILE * stride;
  load_x_tile(x, B, nc, tile, lds, lane);
  load_x_tile(u_rows, B, nc, tile, Ut, lane);
  const int32_t* rec = pp.rec;
  const int32_t* al_idx = pp.align_idx;
  const float* ref = pp.ref_c;
  if (TABLES_LDS) {
    int32_t* L = reinterpret_cast<int32_t*>(Qt + (Q_LDS ? CVF_TILE * qstride : 0));
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
  const int64_t frame = tile * CVF_TILE + lane;
  const bool valid = frame < B;   // tail lanes work on a copy of the last frame; only valid rows leave
  const float* ax = aux_tiled + tile * CVF_AUX_ROWS * CVF_TILE + lane;
  float R[9], Kinv[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const Centre c = centre_of(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
#pragma unroll
  for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
  V3 ubar = v3(0, 0, 0);
  float dR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (pp.has_position) {
    // (weighted alignment: atom b's share of the centroid is align_w[b] / n_align, and ref_c holds align_w[b] * ref_b)
    for (int b = 0; b < pp.n_align; ++b) ubar = ubar + (pp.align_w ? pp.align_w[b] : 1.0f) * atom_xyz(mu, al_idx[b]);
    ubar = (1.0f / (float)pp.n_align) * ubar;
    float dH[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < pp.n_align; ++b)
      outer_add(dH, atom_xyz(mu, al_idx[b]) - ubar, v3(ref[3 * b], ref[3 * b + 1], ref[3 * b + 2]));
    rotation_term(R, Kinv, dH, dR);
  }
  float* Ql = Q_LDS ? Qt + lane * qstride : q_rows + (valid ? frame : 0) * dr;
  auto put = [&](int o, float v) {
    if (Q_LDS || valid) Ql[o] = v;
  };
  for (int r = 0; r < pp.n_rec; ++r) {
    const Rec rc = load_rec(rec, r);
    if (rc.type == CVF_FEAT_POSITION) {
      const V3 qa = position_jvp(R, dR, atom_xyz(mu, rc.a[0]) - ubar, centred(my, rc.a[0], c));
      put(rc.out, qa.x);
      put(rc.out + 1, qa.y);
      put(rc.out + 2, qa.z);
    } else {
      invariant_jvp(rc.type, pp.use_angle_value, [&](int k) { return atom_xyz(my, rc.a[k]); },
                    [&](int k) { return atom_xyz(mu, rc.a[k]); }, [&](int j, float v) { put(rc.out + j, v); });
    }
  }
  if (!Q_LDS) return;
  lds_barrier();
  // copy-out: the tile's valid frames are one contiguous run of q_rows
  const int64_t f0 = tile * CVF_TILE;
  const int nvalid = (int)(B - f0 < CVF_TILE ? B - f0 : CVF_TILE);
  float* dst = q_rows + f0 * dr;
  const int total = nvalid * dr, dfr = CVF_WAVE / dr, dj = CVF_WAVE - dfr * dr;
  int fr = lane / dr, j = lane - fr * dr;
  for (int e = lane; e < total; e += CVF_WAVE) {
    dst[e] = Qt[fr * qstride + j];
    fr += dfr;
    j += dj;
    if (j >= dr) { j -= dr; ++fr; }
  }
}

// ------------------------------------------------------------------------------------
// large frames: one workgroup per frame.  LDS: kLargeSums partial sums per wave.
// Phase 1, align atom b = tid, tid + 256, ...: sum_b w_b u_b, sum_b u_b (x) ref_b and sum_b ref_b in one pass over the align atoms of
// u (dH = sum_b u_b (x) ref_b - ubar (x) sum_b ref_b; the stored ref_c sums to zero up to its own rounding, which this keeps).
// Phase 2, record r = tid, tid + 256, ... of mrec: the record's atoms of x and u through slot_atom, its outputs to q_rows (the
// records lie sorted by type with their outputs in list order: neighbouring threads write neighbouring outputs).
// WEIGHTED: per-atom alignment weights (cvf_pp_desc.align_w) in the centroid's tangent.
// ------------------------------------------------------------------------------------
template <bool WEIGHTED>
__global__ __launch_bounds__(kLargeThreads) void jvp_large_kernel(cvf_pp_desc pp, const float* __restrict__ x,
                                                                   const float* __restrict__ aux_tiled,
                                                                   const float* __restrict__ u_rows, float* __restrict__ q_rows) {
  constexpr int kWaves = kLargeThreads / CVF_WAVE;
  __shared__ float red[kWaves][kLargeSums + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t frame = blockIdx.x;
  const int nc = pp.n_coord;
  const float* xf = x + frame * nc;
  const float* uf = u_rows + frame * nc;
  float* qf = q_rows + frame * pp.d_r;
  const float* ax = aux_tiled + (frame / CVF_TILE) * CVF_AUX_ROWS * CVF_TILE + (frame % CVF_TILE);
  float R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const V3 c = v3(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
  V3 ubar = v3(0, 0, 0);
  float dR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (pp.has_position) {   // (uniform over the workgroup: the barrier below is taken by all threads or by none)
    float acc[kLargeSums];
#pragma unroll
    for (int i = 0; i < kLargeSums; ++i) acc[i] = 0.0f;
    for (int b = tid; b < pp.n_align; b += kLargeThreads) {
      const V3 u = atom_xyz(uf, pp.align_idx[b]);
      const V3 rf = v3(pp.ref_c[3 * b], pp.ref_c[3 * b + 1], pp.ref_c[3 * b + 2]);
      const V3 wu = WEIGHTED ? pp.align_w[b] * u : u;
      acc[0] += wu.x; acc[1] += wu.y; acc[2] += wu.z;
      outer_add(acc + 3, u, rf);
      acc[12] += rf.x; acc[13] += rf.y; acc[14] += rf.z;
    }
    // over the workgroup: DPP sums inside each wave, then the waves in order (fixed order: reproducible).  Each wave sum is
    // stored as soon as it is formed, so that the uniform sums do not pile up in the scalar registers.
#pragma unroll
    for (int i = 0; i < kLargeSums; ++i) {
      const float v = wave_sumf(acc[i]);
      if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    float tot[kLargeSums];
#pragma unroll
    for (int i = 0; i < kLargeSums; ++i) {
      float v = red[0][i];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += red[w][i];
      tot[i] = v;
    }
    ubar = (1.0f / (float)pp.n_align) * v3(tot[0], tot[1], tot[2]);
    float dH[9], Kinv[6];
    const float ub[3] = {ubar.x, ubar.y, ubar.z};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) dH[3 * i + j] = tot[3 + 3 * i + j] - ub[i] * tot[12 + j];
#pragma unroll
    for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
    rotation_term(R, Kinv, dH, dR);
  }
  for (int r = tid; r < pp.n_mrec; r += kLargeThreads) {
    const int4 m0 = reinterpret_cast<const int4*>(pp.mrec)[2 * r];   // (type + 1) | out << 3, the slots of the four atoms
    const int type = (m0.x & 7) - 1, out = (int)((unsigned)m0.x >> 3);
    const int s[4] = {m0.y & 0xffff, (int)((unsigned)m0.y >> 16), m0.z & 0xffff, (int)((unsigned)m0.z >> 16)};
    if (type == CVF_FEAT_POSITION) {
      const int a = pp.slot_atom[s[0]];
      const V3 qa = position_jvp(R, dR, atom_xyz(uf, a) - ubar, atom_xyz(xf, a) - c);
      qf[out] = qa.x;
      qf[out + 1] = qa.y;
      qf[out + 2] = qa.z;
    } else if (type >= 0) {
      invariant_jvp(type, pp.use_angle_value, [&](int k) { return atom_xyz(xf, pp.slot_atom[s[k]]); },
                    [&](int k) { return atom_xyz(uf, pp.slot_atom[s[k]]); }, [&](int j, float v) { qf[out + j] = v; });
    }
  }
}

}  // namespace

// Which kernel cvf_align_feature_jvp launches, with its LDS and grid (cvf_align_feature_deriv_route answers with it, the entry point
// launches by it): host arithmetic on the descriptor's counts and flags - no pointer of the descriptor is read but align_w, for NULL.
int cvf_jvp_plan(const cvf_pp_desc* pp, int64_t B, cvf_deriv_plan* P) {
  *P = cvf_deriv_plan{};
  CVF_REQUIRE(pp && B > 0, "cvf_align_feature_jvp: null descriptor or empty batch (B=%lld)", (long long)B);
  P->rows_per_launch = P->launches = 1;
  if (pp->mode == CVF_PP_IDENTITY) {
    CVF_REQUIRE(pp->d_r == pp->n_coord, "identity preprocessing needs d_r == n_coord");
    return P->family = CVF_DERIV_ROUTE_IDENTITY, 0;
  }
  if (pp->mode == CVF_PP_FEATURES) return cvf_features_deriv_plan(pp, B, CVF_DERIV_JVP, 1, P);   // (csrc/k1_features.hip)
  CVF_REQUIRE(pp->mode != CVF_PP_FACTORED,
              "cvf_align_feature_jvp: CVF_PP_FACTORED records come from a torch module, which is differentiated by its own autograd");
  CVF_REQUIRE(pp->mode == CVF_PP_ALIGN, "unknown pp mode %d", pp->mode);
  CVF_REQUIRE(pp->n_coord % 3 == 0 && pp->n_align >= 3 && pp->d_r >= 1,
              "cvf_align_feature_jvp: malformed descriptor (n_coord=%d n_align=%d d_r=%d)", pp->n_coord, pp->n_align, pp->d_r);
  CVF_REQUIRE(!pp->align_w || pp->flags == 0 || pp->n_coord > kLanePerFrameMaxCoord,
              "cvf_align_feature_jvp: per-atom alignment weights on frames of at most %d coordinates need flags == 0",
              kLanePerFrameMaxCoord);
  P->weighted = pp->align_w != nullptr;
  if (pp->n_coord <= kLanePerFrameMaxCoord) {
    const size_t tiles = (size_t)2 * CVF_TILE * x_tile_stride(pp->n_coord) * sizeof(float);
    const size_t qimg = (size_t)CVF_TILE * (pp->d_r | 1) * sizeof(float);
    const size_t tables = ((size_t)6 * pp->n_rec + 4 * (size_t)pp->n_align) * sizeof(float);
    const size_t limit = 160 * 1024;
    P->family = CVF_DERIV_ROUTE_SMALL;
    P->q_lds = tiles + qimg <= limit;
    P->tables_lds = P->q_lds && tiles + qimg + tables <= limit;
    P->lds_bytes = (int64_t)(tiles + (P->q_lds ? qimg : 0) + (P->tables_lds ? tables : 0));
    P->grid = cvf_ntiles(B);
    return 0;
  }
  CVF_REQUIRE(pp->n_mrec > 0 && pp->n_slot > 0,
              "cvf_align_feature_jvp: frames of more than %d coordinates need the slot tables (slot_atom, mrec)",
              kLanePerFrameMaxCoord);
  CVF_REQUIRE(B <= 0x7fffffff, "cvf_align_feature_jvp: at most 2^31 - 1 frames per call");
  P->family = CVF_DERIV_ROUTE_LARGE;
  P->grid = B;
  return 0;
}

extern "C" int cvf_align_feature_jvp(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled,
                                     const float* u_rows, float* q_rows, void* stream) {
  CVF_REQUIRE(pp && B >= 0, "cvf_align_feature_jvp: null descriptor or negative batch (B=%lld)", (long long)B);
  if (B == 0) return 0;
  CVF_REQUIRE(u_rows && q_rows, "cvf_align_feature_jvp: null u_rows or q_rows");
  hipStream_t s = (hipStream_t)stream;
  cvf_deriv_plan P;
  if (const int rc = cvf_jvp_plan(pp, B, &P)) return rc;
  if (P.family == CVF_DERIV_ROUTE_IDENTITY) {
    const hipError_t e = hipMemcpyAsync(q_rows, u_rows, (size_t)B * pp->n_coord * sizeof(float), hipMemcpyDeviceToDevice, s);
    CVF_REQUIRE(e == hipSuccess, "cvf_align_feature_jvp: identity copy: %s", hipGetErrorString(e));
    return 0;
  }
  if (P.family == CVF_DERIV_ROUTE_FEATURES) return cvf_features_jvp_launch(pp, x, B, u_rows, q_rows, s);   // (csrc/k1_features.hip, by the same plan)
  CVF_REQUIRE(x && aux_tiled, "cvf_align_feature_jvp: align mode needs x and the forward's aux rows");
  CVF_REQUIRE(pp->align_idx && pp->ref_c && pp->rec,
              "cvf_align_feature_jvp: malformed descriptor (n_coord=%d n_align=%d d_r=%d)", pp->n_coord, pp->n_align, pp->d_r);
  if (P.family == CVF_DERIV_ROUTE_SMALL) {
    const size_t lds = (size_t)P.lds_bytes;
    auto launch = [&](auto kernel) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(64), lds, s, *pp, x, B, aux_tiled, u_rows, q_rows);
    };
    if (P.tables_lds) launch(jvp_align_kernel<true, true>);
    else if (P.q_lds) launch(jvp_align_kernel<false, true>);
    else launch(jvp_align_kernel<false, false>);
    return cvf_check_launch("jvp_align_kernel");
  }
  CVF_REQUIRE(pp->mrec && pp->slot_atom,
              "cvf_align_feature_jvp: frames of more than %d coordinates need the slot tables (slot_atom, mrec)",
              kLanePerFrameMaxCoord);
  CVF_REQUIRE(((uintptr_t)pp->mrec & 15) == 0, "cvf_align_feature_jvp: mrec must be 16-byte aligned");
  if (P.weighted) hipLaunchKernelGGL(jvp_large_kernel<true>, dim3((unsigned)P.grid), dim3(kLargeThreads), 0, s, *pp, x, aux_tiled, u_rows, q_rows);
  else hipLaunchKernelGGL(jvp_large_kernel<false>, dim3((unsigned)P.grid), dim3(kLargeThreads), 0, s, *pp, x, aux_tiled, u_rows, q_rows);
  return cvf_check_launch("jvp_large_kernel");
}
