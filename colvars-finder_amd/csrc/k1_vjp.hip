// VJP of K1: gx = J(x)^T g per frame, J the Jacobian of the alignment + feature map r(x) (cvf_align_feature_vjp).
// The rotation, centroid and Kinv come from the forward's aux rows; nothing is recomputed but the features' own gradients.
//
//   G_a = s_a + d_a,   s_a = sum over the records that read atom a of (their gradient vectors) x (their upstream rows)
//                      d_b = Z ref_b - w_b shift  on the align atoms   (Z = R [Kinv ax(R^T M)]x, shift = sum_p / n_align,
//                                                                       M = sum_p xc_p (x) g_p, sum_p = sum_p R g_p over the
//                                                                       position records p; 0 without position records)
// (the derivation: csrc/metric_large.hip, header; csrc/k1_align.hip, metric_align_kernel - pass 1 of that kernel is the first
// kernel below for one upstream row instead of k nets).
//
// Frames of at most 192 coordinates: one lane = one frame, the 64-frame tile of x, the tables and the gradient image G in LDS,
// every sum sequential per lane.  Larger frames: one workgroup per frame, the records over the threads; each (record, atom)
// pair writes its own contribution row (the mrec / slot_row tables of cvf_pp_desc), each slot sums its rows in order, the dense
// row of 3N floats leaves in 16-byte stores.  No atomics anywhere: two calls give the same bits.
#include "cvf_features.hpp"
#include "cvf_metric.hpp"

int cvf_features_vjp_launch(const cvf_pp_desc* pp, const float* x, int64_t B, int k, const float* g_rows, float* gx_rows, hipStream_t s);

namespace {

constexpr int kLanePerFrameMaxCoord = 192;   // as cvf_align_feature_fwd (k1_align.hip): aux rows are the same on both paths
constexpr int kLargeThreads = 256;

// ------------------------------------------------------------------------------------
// small frames: one lane per frame.  LDS: x tile [64][stride] | G [64][stride] | (TABLES_LDS) rec, align_idx, ref_c.
// G shares the x tile's odd row stride: the per-lane accumulation (lane = frame) and the coalesced copy-out (consecutive lanes
// = consecutive coordinates of one frame) are both free of bank conflicts.
// ------------------------------------------------------------------------------------
template <bool TABLES_LDS>
__global__ __launch_bounds__(64) void vjp_align_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B,
                                                        const float* __restrict__ aux_tiled, const float* __restrict__ g_rows,
                                                        float* __restrict__ gx_rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int nc = pp.n_coord, stride = x_tile_stride(nc);
  load_x_tile(x, B, nc, tile, lds, lane);
  float* Gt = lds + CVF_TILE * stride;
  for (int j = lane; j < CVF_TILE * stride; j += CVF_WAVE) Gt[j] = 0.0f;
  const int32_t* rec = pp.rec;
  const int32_t* al_idx = pp.align_idx;
  const float* ref = pp.ref_c;
  if (TABLES_LDS) {
    int32_t* L = reinterpret_cast<int32_t*>(Gt + CVF_TILE * stride);
    const int n1 = 6 * pp.n_rec, n2 = n1 + pp.n_align, n3 = n2 + 3 * pp.n_align;
    for (int i = lane; i < n3; i += CVF_WAVE)
      L[i] = i < n1 ? pp.rec[i] : (i < n2 ? pp.align_idx[i - n1] : reinterpret_cast<const int32_t*>(pp.ref_c)[i - n2]);
    rec = L;
    al_idx = L + n1;
    ref = reinterpret_cast<const float*>(L + n2);
  }
  __syncthreads();
  const float* my = lds + lane * stride;
  float* Gl = Gt + lane * stride;
  const int64_t frame = tile * CVF_TILE + lane;
  const float* gr = g_rows + (frame < B ? frame : B - 1) * pp.d_r;   // tail lanes repeat the last frame; only valid rows leave
  const float* ax = aux_tiled + tile * CVF_AUX_ROWS * CVF_TILE + lane;
  float R[9], Kinv[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const Centre c = centre_of(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
#pragma unroll
  for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
  auto addG = [&](int atm, V3 v) {
    Gl[3 * atm] += v.x;
    Gl[3 * atm + 1] += v.y;
    Gl[3 * atm + 2] += v.z;
  };
  V3 sump = v3(0, 0, 0);
  float M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = 0; r < pp.n_rec; ++r) {
    const int32_t* p = rec + 6 * r;   // (type, atoms 0..3, out) as Rec, read field by field
    const int type = p[0], out = p[5];
    if (type == CVF_FEAT_POSITION) {
      const V3 g = v3(gr[out], gr[out + 1], gr[out + 2]);
      const V3 pr = mat_times(R, g);
      addG(p[1], pr);
      sump = sump + pr;
      outer_add(M, centred(my, p[1], c), g);
    } else {
      invariant_vjp(type, pp.use_angle_value, 1, [&](int k) { return atom_xyz(my, p[1 + k]); },
                    [&](int, int j) { return gr[out + j]; }, [&](int, int k, V3 v) { addG(p[1 + k], v); });
    }
  }
  if (pp.has_position) {
    float Z[9];
    rotation_term(R, Kinv, M, Z);
    // (weighted alignment: atom b's share of the centroid is align_w[b] / n_align, and ref_c holds align_w[b] * ref_b)
    const V3 shift = (1.0f / (float)pp.n_align) * sump;
    for (int b = 0; b < pp.n_align; ++b) {
      const V3 rf = v3(ref[3 * b], ref[3 * b + 1], ref[3 * b + 2]);
      const float wb = pp.align_w ? pp.align_w[b] : 1.0f;
      addG(al_idx[b], mat_times(Z, rf) - wb * shift);
    }
  }
  lds_barrier();
  // copy-out: the tile's valid frames are one contiguous run of gx_rows
  const int64_t f0 = tile * CVF_TILE;
  const int nvalid = (int)(B - f0 < CVF_TILE ? B - f0 : CVF_TILE);
  float* dst = gx_rows + f0 * nc;
  const int total = nvalid * nc, dfr = CVF_WAVE / nc, dj = CVF_WAVE - dfr * nc;
  int fr = lane / nc, j = lane - fr * nc;
  for (int e = lane; e < total; e += CVF_WAVE) {
    dst[e] = Gt[fr * stride + j];
    fr += dfr;
    j += dj;
    if (j >= nc) { j -= nc; ++fr; }
  }
}

// ------------------------------------------------------------------------------------
// large frames: one workgroup per frame.  LDS: the contribution rows [n_ref][3] (after phase B the first row of every slot
// holds the slot's sum s_t) and 12 partial sums per wave.
// ------------------------------------------------------------------------------------
// (vjp_large_kernel and vjp_rows_large_kernel - the k-cotangent form described further down - live in k1_vjp_large.hpp, which is
//  included once per weighting: uniform, and per-atom weights d_b = Z ref_b - w_b shift)
#define CVF_VJP_LARGE_KERNEL vjp_large_kernel
#define CVF_VJP_ROWS_LARGE_KERNEL vjp_rows_large_kernel
#define CVF_VJP_WEIGHTED false
#include "k1_vjp_large.hpp"
#undef CVF_VJP_LARGE_KERNEL
#undef CVF_VJP_ROWS_LARGE_KERNEL
#undef CVF_VJP_WEIGHTED
#define CVF_VJP_LARGE_KERNEL vjp_weighted_large_kernel
#define CVF_VJP_ROWS_LARGE_KERNEL vjp_rows_weighted_large_kernel
#define CVF_VJP_WEIGHTED true
#include "k1_vjp_large.hpp"
#undef CVF_VJP_LARGE_KERNEL
#undef CVF_VJP_ROWS_LARGE_KERNEL
#undef CVF_VJP_WEIGHTED
}  // namespace

// Which kernel cvf_align_feature_vjp (which = CVF_DERIV_VJP) or cvf_align_feature_vjp_rows (CVF_DERIV_VJP_ROWS, k cotangents) launches,
// with its LDS, grid and row grouping (cvf_align_feature_deriv_route answers with it, the two entry points launch by it): host arithmetic
// on the descriptor's counts and flags - no pointer of the descriptor is read but align_w, for NULL.
int cvf_vjp_plan(const cvf_pp_desc* pp, int64_t B, int which, int k, int out_aligned16, cvf_deriv_plan* P) {
  *P = cvf_deriv_plan{};
  const bool rows = which == CVF_DERIV_VJP_ROWS;
  const char* who = rows ? "cvf_align_feature_vjp_rows" : "cvf_align_feature_vjp";
  if (!rows) k = 1;
  CVF_REQUIRE(pp && B > 0 && k >= 1 && k <= CVF_MAX_NETS, "%s: null argument, empty batch or k outside 1..%d (B=%lld k=%d)", who,
              CVF_MAX_NETS, (long long)B, k);
  P->rows_per_launch = P->launches = 1;
  if (pp->mode == CVF_PP_IDENTITY) {
    CVF_REQUIRE(pp->d_r == pp->n_coord, "identity preprocessing needs d_r == n_coord");
    return P->family = CVF_DERIV_ROUTE_IDENTITY, P->rows_per_launch = k, 0;
  }
  if (pp->mode == CVF_PP_FEATURES) return cvf_features_deriv_plan(pp, B, which, k, P);   // (csrc/k1_features.hip)
  CVF_REQUIRE(pp->mode != CVF_PP_FACTORED,
              "%s: CVF_PP_FACTORED records come from a torch module, which is differentiated by its own autograd", who);
  CVF_REQUIRE(pp->mode == CVF_PP_ALIGN, "unknown pp mode %d", pp->mode);
  CVF_REQUIRE(pp->n_coord % 3 == 0 && pp->n_align >= 3, "%s: malformed descriptor (n_coord=%d n_align=%d)", who, pp->n_coord, pp->n_align);
  CVF_REQUIRE(!pp->align_w || pp->flags == 0 || pp->n_coord > kLanePerFrameMaxCoord,
              "%s: per-atom alignment weights on frames of at most %d coordinates need flags == 0", who, kLanePerFrameMaxCoord);
  P->weighted = pp->align_w != nullptr;
  const size_t limit = 160 * 1024;
  if (pp->n_coord <= kLanePerFrameMaxCoord) {
    const size_t img = (size_t)CVF_TILE * x_tile_stride(pp->n_coord) * sizeof(float);
    const size_t tables = ((size_t)6 * pp->n_rec + 4 * (size_t)pp->n_align) * sizeof(float);
    P->family = CVF_DERIV_ROUTE_SMALL;
    P->grid = cvf_ntiles(B);
    if (!rows) {   // the x tile and one gradient image; the tables join them while they fit
      P->tables_lds = 2 * img + tables <= limit;
      P->lds_bytes = (int64_t)(2 * img + (P->tables_lds ? tables : 0));
      return 0;
    }
    // images per pass: as many rows as keep the LDS within 40 KB (four workgroups per CU, as the single-cotangent kernel
    // at config 3 - one row per pass there), at least one
    const size_t per_row = img + (size_t)12 * CVF_TILE * sizeof(float);
    const size_t budget = 40 * 1024;
    P->tables_lds = img + per_row + tables <= limit;
    const size_t fixed = img + (P->tables_lds ? tables : 0);
    int kg = fixed + per_row * k <= budget ? k : (int)((budget > fixed + per_row ? budget - fixed : per_row) / per_row);
    kg = kg < 1 ? 1 : kg;
    const size_t lds = fixed + per_row * kg;
    CVF_REQUIRE(lds <= limit, "%s: frames of %d coordinates do not fit the LDS", who, pp->n_coord);
    P->rows_per_launch = kg;
    P->lds_bytes = (int64_t)lds;
    return 0;
  }
  CVF_REQUIRE(pp->n_slot > 0 && pp->n_ref > 0,
              "%s: frames of more than %d coordinates need the slot and contribution-row tables "
              "(atom_align, atom_slot, slot_atom, mrec, slot_row)", who, kLanePerFrameMaxCoord);
  CVF_REQUIRE(B <= 0x7fffffff, "%s: at most 2^31 - 1 frames per call", who);
  P->family = CVF_DERIV_ROUTE_LARGE;
  P->vec4 = pp->n_coord % 4 == 0 && out_aligned16;
  P->grid = B;
  if (!rows) {
    const size_t lds = (size_t)pp->n_ref * 3 * sizeof(float);
    CVF_REQUIRE(lds + sizeof(float) * 12 * (kLargeThreads / CVF_WAVE) <= limit,
                "%s: %d contribution rows (atoms summed over the features) do not fit the LDS", who, pp->n_ref);
    P->lds_bytes = (int64_t)lds;
    return 0;
  }
  // one launch per group of kg rows whose contribution rows share 64 KB (at config 5 all k rows fit one launch)
  const size_t per_row = ((size_t)pp->n_ref * 3 + (size_t)12 * (kLargeThreads / CVF_WAVE) + 12) * sizeof(float);
  CVF_REQUIRE(per_row <= limit, "%s: %d contribution rows (atoms summed over the features) do not fit the LDS", who, pp->n_ref);
  const size_t budget = 64 * 1024;
  int kg = per_row * k <= budget ? k : (int)(budget / per_row);
  kg = kg < 1 ? 1 : kg;
  P->rows_per_launch = kg;
  P->launches = (k + kg - 1) / kg;
  P->lds_bytes = (int64_t)(per_row * kg);
  return 0;
}

extern "C" int cvf_align_feature_deriv_route(const cvf_pp_desc* pp, int64_t B, int which, int k, int out_aligned16, cvf_deriv_plan* plan) {
  CVF_REQUIRE(plan, "cvf_align_feature_deriv_route: null plan");
  switch (which) {
    case CVF_DERIV_VJP:
    case CVF_DERIV_VJP_ROWS: return cvf_vjp_plan(pp, B, which, k, out_aligned16 != 0, plan);
    case CVF_DERIV_JVP: return cvf_jvp_plan(pp, B, plan);
    case CVF_DERIV_HVP: return cvf_hvp_plan(pp, B, out_aligned16 != 0, plan);
    case CVF_DERIV_FEATURES_FWD:
    case CVF_DERIV_FEATURES_METRIC:
      *plan = cvf_deriv_plan{};
      CVF_REQUIRE(pp && B > 0, "cvf_align_feature_deriv_route: null descriptor or empty batch (B=%lld)", (long long)B);
      CVF_REQUIRE(pp->mode == CVF_PP_FEATURES, "cvf_align_feature_deriv_route: call %d is answered for CVF_PP_FEATURES only "
                  "(cvf_align_feature_route and cvf_metric_route answer for the other modes)", which);
      return cvf_features_deriv_plan(pp, B, which, k, plan);
    default: break;
  }
  *plan = cvf_deriv_plan{};
  CVF_REQUIRE(false, "cvf_align_feature_deriv_route: unknown call %d", which);
}

extern "C" int cvf_align_feature_vjp(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled,
                                     const float* g_rows, float* gx_rows, void* stream) {
  CVF_REQUIRE(pp && g_rows && gx_rows && B > 0, "cvf_align_feature_vjp: null argument or empty batch (B=%lld)", (long long)B);
  hipStream_t s = (hipStream_t)stream;
  cvf_deriv_plan P;
  if (const int rc = cvf_vjp_plan(pp, B, CVF_DERIV_VJP, 1, ((uintptr_t)gx_rows & 15) == 0, &P)) return rc;
  if (P.family == CVF_DERIV_ROUTE_IDENTITY) {
    const hipError_t e = hipMemcpyAsync(gx_rows, g_rows, (size_t)B * pp->n_coord * sizeof(float), hipMemcpyDeviceToDevice, s);
    CVF_REQUIRE(e == hipSuccess, "cvf_align_feature_vjp: identity copy: %s", hipGetErrorString(e));
    return 0;
  }
  if (P.family == CVF_DERIV_ROUTE_FEATURES) return cvf_features_vjp_launch(pp, x, B, 1, g_rows, gx_rows, s);   // (csrc/k1_features.hip, by the same plan)
  CVF_REQUIRE(x && aux_tiled, "cvf_align_feature_vjp: align mode needs x and the forward's aux rows");
  CVF_REQUIRE(pp->align_idx && pp->ref_c && pp->rec, "cvf_align_feature_vjp: malformed descriptor (n_coord=%d n_align=%d)", pp->n_coord,
              pp->n_align);
  const size_t lds = (size_t)P.lds_bytes;
  if (P.family == CVF_DERIV_ROUTE_SMALL) {
    auto launch = [&](auto kernel) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(64), lds, s, *pp, x, B, aux_tiled, g_rows, gx_rows);
    };
    if (P.tables_lds) launch(vjp_align_kernel<true>);
    else launch(vjp_align_kernel<false>);
    return cvf_check_launch("vjp_align_kernel");
  }
  CVF_REQUIRE(pp->mrec && pp->slot_row && pp->slot_atom && pp->atom_align && pp->atom_slot,
              "cvf_align_feature_vjp: frames of more than %d coordinates need the slot and contribution-row tables "
              "(atom_align, atom_slot, slot_atom, mrec, slot_row)", kLanePerFrameMaxCoord);
  CVF_REQUIRE(((uintptr_t)pp->mrec & 15) == 0, "cvf_align_feature_vjp: mrec must be 16-byte aligned");
  auto launch = [&](auto kernel) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(kLargeThreads), lds, s, *pp, x, aux_tiled, g_rows, gx_rows);
  };
  if (P.weighted) {
    if (P.vec4) launch(vjp_weighted_large_kernel<true>);
    else launch(vjp_weighted_large_kernel<false>);
  } else {
    if (P.vec4) launch(vjp_large_kernel<true>);
    else launch(vjp_large_kernel<false>);
  }
  return cvf_check_launch("vjp_large_kernel");
}

// ====================================================================================
// k cotangents per frame in one launch (cvf_align_feature_vjp_rows): gx_rows[b][i] = J(x_b)^T g_rows[b][i], i < k.
// The per-frame work is shared by the rows: the x tile / gathers, the tables, the aux rows (R, centroid, Kinv) and every
// record's geometry (the gradient vectors of bond_eval / angle_eval / dihedral_eval) are taken once per frame and group of
// rows; only the products with the cotangents are per row.  Row i sums in the single-cotangent kernels' order (records in
// order into the gradient image, M and sum_p over the position records in order, the workgroup sums in wave order, every
// slot's rows in order), so it equals cvf_align_feature_vjp on g_rows[:, i] bit for bit.  No atomics.
// ====================================================================================
namespace {

// small frames: one lane per frame, as vjp_align_kernel, with `kg` gradient images side by side.
// LDS: x tile [64][stride] | G [kg][64][stride] | acc [kg][12][64] (M, sum_p of each row and lane) | (TABLES_LDS) tables.
template <bool TABLES_LDS>
__global__ __launch_bounds__(64) void vjp_rows_small_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B,
                                                             const float* __restrict__ aux_tiled, int k, int kg,
                                                             const float* __restrict__ g_rows, float* __restrict__ gx_rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int nc = pp.n_coord, stride = x_tile_stride(nc), img = CVF_TILE * stride;
  load_x_tile(x, B, nc, tile, lds, lane);
  float* Gt = lds + img;
  float* acc = Gt + kg * img;
  const int32_t* rec = pp.rec;
  const int32_t* al_idx = pp.align_idx;
  const float* ref = pp.ref_c;
  if (TABLES_LDS) {
    int32_t* L = reinterpret_cast<int32_t*>(acc + kg * 12 * CVF_TILE);
    const int n1 = 6 * pp.n_rec, n2 = n1 + pp.n_align, n3 = n2 + 3 * pp.n_align;
    for (int i = lane; i < n3; i += CVF_WAVE)
      L[i] = i < n1 ? pp.rec[i] : (i < n2 ? pp.align_idx[i - n1] : reinterpret_cast<const int32_t*>(pp.ref_c)[i - n2]);
    rec = L;
    al_idx = L + n1;
    ref = reinterpret_cast<const float*>(L + n2);
  }
  __syncthreads();
  const float* my = lds + lane * stride;
  const int64_t frame = tile * CVF_TILE + lane;
  const float* gf = g_rows + (frame < B ? frame : B - 1) * (int64_t)k * pp.d_r;   // tail lanes repeat the last frame
  const float* ax = aux_tiled + tile * CVF_AUX_ROWS * CVF_TILE + lane;
  float R[9], Kinv[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const Centre c = centre_of(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
#pragma unroll
  for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
  const int64_t f0 = tile * CVF_TILE;
  const int nvalid = (int)(B - f0 < CVF_TILE ? B - f0 : CVF_TILE);
  for (int i0 = 0; i0 < k; i0 += kg) {
    const int ng = k - i0 < kg ? k - i0 : kg;
    for (int j = 0; j < ng * stride; ++j) Gt[(j / stride) * img + lane * stride + (j % stride)] = 0.0f;   // this lane's rows
    for (int j = 0; j < ng * 12; ++j) acc[j * CVF_TILE + lane] = 0.0f;
    auto addG = [&](int ii, int atm, V3 v) {
      float* Gl = Gt + ii * img + lane * stride;
      Gl[3 * atm] += v.x;
      Gl[3 * atm + 1] += v.y;
      Gl[3 * atm + 2] += v.z;
    };
    for (int r = 0; r < pp.n_rec; ++r) {
      const Rec rc = load_rec(rec, r);
      if (rc.type == CVF_FEAT_POSITION) {
        const V3 xc = centred(my, rc.a[0], c);
        for (int ii = 0; ii < ng; ++ii) {
          const float* gr = gf + (i0 + ii) * pp.d_r;
          const V3 g = v3(gr[rc.out], gr[rc.out + 1], gr[rc.out + 2]);
          const V3 pr = mat_times(R, g);
          addG(ii, rc.a[0], pr);
          float* A = acc + ii * 12 * CVF_TILE + lane;
          outer_add<CVF_TILE>(A, xc, g);
          A[9 * CVF_TILE] = A[9 * CVF_TILE] + pr.x;
          A[10 * CVF_TILE] = A[10 * CVF_TILE] + pr.y;
          A[11 * CVF_TILE] = A[11 * CVF_TILE] + pr.z;
        }
      } else {
        invariant_vjp(rc.type, pp.use_angle_value, ng, [&](int k) { return atom_xyz(my, rc.a[k]); },
                      [&](int ii, int j) { return gf[(i0 + ii) * pp.d_r + rc.out + j]; },
                      [&](int ii, int k, V3 v) { addG(ii, rc.a[k], v); });
      }
    }
    if (pp.has_position) {
      for (int ii = 0; ii < ng; ++ii) {
        const float* A = acc + ii * 12 * CVF_TILE + lane;
        float M[9], Z[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) M[j] = A[j * CVF_TILE];
        rotation_term(R, Kinv, M, Z);
        const V3 shift = (1.0f / (float)pp.n_align) * v3(A[9 * CVF_TILE], A[10 * CVF_TILE], A[11 * CVF_TILE]);
        for (int b = 0; b < pp.n_align; ++b) {
          const V3 rf = v3(ref[3 * b], ref[3 * b + 1], ref[3 * b + 2]);
          const float wb = pp.align_w ? pp.align_w[b] : 1.0f;
          addG(ii, al_idx[b], mat_times(Z, rf) - wb * shift);
        }
      }
    }
    lds_barrier();
    // copy-out: rows i0 .. i0+ng-1 of a frame are one contiguous run of ng * nc floats in gx_rows [B][k][nc]
    const int run = ng * nc, total = nvalid * run;
    for (int e = lane; e < total; e += CVF_WAVE) {
      const int fr = e / run, rem = e - fr * run, ii = rem / nc, j = rem - ii * nc;
      gx_rows[((f0 + fr) * k + i0) * nc + rem] = Gt[ii * img + fr * stride + j];
    }
    lds_barrier();   // (the next group zeroes the images this copy-out reads)
  }
}

// large frames: one workgroup per frame, as vjp_large_kernel, for rows i0 .. i0+ng-1 of the k, their contribution rows side
// by side.  LDS: rows [ng][n_ref * 3] | red [ng][4][12] | zs [ng][12] (Z, shift of each row).  (k1_vjp_large.hpp)
// M = G Q^T per frame: m[b][i][j] = sum_r g[b][i][r] q[b][j][r] for i <= j, r in order, mirrored below the diagonal.
// One lane per frame; every (i, j) sum lives in a register while g and q stream through once (coalesced tiled rows).
template <int K>
__global__ __launch_bounds__(64) void metric_gram_kernel(int64_t B, int d_r, const float* __restrict__ g_tiled,
                                                          const float* __restrict__ q_tiled, float* __restrict__ m_rows) {
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x, frame = tile * CVF_TILE + lane;
  const float* g = g_tiled + tile * K * d_r * CVF_TILE + lane;
  const float* q = q_tiled + tile * K * d_r * CVF_TILE + lane;
  float s[K * (K + 1) / 2];
#pragma unroll
  for (int p = 0; p < K * (K + 1) / 2; ++p) s[p] = 0.0f;
  for (int r = 0; r < d_r; ++r) {
    float gv[K], qv[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      gv[i] = g[(i * d_r + r) * CVF_TILE];
      qv[i] = q[(i * d_r + r) * CVF_TILE];
    }
    int p = 0;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = i; j < K; ++j) s[p++] += gv[i] * qv[j];
  }
  if (frame >= B) return;
  float* m = m_rows + frame * K * K;
  int p = 0;
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = i; j < K; ++j) {
      m[i * K + j] = s[p];
      m[j * K + i] = s[p];
      ++p;
    }
}

}  // namespace

extern "C" int cvf_align_feature_vjp_rows(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled, int k,
                                          const float* g_rows, float* gx_rows, void* stream) {
  CVF_REQUIRE(pp && g_rows && gx_rows && B > 0 && k >= 1 && k <= CVF_MAX_NETS,
              "cvf_align_feature_vjp_rows: null argument, empty batch or k outside 1..%d (B=%lld k=%d)", CVF_MAX_NETS,
              (long long)B, k);
  hipStream_t s = (hipStream_t)stream;
  cvf_deriv_plan P;
  if (const int rc = cvf_vjp_plan(pp, B, CVF_DERIV_VJP_ROWS, k, ((uintptr_t)gx_rows & 15) == 0, &P)) return rc;
  if (P.family == CVF_DERIV_ROUTE_IDENTITY) {
    const hipError_t e = hipMemcpyAsync(gx_rows, g_rows, (size_t)B * k * pp->n_coord * sizeof(float), hipMemcpyDeviceToDevice, s);
    CVF_REQUIRE(e == hipSuccess, "cvf_align_feature_vjp_rows: identity copy: %s", hipGetErrorString(e));
    return 0;
  }
  if (P.family == CVF_DERIV_ROUTE_FEATURES) return cvf_features_vjp_launch(pp, x, B, k, g_rows, gx_rows, s);   // (csrc/k1_features.hip, by the same plan)
  CVF_REQUIRE(x && aux_tiled, "cvf_align_feature_vjp_rows: align mode needs x and the forward's aux rows");
  CVF_REQUIRE(pp->align_idx && pp->ref_c && pp->rec, "cvf_align_feature_vjp_rows: malformed descriptor (n_coord=%d n_align=%d)",
              pp->n_coord, pp->n_align);
  const int kg = P.rows_per_launch;
  if (P.family == CVF_DERIV_ROUTE_SMALL) {
    const size_t lds = (size_t)P.lds_bytes;
    auto launch = [&](auto kernel) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(64), lds, s, *pp, x, B, aux_tiled, k, kg, g_rows, gx_rows);
    };
    if (P.tables_lds) launch(vjp_rows_small_kernel<true>);
    else launch(vjp_rows_small_kernel<false>);
    return cvf_check_launch("vjp_rows_small_kernel");
  }
  CVF_REQUIRE(pp->mrec && pp->slot_row && pp->slot_atom && pp->atom_align && pp->atom_slot,
              "cvf_align_feature_vjp_rows: frames of more than %d coordinates need the slot and contribution-row tables "
              "(atom_align, atom_slot, slot_atom, mrec, slot_row)", kLanePerFrameMaxCoord);
  CVF_REQUIRE(((uintptr_t)pp->mrec & 15) == 0, "cvf_align_feature_vjp_rows: mrec must be 16-byte aligned");
  const size_t per_row = (size_t)P.lds_bytes / kg;
  for (int i0 = 0; i0 < k; i0 += kg) {   // P.launches launches, one per group of kg rows
    const int ng = k - i0 < kg ? k - i0 : kg;
    const size_t lds = per_row * ng;
    auto launch = [&](auto kernel) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(kLargeThreads), lds, s, *pp, x, aux_tiled, k, i0, ng, g_rows, gx_rows);
    };
    if (P.weighted) {
      if (P.vec4) launch(vjp_rows_weighted_large_kernel<true>);
      else launch(vjp_rows_weighted_large_kernel<false>);
    } else {
      if (P.vec4) launch(vjp_rows_large_kernel<true>);
      else launch(vjp_rows_large_kernel<false>);
    }
    const int rc = cvf_check_launch("vjp_rows_large_kernel");
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" int cvf_metric_gram(int k, int64_t B, int d_r, const float* g_tiled, const float* q_tiled, float* m_rows,
                               void* stream) {
  CVF_REQUIRE(g_tiled && q_tiled && m_rows && B > 0 && d_r > 0 && k >= 1 && k <= CVF_MAX_NETS,
              "cvf_metric_gram: bad argument (B=%lld k=%d d_r=%d)", (long long)B, k, d_r);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cvf_ntiles(B)), block(64);
  switch (k) {
    case 1: hipLaunchKernelGGL(metric_gram_kernel<1>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
    case 2: hipLaunchKernelGGL(metric_gram_kernel<2>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
    case 3: hipLaunchKernelGGL(metric_gram_kernel<3>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
    case 4: hipLaunchKernelGGL(metric_gram_kernel<4>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
    case 5: hipLaunchKernelGGL(metric_gram_kernel<5>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
    case 6: hipLaunchKernelGGL(metric_gram_kernel<6>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
    case 7: hipLaunchKernelGGL(metric_gram_kernel<7>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
    default: hipLaunchKernelGGL(metric_gram_kernel<8>, grid, block, 0, s, B, d_r, g_tiled, q_tiled, m_rows); break;
  }
  return cvf_check_launch("metric_gram_kernel");
}
