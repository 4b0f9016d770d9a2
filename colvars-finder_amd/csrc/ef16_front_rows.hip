// The generator-mode front launch of the 16-frames-per-wave step for a RESIDENT batch (see ef16_front.hip for the step itself).
//
// The alignment record of a frame (rotation, centroid, K^-1: kAuxP floats) depends on the frame's coordinates and the layer's
// reference only - not on the parameters.  A training loop that replays the same static batches every epoch
// (EigenFunctionTask.train(): shuffle=False) therefore re-derives, in every epoch after the first, records it already had.
// The same holds for the features - aligned positions, ef16_feature() of the coordinates and the record - which the front
// kernel rebuilt in LDS on every visit and copied out as the backward kernel's feature tile (264 bytes per frame at d_r = 66).
//   cvf_ef16_align_rows      : the records of a batch, once -> `rows` (cvf_ef16_align_rows_floats(B) floats).  One wave per unit of
//                              16 frames running ef16_align_unit, the code wave 0 of the solving front kernel runs: same bits.
//   cvf_ef16_align_rows_tile : the same launch also writes the batch's feature tile, [tile][feature][64] with the padding of
//                              cvf_ef16_front (every unit of 4 * cvf_ntiles(B), frames past B as replicas of the last one).
//   cvf_ef16_front_rows      : cvf_ef16_front starting from those rows AND that tile - ef16_front_kernel<.., ROWS = true>: no
//                              covariance, no 3x3 solve (the kernel's fp64), no feature phase, no tile store, one barrier
//                              instead of three; everything else is the same code, so the outputs are bit for bit those of
//                              cvf_ef16_front on the same frames.
// A translation unit of its own: the 192 ROWS instances compile beside the 208 of ef16_front.hip.
#include "ef16_front_kernel.hpp"

namespace {
// block = one wave = one unit.  Stages the unit's coordinates and the reference exactly as the front kernel does (frames past
// B as load_x_tile pads them), solves, and copies the unit's records out of LDS as 16-byte pieces.  feat_tiled != NULL: the
// unit's 16 columns of the feature tile as well - lane p of frame f takes the atoms p, p + 4, ..
__global__ __launch_bounds__(64) void ef16_align_rows_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B, int64_t units,
                                                            float* __restrict__ rows, float* __restrict__ feat_tiled) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = (int)threadIdx.x, lane = tid;
  const int64_t unit = blockIdx.x;
  const int nc = pp.n_coord, nal = pp.n_align;
  const int stride = x_tile_stride(nc);
  float* xt = lds;
  float* refL = lds + kU * stride;
  float* auxL = refL + ((3 * nal + 3) & ~3);
  float* rsL = auxL + kRowsUnit;
  if (stride == nc && (unit + 1) * kU <= B && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    const float4* src = reinterpret_cast<const float4*>(x + unit * (int64_t)(kU * nc));
    float4* dst = reinterpret_cast<float4*>(xt);
    const int n4 = (kU * nc) >> 2;
    for (int v = tid; v < n4; v += 64) dst[v] = src[v];
  } else {
    load_x_tile<6>(x, B, nc, unit, xt, tid, 64, kU);
  }
  for (int j = tid; j < 3 * nal; j += 64) refL[j] = pp.ref_c[j];
  __syncthreads();
  ef16_align_unit<false>(xt + (lane >> 2) * stride, refL, nal, lane, auxL, rsL);
  __syncthreads();
  float4* dst = reinterpret_cast<float4*>(rows + unit * (int64_t)kRowsUnit);
  const float4* src = reinterpret_cast<const float4*>(auxL);
  for (int v = tid; v < kRowsUnit / 4; v += 64) dst[v] = src[v];
  // (the sum of the reference is the same in every unit: the first one leaves it behind the last unit's records)
  if (unit == 0 && tid < 4) rows[units * (int64_t)kRowsUnit + tid] = tid < 3 ? rsL[tid] : 0.0f;
  if (feat_tiled == nullptr) return;   // (uniform)
  const int f = lane >> 2, p = lane & 3, N = pp.n_rec;
  const float* my = xt + f * stride;
  float R[9];
  const float* ar = auxL + f * kAuxP;
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ar[i];
  Centre c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    c.hi[i] = ar[9 + i];
    c.lo[i] = ar[18 + i];
  }
  float* ft = feat_tiled + (unit >> 2) * (int64_t)(3 * N) * CVF_TILE + kU * (int)(unit & 3) + f;
  for (int at = p; at < N; at += 4) {
    const V3 al = ef16_feature(my, at, c, R);
    ft[(3 * at) * CVF_TILE] = al.x;
    ft[(3 * at + 1) * CVF_TILE] = al.y;
    ft[(3 * at + 2) * CVF_TILE] = al.z;
  }
}
}  // namespace

extern "C" int64_t cvf_ef16_align_rows_floats(int64_t B) { return B > 0 ? 4 * cvf_ntiles(B) * kRowsUnit + 4 : 0; }

static int ef16_align_rows_go(const cvf_pp_desc* pp, const float* x, int64_t B, float* rows, float* feat_tiled, void* stream) {
  CVF_REQUIRE(pp && pp->mode == CVF_PP_ALIGN && !pp->align_w && pp->n_align >= 3 && pp->n_align <= pp->n_rec &&
              3 * pp->n_align <= pp->n_coord && pp->n_coord <= 192,
              "cvf_ef16_align_rows: layer not covered (the fast layout of cvf_ef16_supported())");
  CVF_REQUIRE(x && rows && B > 0, "cvf_ef16_align_rows: bad argument");
  CVF_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "cvf_ef16_align_rows: rows must be 16-byte aligned");
  const int64_t units = 4 * cvf_ntiles(B);
  CVF_REQUIRE(units < (int64_t)1 << 31, "cvf_ef16_align_rows: batch too large for one launch");
  const size_t lds = ((size_t)kU * x_tile_stride(pp->n_coord) + ((3 * pp->n_align + 3) & ~3) + kRowsUnit + 4) * sizeof(float);
  hipLaunchKernelGGL(ef16_align_rows_kernel, dim3((unsigned)units), dim3(64), lds, (hipStream_t)stream, *pp, x, B, units, rows,
                     feat_tiled);
  return cvf_check_launch("ef16_align_rows_kernel");
}

extern "C" int cvf_ef16_align_rows(const cvf_pp_desc* pp, const float* x, int64_t B, float* rows, void* stream) {
  return ef16_align_rows_go(pp, x, B, rows, nullptr, stream);
}

extern "C" int cvf_ef16_align_rows_tile(const cvf_pp_desc* pp, const float* x, int64_t B, float* rows, float* feat_tiled, void* stream) {
  CVF_REQUIRE(feat_tiled, "cvf_ef16_align_rows_tile: feat_tiled missing");
  CVF_REQUIRE(pp && pp->n_rec >= 1 && pp->d_r == 3 * pp->n_rec && 3 * pp->n_rec <= pp->n_coord,
              "cvf_ef16_align_rows_tile: the features must be the positions of the first n_rec atoms (cvf_ef16_supported())");
  return ef16_align_rows_go(pp, x, B, rows, feat_tiled, stream);
}

extern "C" int cvf_ef16_front_rows(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                   const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, float* y_tiled, float* saved,
                                   float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg, const float* w, double* scratch,
                                   double* stats, double* loss_vec, double* coef, const float* rows, void* stream) {
  CVF_REQUIRE(rows && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
              "cvf_ef16_front_rows: rows (cvf_ef16_align_rows_tile of this batch) missing or not 16-byte aligned");
  return ef16_front_go<true>("cvf_ef16_front_rows", mlp, theta, packed, feat_tiled, pp, x, B, a, y_tiled, saved, q_tiled, e_tiled, cfg, w,
                             scratch, stats, loss_vec, coef, rows, stream);
}

// ... with an isotropic metric (see cvf_ef16_front_iso): bit for bit the outputs of cvf_ef16_front_iso on the same frames.  The
// head of the block requests no coordinates: the passes read the features, which the waves copy from layer 0's operand into LDS.
extern "C" int cvf_ef16_front_rows_iso(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                       const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, float* y_tiled, float* saved,
                                       float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg, const float* w, double* scratch,
                                       double* stats, double* loss_vec, double* coef, const float* rows, void* stream) {
  CVF_REQUIRE(rows && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
              "cvf_ef16_front_rows_iso: rows (cvf_ef16_align_rows_tile of this batch) missing or not 16-byte aligned");
  return ef16_front_go<true>("cvf_ef16_front_rows_iso", mlp, theta, packed, feat_tiled, pp, x, B, a, y_tiled, saved, q_tiled, e_tiled, cfg,
                             w, scratch, stats, loss_vec, coef, rows, stream, true);
}
