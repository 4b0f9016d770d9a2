// The generator-mode front launch of the 16-frames-per-wave step for a RESIDENT batch (see ef16_front.hip for the step itself).
//
// The alignment record of a frame (rotation, centroid, K^-1: kAuxP floats) depends on the frame's coordinates and the layer's
// reference only - not on the parameters.  A training loop that replays the same static batches every epoch
// (EigenFunctionTask.train(): shuffle=False) therefore re-derives, in every epoch after the first, records it already had.
//   cvf_ef16_align_rows : the records of a batch, once -> `rows` (cvf_ef16_align_rows_floats(B) floats).  One wave per unit of
//                         16 frames running ef16_align_unit, the code wave 0 of the solving front kernel runs: same bits.
//   cvf_ef16_front_rows : cvf_ef16_front starting from those rows - ef16_front_kernel<.., ROWS = true>: no covariance, no 3x3
//                         solve (the kernel's fp64), one barrier less; everything behind the records is the same code, so the
//                         outputs are bit for bit those of cvf_ef16_front on the same frames.
// A translation unit of its own: the 192 ROWS instances compile beside the 208 of ef16_front.hip.
#include "ef16_front_kernel.hpp"

namespace {
// block = one wave = one unit.  Stages the unit's coordinates and the reference exactly as the front kernel does (frames past
// B as load_x_tile pads them), solves, and copies the unit's records out of LDS as 16-byte pieces.
__global__ __launch_bounds__(64) void ef16_align_rows_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B, int64_t units,
                                                            float* __restrict__ rows) {
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
}
}  // namespace

extern "C" int64_t cvf_ef16_align_rows_floats(int64_t B) { return B > 0 ? 4 * cvf_ntiles(B) * kRowsUnit + 4 : 0; }

extern "C" int cvf_ef16_align_rows(const cvf_pp_desc* pp, const float* x, int64_t B, float* rows, void* stream) {
  CVF_REQUIRE(pp && pp->mode == CVF_PP_ALIGN && !pp->align_w && pp->n_align >= 3 && pp->n_align <= pp->n_rec &&
              3 * pp->n_align <= pp->n_coord && pp->n_coord <= 192,
              "cvf_ef16_align_rows: layer not covered (the fast layout of cvf_ef16_supported())");
  CVF_REQUIRE(x && rows && B > 0, "cvf_ef16_align_rows: bad argument");
  CVF_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "cvf_ef16_align_rows: rows must be 16-byte aligned");
  const int64_t units = 4 * cvf_ntiles(B);
  CVF_REQUIRE(units < (int64_t)1 << 31, "cvf_ef16_align_rows: batch too large for one launch");
  const size_t lds = ((size_t)kU * x_tile_stride(pp->n_coord) + ((3 * pp->n_align + 3) & ~3) + kRowsUnit + 4) * sizeof(float);
  hipLaunchKernelGGL(ef16_align_rows_kernel, dim3((unsigned)units), dim3(64), lds, (hipStream_t)stream, *pp, x, B, units, rows);
  return cvf_check_launch("ef16_align_rows_kernel");
}

extern "C" int cvf_ef16_front_rows(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                   const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, float* y_tiled, float* saved,
                                   float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg, const float* w, double* scratch,
                                   double* stats, double* loss_vec, double* coef, const float* rows, void* stream) {
  CVF_REQUIRE(rows && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
              "cvf_ef16_front_rows: rows (cvf_ef16_align_rows of this batch) missing or not 16-byte aligned");
  return ef16_front_go<true>("cvf_ef16_front_rows", mlp, theta, packed, feat_tiled, pp, x, B, a, y_tiled, saved, q_tiled, e_tiled, cfg, w,
                             scratch, stats, loss_vec, coef, rows, stream);
}
