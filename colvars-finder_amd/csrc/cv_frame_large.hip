// xi(x) and d xi / d x of a trained CV per frame in ONE launch for frames of ANY size: one WORKGROUP (256 threads) = one frame
// (cvf_cv_frame_large_*).  The kernel's body, its LDS layout and its predicate live in
// cv_frame_large_kernel.hpp (the account of the design is there); this file instantiates the body on dense arrays - x [B][n_coord]
// in, the seed of the contracted sweep from the global coef [B][k], gx_rows written - and holds the entry points.
#include "cv_frame_large_kernel.hpp"

namespace {
using namespace cvfl;

struct DenseIO {
  const float* x;
  const float* coef;
  float* gx_rows;
  int nc;
  static constexpr bool kByAtom = false, kCell = false;
  __device__ __forceinline__ const float* atom(int64_t frame, int a) const { return x + frame * nc + 3 * a; }
  __device__ __forceinline__ const float* seeds(float*, const float*, int64_t frame, int k, int) const {
    return coef != nullptr ? coef + frame * k : nullptr;
  }
  __device__ __forceinline__ float* out(int64_t frame, int kk, int n) const { return gx_rows + frame * (int64_t)kk * n; }
  __device__ __forceinline__ void put(float* rows, int n, int ii, int j, int, int, float v) const { rows[ii * (int64_t)n + j] = v; }
};

// MODE: 0 CVF_PP_FEATURES, 1 CVF_PP_ALIGN with uniform weights, 2 CVF_PP_ALIGN with align_w (instances, not branches: the uniform
// values of the other modes stay out of the scalar registers); SHARED: form C
template <bool VEC4, int MODE, bool SHARED>
__global__ __launch_bounds__(kThreads) void cv_frame_large_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, LgLayout lay,
                                                                  const float* __restrict__ theta, const float* __restrict__ x,
                                                                  const float* __restrict__ coef, float* __restrict__ xi_rows,
                                                                  float* __restrict__ gx_rows) {
  cv_frame_large_body<VEC4, MODE, SHARED>(mlp, pp, lay, theta, xi_rows, coef != nullptr, DenseIO{x, coef, gx_rows, pp.n_coord});
}

template <bool SHARED>
int cvfl_launch(const char* name, const cvf_mlp_desc* mlp, const LgLayout& lay, const float* theta, const cvf_pp_desc* pp, const float* x,
                int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream) {
  CVF_REQUIRE(B >= 0 && B <= 0x7fffffff, "%s: B = %lld frames (one call takes 0 to 2^31 - 1)", name, (long long)B);
  if (B == 0) return 0;
  CVF_REQUIRE(theta && x && xi_rows && gx_rows, "%s: null argument", name);
  // with coef the coordinate part has one row: the launch takes the LDS of that one row
  const int rows_now = coef != nullptr ? 1 : lay.rpp;
  const size_t lds = ((size_t)lay.rows + (size_t)rows_now * 3 * (size_t)pp->n_ref) * sizeof(float);
  const bool vec4 = pp->n_coord % 4 == 0 && ((uintptr_t)gx_rows & 15) == 0;   // 16-byte stores of the dense rows
  const int mode = pp->mode != CVF_PP_ALIGN ? 0 : (pp->align_w == nullptr ? 1 : 2);
  const auto kernel = vec4 ? (mode == 0 ? cv_frame_large_kernel<true, 0, SHARED> : mode == 1 ? cv_frame_large_kernel<true, 1, SHARED> : cv_frame_large_kernel<true, 2, SHARED>)
                           : (mode == 0 ? cv_frame_large_kernel<false, 0, SHARED> : mode == 1 ? cv_frame_large_kernel<false, 1, SHARED> : cv_frame_large_kernel<false, 2, SHARED>);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    CVF_REQUIRE(e == hipSuccess, "%s: %zu bytes of dynamic LDS: %s", name, lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kThreads), lds, (hipStream_t)stream, *mlp, *pp, lay, theta, x, coef, xi_rows, gx_rows);
  return cvf_check_launch("cv_frame_large_kernel");
}

}  // namespace

extern "C" int cvf_cv_frame_large_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  const char* why = cvfl_why(mlp, upto_layer, pp, nullptr);
  if (why != nullptr) {
    cvf_set_error("cvf_cv_frame_large: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_cv_frame_large_lds_bytes(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp, int32_t* rows_per_pass) {
  LgLayout lay;
  const char* why = cvfl_why(mlp, upto_layer, pp, &lay);
  CVF_REQUIRE(why == nullptr, "cvf_cv_frame_large_lds_bytes: %s", why);
  if (rows_per_pass != nullptr) *rows_per_pass = lay.rpp;
  return (int64_t)lay.total * (int64_t)sizeof(float);
}

extern "C" int cvf_cv_frame_large_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                       const float* x, int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream) {
  LgLayout lay;
  const char* why = cvfl_why(mlp, upto_layer, pp, &lay);
  CVF_REQUIRE(why == nullptr, "cvf_cv_frame_large_eval: %s", why);
  return cvfl_launch<false>("cvf_cv_frame_large_eval", mlp, lay, theta, pp, x, B, coef, xi_rows, gx_rows, stream);
}

extern "C" int cvf_cv_frame_large_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  const char* why = cvfl_shared_why(mlp, n_shared, pp, nullptr);
  if (why != nullptr) {
    cvf_set_error("cvf_cv_frame_large_shared: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_cv_frame_large_shared_lds_bytes(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp, int32_t* rows_per_pass) {
  LgLayout lay;
  const char* why = cvfl_shared_why(mlp, n_shared, pp, &lay);
  CVF_REQUIRE(why == nullptr, "cvf_cv_frame_large_shared_lds_bytes: %s", why);
  if (rows_per_pass != nullptr) *rows_per_pass = lay.rpp;
  return (int64_t)lay.total * (int64_t)sizeof(float);
}

extern "C" int cvf_cv_frame_large_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                              const float* x, int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream) {
  LgLayout lay;
  const char* why = cvfl_shared_why(mlp, n_shared, pp, &lay);
  CVF_REQUIRE(why == nullptr, "cvf_cv_frame_large_shared_eval: %s", why);
  return cvfl_launch<true>("cvf_cv_frame_large_shared_eval", mlp, lay, theta, pp, x, B, coef, xi_rows, gx_rows, stream);
}
