// xi(x) and d xi / d x of a trained CV per frame in ONE launch: one wave = one frame (cvf_cv_frame_*).
// The kernel's body, its LDS layout and its predicate live in cv_frame_kernel.hpp (the account of the design is there); this file
// instantiates the body on dense arrays - x [B][n_coord] in, the seed of the contracted sweep from the global coef [B][k],
// gx_rows written - and holds the entry points.
#include "cv_frame_kernel.hpp"

namespace {
using namespace cvfr;

struct DenseIO {
  const float* x;
  const float* coef;
  float* gx_rows;
  static constexpr bool kCell = false;
  __device__ __forceinline__ float load(int64_t frame, int nc, int j) const { return x[frame * nc + j]; }
  __device__ __forceinline__ const float* seeds(float*, const float*, int64_t frame, int k, int) const {
    return coef != nullptr ? coef + frame * k : nullptr;
  }
  __device__ __forceinline__ void store(int64_t frame, int kk, int nc, int e, float v) const { gx_rows[frame * kk * nc + e] = v; }
};

// SHARED: form C (an instance of its own: forms A and B keep their code)
template <bool SHARED>
__global__ __launch_bounds__(64) void cv_frame_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, FrLayout lay,
                                                       const float* __restrict__ theta, const float* __restrict__ x,
                                                       const float* __restrict__ coef, float* __restrict__ xi_rows,
                                                       float* __restrict__ gx_rows) {
  cv_frame_body<SHARED>(mlp, pp, lay, theta, xi_rows, coef != nullptr, DenseIO{x, coef, gx_rows});
}

}  // namespace

extern "C" int cvf_cv_frame_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  const char* why = cvfr_why(mlp, upto_layer, pp, nullptr);
  if (why != nullptr) {
    cvf_set_error("cvf_cv_frame: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int cvf_cv_frame_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp, const float* x,
                                 int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream) {
  FrLayout lay;
  const char* why = cvfr_why(mlp, upto_layer, pp, &lay);
  CVF_REQUIRE(why == nullptr, "cvf_cv_frame_eval: %s", why);
  CVF_REQUIRE(B >= 0 && B <= 0x7fffffff, "cvf_cv_frame_eval: B = %lld frames (one call takes 0 to 2^31 - 1)", (long long)B);
  if (B == 0) return 0;
  CVF_REQUIRE(theta && x && xi_rows && gx_rows, "cvf_cv_frame_eval: null argument");
  const size_t lds = (size_t)lay.total * sizeof(float);
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)cv_frame_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(cv_frame_kernel<false>, dim3((unsigned)B), dim3(CVF_WAVE), lds, (hipStream_t)stream, *mlp, *pp, lay, theta, x,
                     coef, xi_rows, gx_rows);
  return cvf_check_launch("cv_frame_kernel");
}

extern "C" int cvf_cv_frame_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  const char* why = cvfr_shared_why(mlp, n_shared, pp, nullptr);
  if (why != nullptr) {
    cvf_set_error("cvf_cv_frame_shared: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int cvf_cv_frame_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                        const float* x, int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream) {
  FrLayout lay;
  const char* why = cvfr_shared_why(mlp, n_shared, pp, &lay);
  CVF_REQUIRE(why == nullptr, "cvf_cv_frame_shared_eval: %s", why);
  CVF_REQUIRE(B >= 0 && B <= 0x7fffffff, "cvf_cv_frame_shared_eval: B = %lld frames (one call takes 0 to 2^31 - 1)", (long long)B);
  if (B == 0) return 0;
  CVF_REQUIRE(theta && x && xi_rows && gx_rows, "cvf_cv_frame_shared_eval: null argument");
  const size_t lds = (size_t)lay.total * sizeof(float);
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)cv_frame_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(cv_frame_kernel<true>, dim3((unsigned)B), dim3(CVF_WAVE), lds, (hipStream_t)stream, *mlp, *pp, lay, theta, x,
                     coef, xi_rows, gx_rows);
  return cvf_check_launch("cv_frame_kernel<shared>");
}
