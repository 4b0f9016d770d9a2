// Bias energy and forces along a trained CV in ONE launch, in the MD engine's own arrays (cvf_cv_*_bias_*).
// The two one-launch kernels of csrc/cv_frame_kernel.hpp (one wave per frame) and csrc/cv_frame_large_kernel.hpp (one workgroup per
// frame) under another IO policy - their arithmetic from the coordinates in LDS to the gradient image is the namesakes', text for
// text:
//
//   frame   atom a of replica b from x_all[b x_frame_stride + atom_index[a] atom_stride + c] (cvf_md_layout; NULL: dense)
//   seed    once xi is in LDS, lane i < k sums its terms' U_t(xi_i) and U_t'(xi_i) in term order (cvf_bias.hpp; of a joint grid
//           term on (cv, cv2) lane cv takes U and dU/dxi_cv, lane cv2 dU/dxi_cv2: DESIGN.md section 4.19), writes du_rows,
//           stores -du_i and its share of U to 2 k LDS floats; behind a barrier thread 0 adds the k shares in index order into
//           u_rows, and the contracted sweep (coef form: one cotangent row) reads its seed from the LDS row instead of a global coef
//   force   f_all[b f_frame_stride + atom_index[a] atom_stride + c] += the row, each element by the one thread that owns it
//
// No atomics, no scratch, no aux; the bias table is read at launch time.
#include "cv_frame_kernel.hpp"
#include "cv_frame_large_kernel.hpp"
#include "cvf_bias.hpp"

namespace {

// the engine's arrays, as the kernels take them (a NULL cvf_md_layout: stride 3, frame strides n_coord, no index)
struct MdArgs {
  const float* x_all;
  float* f_all;
  const int32_t* atom_index;
  int64_t x_frame_stride, f_frame_stride;
  int32_t atom_stride;
  float* u_rows;
  float* du_rows;
};

__device__ __forceinline__ int64_t md_atom(const MdArgs& md, int a) {
  return (int64_t)(md.atom_index != nullptr ? md.atom_index[a] : a) * md.atom_stride;
}

// the seed row of the frame in spare[0..k) (spare holds 2 k floats), u_rows and du_rows written; every thread of the frame calls it
__device__ __forceinline__ const float* bias_seeds(const cvf_bias_desc& bias, const MdArgs& md, float* spare, const float* top,
                                                   int64_t frame, int k, int idx) {
  if (idx < k) {
    float u, du;
    cvf_bias_cv_eval(bias, idx, top, &u, &du);   // (the whole row: a joint grid term reads two of its k values)
    spare[idx] = -du;
    spare[k + idx] = u;
    if (md.du_rows != nullptr) md.du_rows[frame * k + idx] = du;
  }
  lds_barrier();
  if (idx == 0) {
    float U = spare[k];
    for (int i = 1; i < k; ++i) U += spare[k + i];
    md.u_rows[frame] = U;
  }
  return spare;
}

struct WaveIO {
  const cvf_bias_desc& bias;
  const MdArgs& md;
  __device__ __forceinline__ float load(int64_t frame, int, int j) const {
    const int a = j / 3;
    return md.x_all[frame * md.x_frame_stride + md_atom(md, a) + (j - 3 * a)];
  }
  __device__ __forceinline__ const float* seeds(float* spare, const float* top, int64_t frame, int k, int lane) const {
    return bias_seeds(bias, md, spare, top, frame, k, lane);
  }
  __device__ __forceinline__ void store(int64_t frame, int, int, int e, float v) const {   // (one row: e is the coordinate)
    const int a = e / 3;
    md.f_all[frame * md.f_frame_stride + md_atom(md, a) + (e - 3 * a)] += v;
  }
};

template <bool SHARED>
__global__ __launch_bounds__(64) void cv_frame_bias_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, cvfr::FrLayout lay, cvf_bias_desc bias,
                                                            MdArgs md, const float* __restrict__ theta, float* __restrict__ xi_rows) {
  cvfr::cv_frame_body<SHARED>(mlp, pp, lay, theta, xi_rows, true, WaveIO{bias, md});
}

struct GroupIO {
  const cvf_bias_desc& bias;
  const MdArgs& md;
  __device__ __forceinline__ const float* atom(int64_t frame, int a) const { return md.x_all + frame * md.x_frame_stride + md_atom(md, a); }
  __device__ __forceinline__ const float* seeds(float* spare, const float* top, int64_t frame, int k, int tid) const {
    return bias_seeds(bias, md, spare, top, frame, k, tid);
  }
  __device__ __forceinline__ float* out(int64_t frame, int, int) const { return md.f_all + frame * md.f_frame_stride; }
  static constexpr bool kByAtom = true;   // (an engine's atom is three adjacent floats: one index load, three accumulations in flight)
  __device__ __forceinline__ void put_atom(float* rows, int, int, int A, V3 v) const {   // (one row)
    float* p = rows + md_atom(md, A);
    const float f0 = p[0], f1 = p[1], f2 = p[2];
    p[0] = f0 + v.x;
    p[1] = f1 + v.y;
    p[2] = f2 + v.z;
  }
};

template <int MODE, bool SHARED>
__global__ __launch_bounds__(cvfl::kThreads) void cv_frame_large_bias_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, cvfl::LgLayout lay,
                                                                             cvf_bias_desc bias, MdArgs md, const float* __restrict__ theta,
                                                                             float* __restrict__ xi_rows) {
  cvfl::cv_frame_large_body<false, MODE, SHARED>(mlp, pp, lay, theta, xi_rows, true, GroupIO{bias, md});
}

// nullptr and *md filled, or why the call is refused (the model's own check has passed: k CVs, pp is a coordinate mode)
const char* md_why(const cvf_pp_desc* pp, int k, const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* theta, const float* x_all,
                   int64_t B, float* xi_rows, float* u_rows, float* du_rows, float* f_all, MdArgs* md) {
  static thread_local char buf[240];
  const char* why = cvf_bias_why(bias, k, buf, sizeof buf);
  if (why != nullptr) return why;
#define CVFB_NO(...)                       \
  do {                                     \
    snprintf(buf, sizeof buf, __VA_ARGS__); \
    return buf;                            \
  } while (0)
  if (B < 0 || B > 0x7fffffff) CVFB_NO("B = %lld frames (one call takes 0 to 2^31 - 1)", (long long)B);
  const int nc = pp->n_coord;
  MdArgs m = {x_all, f_all, nullptr, nc, nc, 3, u_rows, du_rows};
  if (layout != nullptr) {
    if (layout->atom_stride < 3) CVFB_NO("layout.atom_stride = %d: an atom has at least 3 floats", layout->atom_stride);
    if (layout->x_frame_stride < 0 || layout->f_frame_stride < 0)
      CVFB_NO("layout.x_frame_stride = %lld, layout.f_frame_stride = %lld: negative", (long long)layout->x_frame_stride, (long long)layout->f_frame_stride);
    if (layout->atom_index != nullptr && nc % 3 != 0)
      CVFB_NO("layout.atom_index with n_coord = %d%s: an atom index needs frames of whole atoms (n_coord %% 3 == 0)", nc,
              pp->mode == CVF_PP_IDENTITY ? " (CVF_PP_IDENTITY)" : "");
    if (B > 1) {
      // Two frames' force elements must not coincide: each is accumulated by one thread of its own workgroup.  n_coord / 3 distinct
      // atoms reach at least atom n_coord / 3 - 1, so a frame of forces spans at least `extent` floats (exactly that without an
      // index; with one the true extent is the caller's knowledge).  x_all is only read: frames may overlap or repeat there.
      const int64_t extent = (int64_t)((nc + 2) / 3 - 1) * layout->atom_stride + (nc % 3 == 0 ? 3 : nc % 3);
      if (layout->f_frame_stride < extent)
        CVFB_NO("layout.f_frame_stride = %lld with B = %lld: the force frames of the batch overlap (one frame spans at least %lld floats)",
                (long long)layout->f_frame_stride, (long long)B, (long long)extent);
    }
    m.atom_index = layout->atom_index;
    m.atom_stride = layout->atom_stride;
    m.x_frame_stride = layout->x_frame_stride;
    m.f_frame_stride = layout->f_frame_stride;
  }
  if (B > 0 && !(theta && x_all && xi_rows && u_rows && f_all)) CVFB_NO("null argument");
#undef CVFB_NO
  *md = m;
  return nullptr;
}

template <bool SHARED>
int wave_eval(const char* name, const cvf_mlp_desc* mlp, const float* theta, int cut, const cvf_pp_desc* pp, const cvf_bias_desc* bias,
              const cvf_md_layout* layout, const float* x_all, int64_t B, float* xi_rows, float* u_rows, float* du_rows, float* f_all,
              void* stream) {
  cvfr::FrLayout lay;
  const char* why = SHARED ? cvfr::cvfr_shared_why(mlp, cut, pp, &lay, "cvf_cv_frame_bias_eval", 2) : cvfr::cvfr_why(mlp, cut, pp, &lay, 0, 2);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  MdArgs md;
  why = md_why(pp, lay.k, bias, layout, theta, x_all, B, xi_rows, u_rows, du_rows, f_all, &md);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  if (B == 0) return 0;
  const size_t lds = ((size_t)lay.total + 2 * (size_t)lay.k) * sizeof(float);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)cv_frame_bias_kernel<SHARED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    CVF_REQUIRE(e == hipSuccess, "%s: %zu bytes of dynamic LDS: %s", name, lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(cv_frame_bias_kernel<SHARED>, dim3((unsigned)B), dim3(CVF_WAVE), lds, (hipStream_t)stream, *mlp, *pp, lay, *bias, md,
                     theta, xi_rows);
  return cvf_check_launch("cv_frame_bias_kernel");
}

template <bool SHARED>
int group_eval(const char* name, const cvf_mlp_desc* mlp, const float* theta, int cut, const cvf_pp_desc* pp, const cvf_bias_desc* bias,
               const cvf_md_layout* layout, const float* x_all, int64_t B, float* xi_rows, float* u_rows, float* du_rows, float* f_all,
               void* stream) {
  cvfl::LgLayout lay;
  const char* why = SHARED ? cvfl::cvfl_shared_why(mlp, cut, pp, &lay, "cvf_cv_frame_large_bias_eval") : cvfl::cvfl_why(mlp, cut, pp, &lay);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  MdArgs md;
  why = md_why(pp, lay.k, bias, layout, theta, x_all, B, xi_rows, u_rows, du_rows, f_all, &md);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  if (B == 0) return 0;
  const size_t lds = ((size_t)lay.rows + 3 * (size_t)pp->n_ref) * sizeof(float);   // one cotangent row (the seeds sit in the moments' LDS)
  const int mode = pp->mode != CVF_PP_ALIGN ? 0 : (pp->align_w == nullptr ? 1 : 2);
  const auto kernel = mode == 0 ? cv_frame_large_bias_kernel<0, SHARED> : mode == 1 ? cv_frame_large_bias_kernel<1, SHARED> : cv_frame_large_bias_kernel<2, SHARED>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    CVF_REQUIRE(e == hipSuccess, "%s: %zu bytes of dynamic LDS: %s", name, lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(cvfl::kThreads), lds, (hipStream_t)stream, *mlp, *pp, lay, *bias, md, theta, xi_rows);
  return cvf_check_launch("cv_frame_large_bias_kernel");
}

int answer(const char* name, const char* why) {
  if (why != nullptr) {
    cvf_set_error("%s: %s", name, why);
    return 0;
  }
  return 1;
}

}  // namespace

extern "C" int cvf_cv_bias_check(const cvf_bias_desc* bias, int k) {
  char buf[240];
  return answer("cvf_cv_bias_check", cvf_bias_why(bias, k, buf, sizeof buf));
}

extern "C" int cvf_cv_frame_bias_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_bias", cvfr::cvfr_why(mlp, upto_layer, pp, nullptr, 0, 2));
}

extern "C" int cvf_cv_frame_bias_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_bias_shared", cvfr::cvfr_shared_why(mlp, n_shared, pp, nullptr, "cvf_cv_frame_bias_eval", 2));
}

extern "C" int cvf_cv_frame_large_bias_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_large_bias", cvfl::cvfl_why(mlp, upto_layer, pp, nullptr));
}

extern "C" int cvf_cv_frame_large_bias_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_large_bias_shared", cvfl::cvfl_shared_why(mlp, n_shared, pp, nullptr, "cvf_cv_frame_large_bias_eval"));
}

extern "C" int cvf_cv_frame_bias_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                      const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                      float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return wave_eval<false>("cvf_cv_frame_bias_eval", mlp, theta, upto_layer, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all, stream);
}

extern "C" int cvf_cv_frame_bias_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                             const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                             float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return wave_eval<true>("cvf_cv_frame_bias_shared_eval", mlp, theta, n_shared, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all,
                         stream);
}

extern "C" int cvf_cv_frame_large_bias_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                            const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                            float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return group_eval<false>("cvf_cv_frame_large_bias_eval", mlp, theta, upto_layer, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all,
                           stream);
}

extern "C" int cvf_cv_frame_large_bias_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                                   const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                                   float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return group_eval<true>("cvf_cv_frame_large_bias_shared_eval", mlp, theta, n_shared, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows,
                          f_all, stream);
}
