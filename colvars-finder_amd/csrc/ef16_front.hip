// EigenFunctionTask generator-mode step for the fast layout (pure position features on a contiguous align set, d_r <= 72)
// with SIXTEEN frames per wave: the matrix instruction's N is 16 frames, so a wave that owns 16 frames (one "unit") runs a
// quarter of the dependent chain of the 64-frames-per-wave kernels in ef_mfma.hip, the launch has four times as many waves
// and each needs half the registers - three to five waves share a SIMD and cover each other's LDS / L2 round trips
// (the 64-frame kernels ran one 65-72 k-cycle chain per SIMD at the reference's batch size: 10 % / 14 % of the fp32 peak).
//
//   front  (cvf_ef16_front):    block = unit of 16 consecutive frames, one wave per net.
//     stage the 16 x 3N coordinates (one contiguous run) -> wave 0: centroid + covariance with FOUR lanes per frame
//     (lane = 4 f + p takes atoms = p mod 4, quad-permute DPP sums) and the 3x3 solve -> all waves: aligned positions =
//     features into an LDS image [frame][feature] (+ the tiled copy the backward kernel reads) -> wave = net: forward chain,
//     d chain and g = W_1^T d_1 on the matrix cores (activations never leave registers; g lands in the wave's own LDS image
//     as 16-byte writes) -> the three passes of q = J A J^T g, E = g^T J A J^T g with four lanes per frame on that image ->
//     wave 0: the unit's row of batch sums (fp64, fixed order).
//   back   (cvf_ef16_backward): ef_bwd_mfma_kernel<H, NH, 4, SAVED16> in ef_mfma.hip - four waves per 64-frame tile, 16
//     frames each - reading the hidden activations in the layout this file's front kernel leaves them.
//
// Replaces, for these shapes, cvf_ef_align_fwd_metric_stats / cvf_ef_backward (core.py:403-457, 517).
#include "ef16_front_kernel.hpp"


extern "C" int cvf_ef16_supported(const cvf_mlp_desc* mlp, const cvf_pp_desc* pp) {
  int H, NH;
  if (!mlp || !pp || !ef16_shape(mlp, &H, &NH) || getenv("CVF_NO_EF16")) return 0;
  if (!ef16_dispatch(H, NH, [](auto, auto) {})) return 0;
  const int fast = CVF_PP_ALIGN_CONTIG | CVF_PP_PURE_POSITION;
  if (pp->mode != CVF_PP_ALIGN || pp->align_w || (pp->flags & fast) != fast || pp->n_align > pp->n_rec || pp->n_align < 3) return 0;
  if (pp->d_r != 3 * pp->n_rec || pp->d_r != mlp->dims[0] || pp->d_r > 72 || pp->n_coord > 192 || pp->n_coord < pp->d_r) return 0;
  if (mlp->n_nets < 1 || mlp->n_nets > CVF_MAX_NETS) return 0;
  return (size_t)front16_lds(pp->n_coord, pp->n_align, mlp->n_nets).total * sizeof(float) <= 64 * 1024;
}

// rows of per-unit batch sums the front launch leaves in `scratch` (+ room for the two-stage fallback of large batches)
extern "C" int64_t cvf_ef16_scratch_doubles(int64_t B, int k) {
  const int64_t units = 4 * cvf_ntiles(B);
  const int64_t rows = units <= kMaxRows16 ? units : 0;
  return rows * cvf_ef_nstats(k, 1) + cvf_ef_stats_scratch_doubles(k, 1);   // (the time-lagged sums are the longer vector)
}

// units whose rows of batch sums cvf_ef16_front leaves in `scratch` for cvf_ef16_finish (0: the batch is too large for one
// finishing launch - give cvf_ef16_front `stats` and it runs the two-stage reduction itself)
extern "C" int64_t cvf_ef16_rows(int64_t B) {
  const int64_t units = 4 * cvf_ntiles(B);
  return units <= kMaxRows16 ? units : 0;
}
extern "C" int cvf_ef16_finish(const cvf_ef_cfg* cfg, int64_t B, const double* scratch, double* stats, double* loss_vec, double* coef,
                               void* stream) {
  CVF_REQUIRE(cfg && scratch && stats && cvf_ef16_rows(B) > 0, "cvf_ef16_finish: bad argument");
  CVF_REQUIRE(loss_vec == nullptr || coef != nullptr, "cvf_ef16_finish: loss_vec without coef");
  return cvf_ef_stats_finish_impl(cfg, (int)cvf_ef16_rows(B), 1, scratch, stats, loss_vec, coef, (hipStream_t)stream);
}

// data-parallel step: the units' rows -> this rank's sums -> the sum over ranks (peer-to-peer exchange inside the launch,
// cvf_p2p.hpp) -> loss tail and coefficients.  One launch where the step had three (finish, all-reduce, cvf_ef_loss).
extern "C" int cvf_ef16_finish_dp(const cvf_ef_cfg* cfg, int64_t B, const double* scratch, double* stats, double* loss_vec, double* coef,
                                  void* p2p_comm, void* stream) {
  CVF_REQUIRE(cfg && scratch && stats && loss_vec && coef && cvf_ef16_rows(B) > 0, "cvf_ef16_finish_dp: bad argument");
  const P2PLL* ll = cvf_p2p_ll(p2p_comm, 0);
  if (ll == nullptr) return -1;
  return cvf_ef_stats_finish_ll(cfg, (int)cvf_ef16_rows(B), 1, scratch, stats, loss_vec, coef, (hipStream_t)stream, ll);
}

extern "C" int64_t cvf_ef16_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles) {
  int H, NH;
  if (!mlp || !ef16_shape(mlp, &H, &NH)) return 0;
  return n_tiles * mlp->n_nets * (2 * NH) * (int64_t)((H + 3) / 4) * 256;
}

extern "C" int cvf_ef16_front(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                              const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, float* y_tiled, float* saved,
                              float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg, const float* w, double* scratch, double* stats,
                              double* loss_vec, double* coef, void* stream) {
  return ef16_front_go<false>("cvf_ef16_front", mlp, theta, packed, feat_tiled, pp, x, B, a, y_tiled, saved, q_tiled, e_tiled, cfg, w, scratch,
                              stats, loss_vec, coef, nullptr, stream);
}

// ... with an ISOTROPIC metric: `a` holds ONE coefficient per record atom, repeated over its x, y and z (the reference's default of
// ones and its 1 / mass form), and q = J A J^T g is formed in the aligned frame (see the kernel).  The caller answers for that.
extern "C" int cvf_ef16_front_iso(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                  const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, float* y_tiled, float* saved,
                                  float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg, const float* w, double* scratch, double* stats,
                                  double* loss_vec, double* coef, void* stream) {
  return ef16_front_go<false>("cvf_ef16_front_iso", mlp, theta, packed, feat_tiled, pp, x, B, a, y_tiled, saved, q_tiled, e_tiled, cfg, w,
                              scratch, stats, loss_vec, coef, nullptr, stream, true);
}


// ------------------------------------------------------------------------------------------------------------------
// transfer-operator mode (lag_tau > 0; core.py:403,414,420-431,440): y on the frames and on their lagged partners, then the
// backward pass of both with the coefficients of the time-lagged loss.  Same kernels, same hand-off layout; the front
// kernel stops after y (no derivative passes), the backward kernel is compiled without the tangent chain.
// ------------------------------------------------------------------------------------------------------------------
static int ef16_front_transfer_impl(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                    const cvf_pp_desc* pp, const float* x, const float* x_lag, int64_t B, float* y_tiled, float* saved,
                                    const float* w, const float* w_lag, double* rows_out, void* stream, const char* what) {
  CVF_REQUIRE(pp && pp->mode != CVF_PP_FACTORED, "%s: takes coordinates, not CVF_PP_FACTORED records", what);
  CVF_REQUIRE(cvf_ef16_supported(mlp, pp), "%s: shape not covered (cvf_ef16_supported() == 0)", what);
  CVF_REQUIRE(theta && packed && feat_tiled && x && x_lag && y_tiled && saved && B > 0, "%s: bad argument", what);
  int H, NH;
  ef16_shape(mlp, &H, &NH);
  const int k = mlp->n_nets;
  const int64_t T = cvf_ntiles(B), units = 4 * T;
  CVF_REQUIRE(2 * units < (int64_t)1 << 31, "%s: batch too large for one launch", what);
  // a unit and its lagged partner in one block, one after the other (CVF_EF16_UNPAIRED=1: one unit per block, the two sets one after the
  // other in the grid - the launch of rounds 2-3, kept as a developer switch)
  const bool paired = rows_out != nullptr || getenv("CVF_EF16_UNPAIRED") == nullptr;
  const size_t lds1 = ((size_t)front16_lds(pp->n_coord, pp->n_align, k).g + 16) * sizeof(float);   // (no g images in this instance; + the partners' weights)
  const int upb = paired ? ef16_units_per_wg(units, k, lds1) : 1;
  const size_t lds = lds1 * upb;
  ef16_dispatch(H, NH, [&](auto h_, auto nh_) {
    constexpr int kH = decltype(h_)::value, kNH = decltype(nh_)::value;
    auto kernel = ef16_front_kernel<kH, kNH, 0, true>;   // NIT = 0: the transfer-operator instance
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(paired ? (units + upb - 1) / upb : 2 * units)), dim3(64 * k * upb), lds, (hipStream_t)stream, *mlp,
                       theta, packed, *pp, x, B, (const float*)nullptr, w, feat_tiled, y_tiled, saved, (float*)nullptr, (float*)nullptr,
                       rows_out, upb | (paired ? 256 : 0), x_lag, units, w_lag, (const float*)nullptr);
  });
  return cvf_check_launch("ef16_front_kernel");
}

extern "C" int cvf_ef16_front_transfer(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                       const cvf_pp_desc* pp, const float* x, const float* x_lag, int64_t B, float* y_tiled,
                                       float* saved, void* stream) {
  return ef16_front_transfer_impl(mlp, theta, packed, feat_tiled, pp, x, x_lag, B, y_tiled, saved, nullptr, nullptr, nullptr, stream,
                                  "cvf_ef16_front_transfer");
}

// ... and the units' rows of the time-lagged batch sums in the same launch (cvf_ef16_transfer_rows(B, k) > 0): follow with
// cvf_ef16_finish / cvf_ef16_finish_dp (cfg.lag_idx > 0) instead of cvf_ef_stats
extern "C" int64_t cvf_ef16_transfer_rows(int64_t B, int k) { return k >= 1 ? cvf_ef16_rows(B) : 0; }
extern "C" int cvf_ef16_front_transfer_rows(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                            const cvf_pp_desc* pp, const float* x, const float* x_lag, int64_t B, float* y_tiled,
                                            float* saved, const float* w, const float* w_lag, double* scratch, void* stream) {
  CVF_REQUIRE(w && w_lag && scratch && mlp && cvf_ef16_transfer_rows(B, mlp->n_nets) > 0, "cvf_ef16_front_transfer_rows: bad argument");
  return ef16_front_transfer_impl(mlp, theta, packed, feat_tiled, pp, x, x_lag, B, y_tiled, saved, w, w_lag, scratch, stream,
                                  "cvf_ef16_front_transfer_rows");
}
