// AutoEncoderTask step for chains of ANY width (cvf_ae_general_*): the chains cvf_ae_step refuses because their parameters and
// a tile's activation images do not fit 160 KiB of LDS (csrc/ae.hip).  One chain (n_nets == 1, dims[0] == dims[L]) of 1 to
// CVF_MAX_LAYERS layers, widths 1 to 4096, d0 <= 65536, any activation code of include/cvf.h.  Where ae_mfma_kernel keeps a
// 64-frame tile's whole chain in LDS, here every product of the step is ONE launch over all tiles, and the activations are
// handed from launch to launch through HBM (the decomposition of csrc/ef_general.hip).  The gather,
// layer, weight-gradient and loss-sum kernels live in csrc/aeg_kernels.hpp, which RegAutoEncoderTask's route
// (csrc/regae_general.hip) includes too; aeg_err_kernel is this file's own:
//
//   aeg_gather_kernel   feat_rows[idx] (row-major [n][d0]) -> a_0 [tile][d0][64]; padded frames of the last tile are zero
//   aeg_layer_kernel    [M x K] x [K x 64 frames] per (tile, 64-row block): W_l (forward) or W_l^T (backward) as the A operand,
//                       an activation image as the B operand; the epilogue adds the bias and applies act, or multiplies by act'
//   aeg_err_kernel      zbar_L = 2 w (out - f) inv_wsum .* act'_{L-1}(out) in place of out, and the tile's fp64 sums of w err, w
//   aeg_wgrad_kernel    dW_l | db_l = sum_frames zbar_{l+1} (x) [a_l ; 1] (K = frames), the tiles split over a fixed number of
//                       slab rows (row rho sums tiles rho, rho + R, ... in that order)
//   aeg_loss_sum_kernel loss-only calls: the tiles' pairs -> out2 (with a gradient they ride in cvf_slab_reduce_impl's launch)
//
// Mathematics (layers l = 0..L-1, a_0 = f):  a_{l+1} = act_l(W_l a_l + b_l), out = a_L, loss = sum w |out - f|^2 / sum w,
//   zbar_L = 2 w (out - f) / sum w .* act'_{L-1}(a_L),  zbar_l = (W_l^T zbar_{l+1}) .* act'_{l-1}(a_l)   (act' through the output),
//   dW_l = sum_frames zbar_{l+1} (x) a_l,  db_l = sum_frames zbar_{l+1}.
//
// All products run on v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulation.  No atomics: every slab entry is written by one
// thread and the sum order of every entry is fixed by the grid, so two calls on the same inputs give the same bits.  Nothing is
// read from scratch that the same call did not write.
#include "aeg_kernels.hpp"

// (csrc/ef_mfma.hip) fixed-order sum of slab rows [+ Adam] [+ one extra block adding n_pair [a, b] rows -> [a, b, a / b]]
int cvf_slab_reduce_impl(const float* slab, int64_t n_rows, int64_t n_params, float* grad, const float* mask,
                         const cvf_adam_args* adam, void* stream, const double* pair_partial = nullptr, int n_pair = 0,
                         double* pair_out = nullptr);

namespace {

// the output error of one tile: err = sum_i (out_i - f_i)^2 per frame, partial[tile] = {sum w err, sum w} in fp64, and (with a
// gradient) zbar_L = 2 w (out - f) inv_wsum .* act'(out) in place of out.  Wave j takes rows j, j + 4, ...; the four waves' sums
// of a frame are added in the order 0, 1, 2, 3.
__global__ __launch_bounds__(256) void aeg_err_kernel(float* __restrict__ out, const float* __restrict__ a0, const float* __restrict__ w,
                                                      int64_t B, int d0, int act, double inv_wsum, int with_grad,
                                                      double* __restrict__ partial, int32_t* __restrict__ step) {
  __shared__ double part[4][CVF_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t frame = tile * CVF_TILE + lane;
  const float wb = frame < B ? w[frame] : 0.0f;
  const float s = (float)(2.0 * (double)wb * inv_wsum);
  float* op = out + tile * d0 * CVF_TILE;
  const float* fp = a0 + tile * d0 * CVF_TILE;
  double e = 0.0;
  for (int i = wave; i < d0; i += 4) {
    const float o = op[(int64_t)i * CVF_TILE + lane];
    const float d = o - fp[(int64_t)i * CVF_TILE + lane];
    e += (double)d * (double)d;
    if (with_grad) op[(int64_t)i * CVF_TILE + lane] = s * d * cvf_act_d1(act, o);
  }
  part[wave][lane] = e;
  __syncthreads();
  if (wave == 0) {
    const double err = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    const double a = wave_sum((double)wb * err), b = wave_sum((double)wb);
    if (lane == 0) {
      partial[2 * tile] = a;
      partial[2 * tile + 1] = b;
      if (step != nullptr && tile == 0) *step += 1;
    }
  }
}

// ---- scratch: a_0, a_1..a_{L-1} ([tile][width][64] each), two ping-pong images of zbar (widest of dims[1..L]; zbar_l and the
// chain's output sit in image l & 1), the slab rows, the tiles' partial pairs (doubles, 8-byte aligned)
struct AegLayout {
  int64_t a[CVF_MAX_LAYERS], zb[2], slab, partial, total;
  int64_t rows;
  int wmax;
};

AegLayout aeg_layout(const cvf_mlp_desc* mlp, int64_t n_tiles) {
  AegLayout L = {};
  const int64_t per = n_tiles * CVF_TILE;   // floats of one row of every tile
  int64_t pos = 0;
  L.wmax = 1;
  for (int l = 0; l < mlp->n_layers; ++l) {
    L.a[l] = pos;
    pos += per * mlp->dims[l];
    L.wmax = mlp->dims[l + 1] > L.wmax ? mlp->dims[l + 1] : L.wmax;
  }
  for (int i = 0; i < 2; ++i) {
    L.zb[i] = pos;
    pos += per * L.wmax;
  }
  L.rows = g64_rows(mlp, n_tiles);
  L.slab = pos;
  pos += L.rows * mlp->n_params;
  L.partial = (pos + 1) & ~(int64_t)1;
  L.total = L.partial + 4 * n_tiles;
  return L;
}

const char* aeg_why(const cvf_mlp_desc* mlp) {
  static thread_local char buf[160];
  if (mlp == nullptr) return "no chain description";
  if (mlp->n_nets != 1) {
    snprintf(buf, sizeof buf, "%d nets: one chain is expected", mlp->n_nets);
    return buf;
  }
  const char* why = g64_why(mlp, mlp->n_layers, G64Chain{1, "hidden layer", "chain", true, true}, buf, sizeof buf);
  if (why != nullptr) return why;
  if (mlp->dims[mlp->n_layers] != mlp->dims[0]) {
    snprintf(buf, sizeof buf, "output width %d != input width %d", mlp->dims[mlp->n_layers], mlp->dims[0]);
    return buf;
  }
  return nullptr;
}

}  // namespace

extern "C" int cvf_ae_general_supported(const cvf_mlp_desc* mlp) {
  const char* why = aeg_why(mlp);
  if (why != nullptr) {
    cvf_set_error("cvf_ae_general: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_ae_general_scratch_floats(const cvf_mlp_desc* mlp, int64_t B) {
  if (aeg_why(mlp) != nullptr || B < 1) return 0;
  return aeg_layout(mlp, cvf_ntiles(B)).total;
}

extern "C" int cvf_ae_general_step(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx,
                                   int64_t B, const float* w, double inv_wsum, float* scratch, double* out2, float* grad,
                                   int32_t* step_count, const cvf_adam_args* adam, void* stream) {
  const char* why = aeg_why(mlp);
  CVF_REQUIRE(why == nullptr, "cvf_ae_general_step: %s", why);
  CVF_REQUIRE(theta && feat_rows && w && scratch && out2 && B > 0, "cvf_ae_general_step: bad argument");
  CVF_REQUIRE(adam == nullptr || (grad && adam->theta && adam->m && adam->v && adam->step_count),
              "cvf_ae_general_step: incomplete adam arguments");
  const int64_t T = cvf_ntiles(B);
  CVF_REQUIRE(T <= 0x7fffffff, "cvf_ae_general_step: %lld frames are more than one call takes", (long long)B);
  hipStream_t s = (hipStream_t)stream;
  const int L = mlp->n_layers, d0 = mlp->dims[0];
  const AegLayout lay = aeg_layout(mlp, T);
  auto A = [&](int l) { return scratch + lay.a[l]; };           // a_l, l = 0..L-1
  auto Z = [&](int l) { return scratch + lay.zb[l & 1]; };      // zbar_l, l = 1..L (a_L = out before aeg_err_kernel)
  auto ts = [&](int l) { return (int64_t)mlp->dims[l] * CVF_TILE; };
  float* slab = scratch + lay.slab;
  double* partial = reinterpret_cast<double*>(scratch + lay.partial);

  hipLaunchKernelGGL(aeg_gather_kernel, dim3((unsigned)T), dim3(256), 0, s, feat_rows, idx, B, d0, A(0), T,
                     (int64_t)0);
  if (cvf_check_launch("aeg_gather_kernel")) return -1;

  auto layer = [&](const AegLayerArgs& a) {
    hipLaunchKernelGGL(aeg_layer_kernel, dim3((unsigned)T, (unsigned)((a.M + 63) / 64)), dim3(256), 0, s, theta, a);
    return cvf_check_launch("aeg_layer_kernel");
  };
  // forward: a_{l+1} = act_l(W_l a_l + b_l); the chain's output goes to the zbar image of layer L
  for (int l = 0; l < L; ++l) {
    AegLayerArgs a = {};
    a.w_off = mlp->w_off[0][l];
    a.b_off = mlp->b_off[0][l];
    a.ldw = mlp->dims[l];
    a.M = mlp->dims[l + 1];
    a.K = mlp->dims[l];
    a.epi = EPI_ACT;
    a.act = mlp->act[l];
    a.x = A(l);
    a.xs = ts(l);
    a.out = l + 1 < L ? A(l + 1) : Z(L);
    a.os = ts(l + 1);
    if (layer(a)) return -1;
  }
  hipLaunchKernelGGL(aeg_err_kernel, dim3((unsigned)T), dim3(256), 0, s, Z(L), A(0), w, B, d0, mlp->act[L - 1], inv_wsum,
                     grad != nullptr ? 1 : 0, partial, grad != nullptr ? step_count : nullptr);
  if (cvf_check_launch("aeg_err_kernel")) return -1;
  if (grad == nullptr) {
    hipLaunchKernelGGL(aeg_loss_sum_kernel, dim3(1), dim3(64), 0, s, partial, T, out2);
    return cvf_check_launch("aeg_loss_sum_kernel");
  }

  const int R = (int)lay.rows;
  for (int l = L - 1; l >= 0; --l) {
    {  // layer l's gradient from zbar_{l+1} and a_l
      AegGradArgs g = {};
      g.w_off = mlp->w_off[0][l];
      g.b_off = mlp->b_off[0][l];
      g.Mo = mlp->dims[l + 1];
      g.Ki = mlp->dims[l];
      g.n_tiles = T;
      g.B = B;
      g.rows = R;
      g.n_params = mlp->n_params;
      g.z = Z(l + 1);
      g.zs = ts(l + 1);
      g.h = A(l);
      g.hs = ts(l);
      const int nb = ((g.Mo + 63) / 64) * ((g.Ki + 1 + 63) / 64);
      hipLaunchKernelGGL(aeg_wgrad_kernel, dim3((unsigned)R, (unsigned)nb), dim3(256), 0, s, g, slab);
      if (cvf_check_launch("aeg_wgrad_kernel")) return -1;
    }
    if (l == 0) break;
    // zbar_l = (W_l^T zbar_{l+1}) .* act'_{l-1}(a_l)
    AegLayerArgs a = {};
    a.w_off = mlp->w_off[0][l];
    a.b_off = -1;
    a.ldw = mlp->dims[l];
    a.trans = 1;
    a.M = mlp->dims[l];
    a.K = mlp->dims[l + 1];
    a.epi = EPI_BWD;
    a.act = mlp->act[l - 1];
    a.x = Z(l + 1);
    a.xs = ts(l + 1);
    a.out = Z(l);
    a.os = ts(l);
    a.eh = A(l);
    a.es = ts(l);
    if (layer(a)) return -1;
  }
  // fixed-order sum of the slab rows (+ the Adam update when asked for), the loss pairs in one extra block of the same launch
  cvf_adam_args ad;
  if (adam != nullptr) {
    ad = *adam;
    ad.mlp = nullptr;      // an AutoEncoder has no MFMA fragment copy to refresh
    ad.packed = nullptr;
  }
  return cvf_slab_reduce_impl(slab, R, mlp->n_params, grad, nullptr, adam != nullptr ? &ad : nullptr, stream, partial, (int)T, out2);
}
