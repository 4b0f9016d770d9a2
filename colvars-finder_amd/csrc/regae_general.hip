// RegAutoEncoderTask's chain on the per-layer kernels (cvf_regae_general_*): the merged chains regae_launch (csrc/ae.hip) refuses
// because their parameters and a tile's activation images do not fit 160 KiB of LDS.  The chain is the one _RegFlatParams
// builds - the encoder, then the decoder and the K regulariser nets side by side as dense layers with structural zeros - so its
// last layer is [reconstruction (d_0 rows) | y_1..y_K].  The call contract is cvf_regae_forward's / cvf_regae_backward's; the
// decomposition is csrc/ae_general.hip's (DESIGN.md sections 4.10 / 4.11), one launch per layer and pass over ALL tiles:
//
//   aeg_gather_kernel    tiles 0..T-1 = rows idx, tiles T..2T-1 = rows idx + lag_input (only when K > 0 and lag_input > 0)
//   aeg_layer_kernel     forward, layer by layer; the dense product IS the block product (theta holds zeros off the blocks)
//   regaeg_out_kernel    y_tiled, enc_tiled, the base tiles' fp64 pairs {sum w err, sum w} against the rows idx + lag_target; with
//                        a gradient: zbar_L in place of the output (reconstruction rows of base tiles, 0 on lagged tiles, the
//                        transfer-operator output gradient on the head rows), every row times act'_{L-1}
//   aeg_layer_kernel     transposed (EPI_BWD), aeg_wgrad_kernel into R slab rows; regaeg_enc_kernel adds the latent penalties'
//                        gradient to zbar_{n_enc} of the base tiles
//   cvf_slab_reduce_impl fixed-order sum of the slab rows, times mask, + Adam
//
// Padded frames (the ragged last tile of each half) are gathered as zeros and seeded with exactly 0.0, so every later adjoint
// and every gradient product of those frames vanishes: aeg_wgrad_kernel is told that all frames of the 2 T tiles are valid.
// No atomics.  Nothing is read from scratch that the same call did not write, apart from the hand-off from
// cvf_regae_general_forward to cvf_regae_general_backward_reuse (the images a_0..a_{L-1} and the chain's output).
//
// A decoder and regulariser nets of DIFFERENT depths (cvf_regae_ragged_*, the second half of this file; the chain of
// _RegRaggedFlatParams) run on the same kernels: regaeg_out_kernel takes the reconstruction and the heads as two views, which the
// calls above point into the one image Z(L) and the ragged calls into the images where the two groups end.
#include "aeg_kernels.hpp"

int cvf_slab_reduce_impl(const float* slab, int64_t n_rows, int64_t n_params, float* grad, const float* mask,
                         const cvf_adam_args* adam, void* stream, const double* pair_partial = nullptr, int n_pair = 0,
                         double* pair_out = nullptr);

namespace {

// One group's rows of an image: where its values are read and (with a gradient) where its adjoint goes.  The two coincide in the
// chain's last image (Z(L): zbar_L takes the output's place) and differ for the rows a shallower group has finished in an inner
// image (a_ls -> zbar_ls, the ragged chains below).
struct RegaegView {
  const float* in;   // NULL: these rows are not this launch's
  float* zb;
  int64_t is, zs;    // tile strides
  int act;           // the activation behind these rows
};

struct RegaegOutArgs {
  int d0, K;                 // reconstruction rows, heads
  RegaegView rec, head;      // [d0][64] and [K][64] per tile
  int with_grad;
  int64_t T, B;              // base tiles (tiles T.. are the lagged ones), frames
  int64_t lag_t;             // reconstruction target row = idx + lag_t
  const float* feat_rows;
  const int64_t* idx;
  const float* w;
  const float* w_lag;
  double mse_scale, head_scale;
  const double* coef;        // [gS1(K), gS2(K*K), gT(K), gS1'(K), gS2'_ii(K)] (NULL: the regulariser is off)
  const float* y_in;         // with_grad: y_tiled of the forward pass
  float* y_out;              // forward: y_tiled [tiles][K][64] (NULL: not wanted)
  float* enc_out;            // forward: enc_tiled [T][k_enc][64] (NULL: not wanted)
  const float* enc_img;      // the latent image a_{n_enc} [tile][k_enc][64]
  int k_enc;
};

// One tile's outputs.  Reconstruction rows go 64 at a time through an LDS transpose of the target rows (read along the features,
// as aeg_gather_kernel reads its input); wave j takes rows j, j + 4, ... of a chunk and the four waves' sums of a frame are
// added in the order 0, 1, 2, 3 (aeg_err_kernel's rule).  The loss pairs and the step counter go with the reconstruction's launch.
__global__ __launch_bounds__(256) void regaeg_out_kernel(RegaegOutArgs a, double* __restrict__ partial, int32_t* __restrict__ step) {
  __shared__ float S[CVF_TILE * kTP];   // [frame][feature] of the target rows
  __shared__ double part[4][CVF_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const bool lagged = tile >= a.T;
  const int64_t t0 = lagged ? tile - a.T : tile;
  const int64_t frame = t0 * CVF_TILE + lane;
  const bool valid = frame < a.B;
  const float wraw = valid ? a.w[frame] : 0.0f;
  const bool do_rec = a.rec.in != nullptr;

  if (do_rec && !lagged) {
    const float* ip = a.rec.in + tile * a.rec.is;
    float* zp = a.rec.zb + tile * a.rec.zs;
    const float s = (float)(2.0 * (double)wraw * a.mse_scale);
    double e = 0.0;
    for (int c0 = 0; c0 < a.d0; c0 += 64) {
#pragma unroll 4
      for (int it = 0; it < 16; ++it) {
        const int fr = wave + 4 * it;
        const int64_t f = t0 * CVF_TILE + fr;
        float v = 0.0f;
        if (f < a.B && c0 + lane < a.d0) {
          const int64_t row = (a.idx != nullptr ? a.idx[f] : f) + a.lag_t;
          v = a.feat_rows[row * a.d0 + c0 + lane];
        }
        S[fr * kTP + lane] = v;
      }
      __syncthreads();
#pragma unroll 4
      for (int it = 0; it < 16; ++it) {
        const int c = wave + 4 * it, i = c0 + c;
        if (i < a.d0) {
          const float o = ip[(int64_t)i * CVF_TILE + lane];
          const float d = o - S[lane * kTP + c];
          if (valid) e += (double)d * (double)d;
          if (a.with_grad) zp[(int64_t)i * CVF_TILE + lane] = valid ? s * d * cvf_act_d1(a.rec.act, o) : 0.0f;
        }
      }
      __syncthreads();
    }
    part[wave][lane] = e;
    if (a.enc_out != nullptr)
      for (int j = wave; j < a.k_enc; j += 4)
        a.enc_out[(t0 * a.k_enc + j) * CVF_TILE + lane] = a.enc_img[(tile * a.k_enc + j) * CVF_TILE + lane];
  } else if (do_rec && a.with_grad) {
    float* zp = a.rec.zb + tile * a.rec.zs;
    for (int i = wave; i < a.d0; i += 4) zp[(int64_t)i * CVF_TILE + lane] = 0.0f;   // no reconstruction error on the lagged rows
  }

  // regulariser head i: its value, and the output gradient of the transfer-operator loss (ae_mfma_kernel's, csrc/ae.hip)
  if (a.head.in != nullptr) {
    const float* ip = a.head.in + tile * a.head.is + lane;
    float* zp = a.head.zb + tile * a.head.zs + lane;
    for (int i = wave; i < a.K; i += 4) {
      const float y = ip[(int64_t)i * CVF_TILE];
      if (a.y_out != nullptr) a.y_out[(tile * a.K + i) * CVF_TILE + lane] = y;
      if (!a.with_grad) continue;
      float zb = 0.0f;
      if (a.coef != nullptr && valid) {
        const float* yb = a.y_in + t0 * a.K * CVF_TILE + lane;
        const float* yl = a.y_in + (a.T + t0) * a.K * CVF_TILE + lane;
        const double g = g64_transfer_grad(a.coef, a.K, i, yb, yl, lagged, wraw, lagged ? a.w_lag[frame] : 0.0f);
        zb = (float)(a.head_scale * g) * cvf_act_d1(a.head.act, y);
      }
      zp[(int64_t)i * CVF_TILE] = zb;
    }
  }

  if (!do_rec || lagged) return;
  __syncthreads();
  if (wave == 0) {
    const double err = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    const double sa = wave_sum((double)wraw * err), sb = wave_sum((double)wraw);
    if (lane == 0) {
      partial[2 * tile] = sa;
      partial[2 * tile + 1] = sb;
      if (step != nullptr && tile == 0) *step += 1;
    }
  }
}

// zbar_{n_enc} += w (gS1_i + sum_j c_ij gS2_ij e_j), c_ii = 2, c_ij = 1, on the base tiles: the gradient of the variance and
// covariance penalties on the latent vector (the latent layer has no activation, so the term adds to zbar as it stands)
__global__ __launch_bounds__(256) void regaeg_enc_kernel(float* __restrict__ zbar, const float* __restrict__ enc_img, int k,
                                                         const float* __restrict__ w, int64_t B, const double* __restrict__ enc_coef) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t frame = tile * CVF_TILE + lane;
  if (frame >= B) return;
  const double wb = (double)w[frame];
  const float* e = enc_img + tile * k * CVF_TILE + lane;
  for (int i = wave; i < k; i += 4) {
    double s = enc_coef[i];
    for (int j = 0; j < k; ++j) s += (j == i ? 2.0 : 1.0) * enc_coef[k + i * k + j] * (double)e[j * CVF_TILE];
    zbar[(tile * k + i) * CVF_TILE + lane] += (float)(wb * s);
  }
}

// ---- scratch, laid out for 2 T tiles whatever the call runs (so that the forward call and the gradient call of one step agree):
// a_0..a_{L-1} ([tile][width][64] each), two ping-pong images of zbar (widest of dims[1..L]; zbar_l and the chain's output sit
// in image l & 1), the slab rows, the base tiles' partial pairs (doubles, 8-byte aligned)
struct RegaegLayout {
  int64_t a[CVF_MAX_LAYERS], zb[2], slab, partial, total;
};

RegaegLayout regaeg_layout(const cvf_mlp_desc* mlp, int64_t T) {
  RegaegLayout L = {};
  const int64_t per = 2 * T * CVF_TILE;
  int64_t pos = 0;
  int wmax = 1;
  for (int l = 0; l < mlp->n_layers; ++l) {
    L.a[l] = pos;
    pos += per * mlp->dims[l];
    wmax = mlp->dims[l + 1] > wmax ? mlp->dims[l + 1] : wmax;
  }
  for (int i = 0; i < 2; ++i) {
    L.zb[i] = pos;
    pos += per * wmax;
  }
  L.slab = pos;
  pos += g64_rows(mlp, 2 * T) * mlp->n_params;
  L.partial = (pos + 1) & ~(int64_t)1;
  L.total = L.partial + 4 * T;
  return L;
}

// aeg_why's limits for the merged chain: dims[L] == dims[0] + K
const char* regaeg_why(const cvf_mlp_desc* mlp, int K, int n_enc_layers, bool with_encoder = true) {
  static thread_local char buf[200];
  if (mlp == nullptr) return "no chain description";
  if (mlp->n_nets != 1) {
    snprintf(buf, sizeof buf, "%d nets: one chain is expected", mlp->n_nets);
    return buf;
  }
  const char* why = g64_why(mlp, mlp->n_layers, G64Chain{2, "layer", "chain", true, true}, buf, sizeof buf);
  if (why != nullptr) return why;
  const int L = mlp->n_layers;
  if (K < 0 || K > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "K = %d regulariser heads: 0 to %d are supported", K, CVF_MAX_NETS);
    return buf;
  }
  if (mlp->dims[L] != mlp->dims[0] + K) {
    snprintf(buf, sizeof buf, "the chain must end in d_0 = %d reconstruction rows + K = %d heads (it has %d outputs)", mlp->dims[0], K,
             mlp->dims[L]);
    return buf;
  }
  if (!with_encoder) return nullptr;
  if (n_enc_layers < 1 || n_enc_layers >= L) {
    snprintf(buf, sizeof buf, "n_enc_layers=%d out of range (1 to %d)", n_enc_layers, L - 1);
    return buf;
  }
  if (mlp->act[n_enc_layers - 1] != CVF_ACT_NONE) return "the encoder's last layer must have no activation";
  if (mlp->dims[n_enc_layers] > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "latent width %d > %d", mlp->dims[n_enc_layers], CVF_MAX_NETS);
    return buf;
  }
  return nullptr;
}

struct RegaegCall {
  const cvf_mlp_desc* mlp;
  const float* theta;
  float* scratch;
  RegaegLayout lay;
  int64_t T, NT;
  hipStream_t s;
  float* A(int l) const { return scratch + lay.a[l]; }              // a_l, l = 0..L-1
  float* Z(int l) const { return scratch + lay.zb[l & 1]; }         // zbar_l, l = 1..L (a_L = the output before regaeg_out_kernel)
  int64_t ts(int l) const { return (int64_t)mlp->dims[l] * CVF_TILE; }
  double* partial() const { return reinterpret_cast<double*>(scratch + lay.partial); }
  int layer(const AegLayerArgs& a) const {
    hipLaunchKernelGGL(aeg_layer_kernel, dim3((unsigned)NT, (unsigned)((a.M + 63) / 64)), dim3(256), 0, s, theta, a);
    return cvf_check_launch("aeg_layer_kernel");
  }
};

int regaeg_begin(RegaegCall& c, const char* who, const cvf_mlp_desc* mlp, const float* theta, int64_t B, int64_t lag_target,
                 int64_t lag_input, int K, int n_enc_layers, float* scratch, void* stream) {
  const char* why = regaeg_why(mlp, K, n_enc_layers);
  CVF_REQUIRE(why == nullptr, "%s: %s", who, why);
  CVF_REQUIRE(lag_target >= 0 && lag_input >= 0, "%s: negative lag", who);
  c.T = cvf_ntiles(B);
  CVF_REQUIRE(2 * c.T <= 0x7fffffff, "%s: %lld frames are more than one call takes", who, (long long)B);
  c.NT = (K > 0 && lag_input > 0) ? 2 * c.T : c.T;
  c.mlp = mlp;
  c.theta = theta;
  c.scratch = scratch;
  c.lay = regaeg_layout(mlp, c.T);
  c.s = (hipStream_t)stream;
  return 0;
}

// gather + the chain forward: a_1..a_{L-1}, the output in Z(L)
int regaeg_chain_forward(const RegaegCall& c, const float* feat_rows, const int64_t* idx, int64_t B, int64_t lag_input) {
  const cvf_mlp_desc* mlp = c.mlp;
  const int L = mlp->n_layers;
  hipLaunchKernelGGL(aeg_gather_kernel, dim3((unsigned)c.NT), dim3(256), 0, c.s, feat_rows, idx, B, mlp->dims[0], c.A(0), c.T, lag_input);
  if (cvf_check_launch("aeg_gather_kernel")) return -1;
  for (int l = 0; l < L; ++l) {
    AegLayerArgs a = {};
    a.w_off = mlp->w_off[0][l];
    a.b_off = mlp->b_off[0][l];
    a.ldw = mlp->dims[l];
    a.M = mlp->dims[l + 1];
    a.K = mlp->dims[l];
    a.epi = EPI_ACT;
    a.act = mlp->act[l];
    a.x = c.A(l);
    a.xs = c.ts(l);
    a.out = l + 1 < L ? c.A(l + 1) : c.Z(L);
    a.os = c.ts(l + 1);
    if (c.layer(a)) return -1;
  }
  return 0;
}

int regaeg_out(const RegaegCall& c, RegaegOutArgs o, int32_t* step_count) {
  const cvf_mlp_desc* mlp = c.mlp;
  const int L = mlp->n_layers;
  o.d0 = mlp->dims[0];
  o.T = c.T;
  // [reconstruction | y_1..y_K] in the one image Z(L), in place
  o.rec = RegaegView{c.Z(L), c.Z(L), c.ts(L), c.ts(L), mlp->act[L - 1]};
  o.head = o.rec;
  o.head.in = o.head.zb = c.Z(L) + (int64_t)o.d0 * CVF_TILE;
  hipLaunchKernelGGL(regaeg_out_kernel, dim3((unsigned)c.NT), dim3(256), 0, c.s, o, c.partial(), step_count);
  return cvf_check_launch("regaeg_out_kernel");
}

int regaeg_backward_impl(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                         int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                         double head_scale, const float* y_tiled, const double* coef, int n_enc_layers, const double* enc_coef,
                         float* scratch, float* grad, const float* mask, int32_t* step_count, const cvf_adam_args* adam,
                         void* stream, bool reuse) {
  const char* who = "cvf_regae_general_backward";
  RegaegCall c;
  if (regaeg_begin(c, who, mlp, theta, B, lag_target, lag_input, K, n_enc_layers, scratch, stream)) return -1;
  CVF_REQUIRE(theta && feat_rows && w && scratch && grad && B > 0, "%s: bad argument", who);
  CVF_REQUIRE(coef == nullptr || (K > 0 && lag_input > 0 && w_lag && y_tiled),
              "%s: the regulariser needs heads, lag_input > 0, w_lag and y_tiled", who);
  CVF_REQUIRE(adam == nullptr || (adam->theta && adam->m && adam->v && adam->step_count), "%s: incomplete adam arguments", who);
  const int L = mlp->n_layers;
  if (!reuse && regaeg_chain_forward(c, feat_rows, idx, B, lag_input)) return -1;
  RegaegOutArgs o = {};
  o.K = K;
  o.with_grad = 1;
  o.B = B;
  o.lag_t = lag_target;
  o.feat_rows = feat_rows;
  o.idx = idx;
  o.w = w;
  o.w_lag = w_lag;
  o.mse_scale = mse_scale;
  o.head_scale = head_scale;
  o.coef = coef;
  o.y_in = y_tiled;
  if (regaeg_out(c, o, step_count)) return -1;

  const int R = (int)g64_rows(mlp, c.NT);
  float* slab = scratch + c.lay.slab;
  for (int l = L - 1; l >= 0; --l) {
    {  // layer l's gradient from zbar_{l+1} and a_l
      AegGradArgs g = {};
      g.w_off = mlp->w_off[0][l];
      g.b_off = mlp->b_off[0][l];
      g.Mo = mlp->dims[l + 1];
      g.Ki = mlp->dims[l];
      g.n_tiles = c.NT;
      g.B = c.NT * CVF_TILE;   // every frame counts: the padded ones carry zero adjoints
      g.rows = R;
      g.n_params = mlp->n_params;
      g.z = c.Z(l + 1);
      g.zs = c.ts(l + 1);
      g.h = c.A(l);
      g.hs = c.ts(l);
      const int nb = ((g.Mo + 63) / 64) * ((g.Ki + 1 + 63) / 64);
      hipLaunchKernelGGL(aeg_wgrad_kernel, dim3((unsigned)R, (unsigned)nb), dim3(256), 0, c.s, g, slab);
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
    a.x = c.Z(l + 1);
    a.xs = c.ts(l + 1);
    a.out = c.Z(l);
    a.os = c.ts(l);
    a.eh = c.A(l);
    a.es = c.ts(l);
    if (c.layer(a)) return -1;
    if (enc_coef != nullptr && l == n_enc_layers) {
      hipLaunchKernelGGL(regaeg_enc_kernel, dim3((unsigned)c.T), dim3(256), 0, c.s, c.Z(l), c.A(l), mlp->dims[l], w, B, enc_coef);
      if (cvf_check_launch("regaeg_enc_kernel")) return -1;
    }
  }
  cvf_adam_args ad;
  if (adam != nullptr) {
    ad = *adam;
    ad.mlp = nullptr;      // no MFMA fragment copy to refresh
    ad.packed = nullptr;
  }
  return cvf_slab_reduce_impl(slab, R, mlp->n_params, grad, mask, adam != nullptr ? &ad : nullptr, stream);
}

// ---- decoder and regulariser nets of different depths (cvf_regae_ragged_*; core._RegRaggedFlatParams builds the chain).  Behind
// the encoder the deeper group's rows come first in every merged layer, so that once the shallower group has ended (in image
// ls = n_enc + min(Ld, Lr), as its last `fin` rows: d_0 reconstruction rows or K heads, without activation) the next layer reads
// the live prefix of that image: its matrix is dense [dims[ls + 1]][dims[ls] - fin], and every other layer's [dims[l + 1]][dims[l]].
// The finished rows stay in the saved image a_ls; their adjoint is seeded into zbar_ls after the transposed product that writes
// the live rows of zbar_ls and before the weight-gradient launch that reads all of it.
struct RagShape {
  int L, ne, ls, fin;
  bool dec_deep;   // the decoder is the deeper group: the chain ends in the reconstruction, the heads end in image ls
  int in(const cvf_mlp_desc* mlp, int l) const { return l == ls ? mlp->dims[l] - fin : mlp->dims[l]; }   // columns of W_l
};

// regaeg_why's limits for the ragged chain; fills `sh` when the answer is NULL
const char* rag_why(const cvf_mlp_desc* mlp, int K, int n_enc, int n_dec, int n_reg, RagShape* sh) {
  static thread_local char buf[200];
  if (mlp == nullptr) return "no chain description";
  if (mlp->n_nets != 1) {
    snprintf(buf, sizeof buf, "%d nets: one chain is expected", mlp->n_nets);
    return buf;
  }
  const char* why = g64_why(mlp, mlp->n_layers, G64Chain{2, "layer", "chain", false, true}, buf, sizeof buf);
  if (why != nullptr) return why;
  const int L = mlp->n_layers;
  if (K < 1 || K > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "K = %d regulariser heads: 1 to %d are supported", K, CVF_MAX_NETS);
    return buf;
  }
  if (n_dec < 1 || n_reg < 1 || n_dec == n_reg) {
    snprintf(buf, sizeof buf, "decoder and regulariser nets of %d and %d layers: two different depths >= 1 are expected (equal depths "
             "take cvf_regae_general_*)", n_dec, n_reg);
    return buf;
  }
  const int deep = n_dec > n_reg ? n_dec : n_reg, shallow = n_dec > n_reg ? n_reg : n_dec;
  if (n_enc < 1 || n_enc + deep != L) {
    snprintf(buf, sizeof buf, "n_enc_layers=%d + max(%d, %d) is not the chain's %d layers", n_enc, n_dec, n_reg, L);
    return buf;
  }
  if (mlp->act[n_enc - 1] != CVF_ACT_NONE) return "the encoder's last layer must have no activation";
  if (mlp->dims[n_enc] > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "latent width %d > %d", mlp->dims[n_enc], CVF_MAX_NETS);
    return buf;
  }
  RagShape s;
  s.L = L;
  s.ne = n_enc;
  s.ls = n_enc + shallow;
  s.dec_deep = n_dec > n_reg;
  s.fin = s.dec_deep ? K : mlp->dims[0];
  const int last = s.dec_deep ? mlp->dims[0] : K;
  if (mlp->dims[L] != last) {
    snprintf(buf, sizeof buf, "the chain must end in the deeper group's %d outputs (it has %d)", last, mlp->dims[L]);
    return buf;
  }
  if (mlp->dims[s.ls] <= s.fin) {
    snprintf(buf, sizeof buf, "layer %d is %d wide: the shallower group's %d outputs leave no row for the deeper one", s.ls,
             mlp->dims[s.ls], s.fin);
    return buf;
  }
  int64_t n = 0;
  for (int l = 0; l < L; ++l) n += (int64_t)mlp->dims[l + 1] * (s.in(mlp, l) + 1);
  if (n != mlp->n_params) return "the flat buffer holds parameters outside the chain";
  for (int l = 0; l < L; ++l)
    if (mlp->w_off[0][l] < 0 || mlp->w_off[0][l] + (int64_t)mlp->dims[l + 1] * s.in(mlp, l) > n || mlp->b_off[0][l] < 0 ||
        mlp->b_off[0][l] + (int64_t)mlp->dims[l + 1] > n)
      return "a layer's parameters lie outside the flat buffer";
  if (sh != nullptr) *sh = s;
  return nullptr;
}

struct RagCall {
  RegaegCall c;
  RagShape sh;
  int K;
  int in(int l) const { return sh.in(c.mlp, l); }
  // the finished rows of image ls (values in a_ls, adjoint in zbar_ls) and the chain's last layer (Z(L), in place)
  RegaegView finished() const {
    const int64_t off = (int64_t)in(sh.ls) * CVF_TILE;
    return RegaegView{c.A(sh.ls) + off, c.Z(sh.ls) + off, c.ts(sh.ls), c.ts(sh.ls), CVF_ACT_NONE};
  }
  RegaegView last() const { return RegaegView{c.Z(sh.L), c.Z(sh.L), c.ts(sh.L), c.ts(sh.L), c.mlp->act[sh.L - 1]}; }
  int out(RegaegOutArgs o, bool rec, bool head, int32_t* step_count) const {
    o.d0 = c.mlp->dims[0];
    o.K = K;
    o.T = c.T;
    if (rec) o.rec = sh.dec_deep ? last() : finished();
    if (head) o.head = sh.dec_deep ? finished() : last();
    hipLaunchKernelGGL(regaeg_out_kernel, dim3((unsigned)c.NT), dim3(256), 0, c.s, o, c.partial(), step_count);
    return cvf_check_launch("regaeg_out_kernel");
  }
};

int rag_begin(RagCall& r, const char* who, const cvf_mlp_desc* mlp, const float* theta, int64_t B, int64_t lag_target,
              int64_t lag_input, int K, int n_enc, int n_dec, int n_reg, float* scratch, void* stream) {
  const char* why = rag_why(mlp, K, n_enc, n_dec, n_reg, &r.sh);
  CVF_REQUIRE(why == nullptr, "%s: %s", who, why);
  CVF_REQUIRE(lag_target >= 0 && lag_input >= 0, "%s: negative lag", who);
  RegaegCall& c = r.c;
  c.T = cvf_ntiles(B);
  CVF_REQUIRE(2 * c.T <= 0x7fffffff, "%s: %lld frames are more than one call takes", who, (long long)B);
  c.NT = lag_input > 0 ? 2 * c.T : c.T;
  c.mlp = mlp;
  c.theta = theta;
  c.scratch = scratch;
  c.lay = regaeg_layout(mlp, c.T);
  c.s = (hipStream_t)stream;
  r.K = K;
  return 0;
}

// gather + the chain forward: a_1..a_{L-1} (a_ls with the finished rows), the output in Z(L).  The layer that ends the shallower
// group is two launches over its row ranges: the live rows take the layer's activation, the finished rows none.
int rag_chain_forward(const RagCall& r, const float* feat_rows, const int64_t* idx, int64_t B, int64_t lag_input) {
  const RegaegCall& c = r.c;
  const cvf_mlp_desc* mlp = c.mlp;
  const int L = mlp->n_layers;
  hipLaunchKernelGGL(aeg_gather_kernel, dim3((unsigned)c.NT), dim3(256), 0, c.s, feat_rows, idx, B, mlp->dims[0], c.A(0), c.T, lag_input);
  if (cvf_check_launch("aeg_gather_kernel")) return -1;
  for (int l = 0; l < L; ++l) {
    const int ki = r.in(l), mo = mlp->dims[l + 1];
    const int live = l + 1 == r.sh.ls ? mo - r.sh.fin : mo;
    for (int r0 = 0; r0 < mo; r0 = r0 == 0 ? live : mo) {   // rows [0, live), then [live, mo) when there are any
      AegLayerArgs a = {};
      a.w_off = mlp->w_off[0][l] + r0 * ki;
      a.b_off = mlp->b_off[0][l] + r0;
      a.ldw = ki;
      a.M = r0 == 0 ? live : mo - live;
      a.K = ki;
      a.epi = EPI_ACT;
      a.act = r0 == 0 ? mlp->act[l] : CVF_ACT_NONE;
      a.x = c.A(l);
      a.xs = c.ts(l);
      a.out = (l + 1 < L ? c.A(l + 1) : c.Z(L)) + (int64_t)r0 * CVF_TILE;
      a.os = c.ts(l + 1);
      if (c.layer(a)) return -1;
    }
  }
  return 0;
}

int rag_backward_impl(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                      int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                      double head_scale, const float* y_tiled, const double* coef, int n_enc, int n_dec, int n_reg,
                      const double* enc_coef, float* scratch, float* grad, const float* mask, int32_t* step_count,
                      const cvf_adam_args* adam, void* stream, bool reuse) {
  const char* who = "cvf_regae_ragged_backward";
  RagCall r;
  if (rag_begin(r, who, mlp, theta, B, lag_target, lag_input, K, n_enc, n_dec, n_reg, scratch, stream)) return -1;
  const RegaegCall& c = r.c;
  CVF_REQUIRE(theta && feat_rows && w && scratch && grad && B > 0, "%s: bad argument", who);
  CVF_REQUIRE(coef == nullptr || (lag_input > 0 && w_lag && y_tiled), "%s: the regulariser needs lag_input > 0, w_lag and y_tiled", who);
  CVF_REQUIRE(adam == nullptr || (adam->theta && adam->m && adam->v && adam->step_count), "%s: incomplete adam arguments", who);
  const int L = mlp->n_layers;
  if (!reuse && rag_chain_forward(r, feat_rows, idx, B, lag_input)) return -1;
  RegaegOutArgs o = {};
  o.with_grad = 1;
  o.B = B;
  o.lag_t = lag_target;
  o.feat_rows = feat_rows;
  o.idx = idx;
  o.w = w;
  o.w_lag = w_lag;
  o.mse_scale = mse_scale;
  o.head_scale = head_scale;
  o.coef = coef;
  o.y_in = y_tiled;
  // zbar_L: the deeper group's seed (the step counter goes with the reconstruction's launch, whichever it is)
  if (r.out(o, r.sh.dec_deep, !r.sh.dec_deep, r.sh.dec_deep ? step_count : nullptr)) return -1;

  const int R = (int)g64_rows(mlp, c.NT);
  float* slab = scratch + c.lay.slab;
  for (int l = L - 1; l >= 0; --l) {
    {  // layer l's gradient from zbar_{l+1} and the rows of a_l it reads
      AegGradArgs g = {};
      g.w_off = mlp->w_off[0][l];
      g.b_off = mlp->b_off[0][l];
      g.Mo = mlp->dims[l + 1];
      g.Ki = r.in(l);
      g.n_tiles = c.NT;
      g.B = c.NT * CVF_TILE;   // every frame counts: the padded ones carry zero adjoints
      g.rows = R;
      g.n_params = mlp->n_params;
      g.z = c.Z(l + 1);
      g.zs = c.ts(l + 1);
      g.h = c.A(l);
      g.hs = c.ts(l);
      const int nb = ((g.Mo + 63) / 64) * ((g.Ki + 1 + 63) / 64);
      hipLaunchKernelGGL(aeg_wgrad_kernel, dim3((unsigned)R, (unsigned)nb), dim3(256), 0, c.s, g, slab);
      if (cvf_check_launch("aeg_wgrad_kernel")) return -1;
    }
    if (l == 0) break;
    // rows [0, in(l)) of zbar_l = (W_l^T zbar_{l+1}) .* act'_{l-1}(a_l)
    AegLayerArgs a = {};
    a.w_off = mlp->w_off[0][l];
    a.b_off = -1;
    a.ldw = r.in(l);
    a.trans = 1;
    a.M = r.in(l);
    a.K = mlp->dims[l + 1];
    a.epi = EPI_BWD;
    a.act = mlp->act[l - 1];
    a.x = c.Z(l + 1);
    a.xs = c.ts(l + 1);
    a.out = c.Z(l);
    a.os = c.ts(l);
    a.eh = c.A(l);
    a.es = c.ts(l);
    if (c.layer(a)) return -1;
    // the finished rows of zbar_ls: the shallower group's seed
    if (l == r.sh.ls && r.out(o, !r.sh.dec_deep, r.sh.dec_deep, r.sh.dec_deep ? nullptr : step_count)) return -1;
    if (enc_coef != nullptr && l == n_enc) {
      hipLaunchKernelGGL(regaeg_enc_kernel, dim3((unsigned)c.T), dim3(256), 0, c.s, c.Z(l), c.A(l), mlp->dims[l], w, B, enc_coef);
      if (cvf_check_launch("regaeg_enc_kernel")) return -1;
    }
  }
  cvf_adam_args ad;
  if (adam != nullptr) {
    ad = *adam;
    ad.mlp = nullptr;      // no MFMA fragment copy to refresh
    ad.packed = nullptr;
  }
  return cvf_slab_reduce_impl(slab, R, mlp->n_params, grad, mask, adam != nullptr ? &ad : nullptr, stream);
}

}  // namespace

extern "C" int cvf_regae_ragged_supported(const cvf_mlp_desc* mlp, int K, int n_enc_layers, int n_dec_layers, int n_reg_layers) {
  const char* why = rag_why(mlp, K, n_enc_layers, n_dec_layers, n_reg_layers, nullptr);
  if (why != nullptr) {
    cvf_set_error("cvf_regae_ragged: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_regae_ragged_scratch_floats(const cvf_mlp_desc* mlp, int64_t B, int K, int n_enc_layers, int n_dec_layers,
                                                   int n_reg_layers) {
  if (B < 1 || rag_why(mlp, K, n_enc_layers, n_dec_layers, n_reg_layers, nullptr) != nullptr) return 0;
  return regaeg_layout(mlp, cvf_ntiles(B)).total;
}

extern "C" int cvf_regae_ragged_forward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx,
                                        int64_t B, int64_t lag_target, int64_t lag_input, int K, const float* w, float* scratch,
                                        float* y_tiled, int n_enc_layers, int n_dec_layers, int n_reg_layers, float* enc_tiled,
                                        double* out2, void* stream) {
  const char* who = "cvf_regae_ragged_forward";
  RagCall r;
  if (rag_begin(r, who, mlp, theta, B, lag_target, lag_input, K, n_enc_layers, n_dec_layers, n_reg_layers, scratch, stream)) return -1;
  CVF_REQUIRE(theta && feat_rows && w && scratch && out2 && B > 0 && y_tiled, "%s: bad argument", who);
  if (rag_chain_forward(r, feat_rows, idx, B, lag_input)) return -1;
  RegaegOutArgs o = {};
  o.B = B;
  o.lag_t = lag_target;
  o.feat_rows = feat_rows;
  o.idx = idx;
  o.w = w;
  o.y_out = y_tiled;
  o.enc_out = enc_tiled;
  o.enc_img = r.c.A(n_enc_layers);
  o.k_enc = mlp->dims[n_enc_layers];
  if (r.out(o, true, true, nullptr)) return -1;
  hipLaunchKernelGGL(aeg_loss_sum_kernel, dim3(1), dim3(64), 0, r.c.s, r.c.partial(), r.c.T, out2);
  return cvf_check_launch("aeg_loss_sum_kernel");
}

extern "C" int cvf_regae_ragged_backward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx,
                                         int64_t B, int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag,
                                         double mse_scale, double head_scale, const float* y_tiled, const double* coef,
                                         int n_enc_layers, int n_dec_layers, int n_reg_layers, const double* enc_coef, float* scratch,
                                         float* grad, const float* mask, int32_t* step_count, const cvf_adam_args* adam,
                                         void* stream) {
  return rag_backward_impl(mlp, theta, feat_rows, idx, B, lag_target, lag_input, K, w, w_lag, mse_scale, head_scale, y_tiled, coef,
                           n_enc_layers, n_dec_layers, n_reg_layers, enc_coef, scratch, grad, mask, step_count, adam, stream, false);
}

extern "C" int cvf_regae_ragged_backward_reuse(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx,
                                               int64_t B, int64_t lag_target, int64_t lag_input, int K, const float* w,
                                               const float* w_lag, double mse_scale, double head_scale, const float* y_tiled,
                                               const double* coef, int n_enc_layers, int n_dec_layers, int n_reg_layers,
                                               const double* enc_coef, float* scratch, float* grad, const float* mask,
                                               int32_t* step_count, const cvf_adam_args* adam, void* stream) {
  return rag_backward_impl(mlp, theta, feat_rows, idx, B, lag_target, lag_input, K, w, w_lag, mse_scale, head_scale, y_tiled, coef,
                           n_enc_layers, n_dec_layers, n_reg_layers, enc_coef, scratch, grad, mask, step_count, adam, stream, true);
}

extern "C" int cvf_regae_general_supported(const cvf_mlp_desc* mlp, int K, int n_enc_layers) {
  const char* why = regaeg_why(mlp, K, n_enc_layers);
  if (why != nullptr) {
    cvf_set_error("cvf_regae_general: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_regae_general_scratch_floats(const cvf_mlp_desc* mlp, int64_t B) {
  if (mlp == nullptr || B < 1 || mlp->n_layers < 2 || mlp->n_layers > CVF_MAX_LAYERS) return 0;
  // (the sizes do not depend on where the encoder ends)
  if (regaeg_why(mlp, mlp->dims[mlp->n_layers] - mlp->dims[0], 0, false) != nullptr) return 0;
  return regaeg_layout(mlp, cvf_ntiles(B)).total;
}

extern "C" int cvf_regae_general_forward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx,
                                         int64_t B, int64_t lag_target, int64_t lag_input, int K, const float* w, float* scratch,
                                         float* y_tiled, int n_enc_layers, float* enc_tiled, double* out2, void* stream) {
  const char* who = "cvf_regae_general_forward";
  RegaegCall c;
  if (regaeg_begin(c, who, mlp, theta, B, lag_target, lag_input, K, n_enc_layers, scratch, stream)) return -1;
  CVF_REQUIRE(theta && feat_rows && w && scratch && out2 && B > 0 && (K == 0 || y_tiled), "%s: bad argument", who);
  if (regaeg_chain_forward(c, feat_rows, idx, B, lag_input)) return -1;
  RegaegOutArgs o = {};
  o.K = K;
  o.B = B;
  o.lag_t = lag_target;
  o.feat_rows = feat_rows;
  o.idx = idx;
  o.w = w;
  o.y_out = K > 0 ? y_tiled : nullptr;
  o.enc_out = enc_tiled;
  o.enc_img = c.A(n_enc_layers);
  o.k_enc = mlp->dims[n_enc_layers];
  if (regaeg_out(c, o, nullptr)) return -1;
  hipLaunchKernelGGL(aeg_loss_sum_kernel, dim3(1), dim3(64), 0, c.s, c.partial(), c.T, out2);
  return cvf_check_launch("aeg_loss_sum_kernel");
}

extern "C" int cvf_regae_general_backward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx,
                                          int64_t B, int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag,
                                          double mse_scale, double head_scale, const float* y_tiled, const double* coef,
                                          int n_enc_layers, const double* enc_coef, float* scratch, float* grad, const float* mask,
                                          int32_t* step_count, const cvf_adam_args* adam, void* stream) {
  return regaeg_backward_impl(mlp, theta, feat_rows, idx, B, lag_target, lag_input, K, w, w_lag, mse_scale, head_scale, y_tiled, coef,
                              n_enc_layers, enc_coef, scratch, grad, mask, step_count, adam, stream, false);
}

extern "C" int cvf_regae_general_backward_reuse(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows,
                                                const int64_t* idx, int64_t B, int64_t lag_target, int64_t lag_input, int K,
                                                const float* w, const float* w_lag, double mse_scale, double head_scale,
                                                const float* y_tiled, const double* coef, int n_enc_layers, const double* enc_coef,
                                                float* scratch, float* grad, const float* mask, int32_t* step_count,
                                                const cvf_adam_args* adam, void* stream) {
  return regaeg_backward_impl(mlp, theta, feat_rows, idx, B, lag_target, lag_input, K, w, w_lag, mse_scale, head_scale, y_tiled, coef,
                              n_enc_layers, enc_coef, scratch, grad, mask, step_count, adam, stream, true);
}
