// K4a / K4b for eigenfunction nets of ANY shape (cvf_ef_general_*): 1 to 11 hidden layers of any widths, one of the
// activation codes of include/cvf.h after each hidden layer, scalar output, k <= CVF_MAX_NETS nets side by side
// (colvarsfinder.nn.EigenFunctions, nn.py:242-293).  The instance kernels of ef_mfma.hip keep a whole 64-frame chain in
// registers, which ties them to compiled widths; here every product of the step is ONE launch over all tiles and nets:
//
//   efg_layer_kernel  [M x K] x [K x 64 frames] per (tile, 64-row block, net) with the weights W (or W^T) as the A operand
//                     and the activations as the B operand, an elementwise transform of B on its way to LDS (sigma'(h) .* x)
//                     and the activation or the adjoint's combination fused into the epilogue;
//   efg_wgrad_kernel  the weight-gradient products, K = frames: [zbar_l | d_l] x [h_{l-1} ; 1 | tdot_{l-1} ; 0]^T, the
//                     tiles split over a fixed number of slab rows (row rho sums tiles rho, rho + R, ... in that order);
//   efg_coef_kernel   the per-frame adjoints of y (alpha) and of q.g (gamma) from the loss coefficients;
//   efg_top_kernel    the adjoints of the last hidden layer (its "incoming" product W_NH^T is a broadcast).
//
// Mathematics (net i, hidden layers l = 0..NH-1, output layer NH, h_{-1} = r, sigma' / sigma'' through the output h):
//   forward     z_l = W_l h_{l-1} + b_l, h_l = sigma(z_l), y = W_NH h_{NH-1} + b_NH
//   g = dy/dr   u_{NH-1} = W_NH^T, delta_l = sigma'_l .* u_l, u_{l-1} = W_l^T delta_l, g = u_{-1}
//   tangent     zdot_0 = W_0 q, zdot_l = W_l (sigma'_{l-1} .* zdot_{l-1})            (tdot_l = sigma'_l .* zdot_l)
//   adjoints    zbar_{NH-1} = sigma'_{NH-1} .* (alpha W_NH^T) + gamma sigma''_{NH-1} .* zdot_{NH-1} .* u_{NH-1}
//               zbar_{l-1}  = sigma'_{l-1} .* (W_l^T zbar_l) + gamma sigma''_{l-1} .* zdot_{l-1} .* u_{l-1},  d_l = gamma sigma'_l .* u_l
//   gradient    dW_l = sum_frames zbar_l (x) h_{l-1} + d_l (x) tdot_{l-1},  db_l = sum_frames zbar_l   (zbar_NH = alpha, d_NH = gamma)
// (the formula of ef_mfma.hip's header; transfer mode has gamma = 0 and no g / tangent).
//
// All products run on v_mfma_f32_16x16x4_f32 (the 64 x 64 core of csrc/cvf_gemm64.hpp): fp32 operands, fp32 accumulation.
// The hand-off between layers goes through the `saved` buffer in HBM (layout: efg_layout).  No atomics: every slab entry is
// written by one thread, and the sum order of every entry is fixed by the grid, so two runs on the same inputs give the same bits.
//
// A SHARED TRUNK (cvf_ef_general_shared_*, generator mode): the k nets have their first n_shared Linear
// layers in common - w_off[i][l] and b_off[i][l] are the same for every net i when l < n_shared, and the flat buffer holds those
// blocks once (RegAutoEncoderTask: the chains regulariser_i o encoder, and the rows of the encoder's last layer).  Then
//   h_l, l < n_shared  does not depend on the net: its forward launch has ONE net in grid z and writes one image, which every
//                      later launch reads through a view of net stride 0;
//   u, zdot, zbar, d   of the shared layers depend on the head and stay per net (grid z = k, the shared weights read in place);
//   dW_l, l < n_shared = sum over the nets of the per-net products: one launch with one net in grid z, whose block walks, per
//                      tile, the nets 0..k-1 in order into one accumulator and writes the slab entry once, at the shared offset.
// n_shared = 0 is the launch list of the plain entries.
//
// THE SAME IN TRANSFER MODE (cvf_ef_general_shared_transfer_*; n_tiles = 2T: the frames, then their lagged partners).  There is no
// tangent chain and no gamma term, so the only per-net quantity of a shared layer is its adjoint, and the adjoint that enters the
// trunk is a sum over the nets - the trunk back-propagates ONCE:
//   heads            zbar_l, l >= n_shared, per net (EPI_BWD_TR, grid z = k), as on the plain route;
//   the boundary     zbar_{ns-1} = sigma'(h_{ns-1}) .* sum_i W_{ns,i}^T zbar_{ns,i}: ONE launch (eftr_trunk_sum_kernel, csrc/ef_general_sum.hip) whose block
//                    walks the nets 0..k-1 in that order into one accumulator and writes one image;
//                    n_shared = NH (the heads are output rows only): the sum belongs to the top step,
//                    zbar_{NH-1} = sigma'(h_{NH-1}) .* sum_i alpha_i W_{NH,i}^T (eftr_top_sum_kernel);
//   below it         one chain, grid z = 1 (efg_layer_kernel, EPI_BWD_TR, the shared weights in place);
//   dW_l, l < ns     ONE product from the summed zbar_l (nets = 1, grid z = 1), written once at the shared offset of the slab row.
// `saved` = 64 n_tiles (sum_{l<ns} d_l + k (sum_{l>=ns} d_l + 2 max_l d_l + 1)) floats over the hidden widths d_l: the trunk's h_l
// once, the heads' h_l per net, two ping-pong images of zbar (a shared layer's single image lies in the same two), alpha.
// (The two summing kernels carry their own prefix: the four efg_ kernels above are unchanged, in code and in resources.)
#include "cvf_gemm64.hpp"
#include "ef_general_sum.hpp"

namespace {

// a tiled tensor over (net, tile, row, lane): element = p[net * ns + tile * ts + row * 64 + lane]
struct EfgView {
  float* p;
  int64_t ts, ns;
};

__device__ __forceinline__ float* at(const EfgView& v, int net, int64_t tile, int row) {
  return v.p + net * v.ns + tile * v.ts + (int64_t)row * CVF_TILE;
}

enum { EPI_STORE = 0, EPI_ACT = 1, EPI_BWD_GEN = 2, EPI_BWD_TR = 3 };

struct EfgLayerArgs {
  int layer;     // Linear layer whose weights form the A operand
  int trans;     // 0: A = W_layer [M = dims[layer+1]][K = dims[layer]];  1: A = W_layer^T [M = dims[layer]][K = dims[layer+1]]
  int M, K;
  int bias;      // add b_layer in the epilogue (EPI_STORE / EPI_ACT)
  int epi;
  int act_x;     // B operand = sigma'(xh) .* x with this activation's sigma' (xh.p != NULL)
  int act_e;     // activation of the epilogue (EPI_ACT: sigma; EPI_BWD_*: sigma', sigma'' of eh)
  int x_bcast;   // B operand row k = W_{n_layers-1}[0][k] for every frame (u_{NH-1} = W_NH^T) instead of x
  EfgView x, xh, out, eh, eu, gam;
};

// out[m][frame] (64 x 64 block) = A[m][:] . op(B)[:][frame] for one (tile, row block, net)
__global__ __launch_bounds__(256) void efg_layer_kernel(cvf_mlp_desc mlp, const float* __restrict__ theta, EfgLayerArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kKC * kPitch];   // [k][m]
  __shared__ __attribute__((aligned(16))) float Bs[kKC * kPitch];   // [k][frame]
  const G64Thread t = g64_thread();
  const int64_t tile = blockIdx.x;
  const int m0 = blockIdx.y * 64, net = blockIdx.z;
  const float* xb = a.x_bcast ? theta + mlp.w_off[net][mlp.n_layers - 1] : nullptr;
  const float* xp = a.x_bcast ? nullptr : at(a.x, net, tile, 0);
  const float* hp = a.xh.p != nullptr ? at(a.xh, net, tile, 0) : nullptr;

  f32x4 acc[2][2];
  g64_layer_product(As, Bs, theta + mlp.w_off[net][a.layer], mlp.dims[a.layer], a.trans, m0, a.M, a.K, t, acc, [&](int k) {
    float bv = xb != nullptr ? xb[k] : xp[(int64_t)k * CVF_TILE + t.lane];
    if (hp != nullptr) bv *= cvf_act_d1(a.act_x, hp[(int64_t)k * CVF_TILE + t.lane]);
    return bv;
  });

  const float* bias = a.bias ? theta + mlp.b_off[net][a.layer] : nullptr;
  const float* gp = a.epi == EPI_BWD_GEN ? at(a.gam, net, tile, 0) : nullptr;
  g64_walk(acc, t, [&](int row, int f, float v) {
    const int m = m0 + row;
    if (m >= a.M) return;
    float* o = at(a.out, net, tile, m) + f;
    if (a.epi == EPI_STORE || a.epi == EPI_ACT) {
      if (bias != nullptr) v += bias[m];
      *o = a.epi == EPI_ACT ? cvf_act(a.act_e, v) : v;
    } else {
      const float h = at(a.eh, net, tile, m)[f];
      const float s1 = cvf_act_d1(a.act_e, h);
      if (a.epi == EPI_BWD_TR) {
        *o = s1 * v;
      } else {   // o holds zdot (read, then overwritten by zbar); eu holds u (overwritten by d)
        float* up = at(a.eu, net, tile, m) + f;
        const float g = gp[f], u = *up, zd = *o;
        *o = s1 * v + g * cvf_act_d2(a.act_e, h) * zd * u;
        *up = g * s1 * u;
      }
    }
  });
}

struct EfgGradArgs {
  int layer;        // Linear layer whose gradient this launch forms: C [Mo = dims[layer+1]][Ki + 1 = dims[layer] + 1]
  int Mo, Ki;
  int64_t n_tiles, T, B;
  int rows;         // slab rows R: row rho sums tiles rho, rho + R, ... in that order
  int act_b2;       // b2h.p != NULL: second B operand = sigma'(b2h) .* b2
  int64_t n_params;
  int nets;         // nets whose products this block sums, blockIdx.z onwards: 1, or k for a shared layer (grid z = 1)
  EfgView a1, b1, a2, b2, b2h;   // a2.p == NULL: one part (transfer mode)
};

__global__ __launch_bounds__(256) void efg_wgrad_kernel(const cvf_mlp_desc mlp, EfgGradArgs a, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float As[64 * kGP];   // [out row][frame]
  __shared__ __attribute__((aligned(16))) float Bs[64 * kGP];   // [in column][frame]
  const int lane = threadIdx.x & 63, net0 = blockIdx.z;
  const int per = a.a2.p != nullptr ? 2 : 1, sh = per - 1;   // part p: net net0 + (p >> sh), that net's part p & sh
  float* row = slab + (int64_t)blockIdx.x * a.n_params;
  g64_wgrad_block<true>(
      As, Bs, a.Mo, a.Ki, a.n_tiles, a.T, a.B, a.rows, per * a.nets, row + mlp.w_off[net0][a.layer],
      row + mlp.b_off[net0][a.layer],
      [&](int64_t tile, int part, int o) { return at((part & sh) == 0 ? a.a1 : a.a2, net0 + (part >> sh), tile, o)[lane]; },
      [&](int64_t tile, int part, int i) {   // the tangent part: sigma'(b2h) .* b2
        const int net = net0 + (part >> sh), sub = part & sh;
        float x = at(sub == 0 ? a.b1 : a.b2, net, tile, i)[lane];
        if (sub == 1 && a.b2h.p != nullptr) x *= cvf_act_d1(a.act_b2, at(a.b2h, net, tile, i)[lane]);
        return x;
      },
      per);
}

// alpha = d loss / d y per frame (and gamma = d loss / d (q . g) in generator mode); the layout of `coef` as cvf_ef_backward
// reads it (ef_mfma.hip: gS1, gS2, gEt, gS1', gS2')
struct EfgCoefArgs {
  int k, lag_idx;
  int64_t B, T, n_tiles;
  EfgView alpha, gamma;
};

__global__ __launch_bounds__(64) void efg_coef_kernel(EfgCoefArgs a, const float* __restrict__ w, const float* __restrict__ w_lag,
                                                      const float* __restrict__ y_tiled, const double* __restrict__ coef,
                                                      int32_t* __restrict__ step) {
  const int lane = threadIdx.x, net = blockIdx.y, k = a.k;
  const int64_t tile = blockIdx.x;
  const int pass = tile >= a.T ? 1 : 0;
  const int64_t t0 = pass ? tile - a.T : tile;
  const int64_t frame = t0 * CVF_TILE + lane;
  const bool valid = frame < a.B;
  const int64_t fc = valid ? frame : a.B - 1;
  const float wb = valid ? w[fc] : 0.0f;
  const float* yb = y_tiled + t0 * k * CVF_TILE + lane;
  float alpha, gamma = 0.0f;
  if (a.lag_idx == 0) {
    const double* gS1 = coef;
    const double* gS2 = coef + k;
    const double* gEt = coef + k + k * k;
    double s = gS1[net];
    for (int j = 0; j < k; ++j) s += (j == net ? 2.0 : 1.0) * gS2[net * k + j] * (double)yb[j * CVF_TILE];
    alpha = (float)((double)wb * s);
    gamma = (float)(2.0 * (double)wb * gEt[net]);
  } else {
    const float* yl = y_tiled + (a.T + t0) * k * CVF_TILE + lane;
    alpha = (float)g64_transfer_grad(coef, k, net, yb, yl, pass != 0, wb, pass && valid ? w_lag[fc] : 0.0f);
  }
  at(a.alpha, net, tile, 0)[lane] = alpha;
  if (a.lag_idx == 0) at(a.gamma, net, tile, 0)[lane] = gamma;
  if (step != nullptr && blockIdx.x == 0 && net == 0 && lane == 0) *step += 1;
}

// zbar_{NH-1} (in place of zdot_{NH-1} in generator mode) and d_{NH-1}: the incoming product W_NH^T is a broadcast
struct EfgTopArgs {
  int H, act, gen;
  EfgView h, z, u, alpha, gamma;
};

__global__ __launch_bounds__(256) void efg_top_kernel(const cvf_mlp_desc mlp, const float* __restrict__ theta, EfgTopArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, net = blockIdx.y;
  const int64_t tile = blockIdx.x;
  const float* wl = theta + mlp.w_off[net][mlp.n_layers - 1];
  const float al = at(a.alpha, net, tile, 0)[lane];
  const float ga = a.gen ? at(a.gamma, net, tile, 0)[lane] : 0.0f;
  for (int j = wave; j < a.H; j += 4) {
    const float h = at(a.h, net, tile, j)[lane];
    const float s1 = cvf_act_d1(a.act, h), wj = wl[j];
    float* zp = at(a.z, net, tile, j) + lane;
    if (a.gen) {
      *zp = s1 * (al * wj) + ga * cvf_act_d2(a.act, h) * *zp * wj;
      at(a.u, net, tile, j)[lane] = ga * s1 * wj;
    } else {
      *zp = s1 * (al * wj);
    }
  }
}

// ---- transfer mode with a shared trunk: the two launches that sum over the nets.  The boundary launch lives in
// csrc/ef_general_sum.hip (eftr_launch_trunk_sum): compiled into this code object it changes the register allocation of
// efg_layer_kernel (53 -> 60 VGPRs), in a code object of its own it leaves the four kernels above as they were.
// n_shared = NH: zbar_{NH-1}[j] = sigma'(h_{NH-1}[j]) (sum_net alpha_net W_{NH,net}[j]), the nets in the order 0..nets-1
struct EftrTopArgs {
  int H, act, nets;
  EfgView h, z, alpha;   // h, z: one image each; alpha per net
};

__global__ __launch_bounds__(256) void eftr_top_sum_kernel(const cvf_mlp_desc mlp, const float* __restrict__ theta, EftrTopArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  float al[CVF_MAX_NETS];
#pragma unroll
  for (int i = 0; i < CVF_MAX_NETS; ++i) al[i] = i < a.nets ? at(a.alpha, i, tile, 0)[lane] : 0.0f;
  for (int j = wave; j < a.H; j += 4) {
    float s = al[0] * theta[mlp.w_off[0][mlp.n_layers - 1] + j];
#pragma unroll
    for (int i = 1; i < CVF_MAX_NETS; ++i)
      if (i < a.nets) s += al[i] * theta[mlp.w_off[i][mlp.n_layers - 1] + j];
    at(a.z, 0, tile, j)[lane] = cvf_act_d1(a.act, at(a.h, 0, tile, j)[lane]) * s;
  }
}

// ---- the `saved` buffer.  Generator mode (n_tiles = T): per hidden layer h_l, u_l (-> d_l), zdot_l (-> zbar_l), then alpha,
// gamma.  Transfer mode (n_tiles = 2T): h_l per hidden layer, two ping-pong images of zbar (widest layer), alpha.
// Every image is [net][tile][width][64]; with a shared trunk the h_l of the shared layers are [tile][width][64], once (and so is,
// in transfer mode, a shared layer's summed zbar, inside the ping-pong image of its parity).
struct EfgLayout {
  int64_t h[CVF_MAX_LAYERS], u[CVF_MAX_LAYERS], z[CVF_MAX_LAYERS], zb[2], alpha, gamma, total;
};

EfgLayout efg_layout(const cvf_mlp_desc* mlp, int64_t n_tiles, bool gen, int n_shared = 0) {
  EfgLayout L = {};
  const int NH = mlp->n_layers - 1;
  const int64_t per = n_tiles * CVF_TILE * mlp->n_nets;   // floats of one row of every (net, tile)
  int64_t pos = 0;
  int maxH = 1;
  for (int l = 0; l < NH; ++l) {
    L.h[l] = pos;
    pos += (l < n_shared ? per / mlp->n_nets : per) * mlp->dims[l + 1];
    maxH = mlp->dims[l + 1] > maxH ? mlp->dims[l + 1] : maxH;
  }
  if (gen) {
    for (int l = 0; l < NH; ++l) {
      L.u[l] = pos;
      pos += per * mlp->dims[l + 1];
      L.z[l] = pos;
      pos += per * mlp->dims[l + 1];
    }
  } else {
    for (int i = 0; i < 2; ++i) {
      L.zb[i] = pos;
      pos += per * maxH;
    }
  }
  L.alpha = pos;
  pos += per;
  L.gamma = pos;
  if (gen) pos += per;
  L.total = pos;
  return L;
}

EfgView img(float* saved, int64_t off, int64_t n_tiles, int width, bool shared = false) {
  return EfgView{saved + off, (int64_t)width * CVF_TILE, shared ? 0 : n_tiles * width * CVF_TILE};
}

const char* efg_why(const cvf_mlp_desc* mlp) {
  static thread_local char buf[160];
  if (mlp == nullptr) return "no net description";
  if (mlp->n_nets < 1 || mlp->n_nets > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "%d nets: 1 to %d are supported", mlp->n_nets, CVF_MAX_NETS);
    return buf;
  }
  if (mlp->n_layers < 2 || mlp->n_layers > CVF_MAX_LAYERS) {
    snprintf(buf, sizeof buf, "%d hidden layers: 1 to %d are supported", mlp->n_layers - 1, CVF_MAX_LAYERS - 1);
    return buf;
  }
  if (mlp->dims[mlp->n_layers] != 1) return "the nets' output must be a scalar";
  const char* why = g64_why(mlp, mlp->n_layers, G64Chain{2, "hidden layer", "nets", true, false}, buf, sizeof buf);
  if (why != nullptr) return why;
  return mlp->act[mlp->n_layers - 1] != CVF_ACT_NONE ? "an activation after the output layer" : nullptr;
}

// The nets with their first n_shared layers in common: the shape checks of efg_why, then the flat buffer - the shared blocks
// stated once by equal offsets, every block inside the buffer, no two blocks overlapping, and nothing else in it.
const char* efg_why_shared(const cvf_mlp_desc* mlp, int n_shared) {
  static thread_local char buf[200];
  if (mlp == nullptr) return "no net description";
  if (mlp->n_nets < 1 || mlp->n_nets > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "%d nets: 1 to %d are supported", mlp->n_nets, CVF_MAX_NETS);
    return buf;
  }
  if (mlp->n_layers < 2 || mlp->n_layers > CVF_MAX_LAYERS) {
    snprintf(buf, sizeof buf, "%d hidden layers: 1 to %d are supported", mlp->n_layers - 1, CVF_MAX_LAYERS - 1);
    return buf;
  }
  const int L = mlp->n_layers, k = mlp->n_nets;
  if (n_shared < 0 || n_shared > L - 1) {
    snprintf(buf, sizeof buf, "n_shared = %d: 0 to %d (the hidden layers) can be shared", n_shared, L - 1);
    return buf;
  }
  if (mlp->dims[L] != 1) return "the nets' output must be a scalar";
  const char* why = g64_why(mlp, L, G64Chain{2, "hidden layer", "nets", false, true}, buf, sizeof buf);
  if (why != nullptr) return why;
  if (mlp->act[L - 1] != CVF_ACT_NONE) return "an activation after the output layer";
  struct Block {
    int64_t lo, hi;
    int net, layer;
  };
  Block blk[2 * CVF_MAX_NETS * CVF_MAX_LAYERS];
  int nb = 0;
  int64_t n = 0;
  for (int l = 0; l < L; ++l) {
    const int64_t nw = (int64_t)mlp->dims[l + 1] * mlp->dims[l], nbias = mlp->dims[l + 1];
    for (int i = 0; i < k; ++i) {
      if (l < n_shared && i > 0) {
        if (mlp->w_off[i][l] != mlp->w_off[0][l] || mlp->b_off[i][l] != mlp->b_off[0][l]) {
          snprintf(buf, sizeof buf, "shared layer %d: net %d's offsets differ from net 0's", l, i);
          return buf;
        }
        continue;
      }
      blk[nb++] = Block{mlp->w_off[i][l], mlp->w_off[i][l] + nw, i, l};
      blk[nb++] = Block{mlp->b_off[i][l], mlp->b_off[i][l] + nbias, i, l};
      n += nw + nbias;
    }
  }
  if (n != mlp->n_params) {
    snprintf(buf, sizeof buf, "the flat buffer holds %lld parameters, the nets with %d shared layers %lld", (long long)mlp->n_params,
             n_shared, (long long)n);
    return buf;
  }
  for (int a = 0; a < nb; ++a)
    if (blk[a].lo < 0 || blk[a].hi > n) return "a layer's parameters lie outside the flat buffer";
  for (int a = 0; a < nb; ++a)
    for (int b = a + 1; b < nb; ++b)
      if (blk[a].lo < blk[b].hi && blk[b].lo < blk[a].hi) {
        snprintf(buf, sizeof buf, "the parameters of net %d, layer %d overlap those of net %d, layer %d", blk[a].net, blk[a].layer,
                 blk[b].net, blk[b].layer);
        return buf;
      }
  return nullptr;
}

// nets: grid z - all of them, or 1 for the forward launch of a shared layer
int launch_layer(const cvf_mlp_desc* mlp, const float* theta, const EfgLayerArgs& a, int64_t n_tiles, hipStream_t s, int nets) {
  dim3 grid((unsigned)n_tiles, (unsigned)((a.M + 63) / 64), (unsigned)nets);
  hipLaunchKernelGGL(efg_layer_kernel, grid, dim3(256), 0, s, *mlp, theta, a);
  return cvf_check_launch("efg_layer_kernel");
}

EfgLayerArgs layer_args(int layer, int trans, int M, int K, int bias, int epi) {
  EfgLayerArgs a = {};
  a.layer = layer;
  a.trans = trans;
  a.M = M;
  a.K = K;
  a.bias = bias;
  a.epi = epi;
  return a;
}

}  // namespace

extern "C" int cvf_ef_general_supported(const cvf_mlp_desc* mlp) {
  const char* why = efg_why(mlp);
  if (why != nullptr) {
    cvf_set_error("cvf_ef_general: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_ef_general_slab_rows(const cvf_mlp_desc* mlp, int64_t n_tiles) {
  if (efg_why(mlp) != nullptr) return 0;
  return g64_rows(mlp, n_tiles);
}

extern "C" int64_t cvf_ef_general_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles, int lag_idx) {
  if (efg_why(mlp) != nullptr || n_tiles < 1) return 0;
  return efg_layout(mlp, n_tiles, lag_idx == 0).total;
}

namespace {

// the launches of cvf_ef_general_fwd; ns: the first ns layers are shared by the nets (0: none)
int efg_fwd(const cvf_mlp_desc* mlp, int ns, const float* theta, const float* feat_tiled, int64_t n_tiles, float* y_tiled,
            float* g_tiled, float* saved, hipStream_t s) {
  const bool gen = g_tiled != nullptr;
  const int NH = mlp->n_layers - 1, k = mlp->n_nets, D = mlp->dims[0];
  const EfgLayout L = efg_layout(mlp, n_tiles, gen, ns);
  const EfgView feat{(float*)feat_tiled, (int64_t)D * CVF_TILE, 0};
  auto H = [&](int l) { return img(saved, L.h[l], n_tiles, mlp->dims[l + 1], l < ns); };
  // hidden layers: h_l = sigma(W_l h_{l-1} + b_l); a shared layer once, for all nets
  for (int l = 0; l < NH; ++l) {
    EfgLayerArgs a = layer_args(l, 0, mlp->dims[l + 1], mlp->dims[l], 1, EPI_ACT);
    a.act_e = mlp->act[l];
    a.x = l == 0 ? feat : H(l - 1);
    a.out = H(l);
    if (launch_layer(mlp, theta, a, n_tiles, s, l < ns ? 1 : k)) return -1;
  }
  {  // y = W_NH h_{NH-1} + b_NH  -> y_tiled [tile][net][64]
    EfgLayerArgs a = layer_args(NH, 0, 1, mlp->dims[NH], 1, EPI_STORE);
    a.x = H(NH - 1);
    a.out = EfgView{y_tiled, (int64_t)k * CVF_TILE, CVF_TILE};
    if (launch_layer(mlp, theta, a, n_tiles, s, k)) return -1;
  }
  if (!gen) return 0;
  // g = dy/dr: u_{l-1} = W_l^T (sigma'(h_l) .* u_l), u_{NH-1} = W_NH^T (a broadcast); u_{-1} = g -> g_tiled [tile][net][d0][64]
  for (int l = NH - 1; l >= 0; --l) {
    EfgLayerArgs a = layer_args(l, 1, mlp->dims[l], mlp->dims[l + 1], 0, EPI_STORE);
    a.act_x = mlp->act[l];
    a.x_bcast = l == NH - 1;
    if (l < NH - 1) a.x = img(saved, L.u[l], n_tiles, mlp->dims[l + 1]);
    a.xh = H(l);
    a.out = l > 0 ? img(saved, L.u[l - 1], n_tiles, mlp->dims[l]) : EfgView{g_tiled, (int64_t)k * D * CVF_TILE, (int64_t)D * CVF_TILE};
    if (launch_layer(mlp, theta, a, n_tiles, s, k)) return -1;
  }
  return 0;
}

// the launches of cvf_ef_general_backward; ns as efg_fwd (transfer mode with ns > 0: the adjoints of the shared layers are summed
// over the nets - one image, one chain, one weight-gradient product per layer)
int efg_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, int ns, const float* theta, int64_t B, const float* w,
                 const float* w_lag, const float* feat_tiled, const float* y_tiled, const float* q_tiled, const double* coef,
                 float* slab, int32_t* step_count, float* saved, hipStream_t s) {
  const bool gen = cfg->lag_idx == 0;
  const int NH = mlp->n_layers - 1, k = mlp->n_nets, D = mlp->dims[0];
  const int64_t T = cvf_ntiles(B), nt = gen ? T : 2 * T;
  const EfgLayout L = efg_layout(mlp, nt, gen, ns);
  const int R = (int)g64_rows(mlp, nt);
  const EfgView feat{(float*)feat_tiled, (int64_t)D * CVF_TILE, 0};
  const EfgView qv{(float*)q_tiled, (int64_t)k * D * CVF_TILE, (int64_t)D * CVF_TILE};
  auto H = [&](int l) { return img(saved, L.h[l], nt, mlp->dims[l + 1], l < ns); };
  auto U = [&](int l) { return img(saved, L.u[l], nt, mlp->dims[l + 1]); };
  auto Z = [&](int l) {
    return gen ? img(saved, L.z[l], nt, mlp->dims[l + 1]) : img(saved, L.zb[l & 1], nt, mlp->dims[l + 1], l < ns);
  };
  const EfgView alpha = img(saved, L.alpha, nt, 1), gamma = img(saved, L.gamma, nt, 1);

  // the tangent chain along q: zdot_0 = W_0 q, zdot_l = W_l (sigma'(h_{l-1}) .* zdot_{l-1})
  if (gen)
    for (int l = 0; l < NH; ++l) {
      EfgLayerArgs a = layer_args(l, 0, mlp->dims[l + 1], mlp->dims[l], 0, EPI_STORE);
      if (l == 0) {
        a.x = qv;
      } else {
        a.x = Z(l - 1);
        a.xh = H(l - 1);
        a.act_x = mlp->act[l - 1];
      }
      a.out = Z(l);
      if (launch_layer(mlp, theta, a, nt, s, k)) return -1;
    }
  {
    EfgCoefArgs c = {k, cfg->lag_idx, B, T, nt, alpha, gamma};
    hipLaunchKernelGGL(efg_coef_kernel, dim3((unsigned)nt, k), dim3(64), 0, s, c, w, w_lag, y_tiled, coef, step_count);
    if (cvf_check_launch("efg_coef_kernel")) return -1;
  }
  // layer l's gradient from zbar_l, d_l (alpha, gamma for the output layer), h_{l-1} and tdot_{l-1} - before the adjoint of
  // layer l-1 overwrites zdot_{l-1}
  auto wgrad = [&](int l) {
    EfgGradArgs g = {};
    g.layer = l;
    g.Mo = mlp->dims[l + 1];
    g.Ki = mlp->dims[l];
    g.n_tiles = nt;
    g.T = T;
    g.B = B;
    g.rows = R;
    g.n_params = mlp->n_params;
    g.a1 = l == NH ? alpha : Z(l);
    g.b1 = l == 0 ? feat : H(l - 1);
    if (gen) {
      g.a2 = l == NH ? gamma : U(l);
      if (l == 0) {
        g.b2 = qv;
      } else {
        g.b2 = Z(l - 1);
        g.b2h = H(l - 1);
        g.act_b2 = mlp->act[l - 1];
      }
    }
    g.nets = l < ns && gen ? k : 1;   // a shared layer: one block sums the nets' products (transfer mode: zbar_l is the sum already)
    const int nb = ((g.Mo + 63) / 64) * ((g.Ki + 1 + 63) / 64);
    hipLaunchKernelGGL(efg_wgrad_kernel, dim3((unsigned)R, (unsigned)nb, l < ns ? 1 : k), dim3(256), 0, s, *mlp, g, slab);
    return cvf_check_launch("efg_wgrad_kernel");
  };
  if (wgrad(NH)) return -1;
  if (!gen && ns == NH) {   // the heads are output rows: the sum over the nets in the top step
    EftrTopArgs t = {mlp->dims[NH], mlp->act[NH - 1], k, H(NH - 1), Z(NH - 1), alpha};
    hipLaunchKernelGGL(eftr_top_sum_kernel, dim3((unsigned)nt), dim3(256), 0, s, *mlp, theta, t);
    if (cvf_check_launch("eftr_top_sum_kernel")) return -1;
  } else {
    EfgTopArgs t = {mlp->dims[NH], mlp->act[NH - 1], gen ? 1 : 0, H(NH - 1), Z(NH - 1), gen ? U(NH - 1) : EfgView{}, alpha, gamma};
    hipLaunchKernelGGL(efg_top_kernel, dim3((unsigned)nt, k), dim3(256), 0, s, *mlp, theta, t);
    if (cvf_check_launch("efg_top_kernel")) return -1;
  }
  for (int l = NH - 1; l >= 0; --l) {
    if (wgrad(l)) return -1;
    if (l == 0) break;
    if (!gen && l == ns) {   // the trunk boundary: zbar_{ns-1} = sigma'(h_{ns-1}) .* sum_i W_{ns,i}^T zbar_{ns,i}, one image
      EftrSumArgs b = {l, mlp->dims[l], mlp->dims[l + 1], k, mlp->act[l - 1], Z(l).p, Z(l).ns, Z(l - 1).p, H(l - 1).p};
      if (eftr_launch_trunk_sum(mlp, theta, b, nt, s)) return -1;
      continue;
    }
    // zbar_{l-1} = sigma'(h_{l-1}) .* (W_l^T zbar_l) [+ gamma sigma''(h_{l-1}) .* zdot_{l-1} .* u_{l-1};  d_{l-1}]
    EfgLayerArgs a = layer_args(l, 1, mlp->dims[l], mlp->dims[l + 1], 0, gen ? EPI_BWD_GEN : EPI_BWD_TR);
    a.x = Z(l);
    a.out = Z(l - 1);
    a.eh = H(l - 1);
    a.act_e = mlp->act[l - 1];
    if (gen) {
      a.eu = U(l - 1);
      a.gam = gamma;
    }
    if (launch_layer(mlp, theta, a, nt, s, !gen && l < ns ? 1 : k)) return -1;   // (below the boundary: one chain)
  }
  return 0;
}

}  // namespace

extern "C" int cvf_ef_general_fwd(const cvf_mlp_desc* mlp, const float* theta, const float* feat_tiled, int64_t n_tiles,
                                  float* y_tiled, float* g_tiled, float* saved, void* stream) {
  const char* why = efg_why(mlp);
  CVF_REQUIRE(why == nullptr, "cvf_ef_general_fwd: %s", why);
  CVF_REQUIRE(theta && feat_tiled && y_tiled && saved && n_tiles > 0, "cvf_ef_general_fwd: bad argument");
  return efg_fwd(mlp, 0, theta, feat_tiled, n_tiles, y_tiled, g_tiled, saved, (hipStream_t)stream);
}

extern "C" int cvf_ef_general_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, int64_t B,
                                       const float* w, const float* w_lag, const float* feat_tiled, const float* y_tiled,
                                       const float* q_tiled, const double* coef, float* slab, int32_t* step_count,
                                       float* saved, void* stream) {
  const char* why = efg_why(mlp);
  CVF_REQUIRE(why == nullptr, "cvf_ef_general_backward: %s", why);
  CVF_REQUIRE(cfg && theta && w && feat_tiled && y_tiled && coef && slab && saved && B > 0, "cvf_ef_general_backward: bad argument");
  CVF_REQUIRE(cfg->k == mlp->n_nets, "cvf_ef_general_backward: cfg.k != number of nets");
  const bool gen = cfg->lag_idx == 0;
  CVF_REQUIRE(!gen || q_tiled, "cvf_ef_general_backward: generator mode needs q");
  CVF_REQUIRE(gen || w_lag, "cvf_ef_general_backward: transfer mode needs w_lag");
  return efg_backward(cfg, mlp, 0, theta, B, w, w_lag, feat_tiled, y_tiled, q_tiled, coef, slab, step_count, saved,
                      (hipStream_t)stream);
}

// ---- nets that share their first n_shared layers (generator mode)
extern "C" int cvf_ef_general_shared_supported(const cvf_mlp_desc* mlp, int n_shared) {
  const char* why = efg_why_shared(mlp, n_shared);
  if (why != nullptr) {
    cvf_set_error("cvf_ef_general_shared: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_ef_general_shared_slab_rows(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared) {
  if (efg_why_shared(mlp, n_shared) != nullptr) return 0;
  return g64_rows(mlp, n_tiles);
}

extern "C" int64_t cvf_ef_general_shared_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared) {
  if (efg_why_shared(mlp, n_shared) != nullptr || n_tiles < 1) return 0;
  return efg_layout(mlp, n_tiles, true, n_shared).total;
}

extern "C" int cvf_ef_general_shared_fwd(const cvf_mlp_desc* mlp, int n_shared, const float* theta, const float* feat_tiled,
                                         int64_t n_tiles, float* y_tiled, float* g_tiled, float* saved, void* stream) {
  const char* why = efg_why_shared(mlp, n_shared);
  CVF_REQUIRE(why == nullptr, "cvf_ef_general_shared_fwd: %s", why);
  CVF_REQUIRE(g_tiled, "cvf_ef_general_shared_fwd: the transfer-mode shared step (no g_tiled) is not built");
  CVF_REQUIRE(theta && feat_tiled && y_tiled && saved && n_tiles > 0, "cvf_ef_general_shared_fwd: bad argument");
  return efg_fwd(mlp, n_shared, theta, feat_tiled, n_tiles, y_tiled, g_tiled, saved, (hipStream_t)stream);
}

extern "C" int cvf_ef_general_shared_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, int n_shared, const float* theta,
                                              int64_t B, const float* w, const float* feat_tiled, const float* y_tiled,
                                              const float* q_tiled, const double* coef, float* slab, int32_t* step_count,
                                              float* saved, void* stream) {
  const char* why = efg_why_shared(mlp, n_shared);
  CVF_REQUIRE(why == nullptr, "cvf_ef_general_shared_backward: %s", why);
  CVF_REQUIRE(cfg, "cvf_ef_general_shared_backward: bad argument");
  CVF_REQUIRE(cfg->lag_idx == 0, "cvf_ef_general_shared_backward: the transfer-mode shared step (cfg.lag_idx = %d) is not built",
              cfg->lag_idx);
  CVF_REQUIRE(theta && w && feat_tiled && y_tiled && q_tiled && coef && slab && saved && B > 0,
              "cvf_ef_general_shared_backward: bad argument");
  CVF_REQUIRE(cfg->k == mlp->n_nets, "cvf_ef_general_shared_backward: cfg.k != number of nets");
  return efg_backward(cfg, mlp, n_shared, theta, B, w, nullptr, feat_tiled, y_tiled, q_tiled, coef, slab, step_count, saved,
                      (hipStream_t)stream);
}

// ---- the same in transfer mode: the shared layers' adjoint summed over the nets, the trunk back-propagated once
extern "C" int cvf_ef_general_shared_transfer_supported(const cvf_mlp_desc* mlp, int n_shared) {
  const char* why = efg_why_shared(mlp, n_shared);
  if (why != nullptr) {
    cvf_set_error("cvf_ef_general_shared_transfer: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_ef_general_shared_transfer_slab_rows(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared) {
  if (efg_why_shared(mlp, n_shared) != nullptr) return 0;
  return g64_rows(mlp, n_tiles);
}

extern "C" int64_t cvf_ef_general_shared_transfer_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared) {
  if (efg_why_shared(mlp, n_shared) != nullptr || n_tiles < 1) return 0;
  return efg_layout(mlp, n_tiles, false, n_shared).total;
}

extern "C" int cvf_ef_general_shared_transfer_fwd(const cvf_mlp_desc* mlp, int n_shared, const float* theta, const float* feat_tiled,
                                                  int64_t n_tiles, float* y_tiled, float* saved, void* stream) {
  const char* why = efg_why_shared(mlp, n_shared);
  CVF_REQUIRE(why == nullptr, "cvf_ef_general_shared_transfer_fwd: %s", why);
  CVF_REQUIRE(theta && feat_tiled && y_tiled && saved && n_tiles > 0, "cvf_ef_general_shared_transfer_fwd: bad argument");
  return efg_fwd(mlp, n_shared, theta, feat_tiled, n_tiles, y_tiled, nullptr, saved, (hipStream_t)stream);
}

extern "C" int cvf_ef_general_shared_transfer_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, int n_shared, const float* theta,
                                                       int64_t B, const float* w, const float* w_lag, const float* feat_tiled,
                                                       const float* y_tiled, const double* coef, float* slab, int32_t* step_count,
                                                       float* saved, void* stream) {
  const char* why = efg_why_shared(mlp, n_shared);
  CVF_REQUIRE(why == nullptr, "cvf_ef_general_shared_transfer_backward: %s", why);
  CVF_REQUIRE(cfg, "cvf_ef_general_shared_transfer_backward: bad argument");
  CVF_REQUIRE(cfg->lag_idx != 0, "cvf_ef_general_shared_transfer_backward: a generator-mode cfg (lag_idx = 0) belongs to "
                                 "cvf_ef_general_shared_backward");
  CVF_REQUIRE(w_lag, "cvf_ef_general_shared_transfer_backward: transfer mode needs w_lag");
  CVF_REQUIRE(theta && w && feat_tiled && y_tiled && coef && slab && saved && B > 0,
              "cvf_ef_general_shared_transfer_backward: bad argument");
  CVF_REQUIRE(cfg->k == mlp->n_nets, "cvf_ef_general_shared_transfer_backward: cfg.k != number of nets");
  return efg_backward(cfg, mlp, n_shared, theta, B, w, w_lag, feat_tiled, y_tiled, nullptr, coef, slab, step_count, saved,
                      (hipStream_t)stream);
}
