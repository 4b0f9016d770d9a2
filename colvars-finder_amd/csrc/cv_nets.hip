// The nets' part of a trained CV and of its coordinate Jacobian (cvf_cv_nets_*): xi = nets(r) and
// G = d xi / d r per frame, for the callers of colvar_model().jacobian() / .metric_tensor() and for a C caller that biases an
// MD engine along a learned CV (cvf_align_feature_fwd -> cvf_cv_nets_eval -> cvf_align_feature_vjp_rows).
// One launch per layer and pass over all 64-frame tiles, the activations handed over through `scratch`, in the decomposition of
// csrc/ef_general.hip and csrc/ae_general.hip, the products on the 64 x 64 core of csrc/cvf_gemm64.hpp:
//
//   aeg_gather_kernel  (csrc/aeg_kernels.hpp) feat_rows [B][d0] -> a_0 [tile][d0][64]; skipped when the caller has tiles
//   cvn_layer_kernel   [M x K] x [K x 64 frames] per (tile, 64-row block, z): W_l (forward) or W_l^T (sweep) as the A operand;
//                      forward: z = net, the epilogue adds the bias, applies act_l and, on the last layer, also writes xi_rows;
//                      sweep:   z = CV index i, the B operand is act_l'(a_{l+1}) .* v_{l+1} formed on its way to LDS, and the
//                               last launch (l = 0) writes g_tiled from the accumulators and g_rows through an LDS transpose
//   cvn_linear_kernel  chains of ONE layer, whose g is the seed itself: act'(xi_i) W_0[i][:]
//
// Mathematics (layers l = 0..L-1, a_0 = r, a_{l+1} = act_l(W_l a_l + b_l), xi = a_L; act' through the output):
//   v_L = e_i,  v_l = W_l^T (act_l'(a_{l+1}) .* v_{l+1}),  d xi_i / d r = v_0.
// v_{L-1} = act_{L-1}'(xi_i) W_{L-1}[i][:] is a row of the weights times one factor per frame: it is never stored, the first
// sweep launch (l = L-2) forms it while staging.  Form A (n_nets = k scalar chains, EigenFunctions) reads net i's own weights
// and activations; form B (one chain cut after `upto_layer` layers, e.g. an encoder) runs the trunk ONCE and sweeps the k rows
// of its last weight matrix through the shared weights and the shared act'(a_l).  Form C (cvf_cv_nets_shared_*; DESIGN.md section
// 4.17) is form A whose first n_shared layers are one set of tensors: those layers are launched with ONE z and zero z strides,
// layer n_shared reads the one image a_{n_shared}, and the sweeps of the k CVs read the shared act'(a_l) images below it.
// The L2 is per XCD and not coherent across the eight of them, and workgroups go to the XCDs round-robin in dispatch order (x
// fastest).  In form A block (tile, z) has the same place in every launch, so it reads what its own XCD wrote.  In form C a trunk
// launch has T blocks and a head launch k T: unless T is a multiple of 8, block (tile, z > 0) lands on another XCD than the trunk
// block of its tile and pays for reading an image just written elsewhere (measured at B = 1: 11.6 us against 8.4 us for the launch
// of layer n_shared; nothing at T = 8 or 16).  So a form-C call rounds grid.x up to a multiple of 8 (CvnArgs.nt: blocks past the
// tiles exit at once): tile t is on XCD t % 8 in EVERY launch of the call, whatever y and z.
//
// All products run on v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulation.  No atomics; a column of the B operand (a frame)
// meets the same instructions in the same order whichever tile and lane it sits in, so a frame's xi and g depend on its
// features and theta only.  Nothing is read from scratch or the outputs that the same call did not write.
#include "aeg_kernels.hpp"
#include "cvf_cv_shared.hpp"

namespace {

enum { CVN_ACT = 0, CVN_SWEEP = 1, CVN_G = 2 };

struct CvnArgs {
  int w_off[CVF_MAX_NETS], b_off[CVF_MAX_NETS];   // per z: the A operand's weights; forward: the bias
  int s_off[CVF_MAX_NETS];                        // per z (seed != 0): the row of the last weight matrix that seeds the sweep
  int ldw;            // row length of W_l (= dims[l])
  int trans;          // 0: A = W [M = dims[l+1]][K = dims[l]];  1: A = W^T [M = dims[l]][K = dims[l+1]]
  int M, K;
  int epi, act;       // CVN_ACT: out = act(acc + b);  sweeps: B = act'(xh) .* x
  int seed, act_top;  // B row k = act_top'(top[frame]) * theta[s_off[z] + k] instead of x
  const float* x;     // B operand [z][tile][K][64]
  const float* xh;    // sweeps: a_{l+1} [z][tile][K][64]
  const float* top;   // seed: a_L, the row of CV z
  float* out;         // CVN_ACT / CVN_SWEEP: [z][tile][M][64]
  int64_t xs, xz, hs, hz, tps, tpz, os, oz;   // tile and z strides of the images (z stride 0: shared)
  float* xi_rows;     // CVN_ACT on the last layer: [B][k], column z * M + m
  float* g_rows;      // CVN_G: [B][k][M]
  float* g_tiled;     // CVN_G: [tile][k][M][64]
  int64_t B;
  int k;
  int nt;             // > 0: grid.x is rounded up past the nt tiles and blocks with blockIdx.x >= nt exit (0: every block works)
};

constexpr int kXcds = 8;   // gfx950
constexpr int kXP = 65;   // pitch of the [frame][m] image of the g_rows transpose
static_assert(CVF_TILE * kXP <= 2 * kKC * kPitch, "the transpose reuses the operand stages");

// out[m][frame] (64 x 64 block) = A[m][:] . B[:][frame] for one (tile, row block, z)
__global__ __launch_bounds__(256) void cvn_layer_kernel(const float* __restrict__ theta, CvnArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[2 * kKC * kPitch];   // As [k][m], then Bs [k][frame]
  const G64Thread t = g64_thread();
  const int lane = t.lane, wave = t.wave;
  if (a.nt > 0 && blockIdx.x >= (unsigned)a.nt) return;   // (the whole block: no barrier has been met)
  const int64_t tile = blockIdx.x;
  const int m0 = blockIdx.y * 64, z = blockIdx.z;
  const float* xp = a.seed ? nullptr : a.x + z * a.xz + tile * a.xs;
  const float* hp = a.xh != nullptr ? a.xh + z * a.hz + tile * a.hs : nullptr;
  const float* sp = a.seed ? theta + a.s_off[z] : nullptr;
  const float sfac = a.seed ? cvf_act_d1(a.act_top, a.top[z * a.tpz + tile * a.tps + lane]) : 0.0f;

  f32x4 acc[2][2];
  g64_layer_product(smem, smem + kKC * kPitch, theta + a.w_off[z], a.ldw, a.trans, m0, a.M, a.K, t, acc, [&](int k) {
    float bv = sp != nullptr ? sfac * sp[k] : xp[(int64_t)k * CVF_TILE + lane];
    if (hp != nullptr) bv *= cvf_act_d1(a.act, hp[(int64_t)k * CVF_TILE + lane]);
    return bv;
  });

  const float* bias = a.epi == CVN_ACT ? theta + a.b_off[z] : nullptr;
  float* op = a.epi != CVN_G ? a.out + z * a.oz + tile * a.os : nullptr;
  float* gt = a.epi == CVN_G && a.g_tiled != nullptr ? a.g_tiled + (tile * a.k + z) * (int64_t)a.M * CVF_TILE : nullptr;
  const bool rows = a.epi == CVN_G && a.g_rows != nullptr;
  g64_walk(acc, t, [&](int mloc, int f, float v) {
    const int m = m0 + mloc;
    if (rows) smem[f * kXP + mloc] = v;   // (the product ended on a barrier: the stages are free)
    if (m >= a.M) return;
    const int64_t o = (int64_t)m * CVF_TILE + f;
    const bool valid = tile * CVF_TILE + f < a.B;
    if (a.epi == CVN_ACT) {
      v = cvf_act(a.act, v + bias[m]);
      op[o] = v;
      if (a.xi_rows != nullptr && valid) a.xi_rows[(tile * CVF_TILE + f) * a.k + z * a.M + m] = v;
    } else if (a.epi == CVN_SWEEP) {
      op[o] = v;
    } else if (gt != nullptr) {
      gt[o] = valid ? v : 0.0f;   // lanes of padded frames hold exactly 0
    }
  });
  if (rows) {   // [frame][m] -> g_rows[frame][z][m0 ..], the stores of a wave along m
    __syncthreads();
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int fr = wave + 4 * it;
      const int64_t frame = tile * CVF_TILE + fr;
      if (frame < a.B && m0 + lane < a.M) a.g_rows[(frame * a.k + z) * a.M + m0 + lane] = smem[fr * kXP + lane];
    }
  }
}

// One-layer chains: xi and, for CV z, g = act'(xi_z) W_0[row z][:] (there is no product to sweep through)
struct CvnLinearArgs {
  int s_off[CVF_MAX_NETS];
  int d0, act, k;
  const float* top;   // a_1: [z][tile][..][64] through tps / tpz
  int64_t tps, tpz, B;
  float* g_rows;
  float* g_tiled;
};

__global__ __launch_bounds__(256) void cvn_linear_kernel(const float* __restrict__ theta, CvnLinearArgs a) {
  __shared__ float sf[CVF_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, z = blockIdx.y;
  const int64_t tile = blockIdx.x;
  const float* sp = theta + a.s_off[z];
  const float s = cvf_act_d1(a.act, a.top[z * a.tpz + tile * a.tps + lane]);
  if (wave == 0) sf[lane] = s;
  __syncthreads();
  if (a.g_tiled != nullptr) {
    float* gt = a.g_tiled + (tile * a.k + z) * (int64_t)a.d0 * CVF_TILE;
    const bool valid = tile * CVF_TILE + lane < a.B;
    for (int c = wave; c < a.d0; c += 4) gt[(int64_t)c * CVF_TILE + lane] = valid ? s * sp[c] : 0.0f;
  }
  if (a.g_rows != nullptr)
    for (int fr = wave; fr < CVF_TILE; fr += 4) {
      const int64_t frame = tile * CVF_TILE + fr;
      if (frame >= a.B) break;
      const float sfr = sf[fr];
      float* gr = a.g_rows + (frame * a.k + z) * a.d0;
      for (int c = lane; c < a.d0; c += 64) gr[c] = sfr * sp[c];
    }
}

constexpr int kMaxValuesK = 4096;   // widest output of a values-only call

// the model's form and k, or the reason it is refused
struct CvnShape {
  int L, k, nn;   // layers evaluated, CVs, forward chains (form A: k, form B: 1)
  bool form_a;
  int ns;         // form C: the chains' first ns layers are one trunk (0: forms A and B)
};

const char* cvn_why(const cvf_mlp_desc* mlp, int upto, int want_g, CvnShape* sh) {
  static thread_local char buf[200];
  if (mlp == nullptr) return "no model description";
  if (mlp->n_nets < 1 || mlp->n_nets > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "%d nets: 1 to %d are supported", mlp->n_nets, CVF_MAX_NETS);
    return buf;
  }
  if (mlp->n_layers < 1 || mlp->n_layers > CVF_MAX_LAYERS) {
    snprintf(buf, sizeof buf, "%d layers: 1 to %d are supported", mlp->n_layers, CVF_MAX_LAYERS);
    return buf;
  }
  if (upto < 1 || upto > mlp->n_layers) {
    snprintf(buf, sizeof buf, "upto_layer=%d out of range (the model has %d layers)", upto, mlp->n_layers);
    return buf;
  }
  const bool form_a = mlp->n_nets > 1;
  if (form_a && upto != mlp->n_layers) {
    snprintf(buf, sizeof buf, "%d nets side by side are evaluated whole: upto_layer must be %d", mlp->n_nets, mlp->n_layers);
    return buf;
  }
  if (form_a && mlp->dims[upto] != 1) {
    snprintf(buf, sizeof buf, "%d nets side by side must be scalar (they have %d outputs each)", mlp->n_nets, mlp->dims[upto]);
    return buf;
  }
  const char* why = g64_why(mlp, upto, G64Chain{1, "layer", "model", false, false}, buf, sizeof buf);
  if (why != nullptr) return why;
  const int k = form_a ? mlp->n_nets : mlp->dims[upto];
  if (k < 1 || k > kMaxValuesK) {
    snprintf(buf, sizeof buf, "%d outputs: 1 to %d are supported", k, kMaxValuesK);
    return buf;
  }
  if (want_g && k > CVF_MAX_NETS) {
    snprintf(buf, sizeof buf, "k = %d outputs: d xi / d r is formed for at most %d (values alone take up to %d)", k, CVF_MAX_NETS,
             kMaxValuesK);
    return buf;
  }
  for (int i = 0; i < (form_a ? mlp->n_nets : 1); ++i)
    for (int l = 0; l < upto; ++l)
      if (mlp->w_off[i][l] < 0 || mlp->b_off[i][l] < 0) return "a negative parameter offset";
  if (sh != nullptr) *sh = CvnShape{upto, k, form_a ? mlp->n_nets : 1, form_a, 0};
  return nullptr;
}

// form C: the aliasing first, then the checks of form A on the whole chains (one head, n_nets = 1, is form B's arithmetic)
const char* cvn_shared_why(const cvf_mlp_desc* mlp, int n_shared, int want_g, CvnShape* sh) {
  static thread_local char buf[240];
  const char* why = cvf_form_c_why(mlp, n_shared, "cvf_cv_nets_eval", buf, sizeof buf);
  if (why == nullptr) why = cvn_why(mlp, mlp->n_layers, want_g, sh);
  if (why == nullptr && sh != nullptr) sh->ns = n_shared;
  return why;
}

// ---- scratch: a_0 (the gathered features; unused when the caller has tiles), a_1..a_L ([chain][tile][width][64] each) and, for
// g on chains of three layers or more, two ping-pong images of v_l, l = 1..L-2 ([CV][tile][widest of dims[1..L-2]][64]).
// Form C holds the trunk's images a_1..a_ns once: 64 T (dims[0] + sum dims[1..ns] + k sum dims[ns+1..L]) + 128 T k vmax with g.
struct CvnLayout {
  int64_t a[CVF_MAX_LAYERS + 1], v[2], total;
  int vmax;
};

CvnLayout cvn_layout(const cvf_mlp_desc* mlp, const CvnShape& sh, int64_t n_tiles, bool want_g) {
  CvnLayout L = {};
  const int64_t per = n_tiles * CVF_TILE;
  int64_t pos = 0;
  L.a[0] = pos;
  pos += per * mlp->dims[0];
  for (int l = 1; l <= sh.L; ++l) {
    L.a[l] = pos;
    pos += per * mlp->dims[l] * (l <= sh.ns ? 1 : sh.nn);
  }
  for (int l = 1; l <= sh.L - 2; ++l) L.vmax = mlp->dims[l] > L.vmax ? mlp->dims[l] : L.vmax;
  if (want_g)
    for (int i = 0; i < 2; ++i) {
      L.v[i] = pos;
      pos += per * L.vmax * sh.k;
    }
  L.total = pos;
  return L;
}

}  // namespace

extern "C" int cvf_cv_nets_supported(const cvf_mlp_desc* mlp, int upto_layer, int want_g) {
  const char* why = cvn_why(mlp, upto_layer, want_g, nullptr);
  if (why != nullptr) {
    cvf_set_error("cvf_cv_nets: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_cv_nets_scratch_floats(const cvf_mlp_desc* mlp, int upto_layer, int64_t B, int want_g) {
  CvnShape sh;
  if (cvn_why(mlp, upto_layer, want_g, &sh) != nullptr || B < 1) return 0;
  return cvn_layout(mlp, sh, cvf_ntiles(B), want_g != 0).total;
}

namespace {

// the launches of one call, for a shape the caller has checked (sh.ns > 0: form C)
int cvn_eval(const char* name, const cvf_mlp_desc* mlp, const CvnShape& sh, const float* theta, const float* feat_rows,
             const float* feat_tiled, int64_t B, float* xi_rows, float* g_rows, float* g_tiled, float* scratch, void* stream) {
  const bool want_g = g_rows != nullptr || g_tiled != nullptr;
  CVF_REQUIRE(theta && scratch && xi_rows && B > 0, "%s: bad argument", name);
  CVF_REQUIRE((feat_rows != nullptr) != (feat_tiled != nullptr), "%s: pass exactly one of feat_rows and feat_tiled", name);
  const int64_t T = cvf_ntiles(B);
  CVF_REQUIRE(T <= 0x7fffffff - kXcds, "%s: %lld frames are more than one call takes", name, (long long)B);
  hipStream_t s = (hipStream_t)stream;
  const int L = sh.L, k = sh.k, nn = sh.nn, ns = sh.ns, d0 = mlp->dims[0];
  const CvnLayout lay = cvn_layout(mlp, sh, T, want_g);
  auto ts = [&](int l) { return (int64_t)mlp->dims[l] * CVF_TILE; };   // tile stride of an image of layer l's width
  auto zs = [&](int l) { return T * ts(l); };                          // chain / CV stride of such an image
  auto A = [&](int l) { return scratch + lay.a[l]; };

  const float* a0 = feat_tiled;
  if (feat_rows != nullptr) {
    hipLaunchKernelGGL(aeg_gather_kernel, dim3((unsigned)T), dim3(256), 0, s, feat_rows, (const int64_t*)nullptr, B, d0, A(0), T,
                       (int64_t)0);
    if (cvf_check_launch("aeg_gather_kernel")) return -1;
    a0 = A(0);
  }

  // form C: grid.x a multiple of the XCD count, so that a tile's blocks meet on one XCD in every launch (the header has the figures)
  const int64_t gx = ns > 0 ? (T + kXcds - 1) / kXcds * kXcds : T;
  auto launch = [&](CvnArgs a, int nz) {
    a.nt = gx != T ? (int)T : 0;
    hipLaunchKernelGGL(cvn_layer_kernel, dim3((unsigned)gx, (unsigned)((a.M + 63) / 64), (unsigned)nz), dim3(256), 0, s, theta, a);
    return cvf_check_launch("cvn_layer_kernel");
  };
  // forward: a_{l+1} = act_l(W_l a_l + b_l), every chain in one launch; the last layer also leaves xi_rows
  for (int l = 0; l < L; ++l) {
    CvnArgs a = {};
    for (int i = 0; i < nn; ++i) {
      a.w_off[i] = mlp->w_off[i][l];
      a.b_off[i] = mlp->b_off[i][l];
    }
    a.ldw = mlp->dims[l];
    a.M = mlp->dims[l + 1];
    a.K = mlp->dims[l];
    a.epi = CVN_ACT;
    a.act = mlp->act[l];
    a.x = l == 0 ? a0 : A(l);
    a.xs = ts(l);
    a.xz = l == 0 || l <= ns ? 0 : zs(l);   // the features, and form C's trunk, are shared by the chains
    a.out = A(l + 1);
    a.os = ts(l + 1);
    a.oz = zs(l + 1);
    a.xi_rows = l + 1 == L ? xi_rows : nullptr;
    a.B = B;
    a.k = k;
    if (launch(a, l < ns ? 1 : nn)) return -1;   // (a trunk layer of form C: one z)
  }
  if (!want_g) return 0;

  // the seed of CV i: the row of the last weight matrix it multiplies, and its output's row of a_L
  int s_off[CVF_MAX_NETS] = {};
  for (int i = 0; i < k; ++i) s_off[i] = sh.form_a ? mlp->w_off[i][L - 1] : mlp->w_off[0][L - 1] + i * mlp->dims[L - 1];
  const int64_t tps = ts(L), tpz = sh.form_a ? zs(L) : CVF_TILE;
  if (L == 1) {
    CvnLinearArgs a = {};
    for (int i = 0; i < k; ++i) a.s_off[i] = s_off[i];
    a.d0 = d0;
    a.act = mlp->act[0];
    a.k = k;
    a.top = A(1);
    a.tps = tps;
    a.tpz = tpz;
    a.B = B;
    a.g_rows = g_rows;
    a.g_tiled = g_tiled;
    hipLaunchKernelGGL(cvn_linear_kernel, dim3((unsigned)T, (unsigned)k), dim3(256), 0, s, theta, a);
    return cvf_check_launch("cvn_linear_kernel");
  }
  // sweep: v_l = W_l^T (act_l'(a_{l+1}) .* v_{l+1}), l = L-2 .. 0, the k CVs in one launch; v_l sits in image l & 1
  for (int l = L - 2; l >= 0; --l) {
    CvnArgs a = {};
    for (int i = 0; i < k; ++i) {
      a.w_off[i] = mlp->w_off[sh.form_a ? i : 0][l];
      a.s_off[i] = s_off[i];
    }
    a.ldw = mlp->dims[l];
    a.trans = 1;
    a.M = mlp->dims[l];
    a.K = mlp->dims[l + 1];
    a.act = mlp->act[l];
    a.xh = A(l + 1);
    a.hs = ts(l + 1);
    a.hz = sh.form_a && l + 1 > ns ? zs(l + 1) : 0;   // forms B and C: the trunk's activations are shared by the CVs
    if (l == L - 2) {
      a.seed = 1;
      a.act_top = mlp->act[L - 1];
      a.top = A(L);
      a.tps = tps;
      a.tpz = tpz;
    } else {
      a.x = scratch + lay.v[(l + 1) & 1];
      a.xs = ts(l + 1);
      a.xz = zs(l + 1);
    }
    a.B = B;
    a.k = k;
    if (l > 0) {
      a.epi = CVN_SWEEP;
      a.out = scratch + lay.v[l & 1];
      a.os = ts(l);
      a.oz = zs(l);
    } else {
      a.epi = CVN_G;
      a.g_rows = g_rows;
      a.g_tiled = g_tiled;
    }
    if (launch(a, k)) return -1;
  }
  return 0;
}

}  // namespace

extern "C" int cvf_cv_nets_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const float* feat_rows,
                                const float* feat_tiled, int64_t B, float* xi_rows, float* g_rows, float* g_tiled,
                                float* scratch, void* stream) {
  CvnShape sh;
  const char* why = cvn_why(mlp, upto_layer, g_rows != nullptr || g_tiled != nullptr, &sh);
  CVF_REQUIRE(why == nullptr, "cvf_cv_nets_eval: %s", why);
  return cvn_eval("cvf_cv_nets_eval", mlp, sh, theta, feat_rows, feat_tiled, B, xi_rows, g_rows, g_tiled, scratch, stream);
}

extern "C" int cvf_cv_nets_shared_supported(const cvf_mlp_desc* mlp, int n_shared, int want_g) {
  const char* why = cvn_shared_why(mlp, n_shared, want_g, nullptr);
  if (why != nullptr) {
    cvf_set_error("cvf_cv_nets_shared: %s", why);
    return 0;
  }
  return 1;
}

extern "C" int64_t cvf_cv_nets_shared_scratch_floats(const cvf_mlp_desc* mlp, int n_shared, int64_t B, int want_g) {
  CvnShape sh;
  if (cvn_shared_why(mlp, n_shared, want_g, &sh) != nullptr || B < 1) return 0;
  return cvn_layout(mlp, sh, cvf_ntiles(B), want_g != 0).total;
}

extern "C" int cvf_cv_nets_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const float* feat_rows,
                                       const float* feat_tiled, int64_t B, float* xi_rows, float* g_rows, float* g_tiled,
                                       float* scratch, void* stream) {
  CvnShape sh;
  const char* why = cvn_shared_why(mlp, n_shared, g_rows != nullptr || g_tiled != nullptr, &sh);
  CVF_REQUIRE(why == nullptr, "cvf_cv_nets_shared_eval: %s", why);
  if (B == 0) return 0;
  return cvn_eval("cvf_cv_nets_shared_eval", mlp, sh, theta, feat_rows, feat_tiled, B, xi_rows, g_rows, g_tiled, scratch, stream);
}
