// xi(x) and d xi / d x of a trained CV per frame in ONE launch: one wave = one frame (cvf_cv_frame_*).
// The deployment form of cvf_align_feature_fwd -> cvf_cv_nets_eval -> cvf_align_feature_vjp_rows for an MD engine that evaluates
// one frame (or a few replicas) per step: those three calls are about ten launches whose first and last run one lane of one wave
// at B = 1.  Here everything between the coordinates and the gradient stays in the workgroup's LDS:
//
//   alignment   one align atom per lane; the weighted centroid and H = sum_b (x_b - c) (x) ref_c[b] by wave_sum (fp64), then every
//               lane runs the solver of cvf_kabsch.hpp on the same H: R, the centroid and Kinv without an aux buffer
//   features    records strided over the lanes -> a_0 = r [d_r]                                  (cvf_features.hpp)
//   forward     lane j owns output units j, j + 64, ..: a_{l+1} = act_l(W_l a_l + b_l), the input broadcast from LDS, each dot
//               product one sequential sum in index order; every layer's activations stay for the sweep
//   sweep       v_L = e_i (or coef), v_l = W_l^T (act_l'(a_{l+1}) .* v_{l+1}), lane i owns input units i, i + 64, ..
//               -> g_i = d xi_i / d r [d_r] per CV, or the one contracted g = sum_i coef_i g_i
//   coordinates phase 1, lane = record: the record's (at most four) gradient vectors times every row's cotangent -> a table in
//               LDS (the geometry is taken once per frame, not once per row); the position records' M = sum_p xc_p (x) g_p and
//               sum_p R g_p by wave_sum;  phase 2, lane = atom: the atom's entries of the table in record order (a scan of rec),
//               then on the align atoms Z ref_b - w_b shift (csrc/k1_vjp.hip)
//
// No atomics, no scratch, no aux.  A frame meets the same instructions in the same order whatever B is and wherever it sits in
// the batch, so its result depends on its coordinates and theta only, bit for bit.
// The three-call recipe remains the route for large batches, large molecules and wide nets: a wave here does for ONE frame the
// table reads, weight reads and solver instructions that a 64-frame tile shares there.
//
// Form C (cvf_cv_frame_shared_*): k scalar chains on one trunk of n_shared layers.  The trunk's
// activations are held ONCE, its forward pass strides dims[l+1] units over the lanes (k * dims[l+1] above it), the k head sweeps
// stop at layer n_shared, and below it the k vectors (or, with coef, their one sum taken at the boundary) are carried through
// the shared weights together, unit (vector, input) over the lanes.  A row's arithmetic is that of form A.
//
// This header holds the kernel's body, its LDS layout and its predicate ONCE, for two translation units.  Where the frame comes
// from, where the sweep's seed comes from and where the gradient goes is an IO policy of the body:
//   csrc/cv_frame.hip   cvf_cv_frame_*        dense x [B][n_coord], the seed from the global coef, gx_rows written
//   csrc/cv_bias.hip    cvf_cv_frame_bias_*   an MD engine's position and force arrays through cvf_md_layout, the seed -dU/dxi
//                                             from the xi in LDS (cvf_bias.hpp), the force accumulated
//   float        IO::load(frame, nc, j)                    coordinate j of the frame
//   const float* IO::seeds(spare, top, frame, k, lane)     once xi = top[0..k) is in LDS: the frame's k seeds of the contracted
//                                                          sweep (global, or in `spare` behind a barrier); unused for k rows
//   void         IO::store(frame, kk, nc, e, v)            element e of the frame's [kk][n_coord] gradient
//   IO::kCell (a compile-time flag): the frame in LDS is made whole first and the gradient image is seen
//   before the store -  void IO::whole(xs, nc, frame, lane)  in place on the staged frame, every lane, behind the load's barrier;
//                       void IO::finish(xs, grad, nc, frame, lane)  the one row about to be stored (the virial)
#pragma once
#include "cvf_cv_shared.hpp"
#include "cvf_cv_shared_sweep.hpp"
#include "cvf_features.hpp"
#include "cvf_metric.hpp"

namespace cvfr {

constexpr int kMaxCoordAlign = 192;      // the limit of the lane-per-frame family (k1_align.hip): at most 64 atoms, one per lane
constexpr int kMaxCoordIdentity = 512;
constexpr int kMaxIn = 512, kMaxInner = 256;
constexpr int kMaxLds = 64 * 1024;
#define CVFR_RECIPE "take the three-call recipe (cvf_align_feature_fwd, cvf_cv_nets_eval, cvf_align_feature_vjp_rows)"

// LDS of a workgroup, offsets in floats
struct FrLayout {
  int a[CVF_MAX_LAYERS + 1];   // layer l's activations, [chain][dims[l]] (a[0]: the features, shared by the chains)
  int xs, v0, v1, g, ctab, gimg, zs, total;
  int L, k, nn, form_a;
  int ns, t0, t1;              // form C: the trunk's layers (a[1..ns] hold one chain), two images [vector][width] of its sweep
};

// The body of a kernel of 64 threads, grid B.  SHARED: form C (an instance of its own: forms A and B keep their code); IO: above.
// `contracted` (uniform): IO::seeds will answer a pointer - the coordinate part has one row.
template <bool SHARED, class IO>
__device__ __forceinline__ void cv_frame_body(const cvf_mlp_desc& mlp, const cvf_pp_desc& pp, const FrLayout& lay,
                                              const float* __restrict__ theta, float* __restrict__ xi_rows, const bool contracted,
                                              const IO& io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const int64_t frame = blockIdx.x;
  const int nc = pp.n_coord, d0 = mlp.dims[0], L = lay.L, k = lay.k, nn = lay.nn;
  const int kk = contracted ? 1 : k;   // cotangent rows of the coordinate part
  const bool identity = pp.mode == CVF_PP_IDENTITY, aligned = pp.mode == CVF_PP_ALIGN;
  float* xs = lds + lay.xs;
  float* a0 = lds + lay.a[0];               // identity: the frame itself
  float* gimg = lds + lay.gimg;
  for (int j = lane; j < nc; j += CVF_WAVE) xs[j] = io.load(frame, nc, j);
  if (!identity) {
    for (int j = lane; j < d0; j += CVF_WAVE) a0[j] = 0.0f;
    for (int j = lane; j < kk * nc; j += CVF_WAVE) gimg[j] = 0.0f;
  }
  lds_barrier();
  if constexpr (IO::kCell) {
    io.whole(xs, nc, frame, lane);
    lds_barrier();
  }

  // ---- alignment: every lane ends with the same R, centroid and Kinv
  float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Kinv[6] = {0, 0, 0, 0, 0, 0};
  Centre c = centre_of(0.0f, 0.0f, 0.0f);
  if (aligned) {
    const bool on = lane < pp.n_align;
    const int b = on ? lane : 0;
    const V3 xb = atom_xyz(xs, pp.align_idx[b]);
    const float wb = on ? (pp.align_w != nullptr ? pp.align_w[b] : 1.0f) : 0.0f;   // (mean 1: the centroid divides by n_align)
    const float on_f = on ? 1.0f : 0.0f;
    const V3 rf = on_f * v3(pp.ref_c[3 * b], pp.ref_c[3 * b + 1], pp.ref_c[3 * b + 2]);   // (carries the weight already)
    const double inv = 1.0 / (double)pp.n_align;
    double cd[3];
    cd[0] = wave_sum((double)wb * (double)xb.x) * inv;
    cd[1] = wave_sum((double)wb * (double)xb.y) * inv;
    cd[2] = wave_sum((double)wb * (double)xb.z) * inv;
    const double dx[3] = {(double)xb.x - cd[0], (double)xb.y - cd[1], (double)xb.z - cd[2]};
    const double rr[3] = {(double)rf.x, (double)rf.y, (double)rf.z};   // 0 on lanes past the align set
    double H[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) H[i][j] = wave_sum(dx[i] * rr[j]);
    KabschOut ko;
    kabsch_from_H(H, ko);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ko.R[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) Kinv[i] = ko.Kinv[i];
    c = centre_of(cd);
  }

  // ---- features: records over the lanes
  if (!identity) {
    for (int r = lane; r < pp.n_rec; r += CVF_WAVE) {
      const Rec rc = load_rec(pp.rec, r);
      if (rc.type == CVF_FEAT_POSITION) {
        const V3 al = aligned ? row_times(centred(xs, rc.a[0], c), R) : atom_xyz(xs, rc.a[0]);
        a0[rc.out] = al.x;
        a0[rc.out + 1] = al.y;
        a0[rc.out + 2] = al.z;
      } else if (rc.type >= 0 && rc.type < CVF_FEAT_POSITION) {
        invariant_values(rc.type, pp.use_angle_value, [&](int q) { return atom_xyz(xs, rc.a[q]); },
                         [&](int j, float v) { a0[rc.out + j] = v; });
      }
    }
    lds_barrier();
  }

  // ---- nets forward: unit u = (chain, output) over the lanes
  for (int l = 0; l < L; ++l) {
    const int din = mlp.dims[l], dout = mlp.dims[l + 1], act = mlp.act[l];
    const float* ain = lds + lay.a[l];
    float* aout = lds + lay.a[l + 1];
    const int nch = SHARED && l < lay.ns ? 1 : nn;   // (the trunk runs once)
    for (int u = lane; u < nch * dout; u += CVF_WAVE) {
      const int ch = u / dout, j = u - ch * dout;
      const float* w = theta + mlp.w_off[ch][l] + (int64_t)j * din;
      const float* ai = ain + (l == 0 || (SHARED && l <= lay.ns) ? 0 : ch * din);
      float acc = 0.0f;
#pragma unroll 4
      for (int i = 0; i < din; ++i) acc = fmaf(w[i], ai[i], acc);
      aout[u] = cvf_act(act, acc + theta[mlp.b_off[ch][l] + j]);
    }
    lds_barrier();
  }
  {
    const float* top = lds + lay.a[L];   // form A: chain i's one output; form B: output i of the chain
    for (int i = lane; i < k; i += CVF_WAVE) xi_rows[frame * k + i] = top[i];
  }
  // the frame's k seeds of the contracted sweep (a policy that derives them from xi has room for 2 k floats behind the layout)
  const float* cf = io.seeds(lds + lay.total, lds + lay.a[L], frame, k, lane);

  // ---- sweep: one per CV, or one per chain with the coefficient as the seed
  float* g = lds + lay.g;
  if (SHARED) {   // form C: the heads down to the boundary, then the kk vectors through the trunk together
    const CvfFormCLds fl = {lay.a, lay.v0, lay.v1, lay.t0, lay.t1, lay.g};
    cvf_form_c_sweep<CVF_WAVE>(mlp, theta, contracted ? cf : nullptr, lds, fl, L, k, lay.ns, lane);
  }
  const int nsweep = SHARED ? 0 : (lay.form_a ? k : kk);
  for (int s = 0; s < nsweep; ++s) {
    const int ch = lay.form_a ? s : 0;
    float* grow = g + (contracted ? 0 : s) * d0;
    const bool accum = contracted && s > 0;
    float* vc = lds + lay.v0;
    float* vn = lds + lay.v1;
    const int dL = mlp.dims[L];
    for (int m = lane; m < dL; m += CVF_WAVE) {
      float seed;
      if (lay.form_a) seed = contracted ? cf[s] : 1.0f;
      else seed = contracted ? cf[m] : (m == s ? 1.0f : 0.0f);
      vc[m] = seed;
    }
    lds_barrier();
    for (int l = L - 1; l >= 0; --l) {
      const int din = mlp.dims[l], dout = mlp.dims[l + 1], act = mlp.act[l];
      const float* ah = lds + lay.a[l + 1] + ch * dout;
      for (int m = lane; m < dout; m += CVF_WAVE) vc[m] *= cvf_act_d1(act, ah[m]);
      lds_barrier();
      const float* w = theta + mlp.w_off[ch][l];
      float* dst = l > 0 ? vn : grow;
      for (int j = lane; j < din; j += CVF_WAVE) {
        float acc = 0.0f;
#pragma unroll 4
        for (int m = 0; m < dout; ++m) acc = fmaf(w[(int64_t)m * din + j], vc[m], acc);
        dst[j] = (l == 0 && accum) ? dst[j] + acc : acc;
      }
      lds_barrier();
      float* t = vc;
      vc = vn;
      vn = t;
    }
  }

  // ---- coordinate part
  if (identity) {   // d xi / d x = d xi / d r
    if constexpr (IO::kCell) io.finish(xs, g, nc, frame, lane);
    for (int e = lane; e < kk * nc; e += CVF_WAVE) io.store(frame, kk, nc, e, g[e]);
    return;
  }
  const int n_rec = pp.n_rec;
  float* ctab = lds + lay.ctab;   // [row][record][4][3]
  // phase 1, lane = record
  for (int r = lane; r < n_rec; r += CVF_WAVE) {
    const Rec rc = load_rec(pp.rec, r);
    if (rc.type == CVF_FEAT_POSITION) {
      for (int ii = 0; ii < kk; ++ii) {
        const float* gr = g + ii * d0 + rc.out;
        const V3 gv = v3(gr[0], gr[1], gr[2]);
        const V3 pr = aligned ? mat_times(R, gv) : gv;
        float* ct = ctab + ((ii * n_rec + r) * 4) * 3;
        ct[0] = pr.x;
        ct[1] = pr.y;
        ct[2] = pr.z;
      }
    } else if (rc.type >= 0 && rc.type < CVF_FEAT_POSITION) {
      invariant_vjp(rc.type, pp.use_angle_value, kk, [&](int q) { return atom_xyz(xs, rc.a[q]); },
                    [&](int ii, int j) { return g[ii * d0 + rc.out + j]; },
                    [&](int ii, int q, V3 v) {
                      float* ct = ctab + ((ii * n_rec + r) * 4 + q) * 3;
                      ct[0] = v.x;
                      ct[1] = v.y;
                      ct[2] = v.z;
                    });
    }
  }
  lds_barrier();
  const bool rot = aligned && pp.has_position != 0;
  float* zs = lds + lay.zs;   // [row][12]: Z, shift
  if (rot) {
    for (int ii = 0; ii < kk; ++ii) {
      float M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      V3 sp = v3(0, 0, 0);
      for (int r = lane; r < n_rec; r += CVF_WAVE) {
        const int32_t* p = pp.rec + 6 * r;
        if (p[0] == CVF_FEAT_POSITION) {
          const float* gr = g + ii * d0 + p[5];
          outer_add(M, centred(xs, p[1], c), v3(gr[0], gr[1], gr[2]));
          const float* ct = ctab + ((ii * n_rec + r) * 4) * 3;
          sp = sp + v3(ct[0], ct[1], ct[2]);
        }
      }
      float Ms[9], Z[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) Ms[j] = (float)wave_sum((double)M[j]);
      const V3 sps = v3((float)wave_sum((double)sp.x), (float)wave_sum((double)sp.y), (float)wave_sum((double)sp.z));
      rotation_term(R, Kinv, Ms, Z);
      const V3 shift = (1.0f / (float)pp.n_align) * sps;
      if (lane == 0) {
        float* z = zs + ii * 12;
#pragma unroll
        for (int j = 0; j < 9; ++j) z[j] = Z[j];
        z[9] = shift.x;
        z[10] = shift.y;
        z[11] = shift.z;
      }
    }
  }
  // phase 2, lane = atom (at most 64 atoms): the atom's entries in record order
  {
    const bool active = 3 * lane < nc;
    for (int r = 0; r < n_rec; ++r) {
      const int32_t* p = pp.rec + 6 * r;
      const int type = p[0];
      const int na = type == CVF_FEAT_POSITION ? 1 : type == CVF_FEAT_BOND ? 2 : type == CVF_FEAT_ANGLE ? 3 : type == CVF_FEAT_DIHEDRAL ? 4 : 0;
      for (int q = 0; q < na; ++q) {
        if (active && p[1 + q] == lane) {
          for (int ii = 0; ii < kk; ++ii) {
            const float* ct = ctab + ((ii * n_rec + r) * 4 + q) * 3;
            float* G = gimg + ii * nc + 3 * lane;
            G[0] += ct[0];
            G[1] += ct[1];
            G[2] += ct[2];
          }
        }
      }
    }
  }
  lds_barrier();
  if (rot && lane < pp.n_align) {   // lane = align atom: Z ref_b - w_b shift
    const int at = pp.align_idx[lane];
    const V3 rf = v3(pp.ref_c[3 * lane], pp.ref_c[3 * lane + 1], pp.ref_c[3 * lane + 2]);
    const float wb = pp.align_w != nullptr ? pp.align_w[lane] : 1.0f;
    for (int ii = 0; ii < kk; ++ii) {
      const float* z = zs + ii * 12;
      const V3 d = mat_times(z, rf) - wb * v3(z[9], z[10], z[11]);
      float* G = gimg + ii * nc + 3 * at;
      G[0] += d.x;
      G[1] += d.y;
      G[2] += d.z;
    }
  }
  lds_barrier();
  if constexpr (IO::kCell) io.finish(xs, gimg, nc, frame, lane);
  for (int e = lane; e < kk * nc; e += CVF_WAVE) io.store(frame, kk, nc, e, gimg[e]);
}

// nullptr and *lay filled, or why the launch declines the model (ns > 0: form C, which the caller has checked with
// cvf_form_c_why - k = n_nets scalar chains, whole, the first ns layers one trunk).  extra_per_k: floats per CV that the launch
// keeps behind the layout (lay->total is the layout's own total; the limit counts both).
inline const char* cvfr_why(const cvf_mlp_desc* mlp, int upto, const cvf_pp_desc* pp, FrLayout* lay, int ns = 0, int extra_per_k = 0) {
  static thread_local char buf[320];
#define CVFR_NO(...)                                              \
  do {                                                            \
    const int n_ = snprintf(buf, sizeof buf, __VA_ARGS__);        \
    if (n_ > 0 && n_ < (int)sizeof buf) snprintf(buf + n_, sizeof buf - n_, "; " CVFR_RECIPE); \
    return buf;                                                   \
  } while (0)
  if (mlp == nullptr || pp == nullptr) CVFR_NO("no model or layer description");
  if (mlp->n_nets < 1 || mlp->n_nets > CVF_MAX_NETS) CVFR_NO("%d nets: 1 to %d are supported", mlp->n_nets, CVF_MAX_NETS);
  if (mlp->n_layers < 1 || mlp->n_layers > CVF_MAX_LAYERS) CVFR_NO("%d layers: 1 to %d are supported", mlp->n_layers, CVF_MAX_LAYERS);
  if (upto < 1 || upto > mlp->n_layers) CVFR_NO("upto_layer=%d out of range (the model has %d layers)", upto, mlp->n_layers);
  const bool form_a = mlp->n_nets > 1 || ns > 0;
  if (form_a && upto != mlp->n_layers) CVFR_NO("%d nets side by side are evaluated whole: upto_layer must be %d", mlp->n_nets, mlp->n_layers);
  if (form_a && mlp->dims[upto] != 1) CVFR_NO("%d nets side by side must be scalar (they have %d outputs each)", mlp->n_nets, mlp->dims[upto]);
  const int k = form_a ? mlp->n_nets : mlp->dims[upto];
  if (k < 1 || k > CVF_MAX_NETS) CVFR_NO("k = %d outputs: 1 to %d are supported", k, CVF_MAX_NETS);
  if (mlp->dims[0] < 1 || mlp->dims[0] > kMaxIn) CVFR_NO("dims[0] = %d: the one-launch kernel takes 1 to %d inputs", mlp->dims[0], kMaxIn);
  for (int l = 1; l < upto; ++l)
    if (mlp->dims[l] < 1 || mlp->dims[l] > kMaxInner) CVFR_NO("layer %d is %d wide: the one-launch kernel takes inner widths 1 to %d", l, mlp->dims[l], kMaxInner);
  for (int l = 0; l < upto; ++l)
    if (mlp->act[l] < CVF_ACT_NONE || mlp->act[l] > CVF_ACT_SOFTPLUS) CVFR_NO("act[%d] = %d is no activation code", l, mlp->act[l]);
  const int nn = form_a ? mlp->n_nets : 1;
  for (int i = 0; i < nn; ++i)
    for (int l = 0; l < upto; ++l)
      if (mlp->w_off[i][l] < 0 || mlp->b_off[i][l] < 0) CVFR_NO("a negative parameter offset");
  const int nc = pp->n_coord;
  if (pp->mode == CVF_PP_FACTORED) CVFR_NO("CVF_PP_FACTORED records come from a torch module: the one-launch kernel takes coordinates");
  if (pp->mode == CVF_PP_IDENTITY) {
    if (nc < 1 || nc > kMaxCoordIdentity) CVFR_NO("identity preprocessing with n_coord = %d: the one-launch kernel takes 1 to %d", nc, kMaxCoordIdentity);
    if (pp->d_r != nc) CVFR_NO("identity preprocessing needs d_r == n_coord");
  } else if (pp->mode == CVF_PP_ALIGN || pp->mode == CVF_PP_FEATURES) {
    if (nc < 3 || nc % 3 != 0) CVFR_NO("malformed descriptor (n_coord=%d)", nc);
    if (nc > kMaxCoordAlign) CVFR_NO("frames of n_coord = %d coordinates: the one-launch kernel takes at most %d (64 atoms, one per lane)", nc, kMaxCoordAlign);
    if (pp->n_rec < 1 || pp->rec == nullptr || pp->d_r < 1) CVFR_NO("malformed descriptor (n_rec=%d d_r=%d)", pp->n_rec, pp->d_r);
    if (pp->mode == CVF_PP_ALIGN && (pp->n_align < 3 || pp->n_align > CVF_WAVE || pp->align_idx == nullptr || pp->ref_c == nullptr))
      CVFR_NO("malformed descriptor or more than 64 align atoms (n_align=%d)", pp->n_align);
  } else {
    CVFR_NO("unknown pp mode %d", pp->mode);
  }
  if (mlp->dims[0] != pp->d_r) CVFR_NO("the nets take %d features, the preprocessing layer gives %d", mlp->dims[0], pp->d_r);
  // the LDS of one frame
  FrLayout L = {};
  L.L = upto; L.k = k; L.nn = nn; L.form_a = form_a ? 1 : 0; L.ns = ns;
  const bool identity = pp->mode == CVF_PP_IDENTITY;
  int64_t pos = 0;
  L.xs = 0;
  pos += nc;
  L.a[0] = identity ? 0 : (int)pos;
  if (!identity) pos += mlp->dims[0];
  int vmax = 1, tmax = 0;   // the widest image of a head's sweep (forms A and B: of the sweep), of the trunk's
  for (int l = 1; l <= upto; ++l) {
    L.a[l] = (int)pos;
    pos += (int64_t)(l <= ns ? 1 : nn) * mlp->dims[l];
    if (l > ns) vmax = mlp->dims[l] > vmax ? mlp->dims[l] : vmax;
    else tmax = mlp->dims[l] > tmax ? mlp->dims[l] : tmax;
  }
  L.v0 = (int)pos; pos += vmax;
  L.v1 = (int)pos; pos += vmax;
  L.t0 = (int)pos; pos += (int64_t)k * tmax;
  L.t1 = (int)pos; pos += (int64_t)k * tmax;
  L.g = (int)pos; pos += (int64_t)k * mlp->dims[0];
  if (!identity) {
    L.ctab = (int)pos; pos += (int64_t)k * pp->n_rec * 12;
    L.gimg = (int)pos; pos += (int64_t)k * nc;
    L.zs = (int)pos; pos += (int64_t)k * 12;
  }
  L.total = (int)(pos < 0x7fffffff / 4 ? pos : 0x7fffffff / 4);
  pos += (int64_t)extra_per_k * k;
  if (pos * 4 > kMaxLds) CVFR_NO("one frame needs %lld bytes of LDS, the one-launch kernel keeps within %d", (long long)pos * 4, kMaxLds);
  if (lay != nullptr) *lay = L;
  return nullptr;
#undef CVFR_NO
}

inline const char* cvfr_shared_why(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp, FrLayout* lay,
                                   const char* plain = "cvf_cv_frame_eval", int extra_per_k = 0) {
  static thread_local char buf[240];
  const char* why = cvf_form_c_why(mlp, n_shared, plain, buf, sizeof buf);
  return why != nullptr ? why : cvfr_why(mlp, mlp->n_layers, pp, lay, n_shared, extra_per_k);
}

}  // namespace cvfr
