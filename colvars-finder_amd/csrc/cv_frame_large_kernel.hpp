// xi(x) and d xi / d x of a trained CV per frame in ONE launch for frames of ANY size: one WORKGROUP (256 threads) = one frame
// (cvf_cv_frame_large_*).  The sibling of csrc/cv_frame.hip (one wave per frame, at most 64 atoms): the
// same nets' arithmetic, the alignment and the coordinate part after the large-frame kernels of the three-call recipe
// (csrc/k1_large.hip, csrc/k1_vjp_large.hpp), everything between the coordinates and the gradient in the workgroup's LDS.  The
// frame itself stays in global memory (60 KB at 5000 atoms: read once into L2).
//
//   alignment   align atoms strided over the threads; the fifteen moments sum w x (3), sum x (x) ref_c (9), sum ref_c (3) of
//               k1_large.hip in fp64: wave_sum inside each wave, the four waves in index order through LDS; then every thread runs
//               the solver of cvf_kabsch.hpp on the same H = sum x (x) ref_c - c (x) sum ref_c: R, the centroid and Kinv without
//               an aux buffer
//   features    mrec records strided over the threads, atoms read through slot_atom -> a_0 = r [d_r]      (cvf_features.hpp)
//   forward     thread j owns output units j, j + 256, ..: a_{l+1} = act_l(W_l a_l + b_l), each dot product one sequential fmaf
//               chain in index order, the bias added last (cv_frame_kernel's arithmetic)
//   sweep       v_L = e_i (or coef), v_l = W_l^T (act_l'(a_{l+1}) .* v_{l+1}) -> g_i = d xi_i / d r [d_r] per CV, or the one
//               contracted g = sum_i coef_i g_i
//   coordinates in passes of rows_per_pass cotangent rows (the row table is n_ref * 12 bytes per row):
//               phase A, thread = record: one row per (record, atom) pair into the LDS row table; M = sum_p xc_p (x) g_p and
//               sum_p R g_p per thread in record order, wave_sumf, the four waves in index order;
//               phase B, thread = slot: the slot's rows slot_row[t] .. slot_row[t+1]-1 summed in order;
//               dense write, thread = coordinates: Z ref_b - w_b shift through atom_align plus the slot sum through atom_slot,
//               an exact 0.0f on every other atom; every element of the [kk][n_coord] output written exactly once, coalesced
//
// No atomics, no scratch, no aux.  A frame meets the same instructions in the same order whatever B is, wherever it sits in the
// batch and whichever pass a row falls in, so its result depends on its coordinates and theta only, bit for bit.
//
// Form C (cvf_cv_frame_large_shared_*) as in csrc/cv_frame.hip: the trunk's activations once, its forward
// pass dims[l+1] units over the threads, the k head sweeps down to layer n_shared, the k vectors (with coef: their one sum)
// through the shared weights together.
//
// This header holds the kernel's body, its LDS layout and its predicate ONCE, for two translation units (as cv_frame_kernel.hpp
// does for the wave kernel).  Where an atom lies, where the sweep's seed comes from and where the gradient goes is an IO policy:
//   csrc/cv_frame_large.hip   cvf_cv_frame_large_*        dense x [B][n_coord], the seed from the global coef, gx_rows written
//   csrc/cv_bias.hip          cvf_cv_frame_large_bias_*   an MD engine's arrays through cvf_md_layout, the seed -dU/dxi from the xi
//                                                         in LDS (cvf_bias.hpp), the force accumulated
//   const float* IO::atom(frame, a)                        the three coordinates of atom a of the frame
//   const float* IO::seeds(spare, top, frame, k, tid)      once xi = top[0..k) is in LDS: the frame's k seeds of the contracted
//                                                          sweep (global, or in `spare` behind a barrier), or unused for k rows
//   float*       IO::out(frame, kk, nc)                    the frame's gradient rows
//   void         IO::put(rows, nc, ii, j, A, c, v)         coordinate j = 3 A + c of row ii of the pass (VEC4 instances write
//                                                          float4s through `rows` themselves: dense policies only), or, with
//   IO::kByAtom: void IO::put_atom(rows, nc, ii, A, v)     the three coordinates of atom A at once, thread = atom
//   IO::kCell (a compile-time flag): the atoms are read as a whole molecule -
//     void IO::prologue(words, red, frame, n_atoms, tid)    every atom's summed image triple into n_atoms LDS words, all threads
//                                                           (red: the moments' LDS, free before the alignment)
//     V3   IO::whole(words, frame, a)                        atom a at its whole position (what xyz and xyz_c below read)
//     void IO::finish(red, frame, tid)                       behind the store loop of a pass, all threads (the virial)
//   `words` lies behind the one row table of the contracted form (lay.rows + 3 n_ref floats in): cvfl_why's `extra` floats.
#pragma once
#include "cvf_cv_shared.hpp"
#include "cvf_cv_shared_sweep.hpp"
#include "cvf_features.hpp"
#include "cvf_metric.hpp"

namespace cvfl {

constexpr int kThreads = 256, kWaves = kThreads / CVF_WAVE;
constexpr int kMaxIn = 512, kMaxInner = 256;   // the nets' limits of cv_frame_kernel
constexpr int kMaxLds = 160 * 1024;            // gfx950: the LDS of a compute unit, all of it for one workgroup
constexpr int kRedD = 2 * kWaves * 16;         // floats: [wave][16] doubles of the alignment's moments
constexpr int kRedF = CVF_MAX_NETS * kWaves * 12, kZs = CVF_MAX_NETS * 12;
#define CVFL_RECIPE "take the three-call recipe (cvf_align_feature_fwd, cvf_cv_nets_eval, cvf_align_feature_vjp_rows)"

// LDS of a workgroup, offsets in floats
struct LgLayout {
  int a[CVF_MAX_LAYERS + 1];   // layer l's activations, [chain][dims[l]] (a[0]: the features, shared by the chains)
  int v0, v1, g, redd, redf, zs, rows, total;
  int L, k, nn, form_a;
  int rpp;                     // cotangent rows per pass of the coordinate part (1 .. k)
  int ns, t0, t1;              // form C: the trunk's layers (a[1..ns] hold one chain), two images [vector][width] of its sweep
};

struct MRec {
  int type, out, s[4], r[4];
};
__device__ __forceinline__ MRec load_mrec(const int32_t* mrec, int r) {   // include/cvf.h: cvf_pp_desc.mrec
  const int4 m0 = reinterpret_cast<const int4*>(mrec)[2 * r];
  const int4 m1 = reinterpret_cast<const int4*>(mrec)[2 * r + 1];
  MRec d;
  d.type = (m0.x & 7) - 1;
  d.out = (int)((unsigned)m0.x >> 3);
  d.s[0] = m0.y & 0xffff; d.s[1] = (int)((unsigned)m0.y >> 16); d.s[2] = m0.z & 0xffff; d.s[3] = (int)((unsigned)m0.z >> 16);
  const int off = m1.y;
  d.r[0] = (m0.w & 0xffff) + (off & 0xff);
  d.r[1] = (int)((unsigned)m0.w >> 16) + ((off >> 8) & 0xff);
  d.r[2] = (m1.x & 0xffff) + ((off >> 16) & 0xff);
  d.r[3] = (int)((unsigned)m1.x >> 16) + (int)((unsigned)off >> 24);
  return d;
}

// The body of a kernel of kThreads threads, grid B.  MODE: 0 CVF_PP_FEATURES, 1 CVF_PP_ALIGN with uniform weights, 2 CVF_PP_ALIGN
// with align_w (instances, not branches: the uniform values of the other modes stay out of the scalar registers); SHARED: form C;
// IO: above.  `contracted` (uniform): IO::seeds answers the seeds - the coordinate part has
// one row.  VEC4 (16-byte stores of the dense rows) is for policies whose rows are dense.
template <bool VEC4, int MODE, bool SHARED, class IO>
__device__ __forceinline__ void cv_frame_large_body(const cvf_mlp_desc& mlp, const cvf_pp_desc& pp, const LgLayout& lay,
                                                    const float* __restrict__ theta, float* __restrict__ xi_rows, const bool contracted,
                                                    const IO& io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t frame = blockIdx.x;
  const int nc = pp.n_coord, d0 = mlp.dims[0], L = lay.L, k = lay.k, nn = lay.nn;
  const int kk = contracted ? 1 : k;   // cotangent rows of the coordinate part
  constexpr bool aligned = MODE != 0, weighted = MODE == 2;
  uint32_t* words = reinterpret_cast<uint32_t*>(lds + lay.rows + 3 * pp.n_ref);   // (kCell only)
  auto xyz = [&](int a) {
    if constexpr (IO::kCell) return io.whole(words, frame, a);
    else return atom_xyz(io.atom(frame, a), 0);
  };
  auto xyz_c = [&](int a, const Centre& ce) {
    if constexpr (IO::kCell) {
      const V3 p = io.whole(words, frame, a);
      const float t[3] = {p.x, p.y, p.z};
      return centred(t, 0, ce);
    } else {
      return centred(io.atom(frame, a), 0, ce);
    }
  };
  float* a0 = lds + lay.a[0];
  // The tables and the output of the dense write, used last, live in VECTOR registers from here on (the kernel has them to spare):
  // as uniform values they would sit in the scalar registers through every phase before, which are what this kernel runs out of.
  const int32_t* t_align = pp.atom_align;
  const int32_t* t_slot = pp.atom_slot;
  const float* t_ref = pp.ref_c;
  const float* t_w = pp.align_w;
  float* gx_frame = io.out(frame, kk, nc);
  asm volatile("" : "+v"(t_align), "+v"(t_slot), "+v"(t_ref), "+v"(t_w), "+v"(gx_frame));
  for (int j = tid; j < d0; j += kThreads) a0[j] = 0.0f;
  if constexpr (IO::kCell) {
    io.prologue(words, lds + lay.redd, frame, nc / 3, tid);
    lds_barrier();
  }

  // ---- alignment: every thread ends with the same R, centroid and Kinv
  float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Kinv[6] = {0, 0, 0, 0, 0, 0};
  Centre c = centre_of(0.0f, 0.0f, 0.0f);
  if (aligned) {
    double acc[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) acc[i] = 0.0;
    for (int b = tid; b < pp.n_align; b += kThreads) {
      const V3 xb = xyz(pp.align_idx[b]);
      const double d[3] = {(double)xb.x, (double)xb.y, (double)xb.z};
      const double e[3] = {(double)pp.ref_c[3 * b], (double)pp.ref_c[3 * b + 1], (double)pp.ref_c[3 * b + 2]};   // (carries the weight already)
      const double wb = weighted ? (double)pp.align_w[b] : 1.0;   // (mean 1: the centroid divides by n_align)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        acc[i] = fma(wb, d[i], acc[i]);
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 + 3 * i + j] = fma(d[i], e[j], acc[3 + 3 * i + j]);
        acc[12 + i] += e[i];
      }
    }
    double* redd = reinterpret_cast<double*>(lds + lay.redd);
#pragma unroll
    for (int i = 0; i < 15; ++i) {
      const double sv = wave_sum(acc[i]);
      if (lane == 0) redd[wave * 16 + i] = sv;
    }
    lds_barrier();
    double t[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) {
      double v = redd[i];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += redd[w * 16 + i];
      t[i] = v;
    }
    const double inv = 1.0 / (double)pp.n_align;
    const double cd[3] = {t[0] * inv, t[1] * inv, t[2] * inv};
    double H[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) H[i][j] = t[3 + 3 * i + j] - cd[i] * t[12 + j];
    KabschOut ko;
    kabsch_from_H(H, ko);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ko.R[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) Kinv[i] = ko.Kinv[i];
    c = centre_of(cd);
  }
  lds_barrier();   // (a_0 is zero everywhere before a record writes into it)

  // ---- features: records over the threads
  for (int r = tid; r < pp.n_mrec; r += kThreads) {
    const MRec rc = load_mrec(pp.mrec, r);
    if (rc.type == CVF_FEAT_POSITION) {
      const int at = pp.slot_atom[rc.s[0]];
      const V3 al = aligned ? row_times(xyz_c(at, c), R) : xyz(at);
      a0[rc.out] = al.x;
      a0[rc.out + 1] = al.y;
      a0[rc.out + 2] = al.z;
    } else if (rc.type >= 0 && rc.type < CVF_FEAT_POSITION) {
      invariant_values(rc.type, pp.use_angle_value, [&](int q) { return xyz(pp.slot_atom[rc.s[q]]); },
                       [&](int j, float v) { a0[rc.out + j] = v; });
    }
  }
  lds_barrier();

  // ---- nets forward: unit u = (chain, output) over the threads
  for (int l = 0; l < L; ++l) {
    const int din = mlp.dims[l], dout = mlp.dims[l + 1], act = mlp.act[l];
    const float* ain = lds + lay.a[l];
    float* aout = lds + lay.a[l + 1];
    const int nch = SHARED && l < lay.ns ? 1 : nn;   // (the trunk runs once)
    for (int u = tid; u < nch * dout; u += kThreads) {
      const int ch = u / dout, j = u - ch * dout;
      const float* w = theta + mlp.w_off[ch][l] + (int64_t)j * din;
      const float* ai = ain + (l == 0 || (SHARED && l <= lay.ns) ? 0 : ch * din);
      float acc = 0.0f;
#pragma unroll 8
      for (int i = 0; i < din; ++i) acc = fmaf(w[i], ai[i], acc);
      aout[u] = cvf_act(act, acc + theta[mlp.b_off[ch][l] + j]);
    }
    lds_barrier();
  }
  {
    const float* top = lds + lay.a[L];   // form A: chain i's one output; form B: output i of the chain
    for (int i = tid; i < k; i += kThreads) xi_rows[frame * k + i] = top[i];
  }
  // the frame's k seeds of the contracted sweep (a policy that derives them from xi has the moments' LDS, free by now, for 2 k floats)
  const float* cf = io.seeds(lds + lay.redd, lds + lay.a[L], frame, k, tid);

  // ---- sweep: one per CV, or one per chain with the coefficient as the seed
  float* g = lds + lay.g;
  if (SHARED) {   // form C: the heads down to the boundary, then the kk vectors through the trunk together
    const CvfFormCLds fl = {lay.a, lay.v0, lay.v1, lay.t0, lay.t1, lay.g};
    cvf_form_c_sweep<kThreads>(mlp, theta, contracted ? cf : nullptr, lds, fl, L, k, lay.ns, tid);
  }
  const int nsweep = SHARED ? 0 : (lay.form_a ? k : kk);
  for (int s = 0; s < nsweep; ++s) {
    const int ch = lay.form_a ? s : 0;
    float* grow = g + (contracted ? 0 : s) * d0;
    const bool accum = contracted && s > 0;
    float* vc = lds + lay.v0;
    float* vn = lds + lay.v1;
    const int dL = mlp.dims[L];
    for (int m = tid; m < dL; m += kThreads) {
      float seed;
      if (lay.form_a) seed = contracted ? cf[s] : 1.0f;
      else seed = contracted ? cf[m] : (m == s ? 1.0f : 0.0f);
      vc[m] = seed;
    }
    lds_barrier();
    for (int l = L - 1; l >= 0; --l) {
      const int din = mlp.dims[l], dout = mlp.dims[l + 1], act = mlp.act[l];
      const float* ah = lds + lay.a[l + 1] + ch * dout;
      for (int m = tid; m < dout; m += kThreads) vc[m] *= cvf_act_d1(act, ah[m]);
      lds_barrier();
      const float* w = theta + mlp.w_off[ch][l];
      float* dst = l > 0 ? vn : grow;
      for (int j = tid; j < din; j += kThreads) {
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

  // ---- coordinate part, rows_per_pass cotangent rows at a time
  const int nrow = 3 * pp.n_ref;
  const bool rot = aligned && pp.has_position != 0;
  float* rows = lds + lay.rows;    // [row of the pass][n_ref][3]
  float* redf = lds + lay.redf;    // [row of the pass][wave][12]: M, sum_p R g_p
  float* zs = lds + lay.zs;        // [row of the pass][12]: Z, shift
  auto put = [&](int ii, int row, V3 v) {
    float* p = rows + ii * nrow + 3 * row;
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
  };
  auto get = [&](int ii, int row) {
    const float* p = rows + ii * nrow + 3 * row;
    return v3(p[0], p[1], p[2]);
  };
  const int rpp = lay.rpp < kk ? lay.rpp : kk;
  for (int i0 = 0; i0 < kk; i0 += rpp) {
    const int ng = kk - i0 < rpp ? kk - i0 : rpp;
    // phase A, position records: row by row (M and sum_p are per-thread sums in the records' order)
    if (pp.has_position) {
      for (int ii = 0; ii < ng; ++ii) {
        const float* gr = g + (i0 + ii) * d0;
        float acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int r = tid; r < pp.n_mrec; r += kThreads) {
          const MRec rc = load_mrec(pp.mrec, r);
          if (rc.type != CVF_FEAT_POSITION) continue;
          const V3 gv = v3(gr[rc.out], gr[rc.out + 1], gr[rc.out + 2]);
          const V3 pr = aligned ? mat_times(R, gv) : gv;
          put(ii, rc.r[0], pr);
          if (rot) {
            outer_add(acc, xyz_c(pp.slot_atom[rc.s[0]], c), gv);
            acc[9] += pr.x; acc[10] += pr.y; acc[11] += pr.z;
          }
        }
        if (rot) {
          // (each wave sum is stored as soon as it is formed: twelve uniform sums alive at once overflow the scalar registers)
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            const float v = wave_sumf(acc[i]);
            if (lane == 0) redf[(ii * kWaves + wave) * 12 + i] = v;
          }
        }
      }
    }
    // phase A, the other records: the geometry once, then one product per row
    for (int r = tid; r < pp.n_mrec; r += kThreads) {
      const MRec rc = load_mrec(pp.mrec, r);
      if (rc.type < 0 || rc.type >= CVF_FEAT_POSITION) continue;
      invariant_vjp(rc.type, pp.use_angle_value, ng, [&](int q) { return xyz(pp.slot_atom[rc.s[q]]); },
                    [&](int ii, int j) { return g[(i0 + ii) * d0 + rc.out + j]; },
                    [&](int ii, int q, V3 v) { put(ii, rc.r[q], v); });
    }
    lds_barrier();
    // phase B, thread = slot: the slot's rows in order into its first row; thread ii < ng forms Z and the shift of row ii
    for (int ii = 0; ii < ng; ++ii) {
      for (int t = tid; t < pp.n_slot; t += kThreads) {
        const int q0 = pp.slot_row[t], q1 = pp.slot_row[t + 1];
        V3 s = get(ii, q0);
        for (int q = q0 + 1; q < q1; ++q) s = s + get(ii, q);
        put(ii, q0, s);
      }
    }
    if (rot && tid < ng) {
      float tot[12], Z[9];
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        float v = redf[(tid * kWaves) * 12 + i];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += redf[(tid * kWaves + w) * 12 + i];
        tot[i] = v;
      }
      rotation_term(R, Kinv, tot, Z);
      const V3 shift = (1.0f / (float)pp.n_align) * v3(tot[9], tot[10], tot[11]);
      float* z = zs + tid * 12;
#pragma unroll
      for (int i = 0; i < 9; ++i) z[i] = Z[i];
      z[9] = shift.x;
      z[10] = shift.y;
      z[11] = shift.z;
    }
    lds_barrier();
    // dense write: an atom's table entries are read once for all rows of the pass
    struct AtomRef {
      int b, q;
      V3 rf;
      float wb;
    };
    auto lookup = [&](int a) {
      AtomRef u;
      u.b = rot ? t_align[a] : -1;
      u.rf = u.b >= 0 ? v3(t_ref[3 * u.b], t_ref[3 * u.b + 1], t_ref[3 * u.b + 2]) : v3(0, 0, 0);
      u.wb = weighted && u.b >= 0 ? t_w[u.b] : 1.0f;
      const int t = t_slot[a];
      u.q = t >= 0 ? pp.slot_row[t] : -1;
      return u;
    };
    auto grad_of = [&](int ii, const AtomRef& u) {
      V3 v = v3(0, 0, 0);
      if (u.b >= 0) {
        const float* z = zs + ii * 12;
        v = mat_times(z, u.rf) - u.wb * v3(z[9], z[10], z[11]);
      }
      if (u.q >= 0) v = v + get(ii, u.q);
      return v;
    };
    float* gx0 = gx_frame + i0 * (int64_t)nc;
    if constexpr (VEC4) {   // nc % 4 == 0 and 16-byte rows: coordinates 4v .. 4v+3 lie in atoms A = 4v/3 and A + 1
      for (int v = tid; v < nc / 4; v += kThreads) {
        const int j0 = 4 * v, A = j0 / 3, k0 = j0 - 3 * A;
        const AtomRef ua = lookup(A), ub = lookup(A + 1);   // (4v + 3 < nc: atom A + 1 exists)
        float4* dst = reinterpret_cast<float4*>(gx0) + v;
#pragma unroll 1
        for (int ii = 0; ii < ng; ++ii, dst += nc / 4) {
          const V3 u = grad_of(ii, ua), w = grad_of(ii, ub);
          float4 o;
          o.x = k0 == 0 ? u.x : (k0 == 1 ? u.y : u.z);
          o.y = k0 == 0 ? u.y : (k0 == 1 ? u.z : w.x);
          o.z = k0 == 0 ? u.z : (k0 == 1 ? w.x : w.y);
          o.w = k0 == 0 ? w.x : (k0 == 1 ? w.y : w.z);
          *dst = o;
        }
      }
    } else if constexpr (IO::kByAtom) {   // thread = atom: its table entries read once, its three coordinates together
      for (int A = tid; A < nc / 3; A += kThreads) {
        const AtomRef ua = lookup(A);
        for (int ii = 0; ii < ng; ++ii) io.put_atom(gx0, nc, ii, A, grad_of(ii, ua));
      }
      if constexpr (IO::kCell) io.finish(redf, frame, tid);
    } else {
      for (int j = tid; j < nc; j += kThreads) {
        const int A = j / 3, kc = j - 3 * A;
        const AtomRef ua = lookup(A);
        for (int ii = 0; ii < ng; ++ii) {
          const V3 u = grad_of(ii, ua);
          io.put(gx0, nc, ii, j, A, kc, kc == 0 ? u.x : (kc == 1 ? u.y : u.z));
        }
      }
    }
    lds_barrier();   // (the next pass overwrites the row table)
  }
}

// nullptr and *lay filled, or why the launch declines the model (ns > 0: form C, which the caller has checked with
// cvf_form_c_why)
// `extra`: floats of LDS that the launch keeps behind ONE row of the contribution table (a contracted launch's own; the limit counts them)
inline const char* cvfl_why(const cvf_mlp_desc* mlp, int upto, const cvf_pp_desc* pp, LgLayout* lay, int ns = 0, int64_t extra = 0) {
  static thread_local char buf[360];
#define CVFL_NO(...)                                              \
  do {                                                            \
    const int n_ = snprintf(buf, sizeof buf, __VA_ARGS__);        \
    if (n_ > 0 && n_ < (int)sizeof buf) snprintf(buf + n_, sizeof buf - n_, "; " CVFL_RECIPE); \
    return buf;                                                   \
  } while (0)
  // the nets: the limits and the words of cv_frame.hip
  if (mlp == nullptr || pp == nullptr) CVFL_NO("no model or layer description");
  if (mlp->n_nets < 1 || mlp->n_nets > CVF_MAX_NETS) CVFL_NO("%d nets: 1 to %d are supported", mlp->n_nets, CVF_MAX_NETS);
  if (mlp->n_layers < 1 || mlp->n_layers > CVF_MAX_LAYERS) CVFL_NO("%d layers: 1 to %d are supported", mlp->n_layers, CVF_MAX_LAYERS);
  if (upto < 1 || upto > mlp->n_layers) CVFL_NO("upto_layer=%d out of range (the model has %d layers)", upto, mlp->n_layers);
  const bool form_a = mlp->n_nets > 1 || ns > 0;
  if (form_a && upto != mlp->n_layers) CVFL_NO("%d nets side by side are evaluated whole: upto_layer must be %d", mlp->n_nets, mlp->n_layers);
  if (form_a && mlp->dims[upto] != 1) CVFL_NO("%d nets side by side must be scalar (they have %d outputs each)", mlp->n_nets, mlp->dims[upto]);
  const int k = form_a ? mlp->n_nets : mlp->dims[upto];
  if (k < 1 || k > CVF_MAX_NETS) CVFL_NO("k = %d outputs: 1 to %d are supported", k, CVF_MAX_NETS);
  if (mlp->dims[0] < 1 || mlp->dims[0] > kMaxIn) CVFL_NO("dims[0] = %d: the one-launch kernel takes 1 to %d inputs", mlp->dims[0], kMaxIn);
  for (int l = 1; l < upto; ++l)
    if (mlp->dims[l] < 1 || mlp->dims[l] > kMaxInner) CVFL_NO("layer %d is %d wide: the one-launch kernel takes inner widths 1 to %d", l, mlp->dims[l], kMaxInner);
  for (int l = 0; l < upto; ++l)
    if (mlp->act[l] < CVF_ACT_NONE || mlp->act[l] > CVF_ACT_SOFTPLUS) CVFL_NO("act[%d] = %d is no activation code", l, mlp->act[l]);
  const int nn = form_a ? mlp->n_nets : 1;
  for (int i = 0; i < nn; ++i)
    for (int l = 0; l < upto; ++l)
      if (mlp->w_off[i][l] < 0 || mlp->b_off[i][l] < 0) CVFL_NO("a negative parameter offset");
  // the layer
  const int nc = pp->n_coord;
  if (pp->mode == CVF_PP_FACTORED) CVFL_NO("CVF_PP_FACTORED records come from a torch module: the one-launch kernel takes coordinates");
  if (pp->mode == CVF_PP_IDENTITY) CVFL_NO("CVF_PP_IDENTITY has no frame to align: the wave kernel (cvf_cv_frame_eval) takes it");
  if (pp->mode != CVF_PP_ALIGN && pp->mode != CVF_PP_FEATURES) CVFL_NO("unknown pp mode %d", pp->mode);
  if (nc < 3 || nc % 3 != 0) CVFL_NO("malformed descriptor (n_coord = %d is no positive multiple of 3)", nc);
  if (pp->d_r < 1) CVFL_NO("malformed descriptor (d_r=%d)", pp->d_r);
  if (pp->n_mrec < 1 || pp->mrec == nullptr) CVFL_NO("no mrec table (n_mrec = %d): the workgroup kernel walks the records through it", pp->n_mrec);
  if (pp->slot_row == nullptr) CVFL_NO("no slot_row table: the workgroup kernel sums an atom's contribution rows through it");
  if (pp->slot_atom == nullptr) CVFL_NO("no slot_atom table: the workgroup kernel reads the feature atoms through it");
  if (pp->atom_slot == nullptr) CVFL_NO("no atom_slot table: the workgroup kernel writes the dense gradient through it");
  if (pp->n_slot < 1 || pp->n_slot > CVF_FEATURES_MAX_SLOT) CVFL_NO("n_slot = %d distinct feature atoms: 1 to %d (CVF_FEATURES_MAX_SLOT)", pp->n_slot, CVF_FEATURES_MAX_SLOT);
  if (pp->n_ref < 1 || pp->n_ref > CVF_FEATURES_MAX_REF) CVFL_NO("n_ref = %d contribution rows: 1 to %d (CVF_FEATURES_MAX_REF)", pp->n_ref, CVF_FEATURES_MAX_REF);
  if (pp->mode == CVF_PP_ALIGN) {
    if (pp->n_align < 3 || pp->align_idx == nullptr || pp->ref_c == nullptr) CVFL_NO("malformed descriptor (n_align=%d)", pp->n_align);
    if (pp->atom_align == nullptr) CVFL_NO("no atom_align table: the workgroup kernel writes the align atoms' gradient through it");
  }
  if (mlp->dims[0] != pp->d_r) CVFL_NO("the nets take %d features, the preprocessing layer gives %d", mlp->dims[0], pp->d_r);
  // the LDS of one frame
  LgLayout Y = {};
  Y.L = upto; Y.k = k; Y.nn = nn; Y.form_a = form_a ? 1 : 0; Y.ns = ns;
  int64_t pos = 0;
  Y.a[0] = 0;
  pos += mlp->dims[0];
  int vmax = 1, tmax = 0;   // the widest image of a head's sweep (forms A and B: of the sweep), of the trunk's
  for (int l = 1; l <= upto; ++l) {
    Y.a[l] = (int)pos;
    pos += (int64_t)(l <= ns ? 1 : nn) * mlp->dims[l];
    if (l > ns) vmax = mlp->dims[l] > vmax ? mlp->dims[l] : vmax;
    else tmax = mlp->dims[l] > tmax ? mlp->dims[l] : tmax;
  }
  Y.v0 = (int)pos; pos += vmax;
  Y.v1 = (int)pos; pos += vmax;
  Y.t0 = (int)pos; pos += (int64_t)k * tmax;
  Y.t1 = (int)pos; pos += (int64_t)k * tmax;
  Y.g = (int)pos; pos += (int64_t)k * mlp->dims[0];
  pos = (pos + 1) & ~(int64_t)1;   // (doubles)
  Y.redd = (int)pos; pos += kRedD;
  Y.redf = (int)pos; pos += kRedF;
  Y.zs = (int)pos; pos += kZs;
  pos = (pos + 3) & ~(int64_t)3;
  Y.rows = (int)pos;
  const int64_t row = 3 * (int64_t)pp->n_ref, room = kMaxLds / 4 - pos - extra;
  const int64_t rpp = room < row ? 0 : (room / row < k ? room / row : k);
  if (rpp < 1 && extra > 0)
    CVFL_NO("one frame needs %lld bytes of LDS with one row of the contribution table (n_ref = %d) and %lld bytes of image counts (4 per atom), the workgroup kernel keeps within %d",
            (long long)(pos + row + extra) * 4, pp->n_ref, (long long)extra * 4, kMaxLds);
  if (rpp < 1)
    CVFL_NO("one frame needs %lld bytes of LDS with one row of the contribution table (n_ref = %d), the workgroup kernel keeps within %d",
            (long long)(pos + row) * 4, pp->n_ref, kMaxLds);
  Y.rpp = (int)rpp;
  Y.total = (int)(pos + rpp * row);
  if (lay != nullptr) *lay = Y;
  return nullptr;
#undef CVFL_NO
}

inline const char* cvfl_shared_why(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp, LgLayout* lay,
                                   const char* plain = "cvf_cv_frame_large_eval", int64_t extra = 0) {
  static thread_local char buf[240];
  const char* why = cvf_form_c_why(mlp, n_shared, plain, buf, sizeof buf);
  return why != nullptr ? why : cvfl_why(mlp, mlp->n_layers, pp, lay, n_shared, extra);
}

}  // namespace cvfl
