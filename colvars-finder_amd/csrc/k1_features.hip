// CVF_PP_FEATURES (include/cvf.h): features of the RAW coordinates - no alignment, no centroid, no rotation.  Forward, J^T g
// (one row and k rows), J u (one tangent) and the generator's metric q = J A J^T g, E = g^T J A J^T g, for frames of ANY atom count: what bounds a
// launch is the feature list (n_slot distinct feature atoms, n_ref (record, atom) pairs), never 3 N.
//
// One decomposition for the three kernels.  A workgroup of 256 threads owns G consecutive frames of one 64-frame tile (G a power
// of two, the largest whose LDS image stays within kLdsBudget; G = 1 at the documented limits).  Work items are (entry, frame)
// pairs with the FRAME fastest: G neighbouring lanes take one table entry for G neighbouring frames, so
//   - every LDS image is [entry][G]: neighbouring lanes, neighbouring banks;
//   - tiled rows (feat_tiled, g_tiled, q_tiled) are read and written in runs of G floats.
// Step 0 of every kernel copies the frames' FEATURE ATOMS to LDS through slot_atom (12 bytes each; slot_atom ascends, so the atoms
// that share a line of the frame are asked for by neighbouring lanes of one instruction).  The frame itself is never streamed:
// a 5000-atom frame with 768 feature atoms costs 9 KB of useful reads, not 60 KB.  Everything after step 0 reads LDS.
//
// The derivative kernels scatter J^T g through the contribution rows of the descriptor (mrec / slot_row: one row per (record,
// atom) pair, the rows of one slot contiguous): phase A one (record, frame) per item writes the record's rows, phase B one
// (slot, frame) per item sums the slot's rows in order.  No atomics; every sum has a fixed order, so two calls give the same
// bits, and row i of the k-row VJP is the one-row VJP bit for bit (the same kernel runs the same code once per row).
// The feature formulas and their chain rule are those of cvf_features.hpp, with the dihedrals' normals in their EXACT form (these
// kernels see raw, un-centred coordinates and any geometry a feature list names); a position record copies the coordinates.
#include "cvf_features.hpp"

namespace {

constexpr int kFeatThreads = 256;
constexpr size_t kLdsBudget = 64 * 1024;   // LDS of a workgroup while G > 1 (two workgroups per CU)
constexpr size_t kMetricBudget = 72 * 1024;   // ... of the metric kernel (beside its 8 KB of static LDS: two workgroups per CU)

// one entry of cvf_pp_desc.mrec: type, first output, the slots of its atoms and the contribution row of each atom
struct MRec {
  int type, out, s[4], row[4], urow[4];
};
__device__ __forceinline__ MRec load_mrec(const int32_t* mrec, int r) {
  const int4 m0 = reinterpret_cast<const int4*>(mrec)[2 * r];
  const int4 m1 = reinterpret_cast<const int4*>(mrec)[2 * r + 1];
  MRec m;
  m.type = (m0.x & 7) - 1;
  m.out = (int)((unsigned)m0.x >> 3);
  m.s[0] = m0.y & 0xffff; m.s[1] = (int)((unsigned)m0.y >> 16); m.s[2] = m0.z & 0xffff; m.s[3] = (int)((unsigned)m0.z >> 16);
  m.urow[0] = m0.w & 0xffff; m.urow[1] = (int)((unsigned)m0.w >> 16); m.urow[2] = m1.x & 0xffff; m.urow[3] = (int)((unsigned)m1.x >> 16);
  const int off = m1.y;
  m.row[0] = m.urow[0] + (off & 0xff); m.row[1] = m.urow[1] + ((off >> 8) & 0xff);
  m.row[2] = m.urow[2] + ((off >> 16) & 0xff); m.row[3] = m.urow[3] + (int)((unsigned)off >> 24);
  return m;
}

// the group of a workgroup: G = 1 << lg frames starting at lane `lane0` of tile `tile`
struct Group {
  int64_t tile, f0;
  int lane0, G, lg;
};
__device__ __forceinline__ Group group_of(int lg) {
  Group g;
  g.lg = lg;
  g.G = 1 << lg;
  const int per_tile = CVF_TILE >> lg;
  g.tile = blockIdx.x / per_tile;
  g.lane0 = (int)(blockIdx.x % per_tile) << lg;
  g.f0 = g.tile * CVF_TILE + g.lane0;
  return g;
}

// V3 images in LDS: entry e of frame f at img[(3 e + c) G + f]
__device__ __forceinline__ V3 img_get(const float* img, int e, int f, int G) {
  return V3{img[(3 * e) * G + f], img[(3 * e + 1) * G + f], img[(3 * e + 2) * G + f]};
}
__device__ __forceinline__ void img_put(float* img, int e, int f, int G, V3 v) {
  img[(3 * e) * G + f] = v.x;
  img[(3 * e + 1) * G + f] = v.y;
  img[(3 * e + 2) * G + f] = v.z;
}

// step 0: the feature atoms of the group's frames (frames past B: copies of the last one)
__device__ __forceinline__ void stage_slots(const cvf_pp_desc& pp, const float* __restrict__ x, int64_t B, const Group& g, float* xs) {
  for (int e = threadIdx.x; e < (pp.n_slot << g.lg); e += kFeatThreads) {
    const int t = e >> g.lg, f = e & (g.G - 1);
    const int64_t frame = g.f0 + f < B ? g.f0 + f : B - 1;
    img_put(xs, t, f, g.G, atom_xyz(x + frame * pp.n_coord, pp.slot_atom[t]));
  }
}

// ------------------------------------------------------------------------------------
// forward: one (rec_slot entry, frame) per item
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFeatThreads) void features_fwd_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B, int lg,
                                                                     float* __restrict__ feat_tiled, float* __restrict__ feat_rows) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const Group g = group_of(lg);
  if (!feat_tiled && g.f0 >= B) return;   // padded frames exist in the tiled output only
  stage_slots(pp, x, B, g, xs);
  __syncthreads();
  const int n_ent = pp.n_rec_slot > 0 ? pp.n_rec_slot : pp.n_rec;
  for (int e = threadIdx.x; e < (n_ent << lg); e += kFeatThreads) {
    const int r = e >> lg, f = e & (g.G - 1);
    const Rec rc = load_rec(pp.rec_slot, r);
    if (rc.type < 0) continue;   // padding of a batch (CVF_PP_SLOT_BATCHED)
    const int64_t frame = g.f0 + f;
    const bool valid = frame < B;
    auto emit = [&](int j, float v) {
      if (feat_tiled) feat_tiled[(g.tile * pp.d_r + rc.out + j) * CVF_TILE + g.lane0 + f] = v;
      if (feat_rows && valid) feat_rows[frame * pp.d_r + rc.out + j] = v;
    };
    auto at = [&](int k) { return img_get(xs, rc.a[k], f, g.G); };
    if (rc.type == CVF_FEAT_POSITION) {
      const V3 p = at(0);
      emit(0, p.x);
      emit(1, p.y);
      emit(2, p.z);
    } else {
      invariant_values<true>(rc.type, pp.use_angle_value != 0, at, emit);
    }
  }
}

// phase A of the derivative kernels: the contribution rows of J^T g for one upstream vector; gval(out) reads it
template <class GVal>
__device__ __forceinline__ void scatter_rows(const cvf_pp_desc& pp, const Group& g, const float* xs, float* rows, GVal gval) {
  for (int e = threadIdx.x; e < (pp.n_mrec << g.lg); e += kFeatThreads) {
    const int r = e >> g.lg, f = e & (g.G - 1);
    const MRec m = load_mrec(pp.mrec, r);
    if (m.type == CVF_FEAT_POSITION) {
      img_put(rows, m.row[0], f, g.G, v3(gval(f, m.out), gval(f, m.out + 1), gval(f, m.out + 2)));
    } else if (m.type >= 0) {
      invariant_vjp<true>(m.type, pp.use_angle_value != 0, 1, [&](int k) { return img_get(xs, m.s[k], f, g.G); },
                    [&](int, int j) { return gval(f, m.out + j); }, [&](int, int k, V3 v) { img_put(rows, m.row[k], f, g.G, v); });
    }
  }
}

// ------------------------------------------------------------------------------------
// VJP: gx_rows[b][i] = J(x_b)^T g_rows[b][i], i < k, one row after the other on the same staged atoms
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFeatThreads) void features_vjp_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B, int lg, int k,
                                                                     const float* __restrict__ g_rows, float* __restrict__ gx_rows) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const Group g = group_of(lg);
  if (g.f0 >= B) return;
  float* rows = xs + 3 * (pp.n_slot << lg);
  const int nc = pp.n_coord;
  stage_slots(pp, x, B, g, xs);
  for (int i = 0; i < k; ++i) {
    __syncthreads();
    scatter_rows(pp, g, xs, rows, [&](int f, int o) {
      const int64_t frame = g.f0 + f < B ? g.f0 + f : B - 1;
      return g_rows[(frame * k + i) * pp.d_r + o];
    });
    __syncthreads();
    for (int e = threadIdx.x; e < (pp.n_slot << lg); e += kFeatThreads) {   // phase B: every slot sums its rows in order
      const int t = e >> lg, f = e & (g.G - 1);
      const int q0 = pp.slot_row[t], q1 = pp.slot_row[t + 1];
      V3 s = img_get(rows, q0, f, g.G);
      for (int q = q0 + 1; q < q1; ++q) s = s + img_get(rows, q, f, g.G);
      img_put(rows, q0, f, g.G, s);
    }
    __syncthreads();
    for (int f = 0; f < g.G && g.f0 + f < B; ++f) {   // the dense rows: the slot's sum on a feature atom, 0 elsewhere
      float* dst = gx_rows + ((g.f0 + f) * k + i) * nc;
      for (int c = threadIdx.x; c < nc; c += kFeatThreads) {
        const int a = c / 3, t = pp.atom_slot[a];
        dst[c] = t >= 0 ? rows[(3 * pp.slot_row[t] + (c - 3 * a)) * g.G + f] : 0.0f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// metric: s_j = J^T g_j (rows), u_j = a s_j on the feature atoms, q_j = J u_j, E_j = s_j . u_j - for kc nets per pass on ONE
// evaluation of every record's geometry and one read of the tables: the g values of the kc nets are in flight together and a
// pass has three barriers whatever kc is (the launch is bound by the latency of its dependent loads, not by their bytes).
// LDS: xs | rows [kc][n_ref][3][G]; E: every thread owns ONE frame (256 % G == 0), sums its slots' terms in order, the threads
// of a frame are added by masked wave sums and the four waves in order.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFeatThreads) void features_metric_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B, int lg,
                                                                        int kc, const float* __restrict__ a, int k,
                                                                        const float* __restrict__ g_tiled, float* __restrict__ q_tiled,
                                                                        float* __restrict__ e_tiled) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  __shared__ float red[kFeatThreads / CVF_WAVE][CVF_MAX_NETS][CVF_TILE];
  const Group g = group_of(lg);
  float* rows = xs + 3 * (pp.n_slot << lg);
  const int net_stride = 3 * (pp.n_ref << lg);   // floats of one net's rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int myf = threadIdx.x & (g.G - 1);       // the frame of every item of this thread
  const bool av = pp.use_angle_value != 0;
  stage_slots(pp, x, B, g, xs);
  for (int j0 = 0; j0 < k; j0 += kc) {
    const int nj = k - j0 < kc ? k - j0 : kc;
    // g / q of (net j0 + i, output o, frame f): base + (i * d_r + o) * 64 + f
    const int64_t base = (g.tile * k + j0) * (int64_t)pp.d_r * CVF_TILE + g.lane0;
    __syncthreads();
    for (int e = threadIdx.x; e < (pp.n_mrec << lg); e += kFeatThreads) {   // phase A: the contribution rows of the nj nets
      const int r = e >> lg, f = e & (g.G - 1);
      const MRec m = load_mrec(pp.mrec, r);
      auto gv = [&](int i, int o) { return g_tiled[base + ((int64_t)i * pp.d_r + m.out + o) * CVF_TILE + f]; };
      if (m.type == CVF_FEAT_POSITION) {
        for (int i = 0; i < nj; ++i) img_put(rows + i * net_stride, m.row[0], f, g.G, v3(gv(i, 0), gv(i, 1), gv(i, 2)));
      } else if (m.type >= 0) {
        invariant_vjp<true>(m.type, av, nj, [&](int kk) { return img_get(xs, m.s[kk], f, g.G); }, gv,
                      [&](int i, int kk, V3 v) { img_put(rows + i * net_stride, m.row[kk], f, g.G, v); });
      }
    }
    __syncthreads();
    float esum[CVF_MAX_NETS];
#pragma unroll
    for (int i = 0; i < CVF_MAX_NETS; ++i) esum[i] = 0.0f;
    for (int e = threadIdx.x; e < (pp.n_slot << lg); e += kFeatThreads) {   // phase B: u = a s on every slot, E's terms
      const int t = e >> lg;
      const int q0 = pp.slot_row[t], q1 = pp.slot_row[t + 1];
      const V3 aa = atom_xyz(a, pp.slot_atom[t]);
#pragma unroll
      for (int i = 0; i < CVF_MAX_NETS; ++i) {
        if (i < nj) {
          float* ri = rows + i * net_stride;
          V3 s = img_get(ri, q0, myf, g.G);
          for (int q = q0 + 1; q < q1; ++q) s = s + img_get(ri, q, myf, g.G);
          const V3 u = v3(aa.x * s.x, aa.y * s.y, aa.z * s.z);
          img_put(ri, q0, myf, g.G, u);
          esum[i] += dot(s, u);
        }
      }
    }
    // E: the threads of frame f are the lanes with lane % G == f of every wave
    for (int f = 0; f < g.G; ++f) {
#pragma unroll
      for (int i = 0; i < CVF_MAX_NETS; ++i) {
        if (i < nj) {
          const float v = wave_sumf(myf == f ? esum[i] : 0.0f);
          if (lane == 0) red[wave][i][f] = v;
        }
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nj * g.G; e += kFeatThreads) {
      const int i = e >> lg, f = e & (g.G - 1);
      float v = red[0][i][f];
#pragma unroll
      for (int w = 1; w < kFeatThreads / CVF_WAVE; ++w) v += red[w][i][f];
      e_tiled[(g.tile * k + j0 + i) * CVF_TILE + g.lane0 + f] = v;
    }
    for (int e = threadIdx.x; e < (pp.n_mrec << lg); e += kFeatThreads) {   // phase C: q = J u
      const int r = e >> lg, f = e & (g.G - 1);
      const MRec m = load_mrec(pp.mrec, r);
      for (int i = 0; i < nj; ++i) {
        const float* ri = rows + i * net_stride;
        auto put = [&](int jj, float v) { q_tiled[base + ((int64_t)i * pp.d_r + m.out + jj) * CVF_TILE + f] = v; };
        if (m.type == CVF_FEAT_POSITION) {
          const V3 u = img_get(ri, m.urow[0], f, g.G);
          put(0, u.x);
          put(1, u.y);
          put(2, u.z);
        } else if (m.type >= 0) {
          invariant_jvp<true>(m.type, av, [&](int kk) { return img_get(xs, m.s[kk], f, g.G); },
                        [&](int kk) { return img_get(ri, m.urow[kk], f, g.G); }, put);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// JVP: q_rows[b] = J(x_b) u_rows[b] (cvf_align_feature_jvp), the transpose of features_vjp_kernel: the feature atoms of x AND of
// u are staged through slot_atom (no other atom of either is read), then one (record, frame) per item - a position record copies
// its atom's tangent, the others go through invariant_jvp on the geometry features_vjp_kernel evaluates.  Every output of every
// record is written once, straight to its row (as features_fwd_kernel writes feat_rows); no sums across items, no atomics.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFeatThreads) void features_jvp_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B, int lg,
                                                                     const float* __restrict__ u_rows, float* __restrict__ q_rows) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const Group g = group_of(lg);
  if (g.f0 >= B) return;
  float* us = xs + 3 * (pp.n_slot << lg);
  stage_slots(pp, x, B, g, xs);
  stage_slots(pp, u_rows, B, g, us);
  __syncthreads();
  for (int e = threadIdx.x; e < (pp.n_mrec << lg); e += kFeatThreads) {
    const int r = e >> lg, f = e & (g.G - 1);
    if (g.f0 + f >= B) continue;   // only rows < B are written
    const MRec m = load_mrec(pp.mrec, r);
    float* q = q_rows + (g.f0 + f) * pp.d_r + m.out;
    if (m.type == CVF_FEAT_POSITION) {
      const V3 u = img_get(us, m.s[0], f, g.G);
      q[0] = u.x;
      q[1] = u.y;
      q[2] = u.z;
    } else if (m.type >= 0) {
      invariant_jvp<true>(m.type, pp.use_angle_value != 0, [&](int kk) { return img_get(xs, m.s[kk], f, g.G); },
                          [&](int kk) { return img_get(us, m.s[kk], f, g.G); }, [&](int j, float v) { q[j] = v; });
    }
  }
}

struct FeatPlan {
  int lg;
  size_t lds;
};
FeatPlan feat_plan(size_t bytes_per_frame, size_t budget = kLdsBudget) {
  FeatPlan p = {6, 0};
  while (p.lg > 0 && (bytes_per_frame << p.lg) > budget) --p.lg;
  p.lds = bytes_per_frame << p.lg;
  return p;
}

// the pointers of the descriptor a launch reads (the counts: cvf_features_deriv_plan)
int features_tables(const cvf_pp_desc* pp, const char* who, bool derivative) {
  CVF_REQUIRE(pp->rec_slot && pp->slot_atom, "%s: CVF_PP_FEATURES needs n_coord = 3 N, the records and the slot tables (rec_slot, slot_atom)", who);
  if (derivative) {
    CVF_REQUIRE(pp->mrec && pp->slot_row && pp->atom_slot,
                "%s: CVF_PP_FEATURES derivatives need the contribution-row tables (atom_slot, mrec, slot_row)", who);
    CVF_REQUIRE(((uintptr_t)pp->mrec & 15) == 0, "%s: mrec must be 16-byte aligned", who);
  }
  return 0;
}

template <class K, class... Args>
int features_launch(K kernel, const char* name, const cvf_deriv_plan& p, hipStream_t s, Args... args) {
  if (p.lds_bytes > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3(kFeatThreads), (size_t)p.lds_bytes, s, args...);
  return cvf_check_launch(name);
}

}  // namespace

// The launch of every CVF_PP_FEATURES kernel (this file and features_hvp_kernel, csrc/k1_hvp.hip): frames per workgroup, LDS, grid,
// and what else the kernel is told (u_lds, nets per pass) - host arithmetic on the descriptor's counts.  `which`: CVF_DERIV_*
// (include/cvf.h); cvf_align_feature_deriv_route answers with it, the launches below launch by it.
int cvf_features_deriv_plan(const cvf_pp_desc* pp, int64_t B, int which, int k, cvf_deriv_plan* P) {
  static const char* const kWho[] = {"cvf_align_feature_vjp", "cvf_align_feature_vjp", "cvf_align_feature_jvp",
                                     "cvf_align_feature_hvp", "cvf_align_feature_fwd", "cvf_metric_apply"};
  *P = cvf_deriv_plan{};
  CVF_REQUIRE(which >= CVF_DERIV_VJP && which <= CVF_DERIV_FEATURES_METRIC, "cvf_align_feature_deriv_route: unknown call %d", which);
  const char* who = kWho[which];
  const bool derivative = which != CVF_DERIV_FEATURES_FWD;
  CVF_REQUIRE((which != CVF_DERIV_VJP_ROWS && which != CVF_DERIV_FEATURES_METRIC) || (k >= 1 && k <= CVF_MAX_NETS),
              "%s: k outside 1..%d (k=%d)", who, CVF_MAX_NETS, k);
  CVF_REQUIRE(pp->n_coord > 0 && pp->n_coord % 3 == 0 && pp->d_r >= 1 && pp->n_rec >= 1 && pp->n_slot >= 1,
              "%s: CVF_PP_FEATURES needs n_coord = 3 N, the records and the slot tables (%s)", who,
              which == CVF_DERIV_HVP ? "slot_atom" : "rec_slot, slot_atom");   // (features_hvp_kernel does not read rec_slot)
  CVF_REQUIRE(pp->n_slot <= CVF_FEATURES_MAX_SLOT, "%s: CVF_PP_FEATURES: n_slot = %d distinct feature atoms; the limit is CVF_FEATURES_MAX_SLOT = %d",
              who, pp->n_slot, CVF_FEATURES_MAX_SLOT);
  if (derivative) {
    CVF_REQUIRE(pp->n_ref <= CVF_FEATURES_MAX_REF, "%s: CVF_PP_FEATURES: n_ref = %d contribution rows; the limit is CVF_FEATURES_MAX_REF = %d", who,
                pp->n_ref, CVF_FEATURES_MAX_REF);
    CVF_REQUIRE(pp->n_mrec >= 1 && pp->n_ref >= pp->n_slot,
                "%s: CVF_PP_FEATURES derivatives need the contribution-row tables (atom_slot, mrec, slot_row)", who);
  }
  const size_t ns = (size_t)pp->n_slot, nr = (size_t)pp->n_ref;
  size_t per_frame = ns * 12, budget = kLdsBudget;
  P->rows_per_launch = 1;
  switch (which) {
    case CVF_DERIV_VJP_ROWS:   // (one row after the other on the same staged atoms)
    case CVF_DERIV_VJP:
      P->rows_per_launch = which == CVF_DERIV_VJP_ROWS ? k : 1;
      per_frame = (ns + nr) * 12;
      break;
    case CVF_DERIV_JVP: per_frame = ns * 24; break;    // the feature atoms of x and of u
    case CVF_DERIV_HVP:                                // the feature atoms of x and, while all fits the LDS, of u; the rows
      P->u_lds = (2 * ns + nr) * 12 <= 160 * 1024;
      per_frame = ((P->u_lds ? 2 : 1) * ns + nr) * 12;
      break;
    case CVF_DERIV_FEATURES_METRIC: {
      // nets per pass: all k while one frame's image stays within the budget, else the fewest equal passes that do
      auto image = [&](int kc) { return ns * 12 + (size_t)kc * nr * 12; };
      int kc = k;
      while (kc > 1 && image(kc) > kMetricBudget) --kc;
      const int passes = (k + kc - 1) / kc;
      kc = (k + passes - 1) / passes;
      P->rows_per_launch = kc;
      per_frame = image(kc);
      budget = kMetricBudget;
      break;
    }
    default: break;
  }
  const FeatPlan p = feat_plan(per_frame, budget);
  const int64_t nb = cvf_ntiles(B) * (CVF_TILE >> p.lg);
  CVF_REQUIRE(nb <= 0x7fffffff, "%s: %lld frames are too many for one launch", who, (long long)B);
  P->family = CVF_DERIV_ROUTE_FEATURES;
  P->lg = p.lg;
  P->launches = 1;
  P->lds_bytes = (int64_t)p.lds;
  P->grid = nb;
  return 0;
}

int cvf_features_fwd_launch(const cvf_pp_desc* pp, const float* x, int64_t B, float* feat_tiled, float* feat_rows, hipStream_t s) {
  cvf_deriv_plan p;
  if (int rc = cvf_features_deriv_plan(pp, B, CVF_DERIV_FEATURES_FWD, 1, &p)) return rc;
  if (int rc = features_tables(pp, "cvf_align_feature_fwd", false)) return rc;
  return features_launch(features_fwd_kernel, "features_fwd_kernel", p, s, *pp, x, B, p.lg, feat_tiled, feat_rows);
}

int cvf_features_vjp_launch(const cvf_pp_desc* pp, const float* x, int64_t B, int k, const float* g_rows, float* gx_rows, hipStream_t s) {
  cvf_deriv_plan p;
  if (int rc = cvf_features_deriv_plan(pp, B, CVF_DERIV_VJP_ROWS, k, &p)) return rc;
  if (int rc = features_tables(pp, "cvf_align_feature_vjp", true)) return rc;
  CVF_REQUIRE(x, "cvf_align_feature_vjp: CVF_PP_FEATURES needs x");
  return features_launch(features_vjp_kernel, "features_vjp_kernel", p, s, *pp, x, B, p.lg, k, g_rows, gx_rows);
}

int cvf_features_jvp_launch(const cvf_pp_desc* pp, const float* x, int64_t B, const float* u_rows, float* q_rows, hipStream_t s) {
  cvf_deriv_plan p;
  if (int rc = cvf_features_deriv_plan(pp, B, CVF_DERIV_JVP, 1, &p)) return rc;
  if (int rc = features_tables(pp, "cvf_align_feature_jvp", true)) return rc;
  CVF_REQUIRE(x, "cvf_align_feature_jvp: CVF_PP_FEATURES needs x");
  return features_launch(features_jvp_kernel, "features_jvp_kernel", p, s, *pp, x, B, p.lg, u_rows, q_rows);
}

int cvf_features_metric_launch(const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, int k, const float* g_tiled,
                               float* q_tiled, float* e_tiled, hipStream_t s) {
  cvf_deriv_plan p;
  if (int rc = cvf_features_deriv_plan(pp, B, CVF_DERIV_FEATURES_METRIC, k, &p)) return rc;
  if (int rc = features_tables(pp, "cvf_metric_apply", true)) return rc;
  CVF_REQUIRE(x, "cvf_metric_apply: CVF_PP_FEATURES needs x");
  return features_launch(features_metric_kernel, "features_metric_kernel", p, s, *pp, x, B, p.lg, p.rows_per_launch, a, k, g_tiled,
                         q_tiled, e_tiled);
}
