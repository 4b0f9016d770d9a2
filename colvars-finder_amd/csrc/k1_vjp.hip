// VJP of K1: gx = J(x)^T g per frame, J the Jacobian of the alignment + feature map r(x) (cvf_align_feature_vjp).
// The rotation, centroid and Kinv come from the forward's aux rows; nothing is recomputed but the features' own gradients.
//
//   G_a = s_a + d_a,   s_a = sum over the records that read atom a of (their gradient vectors) x (their upstream rows)
//                      d_b = Z ref_b - w_b shift  on the align atoms   (Z = R [Kinv ax(R^T M)]x, shift = sum_p / n_align,
//                                                                       M = sum_p xc_p (x) g_p, sum_p = sum_p R g_p over the
//                                                                       position records p; 0 without position records)
// (the derivation: csrc/metric_large.hip, header; csrc/k1_align.hip, metric_align_kernel - pass 1 of that kernel is the first
// kernel below for one upstream row instead of k nets).
//
// Frames of at most 192 coordinates: one lane = one frame, the 64-frame tile of x, the tables and the gradient image G in LDS,
// every sum sequential per lane.  Larger frames: one workgroup per frame, the records over the threads; each (record, atom)
// pair writes its own contribution row (the mrec / slot_row tables of cvf_pp_desc), each slot sums its rows in order, the dense
// row of 3N floats leaves in 16-byte stores.  No atomics anywhere: two calls give the same bits.
#include "cvf_metric.hpp"

namespace {

constexpr int kLanePerFrameMaxCoord = 192;   // as cvf_align_feature_fwd (k1_align.hip): aux rows are the same on both paths
constexpr int kLargeThreads = 256;

__device__ __forceinline__ V3 atom_at(const float* my, int a) { return V3{my[3 * a], my[3 * a + 1], my[3 * a + 2]}; }

// s = Kinv ax(R^T M);  Z = R [s]x   ([s]x rows: (0,-sz,sy), (sz,0,-sx), (-sy,sx,0))
__device__ __forceinline__ void rotation_term(const float* R, const float* Kinv, const float* M, float* Z) {
  float T[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[3 * i + j] = R[i] * M[j] + R[3 + i] * M[3 + j] + R[6 + i] * M[6 + j];
  const V3 s = sym_times(Kinv, v3(T[7] - T[5], T[2] - T[6], T[3] - T[1]));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Z[3 * i + 0] = R[3 * i + 1] * s.z - R[3 * i + 2] * s.y;
    Z[3 * i + 1] = -R[3 * i + 0] * s.z + R[3 * i + 2] * s.x;
    Z[3 * i + 2] = R[3 * i + 0] * s.y - R[3 * i + 1] * s.x;
  }
}

// ------------------------------------------------------------------------------------
// small frames: one lane per frame.  LDS: x tile [64][stride] | G [64][stride] | (TABLES_LDS) rec, align_idx, ref_c.
// G shares the x tile's odd row stride: the per-lane accumulation (lane = frame) and the coalesced copy-out (consecutive lanes
// = consecutive coordinates of one frame) are both free of bank conflicts.
// ------------------------------------------------------------------------------------
template <bool TABLES_LDS>
__global__ __launch_bounds__(64) void vjp_align_kernel(cvf_pp_desc pp, const float* __restrict__ x, int64_t B,
                                                        const float* __restrict__ aux_tiled, const float* __restrict__ g_rows,
                                                        float* __restrict__ gx_rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int nc = pp.n_coord, stride = x_tile_stride(nc);
  load_x_tile(x, B, nc, tile, lds, lane);
  float* Gt = lds + CVF_TILE * stride;
  for (int j = lane; j < CVF_TILE * stride; j += CVF_WAVE) Gt[j] = 0.0f;
  const int32_t* rec = pp.rec;
  const int32_t* al_idx = pp.align_idx;
  const float* ref = pp.ref_c;
  if (TABLES_LDS) {
    int32_t* L = reinterpret_cast<int32_t*>(Gt + CVF_TILE * stride);
    const int n1 = 6 * pp.n_rec, n2 = n1 + pp.n_align, n3 = n2 + 3 * pp.n_align;
    for (int i = lane; i < n3; i += CVF_WAVE)
      L[i] = i < n1 ? pp.rec[i] : (i < n2 ? pp.align_idx[i - n1] : reinterpret_cast<const int32_t*>(pp.ref_c)[i - n2]);
    rec = L;
    al_idx = L + n1;
    ref = reinterpret_cast<const float*>(L + n2);
  }
  __syncthreads();
  const float* my = lds + lane * stride;
  float* Gl = Gt + lane * stride;
  const int64_t frame = tile * CVF_TILE + lane;
  const float* gr = g_rows + (frame < B ? frame : B - 1) * pp.d_r;   // tail lanes repeat the last frame; only valid rows leave
  const float* ax = aux_tiled + tile * CVF_AUX_ROWS * CVF_TILE + lane;
  float R[9], Kinv[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const Centre c = centre_of(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
#pragma unroll
  for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
  auto addG = [&](int atm, V3 v) {
    Gl[3 * atm] += v.x;
    Gl[3 * atm + 1] += v.y;
    Gl[3 * atm + 2] += v.z;
  };
  V3 sump = v3(0, 0, 0);
  float M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = 0; r < pp.n_rec; ++r) {
    const int32_t* p = rec + 6 * r;
    const int type = p[0], out = p[5];
    if (type == CVF_FEAT_POSITION) {
      const V3 g = v3(gr[out], gr[out + 1], gr[out + 2]);
      const V3 pr = mat_times(R, g);
      addG(p[1], pr);
      sump = sump + pr;
      const V3 xc = centred(my, p[1], c);
      M[0] += xc.x * g.x; M[1] += xc.x * g.y; M[2] += xc.x * g.z;
      M[3] += xc.y * g.x; M[4] += xc.y * g.y; M[5] += xc.y * g.z;
      M[6] += xc.z * g.x; M[7] += xc.z * g.y; M[8] += xc.z * g.z;
    } else if (type == CVF_FEAT_BOND) {
      const BondG e = bond_eval(atom_at(my, p[1]), atom_at(my, p[2]));
      const float gs = gr[out];
      addG(p[1], gs * e.ga);
      addG(p[2], gs * e.gb);
    } else if (type == CVF_FEAT_ANGLE) {
      const AngleG e = angle_eval(atom_at(my, p[1]), atom_at(my, p[2]), atom_at(my, p[3]));
      float gs = gr[out];
      if (pp.use_angle_value) gs = -gs / sqrtf(fmaxf(1.0f - e.cs * e.cs, 1e-30f));   // d acos(cs) = -dcs / sin
      addG(p[1], gs * e.ga);
      addG(p[2], gs * e.gb);
      addG(p[3], gs * e.gc);
    } else {
      const DihedralG e = dihedral_eval(atom_at(my, p[1]), atom_at(my, p[2]), atom_at(my, p[3]), atom_at(my, p[4]));
      const float gs = pp.use_angle_value ? gr[out] : (gr[out + 1] * e.cs - gr[out] * e.sn);
      addG(p[1], gs * e.g1);
      addG(p[2], gs * e.g2);
      addG(p[3], gs * e.g3);
      addG(p[4], gs * e.g4);
    }
  }
  if (pp.has_position) {
    float Z[9];
    rotation_term(R, Kinv, M, Z);
    // (weighted alignment: atom b's share of the centroid is align_w[b] / n_align, and ref_c holds align_w[b] * ref_b)
    const V3 shift = (1.0f / (float)pp.n_align) * sump;
    for (int b = 0; b < pp.n_align; ++b) {
      const V3 rf = v3(ref[3 * b], ref[3 * b + 1], ref[3 * b + 2]);
      const float wb = pp.align_w ? pp.align_w[b] : 1.0f;
      addG(al_idx[b], mat_times(Z, rf) - wb * shift);
    }
  }
  lds_barrier();
  // copy-out: the tile's valid frames are one contiguous run of gx_rows
  const int64_t f0 = tile * CVF_TILE;
  const int nvalid = (int)(B - f0 < CVF_TILE ? B - f0 : CVF_TILE);
  float* dst = gx_rows + f0 * nc;
  const int total = nvalid * nc, dfr = CVF_WAVE / nc, dj = CVF_WAVE - dfr * nc;
  int fr = lane / nc, j = lane - fr * nc;
  for (int e = lane; e < total; e += CVF_WAVE) {
    dst[e] = Gt[fr * stride + j];
    fr += dfr;
    j += dj;
    if (j >= nc) { j -= nc; ++fr; }
  }
}

// ------------------------------------------------------------------------------------
// large frames: one workgroup per frame.  LDS: the contribution rows [n_ref][3] (after phase B the first row of every slot
// holds the slot's sum s_t) and 12 partial sums per wave.
// ------------------------------------------------------------------------------------
template <bool VEC4>
__global__ __launch_bounds__(kLargeThreads) void vjp_large_kernel(cvf_pp_desc pp, const float* __restrict__ x,
                                                                   const float* __restrict__ aux_tiled,
                                                                   const float* __restrict__ g_rows, float* __restrict__ gx_rows) {
  extern __shared__ __attribute__((aligned(16))) float rows[];
  __shared__ float red[kLargeThreads / CVF_WAVE][12];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t frame = blockIdx.x;
  const int nc = pp.n_coord;
  const float* xf = x + frame * nc;
  const float* gf = g_rows + frame * pp.d_r;
  const float* ax = aux_tiled + (frame / CVF_TILE) * CVF_AUX_ROWS * CVF_TILE + (frame % CVF_TILE);
  float R[9], Kinv[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  const V3 c = v3(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
#pragma unroll
  for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
  auto at = [&](int slot) {
    const int a = pp.slot_atom[slot];
    return V3{xf[3 * a], xf[3 * a + 1], xf[3 * a + 2]};
  };
  auto put = [&](int row, V3 v) {
    rows[3 * row] = v.x;
    rows[3 * row + 1] = v.y;
    rows[3 * row + 2] = v.z;
  };
  // ---- phase A: one record per thread; atom p of the record writes its row u_p + off_p
  float acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // M (9), sum_p (3)
  for (int r = tid; r < pp.n_mrec; r += kLargeThreads) {
    const int4 m0 = reinterpret_cast<const int4*>(pp.mrec)[2 * r];
    const int4 m1 = reinterpret_cast<const int4*>(pp.mrec)[2 * r + 1];
    const int type = (m0.x & 7) - 1, out = (int)((unsigned)m0.x >> 3);
    const int s0 = m0.y & 0xffff, s1 = (int)((unsigned)m0.y >> 16), s2 = m0.z & 0xffff, s3 = (int)((unsigned)m0.z >> 16);
    const int off = m1.y;
    const int r0 = (m0.w & 0xffff) + (off & 0xff), r1 = (int)((unsigned)m0.w >> 16) + ((off >> 8) & 0xff);
    const int r2 = (m1.x & 0xffff) + ((off >> 16) & 0xff), r3 = (int)((unsigned)m1.x >> 16) + (int)((unsigned)off >> 24);
    if (type == CVF_FEAT_POSITION) {
      const V3 g = v3(gf[out], gf[out + 1], gf[out + 2]);
      const V3 pr = mat_times(R, g);
      put(r0, pr);
      const V3 xc = at(s0) - c;
      acc[0] += xc.x * g.x; acc[1] += xc.x * g.y; acc[2] += xc.x * g.z;
      acc[3] += xc.y * g.x; acc[4] += xc.y * g.y; acc[5] += xc.y * g.z;
      acc[6] += xc.z * g.x; acc[7] += xc.z * g.y; acc[8] += xc.z * g.z;
      acc[9] += pr.x; acc[10] += pr.y; acc[11] += pr.z;
    } else if (type == CVF_FEAT_BOND) {
      const BondG e = bond_eval(at(s0), at(s1));
      const float gs = gf[out];
      put(r0, gs * e.ga);
      put(r1, gs * e.gb);
    } else if (type == CVF_FEAT_ANGLE) {
      const AngleG e = angle_eval(at(s0), at(s1), at(s2));
      float gs = gf[out];
      if (pp.use_angle_value) gs = -gs / sqrtf(fmaxf(1.0f - e.cs * e.cs, 1e-30f));
      put(r0, gs * e.ga);
      put(r1, gs * e.gb);
      put(r2, gs * e.gc);
    } else if (type == CVF_FEAT_DIHEDRAL) {
      const DihedralG e = dihedral_eval(at(s0), at(s1), at(s2), at(s3));
      const float gs = pp.use_angle_value ? gf[out] : (gf[out + 1] * e.cs - gf[out] * e.sn);
      put(r0, gs * e.g1);
      put(r1, gs * e.g2);
      put(r2, gs * e.g3);
      put(r3, gs * e.g4);
    }
  }
  // M and sum_p over the workgroup: DPP sums inside each wave, then the waves in order (fixed order: reproducible)
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = wave_sumf(acc[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) red[wave][i] = acc[i];
  }
  __syncthreads();
  // ---- phase B: slot t sums its rows slot_row[t] .. slot_row[t+1]-1 in order into its first row
  for (int t = tid; t < pp.n_slot; t += kLargeThreads) {
    const int q0 = pp.slot_row[t], q1 = pp.slot_row[t + 1];
    V3 s = v3(rows[3 * q0], rows[3 * q0 + 1], rows[3 * q0 + 2]);
    for (int q = q0 + 1; q < q1; ++q) s = s + v3(rows[3 * q], rows[3 * q + 1], rows[3 * q + 2]);
    put(q0, s);
  }
  float tot[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    float v = red[0][i];
#pragma unroll
    for (int w = 1; w < kLargeThreads / CVF_WAVE; ++w) v += red[w][i];
    tot[i] = v;
  }
  float Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  V3 shift = v3(0, 0, 0);
  if (pp.has_position) {
    rotation_term(R, Kinv, tot, Z);
    shift = (1.0f / (float)pp.n_align) * v3(tot[9], tot[10], tot[11]);
  }
  __syncthreads();
  // ---- phase 2: the dense row, d_b on align atoms plus s_t on feature atoms, 0 elsewhere
  auto grad_of = [&](int a) {
    V3 v = v3(0, 0, 0);
    const int b = pp.atom_align[a];
    if (b >= 0) v = mat_times(Z, v3(pp.ref_c[3 * b], pp.ref_c[3 * b + 1], pp.ref_c[3 * b + 2])) - shift;
    const int t = pp.atom_slot[a];
    if (t >= 0) {
      const int q = pp.slot_row[t];
      v = v + v3(rows[3 * q], rows[3 * q + 1], rows[3 * q + 2]);
    }
    return v;
  };
  float* gxf = gx_rows + frame * nc;
  if (VEC4) {   // nc % 4 == 0 and 16-byte rows: coordinates 4v..4v+3 lie in atoms A = 4v/3 and A + 1
    for (int v = tid; v < nc / 4; v += kLargeThreads) {
      const int j0 = 4 * v, A = j0 / 3, k0 = j0 - 3 * A;
      const V3 u = grad_of(A), w = grad_of(A + 1);
      float4 o;
      o.x = k0 == 0 ? u.x : (k0 == 1 ? u.y : u.z);
      o.y = k0 == 0 ? u.y : (k0 == 1 ? u.z : w.x);
      o.z = k0 == 0 ? u.z : (k0 == 1 ? w.x : w.y);
      o.w = k0 == 0 ? w.x : (k0 == 1 ? w.y : w.z);
      reinterpret_cast<float4*>(gxf)[v] = o;
    }
  } else {
    for (int j = tid; j < nc; j += kLargeThreads) {
      const int A = j / 3, k = j - 3 * A;
      const V3 u = grad_of(A);
      gxf[j] = k == 0 ? u.x : (k == 1 ? u.y : u.z);
    }
  }
}

}  // namespace

extern "C" int cvf_align_feature_vjp(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled,
                                     const float* g_rows, float* gx_rows, void* stream) {
  CVF_REQUIRE(pp && g_rows && gx_rows && B > 0, "cvf_align_feature_vjp: null argument or empty batch (B=%lld)", (long long)B);
  hipStream_t s = (hipStream_t)stream;
  if (pp->mode == CVF_PP_IDENTITY) {
    CVF_REQUIRE(pp->d_r == pp->n_coord, "identity preprocessing needs d_r == n_coord");
    const hipError_t e = hipMemcpyAsync(gx_rows, g_rows, (size_t)B * pp->n_coord * sizeof(float), hipMemcpyDeviceToDevice, s);
    CVF_REQUIRE(e == hipSuccess, "cvf_align_feature_vjp: identity copy: %s", hipGetErrorString(e));
    return 0;
  }
  CVF_REQUIRE(pp->mode != CVF_PP_FACTORED,
              "cvf_align_feature_vjp: CVF_PP_FACTORED records come from a torch module, which is differentiated by its own autograd");
  CVF_REQUIRE(pp->mode == CVF_PP_ALIGN, "unknown pp mode %d", pp->mode);
  CVF_REQUIRE(x && aux_tiled, "cvf_align_feature_vjp: align mode needs x and the forward's aux rows");
  CVF_REQUIRE(pp->n_coord % 3 == 0 && pp->n_align >= 3 && pp->align_idx && pp->ref_c && pp->rec,
              "cvf_align_feature_vjp: malformed descriptor (n_coord=%d n_align=%d)", pp->n_coord, pp->n_align);
  CVF_REQUIRE(!pp->align_w || (pp->flags == 0 && pp->n_coord <= kLanePerFrameMaxCoord),
              "cvf_align_feature_vjp: per-atom alignment weights need flags == 0 and at most %d coordinates per frame",
              kLanePerFrameMaxCoord);
  if (pp->n_coord <= kLanePerFrameMaxCoord) {
    const int stride = x_tile_stride(pp->n_coord);
    const size_t base = (size_t)2 * CVF_TILE * stride * sizeof(float);
    const size_t tables = ((size_t)6 * pp->n_rec + 4 * (size_t)pp->n_align) * sizeof(float);
    const bool tables_lds = base + tables <= 160 * 1024;
    const size_t lds = base + (tables_lds ? tables : 0);
    auto launch = [&](auto kernel) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)cvf_ntiles(B)), dim3(64), lds, s, *pp, x, B, aux_tiled, g_rows, gx_rows);
    };
    if (tables_lds) launch(vjp_align_kernel<true>);
    else launch(vjp_align_kernel<false>);
    return cvf_check_launch("vjp_align_kernel");
  }
  CVF_REQUIRE(pp->mrec && pp->slot_row && pp->slot_atom && pp->atom_align && pp->atom_slot && pp->n_slot > 0 && pp->n_ref > 0,
              "cvf_align_feature_vjp: frames of more than %d coordinates need the slot and contribution-row tables "
              "(atom_align, atom_slot, slot_atom, mrec, slot_row)", kLanePerFrameMaxCoord);
  CVF_REQUIRE(((uintptr_t)pp->mrec & 15) == 0, "cvf_align_feature_vjp: mrec must be 16-byte aligned");
  CVF_REQUIRE(B <= 0x7fffffff, "cvf_align_feature_vjp: at most 2^31 - 1 frames per call");
  const size_t lds = (size_t)pp->n_ref * 3 * sizeof(float);
  CVF_REQUIRE(lds + sizeof(float) * 12 * (kLargeThreads / CVF_WAVE) <= 160 * 1024,
              "cvf_align_feature_vjp: %d contribution rows (atoms summed over the features) do not fit the LDS", pp->n_ref);
  const bool vec4 = pp->n_coord % 4 == 0 && ((uintptr_t)gx_rows & 15) == 0;
  auto launch = [&](auto kernel) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kLargeThreads), lds, s, *pp, x, aux_tiled, g_rows, gx_rows);
  };
  if (vec4) launch(vjp_large_kernel<true>);
  else launch(vjp_large_kernel<false>);
  return cvf_check_launch("vjp_large_kernel");
}
