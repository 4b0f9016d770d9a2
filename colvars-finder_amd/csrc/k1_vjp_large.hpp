// The two large-frame kernels of csrc/k1_vjp.hip (one workgroup per frame), included TWICE by that file: once as they always were
// (uniform alignment weights) and once with per-atom weights (cvf_pp_desc.align_w).  The includer defines
//   CVF_VJP_LARGE_KERNEL, CVF_VJP_ROWS_LARGE_KERNEL   the kernels' names
//   CVF_VJP_WEIGHTED                                  false | true
// Two names rather than one more template argument: the uniform kernels stay the code objects they were, name for name.
// (no include guard: meant to be included more than once)

// WEIGHTED (per-atom alignment weights, cvf_pp_desc.align_w): align atom b's share of the centroid is w_b / n_align, so its
// rigid-body term is d_b = Z ref_b - w_b shift (ref_c holds w_b ref_b already), as in vjp_align_kernel.
template <bool VEC4>
__global__ __launch_bounds__(kLargeThreads) void CVF_VJP_LARGE_KERNEL(cvf_pp_desc pp, const float* __restrict__ x,
                                                                       const float* __restrict__ aux_tiled,
                                                                       const float* __restrict__ g_rows, float* __restrict__ gx_rows) {
  constexpr bool WEIGHTED = CVF_VJP_WEIGHTED;
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
  auto at = [&](int slot) { return atom_xyz(xf, pp.slot_atom[slot]); };
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
      outer_add(acc, at(s0) - c, g);
      acc[9] += pr.x; acc[10] += pr.y; acc[11] += pr.z;
    } else if (type == CVF_FEAT_BOND) {
      const BondG e = bond_eval(at(s0), at(s1));
      const float gs = gf[out];
      put(r0, gs * e.ga);
      put(r1, gs * e.gb);
    } else if (type == CVF_FEAT_ANGLE) {
      const AngleG e = angle_eval(at(s0), at(s1), at(s2));
      float gs = gf[out];
      if (pp.use_angle_value) gs = -gs / acos_den(e);
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
    if (b >= 0) {
      const V3 zr = mat_times(Z, v3(pp.ref_c[3 * b], pp.ref_c[3 * b + 1], pp.ref_c[3 * b + 2]));
      v = WEIGHTED ? zr - pp.align_w[b] * shift : zr - shift;
    }
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


template <bool VEC4>
__global__ __launch_bounds__(kLargeThreads) void CVF_VJP_ROWS_LARGE_KERNEL(cvf_pp_desc pp, const float* __restrict__ x,
                                                                            const float* __restrict__ aux_tiled, int k, int i0, int ng,
                                                                            const float* __restrict__ g_rows,
                                                                            float* __restrict__ gx_rows) {
  constexpr bool WEIGHTED = CVF_VJP_WEIGHTED;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kWaves = kLargeThreads / CVF_WAVE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t frame = blockIdx.x;
  const int nc = pp.n_coord, nrow = 3 * pp.n_ref;
  float* red = lds + ng * nrow;
  float* zs = red + ng * kWaves * 12;
  const float* xf = x + frame * nc;
  const float* gf = g_rows + frame * (int64_t)k * pp.d_r;
  const float* ax = aux_tiled + (frame / CVF_TILE) * CVF_AUX_ROWS * CVF_TILE + (frame % CVF_TILE);
  // (R, the centroid and Kinv are read where they are used, per group of rows: the uniform values live across the whole
  //  kernel are what the scalar registers hold)
  auto load_R = [&](float* R) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ax[i * CVF_TILE];
  };
  auto at = [&](int slot) { return atom_xyz(xf, pp.slot_atom[slot]); };
  auto put = [&](int ii, int row, V3 v) {
    float* rows = lds + ii * nrow;
    rows[3 * row] = v.x;
    rows[3 * row + 1] = v.y;
    rows[3 * row + 2] = v.z;
  };
  struct Rec {
    int type, out, s0, s1, s2, s3, r0, r1, r2, r3;
  };
  auto decode = [&](int r) {
    const int4 m0 = reinterpret_cast<const int4*>(pp.mrec)[2 * r];
    const int4 m1 = reinterpret_cast<const int4*>(pp.mrec)[2 * r + 1];
    Rec d;
    d.type = (m0.x & 7) - 1;
    d.out = (int)((unsigned)m0.x >> 3);
    d.s0 = m0.y & 0xffff; d.s1 = (int)((unsigned)m0.y >> 16); d.s2 = m0.z & 0xffff; d.s3 = (int)((unsigned)m0.z >> 16);
    const int off = m1.y;
    d.r0 = (m0.w & 0xffff) + (off & 0xff);
    d.r1 = (int)((unsigned)m0.w >> 16) + ((off >> 8) & 0xff);
    d.r2 = (m1.x & 0xffff) + ((off >> 16) & 0xff);
    d.r3 = (int)((unsigned)m1.x >> 16) + (int)((unsigned)off >> 24);
    return d;
  };
  {
    // ---- phase A, position records: row by row (M and sum_p are per-thread register sums, in the records' order)
    float R[9];
    load_R(R);
    const V3 c = v3(ax[9 * CVF_TILE], ax[10 * CVF_TILE], ax[11 * CVF_TILE]);
    for (int ii = 0; ii < ng; ++ii) {
      const float* gr = gf + (i0 + ii) * pp.d_r;
      float acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (pp.has_position) {
        for (int r = tid; r < pp.n_mrec; r += kLargeThreads) {
          const Rec d = decode(r);
          if (d.type != CVF_FEAT_POSITION) continue;
          const V3 g = v3(gr[d.out], gr[d.out + 1], gr[d.out + 2]);
          const V3 pr = mat_times(R, g);
          put(ii, d.r0, pr);
          outer_add(acc, at(d.s0) - c, g);
          acc[9] += pr.x; acc[10] += pr.y; acc[11] += pr.z;
        }
      }
      // (each wave sum is stored as soon as it is formed: twelve uniform sums alive at once overflow the scalar registers)
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const float v = wave_sumf(acc[i]);
        if (lane == 0) red[(ii * kWaves + wave) * 12 + i] = v;
      }
    }
    // ---- phase A, the other records: geometry once, then one product per row
    for (int r = tid; r < pp.n_mrec; r += kLargeThreads) {
      const Rec d = decode(r);
      if (d.type == CVF_FEAT_BOND) {
        const BondG e = bond_eval(at(d.s0), at(d.s1));
        for (int ii = 0; ii < ng; ++ii) {
          const float gs = gf[(i0 + ii) * pp.d_r + d.out];
          put(ii, d.r0, gs * e.ga);
          put(ii, d.r1, gs * e.gb);
        }
      } else if (d.type == CVF_FEAT_ANGLE) {
        const AngleG e = angle_eval(at(d.s0), at(d.s1), at(d.s2));
        for (int ii = 0; ii < ng; ++ii) {
          float gs = gf[(i0 + ii) * pp.d_r + d.out];
          if (pp.use_angle_value) gs = -gs / acos_den(e);
          put(ii, d.r0, gs * e.ga);
          put(ii, d.r1, gs * e.gb);
          put(ii, d.r2, gs * e.gc);
        }
      } else if (d.type == CVF_FEAT_DIHEDRAL) {
        const DihedralG e = dihedral_eval(at(d.s0), at(d.s1), at(d.s2), at(d.s3));
        for (int ii = 0; ii < ng; ++ii) {
          const float* gr = gf + (i0 + ii) * pp.d_r;
          const float gs = dihedral_adjoint(pp.use_angle_value, e.cs, e.sn, [&](int j) { return gr[d.out + j]; });
          put(ii, d.r0, gs * e.g1);
          put(ii, d.r1, gs * e.g2);
          put(ii, d.r2, gs * e.g3);
          put(ii, d.r3, gs * e.g4);
        }
      }
    }
    __syncthreads();
    // ---- phase B: every slot of every row sums its rows in order into its first row; thread ii < ng forms Z, shift of row ii
    for (int ii = 0; ii < ng; ++ii) {
      float* rows = lds + ii * nrow;
      for (int t = tid; t < pp.n_slot; t += kLargeThreads) {
        const int q0 = pp.slot_row[t], q1 = pp.slot_row[t + 1];
        V3 s = v3(rows[3 * q0], rows[3 * q0 + 1], rows[3 * q0 + 2]);
        for (int q = q0 + 1; q < q1; ++q) s = s + v3(rows[3 * q], rows[3 * q + 1], rows[3 * q + 2]);
        put(ii, q0, s);
      }
    }
    if (tid < ng) {
      float tot[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        float v = red[(tid * kWaves) * 12 + i];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += red[(tid * kWaves + w) * 12 + i];
        tot[i] = v;
      }
      float Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      V3 shift = v3(0, 0, 0);
      if (pp.has_position) {
        float R[9], Kinv[6];
        load_R(R);
#pragma unroll
        for (int i = 0; i < 6; ++i) Kinv[i] = ax[(12 + i) * CVF_TILE];
        rotation_term(R, Kinv, tot, Z);
        shift = (1.0f / (float)pp.n_align) * v3(tot[9], tot[10], tot[11]);
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) zs[tid * 12 + i] = Z[i];
      zs[tid * 12 + 9] = shift.x;
      zs[tid * 12 + 10] = shift.y;
      zs[tid * 12 + 11] = shift.z;
    }
    __syncthreads();
    // ---- phase 2: the dense rows; an atom's table entries are read once for all rows of the group
    struct AtomRef {
      int b, q;
      V3 rf;
      float wb;   // (WEIGHTED: the atom's alignment weight)
    };
    auto lookup = [&](int a) {
      AtomRef u;
      u.b = pp.atom_align[a];
      u.rf = u.b >= 0 ? v3(pp.ref_c[3 * u.b], pp.ref_c[3 * u.b + 1], pp.ref_c[3 * u.b + 2]) : v3(0, 0, 0);
      u.wb = WEIGHTED && u.b >= 0 ? pp.align_w[u.b] : 1.0f;
      const int t = pp.atom_slot[a];
      u.q = t >= 0 ? pp.slot_row[t] : -1;
      return u;
    };
    auto grad_of = [&](int ii, const AtomRef& u) {
      V3 v = v3(0, 0, 0);
      if (u.b >= 0) {
        const float* Z = zs + ii * 12;
        v = WEIGHTED ? mat_times(Z, u.rf) - u.wb * v3(Z[9], Z[10], Z[11]) : mat_times(Z, u.rf) - v3(Z[9], Z[10], Z[11]);
      }
      if (u.q >= 0) {
        const float* rows = lds + ii * nrow;
        v = v + v3(rows[3 * u.q], rows[3 * u.q + 1], rows[3 * u.q + 2]);
      }
      return v;
    };
    float* gx0 = gx_rows + (frame * k + i0) * (int64_t)nc;
    if (VEC4) {
      for (int v = tid; v < nc / 4; v += kLargeThreads) {
        const int j0 = 4 * v, A = j0 / 3, k0 = j0 - 3 * A;
        const AtomRef ua = lookup(A), ub = lookup(A + 1);
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
    } else {
      for (int j = tid; j < nc; j += kLargeThreads) {
        const int A = j / 3, kk = j - 3 * A;
        const AtomRef ua = lookup(A);
        for (int ii = 0; ii < ng; ++ii) {
          const V3 u = grad_of(ii, ua);
          gx0[ii * (int64_t)nc + j] = kk == 0 ? u.x : (kk == 1 ? u.y : u.z);
        }
      }
    }
  }
}

