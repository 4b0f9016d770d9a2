// The sweep of form C for the two one-launch kernels, csrc/cv_frame.hip (one wave per frame: idx = lane,
// STRIDE = 64) and csrc/cv_frame_large.hip (one workgroup per frame: idx = thread, STRIDE = 256): ONE text, so that the two stay
// bit-identical to each other and to form A's rows.  Every thread of the frame's workgroup calls it.
#pragma once
#include "cvf_common.hpp"

// Offsets into the frame's LDS, in floats (FrLayout / LgLayout)
struct CvfFormCLds {
  const int* a;         // a[l]: layer l's activations; a[1..ns] hold one chain, a[ns+1..L] k chains
  int v0, v1, t0, t1;   // two sweep vectors of a head; two images [vector][width] of the trunk's sweep
  int g;                // d xi / d r: [kk][dims[0]]
};

// v_L = 1 (or coef_s), v_l = W_l^T (act_l'(a_{l+1}) .* v_{l+1}).  Heads: chain s from its output down to the boundary, v_ns of CV s
// into row s of the trunk's image - or, with coef_frame (the frame's k coefficients), seeded with coef_s and summed into row 0 in
// the order s = 0, 1, ..  Trunk: the kk = (coef_frame ? 1 : k) vectors side by side through the shared weights and the shared
// act'(a_l), unit u = (vector, input) over the threads.  Each dot product is one fmaf chain in index order.
template <int STRIDE>
__device__ __forceinline__ void cvf_form_c_sweep(const cvf_mlp_desc& mlp, const float* __restrict__ theta, const float* coef_frame,
                                                 float* lds, const CvfFormCLds& lay, int L, int k, int ns, int idx) {
  const int kk = coef_frame != nullptr ? 1 : k, db = mlp.dims[ns];
  float* tc = lds + lay.t0;
  float* tn = lds + lay.t1;
  for (int s = 0; s < k; ++s) {
    float* vc = lds + lay.v0;
    float* vn = lds + lay.v1;
    if (idx == 0) vc[0] = coef_frame != nullptr ? coef_frame[s] : 1.0f;   // (scalar chains: dims[L] == 1)
    lds_barrier();
    for (int l = L - 1; l >= ns; --l) {
      const int din = mlp.dims[l], dout = mlp.dims[l + 1], act = mlp.act[l];
      const float* ah = lds + lay.a[l + 1] + s * dout;
      for (int m = idx; m < dout; m += STRIDE) vc[m] *= cvf_act_d1(act, ah[m]);
      lds_barrier();
      const float* w = theta + mlp.w_off[s][l];
      const bool last = l == ns;
      float* dst = last ? tc + (coef_frame != nullptr ? 0 : s) * db : vn;
      const bool accum = last && coef_frame != nullptr && s > 0;
      for (int j = idx; j < din; j += STRIDE) {
        float acc = 0.0f;
#pragma unroll 4
        for (int m = 0; m < dout; ++m) acc = fmaf(w[(int64_t)m * din + j], vc[m], acc);
        dst[j] = accum ? dst[j] + acc : acc;
      }
      lds_barrier();
      float* t = vc;
      vc = vn;
      vn = t;
    }
  }
  for (int l = ns - 1; l >= 0; --l) {
    const int din = mlp.dims[l], dout = mlp.dims[l + 1], act = mlp.act[l];
    const float* ah = lds + lay.a[l + 1];
    for (int u = idx; u < kk * dout; u += STRIDE) tc[u] *= cvf_act_d1(act, ah[u % dout]);
    lds_barrier();
    const float* w = theta + mlp.w_off[0][l];
    float* dst = l > 0 ? tn : lds + lay.g;
    for (int u = idx; u < kk * din; u += STRIDE) {
      const int i = u / din, j = u - i * din;
      const float* vi = tc + i * dout;
      float acc = 0.0f;
#pragma unroll 4
      for (int m = 0; m < dout; ++m) acc = fmaf(w[(int64_t)m * din + j], vi[m], acc);
      dst[u] = acc;
    }
    lds_barrier();
    float* t = tc;
    tc = tn;
    tn = t;
  }
}
