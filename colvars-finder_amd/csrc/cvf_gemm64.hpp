// The 64 x 64 fp32 product core of the per-layer routes (csrc/ef_general.hip, ae_general.hip, regae_general.hip, cv_nets.hip;
// DESIGN.md section 4.8): one 64 x 64 output block per 256-thread workgroup, four waves of 32 x 32 each, on
// v_mfma_f32_16x16x4_f32.  Device functions, not kernels: a kernel sets up its pointers, gives a callable for a B element and
// one for the epilogue, and calls in.  Two LDS image layouts, each with its own k-step:
//   k-major      As [k][m], Bs [k][frame], 32-deep stages (the layer kernels: K = a layer's width)
//   frames-as-K  As [out row][frame], Bs [in column][frame], one 64-frame tile per stage (the weight-gradient kernels)
// With them: the slab-row rule, the checks the routes' *_why functions share, and the per-frame output gradient of the
// transfer-operator loss.  Everything has internal linkage: each code object carries its own copy of what it uses.
#pragma once
#include "cvf_common.hpp"
#include <stdio.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int kMaxWidth = 4096;     // widest hidden layer the routes accept (d0 up to kMaxD0)
constexpr int kMaxD0 = 65536;
constexpr int64_t kSlabBytes = 128ll << 20;   // slab budget: rows = 128 MiB / (4 n_params), at least 1, at most kMaxRows
constexpr int kMaxRows = 256;
constexpr int kKC = 32;          // K per LDS stage of the k-major images
constexpr int kPitch = 80;       // their LDS pitch (a fragment read spans 4 k-rows of 16 consecutive words)
constexpr int kGP = 68;          // LDS pitch of the [row][frame] images (a fragment read spans 16 rows x 4 consecutive frames)

// a thread's place in the block: wave (wm, wn) owns rows wm.. and columns wn.. of the 64 x 64 block, 32 of each
struct G64Thread {
  int lane, wave, wm, wn, col, kq;
};

__device__ __forceinline__ G64Thread g64_thread() {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return G64Thread{lane, wave, (wave & 1) * 32, (wave >> 1) * 32, lane & 15, lane >> 4};
}

__device__ __forceinline__ void g64_clear(f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// one 32-deep stage of the k-major images: eight k-steps of 4
__device__ __forceinline__ void g64_step_kmajor(const float* As, const float* Bs, const G64Thread& t, f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < kKC; ks += 4) {
    const int kr = (ks + t.kq) * kPitch;
    const float a0 = As[kr + t.wm + t.col], a1 = As[kr + t.wm + 16 + t.col];
    const float b0 = Bs[kr + t.wn + t.col], b1 = Bs[kr + t.wn + 16 + t.col];
    acc[0][0] = mfma4(a0, b0, acc[0][0]);
    acc[0][1] = mfma4(a0, b1, acc[0][1]);
    acc[1][0] = mfma4(a1, b0, acc[1][0]);
    acc[1][1] = mfma4(a1, b1, acc[1][1]);
  }
}

// one tile of the [row][frame] images: sixteen k-steps of 4 frames
__device__ __forceinline__ void g64_step_frames(const float* As, const float* Bs, const G64Thread& t, f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < 64; ks += 4) {
    const int kf = ks + t.kq;
    const float a0 = As[(t.wm + t.col) * kGP + kf], a1 = As[(t.wm + 16 + t.col) * kGP + kf];
    const float b0 = Bs[(t.wn + t.col) * kGP + kf], b1 = Bs[(t.wn + 16 + t.col) * kGP + kf];
    acc[0][0] = mfma4(a0, b0, acc[0][0]);
    acc[0][1] = mfma4(a0, b1, acc[0][1]);
    acc[1][0] = mfma4(a1, b0, acc[1][0]);
    acc[1][1] = mfma4(a1, b1, acc[1][1]);
  }
}

// one 32-deep stage of weights as the A operand: As[kk][ml] = A[m0 + ml][k0 + kk], zero outside M x K, in eight passes.
//   trans (A = W^T, W [K][ldw]): m runs along W's rows, over the lanes; a wave stages one k per pass.
//   else  (A = W [M][ldw], k contiguous): a wave stages 16 rows x 4 k per pass.  Lanes l and l + 1 read two neighbouring k of a
//   row (8 bytes), lanes l + 32 and l + 33 the next two; the 32 lanes of a half write two k-rows 16 words apart (pitch 80) at
//   16 consecutive m: 32 distinct banks.
// (`trans` is tested once per stage, outside the passes: inside them the compiler merges the two forms into one load at a
//  selected address and forms both 64-bit addresses for every element.)
__device__ __forceinline__ void g64_stage_weights(float* As, const float* W, int ldw, int trans, int m0, int k0, int M, int K,
                                                  const G64Thread& t) {
  if (trans) {
#pragma unroll
    for (int it = 0; it < kKC / 4; ++it) {
      const int kk = t.wave + 4 * it, k = k0 + kk, m = m0 + t.lane;
      As[kk * kPitch + t.lane] = m < M && k < K ? W[(int64_t)k * ldw + m] : 0.0f;
    }
  } else {
    const int kl = (t.lane & 1) + 2 * (t.lane >> 5), ml = 16 * t.wave + ((t.lane >> 1) & 15);
#pragma unroll
    for (int it = 0; it < kKC / 4; ++it) {
      const int kk = 4 * it + kl, k = k0 + kk, m = m0 + ml;
      As[kk * kPitch + ml] = m < M && k < K ? W[(int64_t)m * ldw + k] : 0.0f;
    }
  }
}

// acc = A[m0 .. m0 + 63][:] . B[:][64 frames]: A = W or W^T through g64_stage_weights, b(k) = this lane's frame of B row k < K
template <class BElem>
__device__ __forceinline__ void g64_layer_product(float* As, float* Bs, const float* W, int ldw, int trans, int m0, int M, int K,
                                                  const G64Thread& t, f32x4 (&acc)[2][2], BElem&& b) {
  g64_clear(acc);
  for (int k0 = 0; k0 < K; k0 += kKC) {
    g64_stage_weights(As, W, ldw, trans, m0, k0, M, K, t);
#pragma unroll
    for (int it = 0; it < kKC / 4; ++it) {
      const int kk = t.wave + 4 * it, k = k0 + kk;
      Bs[kk * kPitch + t.lane] = k < K ? b(k) : 0.0f;
    }
    __syncthreads();
    g64_step_kmajor(As, Bs, t, acc);
    __syncthreads();
  }
}

// f(row in block, frame or column in block, value) over a thread's accumulators: C row = 4 * (lane >> 4) + r of each 16 x 16
// block, column = lane & 15
template <class F>
__device__ __forceinline__ void g64_walk(const f32x4 (&acc)[2][2], const G64Thread& t, F&& f) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) f(t.wm + 16 * i + 4 * t.kq + r, t.wn + 16 * j + t.col, acc[i][j][r]);
}

// One 64 x 64 block (blockIdx.y) of a layer's [dW | db] [Mo][Ki + 1] in slab row rho = blockIdx.x: the sum over the tiles rho,
// rho + rows, ... in that order and, per tile, over `parts` operand pairs, of A (x) [B ; 1] with K = frames (the bias column
// belongs to part 0).  ael(tile, part, o) / bel(tile, part, i) = this lane's frame of row o < Mo / i < Ki.  Tiles T.. repeat
// the frames of tiles 0..; frames past B contribute nothing: zero on both operands.
// kNets (csrc/ef_general.hip, shared layers): the parts are those of several nets in a row, `per_net` each - part p belongs to net
// p / per_net and is that net's part p % per_net, so the bias column belongs to every per_net-th part.  The callers decode p.
template <bool kNets = false, class AElem, class BElem>
__device__ __forceinline__ void g64_wgrad_block(float* As, float* Bs, int Mo, int Ki, int64_t n_tiles, int64_t T, int64_t B, int rows,
                                                int parts, float* w_row, float* b_row, AElem&& ael, BElem&& bel, int per_net = 1) {
  const G64Thread t = g64_thread();
  const int rho = blockIdx.x;
  const int nbn = (Ki + 1 + 63) / 64;
  const int o0 = (blockIdx.y / nbn) * 64, i0 = (blockIdx.y % nbn) * 64;
  f32x4 acc[2][2];
  g64_clear(acc);
  for (int64_t tile = rho; tile < n_tiles; tile += rows) {
    const int64_t t0 = tile >= T ? tile - T : tile;
    const bool valid = t0 * CVF_TILE + t.lane < B;
    for (int part = 0; part < parts; ++part) {
#pragma unroll 4
      for (int it = 0; it < 16; ++it) {
        const int rr = t.wave + 4 * it;
        const int o = o0 + rr, i = i0 + rr;
        As[rr * kGP + t.lane] = valid && o < Mo ? ael(tile, part, o) : 0.0f;
        float x = 0.0f;
        if (valid) {
          if (i < Ki) x = bel(tile, part, i);
          else if (i == Ki && (kNets ? (part & (per_net - 1)) == 0 : part == 0)) x = 1.0f;   // the bias column: [h ; 1] (a second part has [. ; 0]; per_net is 1 or 2)
        }
        Bs[rr * kGP + t.lane] = x;
      }
      __syncthreads();
      g64_step_frames(As, Bs, t, acc);
      __syncthreads();
    }
  }
  g64_walk(acc, t, [&](int ro, int rc, float v) {
    const int o = o0 + ro, c = i0 + rc;
    if (o >= Mo || c > Ki) return;
    if (c < Ki) w_row[(int64_t)o * Ki + c] = v;
    else b_row[o] = v;
  });
}

// d loss / d y_i of one frame of the transfer-operator loss, in fp64.  coef = [gS1 (k), gS2 (k x k), gT (k), gS1' (k), gS2'_ii (k)];
// yb / yl: the frame's k outputs of the base / the lagged pass (stride CVF_TILE); the value is the gradient at the base output
// (weight wb) or, with `lagged`, at the lagged one (weight wl)
__device__ __forceinline__ double g64_transfer_grad(const double* __restrict__ coef, int k, int i, const float* yb, const float* yl,
                                                    bool lagged, float wb, float wl) {
  const double* gS1 = coef;
  const double* gS2 = coef + k;
  const double* gT = coef + k + k * k;
  const double* gS1l = coef + 2 * k + k * k;
  const double* gS2l = coef + 3 * k + k * k;
  const double diff = (double)yl[i * CVF_TILE] - (double)yb[i * CVF_TILE];
  const double tterm = 2.0 * (double)wb * gT[i] * diff;
  if (lagged) return (double)wl * (gS1l[i] + 2.0 * gS2l[i] * (double)yl[i * CVF_TILE]) + tterm;
  double s = gS1[i];
  for (int j = 0; j < k; ++j) s += (j == i ? 2.0 : 1.0) * gS2[i * k + j] * (double)yb[j * CVF_TILE];
  return (double)wb * s - tterm;
}

// slab rows of the weight gradient: 128 MiB / (4 n_params), at least 1, at most kMaxRows and the tile count
int64_t g64_rows(const cvf_mlp_desc* mlp, int64_t n_tiles) {
  int64_t r = kSlabBytes / (4 * (int64_t)(mlp->n_params > 0 ? mlp->n_params : 1));
  r = r < 1 ? 1 : r > kMaxRows ? kMaxRows : r;
  return n_tiles < r ? (n_tiles < 1 ? 1 : n_tiles) : r;
}

// What a route asks of the first L layers of a description, beyond what the core itself needs
struct G64Chain {
  int min_layers;        // fewest Linear layers
  const char* layer;     // the noun of a refused width: "hidden layer" / "layer"
  const char* owner;     // whose parameters the flat buffer holds: "nets" / "chain"
  bool exact_params;     // the layers' parameters ARE the flat buffer (a slab row mirrors it): count and offsets
  bool grad_blocks;      // a layer's 64 x 64 blocks of [W | b] are the grid.y of a weight-gradient launch
};

// The checks the routes share, in this order: the layer count, the input width, the hidden widths, the gradient blocks, the
// activation codes, the parameter count and offsets.  NULL, or the reason in buf.  (The caller has checked mlp and n_nets.)
const char* g64_why(const cvf_mlp_desc* mlp, int L, const G64Chain& c, char* buf, size_t n_buf) {
  if (mlp->n_layers < c.min_layers || mlp->n_layers > CVF_MAX_LAYERS) {
    snprintf(buf, n_buf, "%d layers: %d to %d are supported", mlp->n_layers, c.min_layers, CVF_MAX_LAYERS);
    return buf;
  }
  if (mlp->dims[0] < 1 || mlp->dims[0] > kMaxD0) {
    snprintf(buf, n_buf, "%d input features: 1 to %d are supported", mlp->dims[0], kMaxD0);
    return buf;
  }
  for (int l = 1; l < L; ++l)
    if (mlp->dims[l] < 1 || mlp->dims[l] > kMaxWidth) {
      snprintf(buf, n_buf, "%s %d is %d wide: 1 to %d units are supported", c.layer, l, mlp->dims[l], kMaxWidth);
      return buf;
    }
  if (c.grad_blocks)
    for (int l = 0; l < L; ++l)
      if ((int64_t)((mlp->dims[l + 1] + 63) / 64) * ((mlp->dims[l] + 1 + 63) / 64) > 65535) {
        snprintf(buf, n_buf, "layer %d (%d x %d) has more than 65535 blocks of 64 x 64 weights", l, mlp->dims[l + 1], mlp->dims[l]);
        return buf;
      }
  for (int l = 0; l < L; ++l)
    if (mlp->act[l] < CVF_ACT_NONE || mlp->act[l] > CVF_ACT_SOFTPLUS) return "an activation code outside include/cvf.h";
  if (!c.exact_params) return nullptr;
  int64_t n = 0;
  for (int l = 0; l < L; ++l) n += (int64_t)mlp->dims[l + 1] * (mlp->dims[l] + 1);
  n *= mlp->n_nets;
  if (n != mlp->n_params) {
    snprintf(buf, n_buf, "the flat buffer holds parameters outside the %s", c.owner);
    return buf;
  }
  for (int i = 0; i < mlp->n_nets; ++i)
    for (int l = 0; l < L; ++l)
      if (mlp->w_off[i][l] < 0 || mlp->w_off[i][l] + (int64_t)mlp->dims[l + 1] * mlp->dims[l] > n || mlp->b_off[i][l] < 0 ||
          mlp->b_off[i][l] + (int64_t)mlp->dims[l + 1] > n)
        return "a layer's parameters lie outside the flat buffer";
  return nullptr;
}

}  // namespace
