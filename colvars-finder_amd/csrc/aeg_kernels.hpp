// The per-layer kernels of the chains that do not fit LDS, shared by the AutoEncoderTask step (csrc/ae_general.hip) and the
// RegAutoEncoderTask route (csrc/regae_general.hip): gather, layer product (forward / transposed), weight gradient into slab
// rows, the tiles' loss pairs.  The two products are calls into the 64 x 64 core of csrc/cvf_gemm64.hpp.  Every kernel has
// internal linkage: each code object that includes this header carries its own copy of the ones it launches.  See
// csrc/ae_general.hip for the decomposition and DESIGN.md sections 4.8 / 4.10 / 4.11.
#pragma once
#include "cvf_gemm64.hpp"

namespace {

// ---- feat_rows[idx] -> [tile][d0][64], 64 features at a time through an LDS transpose (rows are read along the features).
// Tiles t_lag .. take the frames of tiles 0 .. again, at the rows idx + lag (RegAutoEncoderTask's lagged partners); a plain batch
// passes t_lag = the tile count.
constexpr int kTP = 65;
__global__ __launch_bounds__(256) void aeg_gather_kernel(const float* __restrict__ feat_rows, const int64_t* __restrict__ idx,
                                                         int64_t B, int d0, float* __restrict__ a0, int64_t t_lag,
                                                         int64_t lag) {
  __shared__ float S[CVF_TILE * kTP];   // [frame][feature]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t t0 = tile >= t_lag ? tile - t_lag : tile, shift = tile >= t_lag ? lag : 0;
  float* out = a0 + tile * d0 * CVF_TILE;
  for (int c0 = 0; c0 < d0; c0 += 64) {
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int fr = wave + 4 * it;
      const int64_t frame = t0 * CVF_TILE + fr;
      float v = 0.0f;
      if (frame < B && c0 + lane < d0) {
        const int64_t row = (idx != nullptr ? idx[frame] : frame) + shift;
        v = feat_rows[row * d0 + c0 + lane];
      }
      S[fr * kTP + lane] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int c = wave + 4 * it;
      if (c0 + c < d0) out[(int64_t)(c0 + c) * CVF_TILE + lane] = S[lane * kTP + c];
    }
    __syncthreads();
  }
}

enum { EPI_ACT = 0, EPI_BWD = 1 };

struct AegLayerArgs {
  int w_off, b_off;   // offsets of W_layer and b_layer in theta (b_off < 0: no bias)
  int ldw;            // row length of W_layer (= dims[layer])
  int trans;          // 0: A = W [M = dims[layer+1]][K = dims[layer]];  1: A = W^T [M = dims[layer]][K = dims[layer+1]]
  int M, K;
  int epi, act;       // EPI_ACT: out = act(acc + b);  EPI_BWD: out = acc .* act'(eh)
  const float* x;     // B operand [tile][K][64]
  float* out;         // [tile][M][64]
  const float* eh;    // EPI_BWD: [tile][M][64]
  int64_t xs, os, es; // tile strides of the three images
};

// out[m][frame] (64 x 64 block) = A[m][:] . B[:][frame] for one (tile, row block)
__global__ __launch_bounds__(256) void aeg_layer_kernel(const float* __restrict__ theta, AegLayerArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kKC * kPitch];   // [k][m]
  __shared__ __attribute__((aligned(16))) float Bs[kKC * kPitch];   // [k][frame]
  const G64Thread t = g64_thread();
  const int64_t tile = blockIdx.x;
  const int m0 = blockIdx.y * 64;
  const float* xp = a.x + tile * a.xs;

  f32x4 acc[2][2];
  g64_layer_product(As, Bs, theta + a.w_off, a.ldw, a.trans, m0, a.M, a.K, t, acc,
                    [&](int k) { return xp[(int64_t)k * CVF_TILE + t.lane]; });

  const float* bias = a.b_off >= 0 ? theta + a.b_off : nullptr;
  float* op = a.out + tile * a.os;
  const float* ep = a.epi == EPI_BWD ? a.eh + tile * a.es : nullptr;
  g64_walk(acc, t, [&](int row, int f, float v) {
    const int m = m0 + row;
    if (m >= a.M) return;
    const int64_t o = (int64_t)m * CVF_TILE + f;
    if (a.epi == EPI_ACT) {
      if (bias != nullptr) v += bias[m];
      op[o] = cvf_act(a.act, v);
    } else {
      op[o] = cvf_act_d1(a.act, ep[o]) * v;
    }
  });
}

struct AegGradArgs {
  int w_off, b_off;   // where layer's W [Mo][Ki] and b [Mo] sit in a slab row
  int Mo, Ki;
  int64_t n_tiles, B;
  int rows;           // slab rows R: row rho sums tiles rho, rho + R, ... in that order
  int64_t n_params;
  const float* z;     // zbar_{layer+1} [tile][Mo][64]
  const float* h;     // a_layer [tile][Ki][64]
  int64_t zs, hs;
};

// the one-part case of g64_wgrad_block: no lagged repeat (T = n_tiles)
__global__ __launch_bounds__(256) void aeg_wgrad_kernel(AegGradArgs a, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float As[64 * kGP];   // [out row][frame]
  __shared__ __attribute__((aligned(16))) float Bs[64 * kGP];   // [in column][frame]
  const int lane = threadIdx.x & 63;
  float* row = slab + (int64_t)blockIdx.x * a.n_params;
  g64_wgrad_block(
      As, Bs, a.Mo, a.Ki, a.n_tiles, a.n_tiles, a.B, a.rows, 1, row + a.w_off, row + a.b_off,
      [&](int64_t tile, int, int o) { return a.z[tile * a.zs + (int64_t)o * CVF_TILE + lane]; },
      [&](int64_t tile, int, int i) { return a.h[tile * a.hs + (int64_t)i * CVF_TILE + lane]; });
}

// loss-only calls: the tiles' [sum w err, sum w] pairs, fixed order -> out2 = {a, b, a / b} (cvf_ae_step's ae_loss_sum_kernel)
__global__ __launch_bounds__(64) void aeg_loss_sum_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ out2) {
  const int lane = threadIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t g = lane; g < n; g += 64) {
    a0 += partial[2 * g];
    a1 += partial[2 * g + 1];
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (lane == 0) {
    out2[0] = a0;
    out2[1] = a1;
    out2[2] = a0 / a1;
  }
}

}  // namespace
