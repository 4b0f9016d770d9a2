// The per-layer kernels of the chains that do not fit LDS, shared by the AutoEncoderTask step (csrc/ae_general.hip) and the
// RegAutoEncoderTask route (csrc/regae_general.hip): gather, layer product (forward / transposed), weight gradient into slab
// rows, the tiles' loss pairs.  Every kernel has internal linkage: each code object that includes this header carries its own
// copy of the ones it launches.  See csrc/ae_general.hip for the decomposition and DESIGN.md sections 4.10 / 4.11.
#pragma once
#include "cvf_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int kMaxWidth = 4096;     // widest hidden layer cvf_ae_general_supported() accepts (d0 up to kMaxD0)
constexpr int kMaxD0 = 65536;
constexpr int64_t kSlabBytes = 128ll << 20;   // slab budget: rows = 128 MiB / (4 n_params), at least 1, at most kMaxRows
constexpr int kMaxRows = 256;

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

// out[m][frame] (64 x 64 block) = A[m][:] . B[:][frame] for one (tile, row block); 4 waves of 32 x 32
constexpr int kKC = 32;          // K per LDS stage
constexpr int kPitch = 80;       // LDS pitch of the k-major images (a fragment read spans 4 k-rows of 16 consecutive words)
__global__ __launch_bounds__(256) void aeg_layer_kernel(const float* __restrict__ theta, AegLayerArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kKC * kPitch];   // [k][m]
  __shared__ __attribute__((aligned(16))) float Bs[kKC * kPitch];   // [k][frame]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tile = blockIdx.x;
  const int m0 = blockIdx.y * 64;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int col = lane & 15, kq = lane >> 4;
  const float* W = theta + a.w_off;
  const float* xp = a.x + tile * a.xs;
  // W as stored ([m][k], k contiguous): a wave stages 16 rows x 4 k per pass.  Lanes l and l + 1 read two neighbouring k of a
  // row (8 bytes), lanes l + 32 and l + 33 the next two; the 32 lanes of a half write two k-rows 16 words apart (pitch 80) at
  // 16 consecutive m: 32 distinct banks
  const int kl = (lane & 1) + 2 * (lane >> 5), ml = 16 * wave + ((lane >> 1) & 15);

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  for (int k0 = 0; k0 < a.K; k0 += kKC) {
#pragma unroll
    for (int it = 0; it < kKC / 4; ++it) {
      if (a.trans) {   // W^T: m runs along W's rows, over the lanes
        const int kk = wave + 4 * it, k = k0 + kk, m = m0 + lane;
        As[kk * kPitch + lane] = m < a.M && k < a.K ? W[(int64_t)k * a.ldw + m] : 0.0f;
      } else {
        const int kk = 4 * it + kl, k = k0 + kk, m = m0 + ml;
        As[kk * kPitch + ml] = m < a.M && k < a.K ? W[(int64_t)m * a.ldw + k] : 0.0f;
      }
      const int kk = wave + 4 * it, k = k0 + kk;
      Bs[kk * kPitch + lane] = k < a.K ? xp[(int64_t)k * CVF_TILE + lane] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kKC; ks += 4) {
      const int kr = (ks + kq) * kPitch;
      const float a0 = As[kr + wm + col], a1 = As[kr + wm + 16 + col];
      const float b0 = Bs[kr + wn + col], b1 = Bs[kr + wn + 16 + col];
      acc[0][0] = mfma4(a0, b0, acc[0][0]);
      acc[0][1] = mfma4(a0, b1, acc[0][1]);
      acc[1][0] = mfma4(a1, b0, acc[1][0]);
      acc[1][1] = mfma4(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }

  // epilogue: C row = 4 * (lane >> 4) + r of each 16 x 16 block, column (frame) = lane & 15
  const float* bias = a.b_off >= 0 ? theta + a.b_off : nullptr;
  float* op = a.out + tile * a.os;
  const float* ep = a.epi == EPI_BWD ? a.eh + tile * a.es : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + 4 * kq + r;
        const int f = wn + 16 * j + col;
        if (m >= a.M) continue;
        float v = acc[i][j][r];
        const int64_t o = (int64_t)m * CVF_TILE + f;
        if (a.epi == EPI_ACT) {
          if (bias != nullptr) v += bias[m];
          op[o] = cvf_act(a.act, v);
        } else {
          op[o] = cvf_act_d1(a.act, ep[o]) * v;
        }
      }
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

constexpr int kGP = 68;   // LDS pitch of the [row][frame] images (a fragment read spans 16 rows x 4 consecutive frames)
__global__ __launch_bounds__(256) void aeg_wgrad_kernel(AegGradArgs a, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float As[64 * kGP];   // [out row][frame]
  __shared__ __attribute__((aligned(16))) float Bs[64 * kGP];   // [in column][frame]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rho = blockIdx.x;
  const int nbn = (a.Ki + 1 + 63) / 64;
  const int o0 = (blockIdx.y / nbn) * 64, i0 = (blockIdx.y % nbn) * 64;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int col = lane & 15, kq = lane >> 4;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  for (int64_t tile = rho; tile < a.n_tiles; tile += a.rows) {
    const bool valid = tile * CVF_TILE + lane < a.B;   // padded frames contribute nothing: zero on both operands
    const float* zp = a.z + tile * a.zs;
    const float* hp = a.h + tile * a.hs;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int rr = wave + 4 * it;
      const int o = o0 + rr, i = i0 + rr;
      As[rr * kGP + lane] = valid && o < a.Mo ? zp[(int64_t)o * CVF_TILE + lane] : 0.0f;
      float x = 0.0f;
      if (valid) {
        if (i < a.Ki) x = hp[(int64_t)i * CVF_TILE + lane];
        else if (i == a.Ki) x = 1.0f;   // the bias column: [a ; 1]
      }
      Bs[rr * kGP + lane] = x;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 64; ks += 4) {
      const int kf = ks + kq;
      const float a0 = As[(wm + col) * kGP + kf], a1 = As[(wm + 16 + col) * kGP + kf];
      const float b0 = Bs[(wn + col) * kGP + kf], b1 = Bs[(wn + 16 + col) * kGP + kf];
      acc[0][0] = mfma4(a0, b0, acc[0][0]);
      acc[0][1] = mfma4(a0, b1, acc[0][1]);
      acc[1][0] = mfma4(a1, b0, acc[1][0]);
      acc[1][1] = mfma4(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }

  float* row = slab + (int64_t)rho * a.n_params;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + wm + 16 * i + 4 * kq + r;
        const int c = i0 + wn + 16 * j + col;
        if (o >= a.Mo || c > a.Ki) continue;
        if (c < a.Ki) row[a.w_off + (int64_t)o * a.Ki + c] = acc[i][j][r];
        else row[a.b_off + o] = acc[i][j][r];
      }
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

// slab rows of the weight gradient: 128 MiB / (4 n_params), at least 1, at most kMaxRows and the tile count
int64_t aeg_rows(const cvf_mlp_desc* mlp, int64_t n_tiles) {
  int64_t r = kSlabBytes / (4 * (int64_t)(mlp->n_params > 0 ? mlp->n_params : 1));
  r = r < 1 ? 1 : r > kMaxRows ? kMaxRows : r;
  return n_tiles < r ? (n_tiles < 1 ? 1 : n_tiles) : r;
}

}  // namespace
