// The launch that sums over the nets at the trunk boundary of the transfer-mode shared step (cvf_ef_general_shared_transfer_backward,
// csrc/ef_general.hip): the k heads hand their adjoints zbar_{ns,i} to ONE trunk,
//   zbar_{ns-1} = sigma'(h_{ns-1}) .* sum_i W_{ns,i}^T zbar_{ns,i}.
// One block per (tile, 64-row block of the trunk's last width) walks the nets 0..k-1 in that order into one accumulator on the
// 64 x 64 core of csrc/cvf_gemm64.hpp, every net's product in k order, and writes the one image of zbar_{ns-1}: no atomics, one
// thread per entry, a fixed sum order - the same inputs give the same bits, and one net gives the sums of efg_layer_kernel.
#include "cvf_gemm64.hpp"
#include "ef_general_sum.hpp"

namespace {

__global__ __launch_bounds__(256) void eftr_trunk_sum_kernel(cvf_mlp_desc mlp, const float* __restrict__ theta, EftrSumArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kKC * kPitch];   // [k][m]
  __shared__ __attribute__((aligned(16))) float Bs[kKC * kPitch];   // [k][frame]
  const G64Thread t = g64_thread();
  const int64_t tile = blockIdx.x;
  const int m0 = blockIdx.y * 64, ldw = mlp.dims[a.layer];
  f32x4 acc[2][2];
  g64_clear(acc);
  for (int net = 0; net < a.nets; ++net) {
    const float* W = theta + mlp.w_off[net][a.layer];   // [K][ldw = M]: A = W^T
    const float* xp = a.x + net * a.x_ns + tile * a.K * CVF_TILE;
    for (int k0 = 0; k0 < a.K; k0 += kKC) {
      g64_stage_weights(As, W, ldw, 1, m0, k0, a.M, a.K, t);
#pragma unroll
      for (int it = 0; it < kKC / 4; ++it) {
        const int kk = t.wave + 4 * it, k = k0 + kk;
        Bs[kk * kPitch + t.lane] = k < a.K ? xp[(int64_t)k * CVF_TILE + t.lane] : 0.0f;
      }
      __syncthreads();
      g64_step_kmajor(As, Bs, t, acc);
      __syncthreads();
    }
  }
  const int64_t img = tile * a.M * CVF_TILE;
  g64_walk(acc, t, [&](int row, int f, float v) {
    const int m = m0 + row;
    if (m >= a.M) return;
    const int64_t e = img + (int64_t)m * CVF_TILE + f;
    a.out[e] = cvf_act_d1(a.act_e, a.eh[e]) * v;
  });
}

}  // namespace

int eftr_launch_trunk_sum(const cvf_mlp_desc* mlp, const float* theta, const EftrSumArgs& a, int64_t n_tiles, hipStream_t s) {
  hipLaunchKernelGGL(eftr_trunk_sum_kernel, dim3((unsigned)n_tiles, (unsigned)((a.M + 63) / 64)), dim3(256), 0, s, *mlp, theta, a);
  return cvf_check_launch("eftr_trunk_sum_kernel");
}
