// The trunk-boundary launch of the transfer-mode shared step (csrc/ef_general.hip: cvf_ef_general_shared_transfer_backward;
// DESIGN.md section 4.12), in a code object of its own (csrc/ef_general_sum.hip).
#pragma once
#include "cvf_common.hpp"

// zbar_{layer-1} [M = dims[layer]] = sigma'(h_{layer-1}) .* sum_net W_{layer,net}^T zbar_{layer,net}, K = dims[layer + 1].
// Tiled images, element (tile, row, lane) at tile * width * 64 + row * 64 + lane:
//   x    zbar_layer, per net (width K; net stride x_ns floats);  out  zbar_{layer-1}, one image (width M);
//   eh   h_{layer-1}, one image (width M), sigma' of `act_e` through it.
struct EftrSumArgs {
  int layer, M, K, nets, act_e;
  const float* x;
  int64_t x_ns;
  float* out;
  const float* eh;
};

// one launch over (n_tiles, 64-row blocks of M); 0, or -1 with the reason in cvf_last_error()
int eftr_launch_trunk_sum(const cvf_mlp_desc* mlp, const float* theta, const EftrSumArgs& a, int64_t n_tiles, hipStream_t s);
