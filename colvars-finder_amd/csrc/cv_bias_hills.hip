// Hill deposition into a CVF_BIAS_TABLE term on the device (cvf_cv_bias_deposit): metadynamics along a
// trained CV without a host round trip.  The centres are the xi_rows a bias launch (csrc/cv_bias.hip) just wrote; the formulas of a
// hill's height and of its share of a node are csrc/cvf_bias.hpp's, host and device from one text.  Two launches on the caller's
// stream:
//
//   heights  one thread per hill: V_b = the target term's own U at the centre, read through the eval's interpolation from the table
//            BEFORE any hill of this call, w_b = height exp(-V_b inv_kdt); hills[b] = (c1, c2, w_b, V_b)
//   nodes    one thread per node: the node is read once (16 bytes in 2-D, 8 in 1-D), the hills are added in order b = 0 .. B - 1 in
//            registers - staged through LDS CVF_HILL_CHUNK at a time - and the node is written once
//
// Two, because every height must see the table before any workgroup has written to it.  No atomics, no allocation, no host
// synchronisation; a node's bits depend on nothing but its own value and the hills row, so not on the launch geometry.
#include <hip/hip_runtime.h>

#include "cvf_bias.hpp"
#include "cvf_common.hpp"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void hill_heights_kernel(cvf_bias_term term, cvf_hill_desc hill, const float* __restrict__ table,
                                                                const float* __restrict__ xi_rows, int k, int B,
                                                                float* __restrict__ hills) {
  const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;   // (64 bits: B may lie within a workgroup of 2^31 - 1)
  if (b >= B) return;
  float row[4];
  cvf_hill_row(term, table, hill, xi_rows + b * k, row);
  for (int i = 0; i < 4; ++i) hills[4 * b + i] = row[i];
}

template <bool TWO_D>
__global__ __launch_bounds__(kThreads) void hill_nodes_kernel(cvf_bias_term term, cvf_hill_desc hill, const float* __restrict__ hills, int B,
                                                              float* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) float stage[4 * CVF_HILL_CHUNK];
  constexpr int W = TWO_D ? 4 : 2;
  const int n2 = TWO_D ? term.n_nodes2 : 1;
  const int n = term.n_nodes * n2;   // (cvf_bias_why: 4 n fits n_table, an int32)
  const int node = blockIdx.x * kThreads + threadIdx.x;
  const bool mine = node < n;
  // (a 2-D node is one 16-byte access: cvf_bias_why has checked table and tab_off; a 1-D table is only known to hold floats)
  float* p = (float*)__builtin_assume_aligned(table + term.tab_off + W * (int64_t)(mine ? node : 0), TWO_D ? 16 : 4);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (mine) __builtin_memcpy(acc, p, 4 * W);
  const int j1 = node / n2, j2 = node - j1 * n2;
  const float x1 = cvf_bias_node_pos(term.lo, term.inv_h, j1), x2 = TWO_D ? cvf_bias_node_pos(term.lo2, term.inv_h2, j2) : 0.0f;
  for (int base = 0; base < B; base += CVF_HILL_CHUNK) {   // (every thread of the workgroup takes every barrier)
    const int nb = B - base < CVF_HILL_CHUNK ? B - base : CVF_HILL_CHUNK;
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * nb; i += kThreads) stage[i] = hills[4 * (int64_t)base + i];
    __syncthreads();
    if (mine)
      for (int i = 0; i < nb; ++i) cvf_hill_node_add<TWO_D>(hill, stage + 4 * i, x1, x2, acc);
  }
  if (mine) __builtin_memcpy(p, acc, 4 * W);
}

}  // namespace

extern "C" int cvf_cv_bias_deposit(const cvf_bias_desc* bias, int k, const cvf_hill_desc* hill, const float* xi_rows, int64_t B,
                                   float* table, float* hills, void* stream) {
  const char* name = "cvf_cv_bias_deposit";
  char buf[240];
  const char* why = cvf_bias_why(bias, k, buf, sizeof buf);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  why = cvf_hill_why(bias, hill, buf, sizeof buf);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  CVF_REQUIRE(table != nullptr && table == bias->table, "%s: table = %p, bias->table = %p: the hills go into the table the bias reads", name,
              (void*)table, (const void*)bias->table);
  CVF_REQUIRE(B >= 0 && B <= 0x7fffffff, "%s: B = %lld hills (one call takes 0 to 2^31 - 1)", name, (long long)B);
  if (B == 0) return 0;
  CVF_REQUIRE(xi_rows != nullptr && hills != nullptr, "%s: null argument", name);
  const cvf_bias_term& t = bias->term[hill->term];
  const bool two_d = t.n_nodes2 != 0;
  const int n = t.n_nodes * (two_d ? t.n_nodes2 : 1);
  hipLaunchKernelGGL(hill_heights_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, t, *hill,
                     (const float*)table, xi_rows, k, (int)B, hills);
  int rc = cvf_check_launch("hill_heights_kernel");
  if (rc != 0) return rc;
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
  if (two_d)
    hipLaunchKernelGGL(hill_nodes_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, t, *hill, (const float*)hills, (int)B, table);
  else
    hipLaunchKernelGGL(hill_nodes_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, t, *hill, (const float*)hills, (int)B, table);
  return cvf_check_launch("hill_nodes_kernel");
}
