// Developer tool: v_mfma_f32_4x4x1_16B_f32 on gfx950 - operand layout, issue cost, and a fixed instruction count for a counter run.
//   hipcc -O3 --offload-arch=gfx950 tools/mfma4x4_probe.hip -o /tmp/mfma4x4_probe
//   /tmp/mfma4x4_probe            (a) layout against a host loop, (b) s_memtime ticks per instruction
//   rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES -- /tmp/mfma4x4_probe count
//                                 (c) one wave issues 4096 instructions per kernel: p_count_4x4, p_count_16x16, p_count_mixed (2048 + 2048)
// The instruction computes sixteen independent 4x4 outer products, one per group of four lanes.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 m4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 m16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// (a) D = C + A B, one instruction; out[lane][r]
__global__ void p_layout(const float* a, const float* b, const float* c, float* out) {
  const int lane = threadIdx.x;
  f32x4 acc = {c[4 * lane], c[4 * lane + 1], c[4 * lane + 2], c[4 * lane + 3]};
  acc = m4(a[lane], b[lane], acc);
  for (int r = 0; r < 4; ++r) out[4 * lane + r] = acc[r];
}

// (b) NI instructions between two s_memtime reads, NACC accumulators in rotation; KIND 0: 4x4x1, 1: 16x16x4, 2: alternating
template <int KIND, int NACC, int NI>
__global__ void p_issue(unsigned long long* out, float seed) {
  f32x4 acc[NACC];
  for (int i = 0; i < NACC; ++i) {
    acc[i] = f32x4{seed + i, seed, seed, seed};
    asm volatile("" : "+v"(acc[i]));   // (opaque: identical chains would be merged into one)
  }
  const float a = seed + threadIdx.x, b = seed * 1.0001f;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const bool four = KIND == 0 || (KIND == 2 && (i & 1));
    acc[i % NACC] = four ? m4(a, b, acc[i % NACC]) : m16(a, b, acc[i % NACC]);
  }
  __builtin_amdgcn_sched_barrier(0);
  float s = 0.0f;   // (reading the accumulators waits for the last instruction's result)
  for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  asm volatile("" : "+v"(s));
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_s_waitcnt(0);
  if (threadIdx.x == 0) out[0] = t1 - t0;
  if (s == 1.2345f) out[1] = 1;
}

static unsigned long long run_issue(void (*k)(unsigned long long*, float), unsigned long long* d) {
  unsigned long long best = ~0ull;
  for (int rep = 0; rep < 5; ++rep) {
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d, 1.5f);
    unsigned long long h[2];
    if (hipMemcpy(h, d, 16, hipMemcpyDeviceToHost) != hipSuccess) exit(2);
    if (h[0] < best) best = h[0];
  }
  return best;
}

int main(int argc, char** argv) {
  unsigned long long* d;
  if (hipMalloc(&d, 16) != hipSuccess) return 2;
  if (argc > 1 && !strcmp(argv[1], "count")) {   // (c): 4096 instructions of one wave per kernel
    hipLaunchKernelGGL((p_issue<0, 4, 4096>), dim3(1), dim3(64), 0, 0, d, 1.5f);
    hipLaunchKernelGGL((p_issue<1, 4, 4096>), dim3(1), dim3(64), 0, 0, d, 1.5f);
    hipLaunchKernelGGL((p_issue<2, 4, 4096>), dim3(1), dim3(64), 0, 0, d, 1.5f);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 2;
  }
  // (a)
  float ha[64], hb[64], hc[256], ho[256], *da, *db, *dc, *dout;
  srand(1);
  for (int i = 0; i < 64; ++i) { ha[i] = rand() / (float)RAND_MAX - 0.5f; hb[i] = rand() / (float)RAND_MAX - 0.5f; }
  for (int i = 0; i < 256; ++i) hc[i] = rand() / (float)RAND_MAX - 0.5f;
  if (hipMalloc(&da, 256) != hipSuccess || hipMalloc(&db, 256) != hipSuccess || hipMalloc(&dc, 1024) != hipSuccess || hipMalloc(&dout, 1024) != hipSuccess) return 2;
  (void)hipMemcpy(da, ha, 256, hipMemcpyHostToDevice);
  (void)hipMemcpy(db, hb, 256, hipMemcpyHostToDevice);
  (void)hipMemcpy(dc, hc, 1024, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(p_layout, dim3(1), dim3(64), 0, 0, da, db, dc, dout);
  if (hipMemcpy(ho, dout, 1024, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  // expected: block blk = lane >> 2; register r of lane 4 blk + j = C + A_blk[r] B_blk[j]
  double worst = 0.0;
  for (int blk = 0; blk < 16; ++blk)
    for (int j = 0; j < 4; ++j)
      for (int r = 0; r < 4; ++r) {
        const int lane = 4 * blk + j;
        const float want = fmaf(ha[4 * blk + r], hb[4 * blk + j], hc[4 * lane + r]);
        worst = fmax(worst, fabs((double)want - (double)ho[4 * lane + r]));
      }
  printf("(a) layout  D_b[r][j] in register r of lane 4b+j, A_b[i] / B_b[i] in lane 4b+i: worst |diff| = %.3g  %s\n", worst,
         worst < 1e-6 ? "CONFIRMED" : "NOT THIS LAYOUT");
  // (b)
  struct { const char* name; void (*k)(unsigned long long*, float); int n; } t[] = {
      {"4x4x1   one accumulator  ", p_issue<0, 1, 64>, 64},   {"4x4x1   four accumulators", p_issue<0, 4, 64>, 64},
      {"4x4x1   four acc., 256   ", p_issue<0, 4, 256>, 256}, {"16x16x4 one accumulator  ", p_issue<1, 1, 64>, 64},
      {"16x16x4 four accumulators", p_issue<1, 4, 64>, 64},   {"16x16x4 four acc., 256   ", p_issue<1, 4, 256>, 256},
      {"alternating, four acc.   ", p_issue<2, 4, 64>, 64},   {"alternating, four acc.256", p_issue<2, 4, 256>, 256}};
  for (auto& e : t) {
    const unsigned long long c = run_issue(e.k, d);
    printf("(b) %s %4d instructions: %6llu s_memtime ticks = %6.2f per instruction\n", e.name, e.n, c, c / (double)e.n);
  }
  return worst < 1e-6 ? 0 : 1;
}
