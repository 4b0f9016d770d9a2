// CVF_PP_FACTORED (include/cvf.h): the preprocessing layer is any torch module, evaluated once per frame on the host side.
// A frame is one fp32 record [r (d_r) | L (d_r x rho, row-major)] with L L^T = J A J^T, the feature-space metric of the
// generator loss.  Per frame and net:  t = L^T g,  q = L t,  E = |t|^2.
//
// metric_factor_kernel: one 256-thread workgroup per group of F frames of one 64-frame tile (F in {16, 8, 4, 2, 1}).  The
// group's records are one contiguous range of memory: it is copied to LDS with aligned 16-byte loads (every load of the
// workgroup issued before the first wait: F records in flight), then
//   pass 1  t[f][j][c] = sum_i L[f][i][c] g[f][j][i]   work item (f, c), all k nets per L read  (LDS row reads: conflict-free)
//   pass 2  q[f][j][i] = sum_c L[f][i][c] t[f][j][c]   work item (f, i), all k nets per L read
//   E[f][j] = sum_c t[f][j][c]^2.
// Frames whose record does not fit the staging buffer (F = 1) are cut into row chunks: pass 1 over the chunks, then pass 2 over
// them again (the second read of a chunk comes from the L2 / Infinity Cache the first one filled).
#include "cvf_common.hpp"

namespace {

constexpr int kFactorThreads = 256;
constexpr int kStageCap = 12288;   // floats of staged records (48 KiB)
constexpr int kGCap = 2048;        // floats of staged g (F * k * rows)
constexpr int kTCap = 2048;        // floats of t (F * k * rho)

struct FactorPlan {
  int F;        // frames per workgroup (divides 64)
  int rows;     // rows of L per chunk (d_r: the whole frame)
  int nchunk;   // chunks per frame
  size_t lds;   // bytes
};

FactorPlan factor_plan(int d_r, int rho, int k) {
  const int64_t W = (int64_t)d_r * (1 + rho);
  FactorPlan p = {1, d_r, 1, 0};
  for (int F = 16; F >= 1; F >>= 1) {
    if (F * W + 8 <= kStageCap && F * k * d_r <= kGCap && F * k * rho <= kTCap) {
      p.F = F;
      break;
    }
    if (F == 1) {   // row chunks of one frame
      int r = (kStageCap - 8) / rho;
      if (r > kGCap / k) r = kGCap / k;
      if (r > d_r) r = d_r;
      p.rows = r;
      p.nchunk = (d_r + r - 1) / r;
    }
  }
  const int stage = p.nchunk == 1 ? (int)(p.F * W + 8) : p.rows * rho + 8;
  p.lds = ((size_t)stage + (size_t)p.F * k * p.rows + (size_t)p.F * k * rho) * sizeof(float);
  return p;
}

// First float index at or before `start` whose address is 16-byte aligned (a batch may start anywhere in the resident records).
__device__ __forceinline__ int64_t aligned_start(const float* rec, int64_t start) {
  const int64_t off = (int64_t)((reinterpret_cast<uintptr_t>(rec) >> 2) & 3);
  return ((start + off) & ~(int64_t)3) - off;
}

// Copy the record floats [start, end) to lds[idx - aligned_start(start)] with aligned 16-byte loads, kStageUnroll per thread issued
// before the first LDS store (a workgroup keeps up to 32 KiB of loads in flight); a float4 reaching outside the records buffer
// [0, n_total) is read element by element.
constexpr int kStageUnroll = 8;
__device__ __forceinline__ void stage_range(const float* __restrict__ rec, int64_t n_total, int64_t start, int64_t end,
                                            float* lds) {
  const int64_t a0 = aligned_start(rec, start);
  const int nv = (int)((end - a0 + 3) >> 2);
  float4* dst = reinterpret_cast<float4*>(lds);
  for (int v0 = 0; v0 < nv; v0 += kStageUnroll * kFactorThreads) {
    float4 buf[kStageUnroll];
#pragma unroll
    for (int u = 0; u < kStageUnroll; ++u) {
      const int v = v0 + u * kFactorThreads + (int)threadIdx.x;
      const int64_t g = a0 + 4 * (int64_t)v;
      if (v < nv && g >= 0 && g + 4 <= n_total) {
        buf[u] = *reinterpret_cast<const float4*>(rec + g);
      } else {
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = v < nv && g + e >= 0 && g + e < n_total ? rec[g + e] : 0.0f;
        buf[u] = float4{t[0], t[1], t[2], t[3]};
      }
    }
#pragma unroll
    for (int u = 0; u < kStageUnroll; ++u) {
      const int v = v0 + u * kFactorThreads + (int)threadIdx.x;
      if (v < nv) dst[v] = buf[u];
    }
  }
}

__global__ __launch_bounds__(kFactorThreads) void metric_factor_kernel(const float* __restrict__ rec, int64_t B, int d_r, int rho,
                                                                        int k, int F, int rows, int nchunk,
                                                                        const float* __restrict__ g_tiled,
                                                                        float* __restrict__ q_tiled, float* __restrict__ e_tiled) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int64_t W = (int64_t)d_r * (1 + rho), n_total = B * W;
  const int groups = CVF_TILE / F;
  const int64_t tile = blockIdx.x / groups;
  const int lane0 = (int)(blockIdx.x % groups) * F;          // first lane of the group in its tile
  const int64_t f0 = tile * CVF_TILE + lane0;
  // padded frames (>= B) of the last tile use frame B-1's record
  const int64_t fs = f0 < B ? f0 : B - 1;
  const int64_t fe = f0 + F - 1 < B ? f0 + F - 1 : B - 1;
  const int stage_floats = nchunk == 1 ? (int)(F * W + 8) : rows * rho + 8;
  float* Ls = lds;
  float* Gs = Ls + stage_floats;                             // [f][j][row of the chunk]
  float* Ts = Gs + F * k * rows;                             // [f][j][c]
  const int64_t gbase = tile * k * (int64_t)d_r * CVF_TILE + lane0;   // g / q of (f, j, i): gbase + (j * d_r + i) * 64 + f

  auto chunk_start = [&](int i0) -> int64_t { return nchunk == 1 ? fs * W : fs * W + d_r + (int64_t)i0 * rho; };
  // LDS index of L[frame ff][i][c] while the chunk starting at row i0 is staged
  auto l_index = [&](int64_t ff, int i, int c, int i0) -> int {
    return (int)(ff * W + d_r + (int64_t)i * rho + c - aligned_start(rec, chunk_start(i0)));
  };
  auto stage = [&](int i0, int nr) {
    const int64_t s0 = chunk_start(i0);
    const int64_t s1 = nchunk == 1 ? (fe + 1) * W : s0 + (int64_t)nr * rho;
    stage_range(rec, n_total, s0, s1, Ls);
  };

  // pass 1: t
  for (int ch = 0; ch < nchunk; ++ch) {
    const int i0 = ch * rows, nr = d_r - i0 < rows ? d_r - i0 : rows;
    stage(i0, nr);
    for (int e = tid; e < F * k * nr; e += kFactorThreads) {   // g of the chunk's rows: F consecutive lanes of a tiled row
      const int f = e % F, ji = e / F, j = ji / nr, i = ji % nr;
      Gs[(f * k + j) * rows + i] = g_tiled[gbase + ((int64_t)j * d_r + i0 + i) * CVF_TILE + f];
    }
    __syncthreads();
    for (int wi = tid; wi < F * rho; wi += kFactorThreads) {
      const int f = wi / rho, c = wi % rho;
      const int64_t ff = f0 + f < B ? f0 + f : B - 1;
      const float* Lp = Ls + l_index(ff, i0, c, i0);
      const float* Gp = Gs + f * k * rows;
      float acc[CVF_MAX_NETS];
#pragma unroll
      for (int j = 0; j < CVF_MAX_NETS; ++j) acc[j] = 0.0f;
      for (int i = 0; i < nr; ++i) {
        const float l = Lp[i * rho];
#pragma unroll
        for (int j = 0; j < CVF_MAX_NETS; ++j)
          if (j < k) acc[j] = fmaf(l, Gp[j * rows + i], acc[j]);
      }
#pragma unroll
      for (int j = 0; j < CVF_MAX_NETS; ++j)
        if (j < k) Ts[(f * k + j) * rho + c] = ch == 0 ? acc[j] : Ts[(f * k + j) * rho + c] + acc[j];
    }
    __syncthreads();
  }
  // E
  for (int wi = tid; wi < F * k; wi += kFactorThreads) {
    const int f = wi / k, j = wi % k;
    const float* tp = Ts + (f * k + j) * rho;
    float E = 0.0f;
    for (int c = 0; c < rho; ++c) E = fmaf(tp[c], tp[c], E);
    e_tiled[(tile * k + j) * CVF_TILE + lane0 + f] = E;
  }
  // pass 2: q (the last chunk of pass 1 is still staged)
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int i0 = ch * rows, nr = d_r - i0 < rows ? d_r - i0 : rows;
    if (ch != nchunk - 1) {
      __syncthreads();
      stage(i0, nr);
      __syncthreads();
    }
    for (int wi = tid; wi < F * nr; wi += kFactorThreads) {   // f fastest: F consecutive lanes write one stretch of a tiled row
      const int f = wi % F, i = wi / F;
      const int64_t ff = f0 + f < B ? f0 + f : B - 1;
      const float* Lp = Ls + l_index(ff, i0 + i, 0, i0);
      const float* Tp = Ts + f * k * rho;
      float acc[CVF_MAX_NETS];
#pragma unroll
      for (int j = 0; j < CVF_MAX_NETS; ++j) acc[j] = 0.0f;
      // columns in an order rotated by the row: lanes of neighbouring rows read different banks when rho is even
      int c = i % rho;
      for (int n = 0; n < rho; ++n) {
        const float l = Lp[c];
#pragma unroll
        for (int j = 0; j < CVF_MAX_NETS; ++j)
          if (j < k) acc[j] = fmaf(l, Tp[j * rho + c], acc[j]);
        c = c + 1 == rho ? 0 : c + 1;
      }
#pragma unroll
      for (int j = 0; j < CVF_MAX_NETS; ++j)
        if (j < k) q_tiled[gbase + ((int64_t)j * d_r + i0 + i) * CVF_TILE + f] = acc[j];
    }
  }
}

// features of the records: the first d_r floats of every record (padded frames replicate frame B-1, never read past B)
__global__ __launch_bounds__(64) void k1_factor_kernel(int d_r, int64_t W, const float* __restrict__ rec, int64_t B,
                                                       float* __restrict__ feat_tiled, float* __restrict__ feat_rows) {
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x;
  int64_t frame = tile * CVF_TILE + lane;
  const bool valid = frame < B;
  if (!valid) frame = B - 1;
  const float* src = rec + frame * W;
  for (int j = 0; j < d_r; ++j) {
    const float v = src[j];
    if (feat_tiled) feat_tiled[(tile * d_r + j) * CVF_TILE + lane] = v;
    if (feat_rows && valid) feat_rows[frame * d_r + j] = v;
  }
}

int factor_shape(const cvf_pp_desc* pp, int* rho) {
  CVF_REQUIRE(pp->d_r >= 1 && pp->n_coord > pp->d_r && pp->n_coord % pp->d_r == 0,
              "CVF_PP_FACTORED: n_coord (%d) must be d_r * (1 + rho) with d_r = %d, rho >= 1", pp->n_coord, pp->d_r);
  *rho = pp->n_coord / pp->d_r - 1;
  CVF_REQUIRE((int64_t)pp->d_r * *rho <= 65536, "CVF_PP_FACTORED: d_r * rho = %lld > 65536 floats of factor per frame",
              (long long)pp->d_r * *rho);
  CVF_REQUIRE(*rho <= pp->d_r, "CVF_PP_FACTORED: rho = %d > d_r = %d (the metric is d_r x d_r: its factor needs at most d_r columns)",
              *rho, pp->d_r);
  return 0;
}

}  // namespace

int cvf_factor_feature_launch(const cvf_pp_desc* pp, const float* x, int64_t B, float* feat_tiled, float* feat_rows, hipStream_t s) {
  int rho = 0;
  if (int rc = factor_shape(pp, &rho)) return rc;
  hipLaunchKernelGGL(k1_factor_kernel, dim3((unsigned)cvf_ntiles(B)), dim3(64), 0, s, pp->d_r, (int64_t)pp->n_coord, x, B,
                     feat_tiled, feat_rows);
  return cvf_check_launch("k1_factor_kernel");
}

int cvf_metric_factor_launch(const cvf_pp_desc* pp, const float* x, int64_t B, int k, const float* g_tiled, float* q_tiled,
                             float* e_tiled, hipStream_t s) {
  int rho = 0;
  if (int rc = factor_shape(pp, &rho)) return rc;
  CVF_REQUIRE(x, "cvf_metric_apply: factored mode needs the records x");
  const FactorPlan p = factor_plan(pp->d_r, rho, k);
  const int64_t T = cvf_ntiles(B);
  if (p.lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)metric_factor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL(metric_factor_kernel, dim3((unsigned)(T * (CVF_TILE / p.F))), dim3(kFactorThreads), p.lds, s, x, B, pp->d_r,
                     rho, k, p.F, p.rows, p.nchunk, g_tiled, q_tiled, e_tiled);
  return cvf_check_launch("metric_factor_kernel");
}
