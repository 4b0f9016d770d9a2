// Shared by ef16_front.hip, ef16_front_rows.hip and ef16_back.hip (the 16-frames-per-wave step, split in translation units so that
// they compile side by side): constants of the unit decomposition, the front kernel's LDS layout, the net shapes covered and their dispatch.
#pragma once
#include "cvf_metric.hpp"
#include "ef_frag.hpp"
#include <stdlib.h>
#include <type_traits>


namespace {

constexpr int kU = 16;       // frames per unit
constexpr int kImgP = 76;    // pitch of the [frame][feature] images: = 12 (mod 32), so the four-lanes-per-frame reads (address
                             // 76 f + 3 p + c) and the matrix cores' 16-byte row writes (76 col + 4 q) touch every bank once
constexpr int kAuxP = 21;    // pitch of the per-frame alignment record: R (9), centroid hi (3), K^-1 (6), centroid lo (3)
constexpr int kMaxRows16 = 16384;   // units whose rows of batch sums one finishing launch adds (above: cvf_ef_stats)
template <int NH>
__host__ __device__ constexpr int kHand() { return 2 * NH; }   // vectors of the front -> back hand-off per (tile, net)

__device__ __forceinline__ float quad_sumf16(float v) {
  v += dpp_movf<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v += dpp_movf<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  return v;
}
__device__ __forceinline__ double quad_sumd16(double v) {
  v += dpp_movd<0xB1, 0xf>(v);
  v += dpp_movd<0x4E, 0xf>(v);
  return v;
}

// ------------------------------------------------------------------------------------------------------------------
// Strips of a weight gradient too thin for a matrix tile (the backward kernel's 1 x (H + 1) last layer; a last column tile
// of the first layer with <= 4 useful columns).  A wave holds its 16 frames' hidden vectors in the acc layout (lane = (frame
// `col`, row group q), register j = 4 rt + r = row 4 j + q), so a product summed over the wave's frames is a sum over the 16
// lanes of a DPP row: a fixed tree, no LDS.  The four waves' partial sums then meet in a small LDS area behind a barrier the
// kernel has anyway and are added in wave order - the same order on every run.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float row_sumf16(float v) {   // every lane of the row gets the sum
  v = quad_sumf16(v);
  v += dpp_movf<0x141, 0xf>(v);   // row_half_mirror: the other quad of the lane's eight
  v += dpp_movf<0x140, 0xf>(v);   // row_mirror: the other eight
  return v;
}
// val(rt, r): the lane's value of row 4 (4 rt + r) + q for its frame.  Each of the NG rows is summed over the wave's frames, one
// after the other (one live partial at a time); lane `col == j` keeps the sum of ITS row 4 j + q, so a strip leaves the wave in
// one LDS write per column
template <int H, class F>
__device__ __forceinline__ float strip_rows(F&& val, int col) {
  float pick = 0.0f;
#pragma unroll
  for (int j = 0; j < Hid<H>::NG; ++j) {
    const float s = row_sumf16(val(j >> 2, j & 3));
    pick = col == j ? s : pick;
  }
  return pick;
}
// the four waves' partials of one value (P[wave * stride]), in wave order
__device__ __forceinline__ float strip_total(const float* P, int stride) {
  return ((P[0] + P[stride]) + P[2 * stride]) + P[3 * stride];
}

// ------------------------------------------------------------------------------------------------------------------
// Tiles with 1..4 useful rows (rows 16..19 at H = 20) as 4x4x1 blocks (mfma1): the wave's sixteen blocks are (frame set
// q = lane >> 4) x (column group (lane & 15) >> 2), so register r of lane (c, q) is the partial of entry (row r, column c)
// over frame set q and the four q (lanes l, l ^ 16, l ^ 32, l ^ 48) remain to be added.  Two half-wave swaps and one row
// swap do it for the four registers at once, in the fixed order (q0 + q2) + (q1 + q3); the lanes of DPP row q return the
// total of register q - every lane has one entry to store.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rows_sum_scatter(const f32x4& x) {
  auto swap_add = [](auto swapped) {
    const unsigned a = swapped[0], b = swapped[1];   // (by value, for the same reason)
    return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
  };
  const float x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];   // (by value: see emit_tile on bit casts of vector elements)
  // lanes 0..31: the first operand's two halves added, lanes 32..63: the second's
  const float s02 = swap_add(__builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x0), __builtin_bit_cast(unsigned, x2), false, false));
  const float s13 = swap_add(__builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x1), __builtin_bit_cast(unsigned, x3), false, false));
  // rows 0, 2: s02's row pair added, rows 1, 3: s13's
  return swap_add(__builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, s02), __builtin_bit_cast(unsigned, s13), false, false));
}

struct Front16Lds {   // offsets in floats
  int ref, a, aux, w, rs, y, e, feat, g, total;
};
__host__ __device__ inline Front16Lds front16_lds(int nc, int nal, int k) {
  Front16Lds L;
  const int stride = x_tile_stride(nc);
  L.ref = kU * stride;
  L.a = L.ref + 3 * nal;
  L.aux = (L.a + nc + 3) & ~3;
  L.w = L.aux + ((kU * kAuxP + 3) & ~3);
  L.rs = L.w + kU;      // sum of the (centred) reference over the align atoms: 3 floats (+ 1 pad)
  L.y = L.rs + 4;
  L.e = L.y + k * kU;
  L.feat = L.e + k * kU;              // 16-byte aligned: every term above is a multiple of 4 floats
  L.g = L.feat + kU * kImgP;
  L.total = L.g + k * kU * kImgP;
  return L;
}

// ------------------------------------------------------------------------------------------------------------------
// front
// ------------------------------------------------------------------------------------------------------------------
// NIT = ceil(N / 4) exactly (atoms per lane in the four-lanes-per-frame passes): every iteration but the last is complete, so
// only the last one carries the masks of the ragged end.  ALLAL: every feature atom is an align atom (n_align == n_rec).
bool ef16_shape(const cvf_mlp_desc* m, int* H, int* NH) {
  if (m->n_layers < 2 || m->n_layers > 4 || m->dims[m->n_layers] != 1) return false;
  *H = m->dims[1];
  *NH = m->n_layers - 1;
  for (int l = 1; l < m->n_layers; ++l)
    if (m->dims[l] != *H) return false;
  for (int l = 0; l < m->n_layers; ++l)
    if (m->act[l] != (l + 1 < m->n_layers ? 1 : 0)) return false;
  return true;
}

template <class F>
bool ef16_dispatch(int H, int NH, F&& f) {
#define EF_CASE(H_, NH_)                                                        \
  if (H == H_ && NH == NH_) {                                                   \
    f(std::integral_constant<int, H_>{}, std::integral_constant<int, NH_>{});   \
    return true;                                                                \
  }
#ifdef CVF_DEV_SHAPES   // developer builds (tools/*.hip probes, -S listings): the config-3 instance only - seconds instead of minutes
  EF_CASE(20, 3)
#else
  EF_CASE(8, 1) EF_CASE(8, 2) EF_CASE(8, 3)
  EF_CASE(12, 1) EF_CASE(12, 2) EF_CASE(12, 3)
  EF_CASE(16, 1) EF_CASE(16, 2) EF_CASE(16, 3)
  EF_CASE(20, 1) EF_CASE(20, 2) EF_CASE(20, 3)
  EF_CASE(24, 2) EF_CASE(24, 3)
  EF_CASE(32, 2) EF_CASE(32, 3)
#endif
#undef EF_CASE
  return false;
}

}  // namespace
