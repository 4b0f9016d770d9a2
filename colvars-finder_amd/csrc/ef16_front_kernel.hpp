// The front kernel of the 16-frames-per-wave generator / transfer-operator step, shared by ef16_front.hip (the instances that solve
// the alignment of their 16 frames themselves) and ef16_front_rows.hip (the twins that start from alignment rows a previous
// visit of the same resident batch left in global memory): two translation units so that they compile side by side.
#pragma once
#include "ef16_common.hpp"
#include "cvf_p2p.hpp"

namespace {
// Alignment rows of a batch (cvf_ef16_align_rows): per unit the 16 records of kAuxP floats exactly as ef16_align_unit leaves
// them in LDS (336 floats = 84 16-byte pieces), behind the last unit the three floats of rsL (+ 1 pad).
constexpr int kRowsUnit = kU * kAuxP;
static_assert(kRowsUnit % 4 == 0, "a unit's alignment rows are staged as 16-byte pieces");

// One wave, the 16 frames of a unit staged at xt (pitch `stride`): centroid, covariance (this lane's quarter of the align
// atoms, fp64) and the rotation of frame lane / 4 -> its record in auxL; the sum of the reference -> rsL.  The front kernel's
// wave 0 and the stand-alone kernel that fills the alignment rows run THIS code, so that the rows hold the bits the front
// kernel would have computed.
template <bool kTransfer>
__device__ __forceinline__ void ef16_align_unit(const float* my, const float* refL, const int nal, const int lane, float* auxL,
                                                float* rsL) {
  const int f = lane >> 2, p = lane & 3;
  double acc[15];
#pragma unroll
  for (int i = 0; i < 15; ++i) acc[i] = 0.0;
#pragma unroll 2
  for (int b = p; b < nal; b += 4) {
    const double x0 = (double)my[3 * b], x1 = (double)my[3 * b + 1], x2 = (double)my[3 * b + 2];
    const double r0 = (double)refL[3 * b], r1 = (double)refL[3 * b + 1], r2 = (double)refL[3 * b + 2];
    acc[0] += x0; acc[1] += x1; acc[2] += x2;
    acc[3] = fma(x0, r0, acc[3]); acc[4] = fma(x0, r1, acc[4]); acc[5] = fma(x0, r2, acc[5]);
    acc[6] = fma(x1, r0, acc[6]); acc[7] = fma(x1, r1, acc[7]); acc[8] = fma(x1, r2, acc[8]);
    acc[9] = fma(x2, r0, acc[9]); acc[10] = fma(x2, r1, acc[10]); acc[11] = fma(x2, r2, acc[11]);
    acc[12] += r0; acc[13] += r1; acc[14] += r2;
  }
#pragma unroll
  for (int i = 0; i < 15; ++i) acc[i] = quad_sumd16(acc[i]);
  const double inv = fast_rcp((double)nal);
  const double cd[3] = {acc[0] * inv, acc[1] * inv, acc[2] * inv};
  double Hm[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Hm[i][j] = fma(-cd[i], acc[12 + j], acc[3 + 3 * i + j]);
  KabschOut ko;
  if constexpr (kTransfer) {   // transfer-operator mode: no derivative through the alignment, the rotation alone
    kabsch_from_H<false>(Hm, ko);
#pragma unroll
    for (int i = 0; i < 6; ++i) ko.Kinv[i] = 0.0f;
  } else {
    kabsch_from_H<true>(Hm, ko);
  }
  const Centre c = centre_of(cd);
  const float av[kAuxP] = {ko.R[0], ko.R[1], ko.R[2], ko.R[3], ko.R[4], ko.R[5], ko.R[6], ko.R[7], ko.R[8], c.hi[0], c.hi[1], c.hi[2],
                           ko.Kinv[0], ko.Kinv[1], ko.Kinv[2], ko.Kinv[3], ko.Kinv[4], ko.Kinv[5], c.lo[0], c.lo[1], c.lo[2]};
#pragma unroll
  for (int i = 0; i < kAuxP; ++i)
    if ((i & 3) == p) auxL[f * kAuxP + i] = av[i];   // the four lanes of a frame hold the same record: each writes a quarter
  if (lane < 3) rsL[lane] = (float)(lane == 0 ? acc[12] : lane == 1 ? acc[13] : acc[14]);
}

// The position features of atom `at` of a frame staged at `my`: its aligned position, from the rotation and the centroid
// (hi AND lo part) of the frame's record.  The solving front kernel (into its LDS image and from there into the feature tile) and
// the kernel that fills a resident batch's tile once (ef16_front_rows.hip) evaluate THIS expression: the same bits.
__device__ __forceinline__ V3 ef16_feature(const float* my, const int at, const Centre& c, const float* R) {
  return row_times(centred(my, at, c), R);
}

// Iteration `it` of a four-lanes-per-frame pass: the lane's atom pb + 4 it (pb = lane & 3, made opaque once per pass by the caller).
// Three times its index is ONE register per pass (3 pb) and a constant, so the rows of an array at the lane's atoms are one
// address and immediate offsets of 48 bytes.  Only the last iteration can run past the last atom: there, and only there, the
// index is clamped - the lane works on a duplicate of atom N - 1 with lv = 0.
struct AtomSlot {
  int ac, i3;   // the atom, and three times it
  float lv;     // 1 / 0 past the last atom
};
template <int NIT>
__device__ __forceinline__ AtomSlot atom_slot(const int pb, const int it, const int N) {
  // (the iteration's LDS reads stay behind it: all of a pass's reads requested at once cost up to nine registers.  Nothing in the
  //  language promises this order - the compiler's instruction scheduler does not move memory operations across an `asm volatile`;
  //  results do not depend on it, only the register counts, which tests/test_ef16_front_lean_host.py holds against the parent's)
  asm volatile("");
  const int at = pb + 4 * it;
  if (it < NIT - 1) return AtomSlot{at, 3 * pb + 12 * it, 1.0f};
  const int ac = at >= N ? N - 1 : at;
  return AtomSlot{ac, 3 * ac, at >= N ? 0.0f : 1.0f};
}

// ROWS: the instance starts from what a previous visit of its resident batch left in global memory (cvf_ef16_align_rows_tile)
// instead of deriving it again - the alignment rows (`rows`, see kRowsUnit) and the feature tile (`feat_tiled`, here an INPUT):
//   * wave 0's covariance + solve and the barrier behind it, the feature phase and its barrier, and the tile's store at the
//     end are compiled out;
//   * layer 0's B operand comes from the tile, so nothing in front of the d chain reads LDS: the head of the pass requests
//     the staged pieces (records, coordinates, tables, weight) FIRST and the operand and the first layer's fragments behind
//     them, all before anything is waited for - vector memory returns in issue order, so the LDS stores of the staged
//     pieces wait for those loads alone - and the block's one barrier for the staged data stands where it is first read
//     by another wave, in front of CVF_STAMP(26).
//   * with an isotropic metric (launch bit 9) the head requests and stages no coordinates: the passes read the features, which
//     the waves copy from layer 0's operand into the LDS image beside layer 0.
// Everything else is the code of the solving instance on the same records and features.  Generator instances only.
template <int H, int NH, int NIT, bool ALLAL, bool ROWS = false>
__global__ __launch_bounds__(1024, 4) void ef16_front_kernel(cvf_mlp_desc mlp, const float* __restrict__ theta,
                                                             const float* __restrict__ packed, cvf_pp_desc pp,
                                                             const float* __restrict__ x, int64_t B,
                                                             const float* __restrict__ a, const float* __restrict__ w,
                                                             float* __restrict__ feat_tiled, float* __restrict__ y_tiled,
                                                             float* __restrict__ saved, float* __restrict__ q_tiled,
                                                             float* __restrict__ e_tiled, double* __restrict__ partial, int launch,
                                                             const float* __restrict__ x_lag, int64_t units_x,
                                                             const float* __restrict__ w_lag, const float* __restrict__ rows) {
  static_assert(!ROWS || NIT > 0, "alignment rows: generator instances only");
  constexpr int RT = Hid<H>::RT, NG = Hid<H>::NG, SMAX = 18, CTMAX = 5;
  // NIT == 0: the TRANSFER-OPERATOR instance (cvf_ef16_front_transfer) - the block leaves after y and the hand-off of the hidden
  // activations, and everything behind that point is compiled out: no g images in LDS (11 KB per block instead of 26) and fewer
  // registers, so that the 2 x units of the frames and their lagged partners are resident in ONE round (the generator instance
  // held them in two: 5 blocks per CU by registers and LDS)
  constexpr bool kTransfer = NIT == 0;
  extern __shared__ __attribute__((aligned(16))) float lds_all[];
  // `launch` = units per workgroup | paired << 8 | isotropic << 9.  Several units per workgroup (a developer switch, off by default - measured
  // slower, see ef16_units_per_wg): a workgroup of upb k waves takes upb consecutive units, each on its own k waves and its own
  // copy of the LDS layout, exactly as upb workgroups of one unit would - the units only share the workgroup's barriers.
  const int upb = launch & 0xff;
  const int k = mlp.n_nets, D = mlp.dims[0];
  // (the wave number through an SGPR: derived from threadIdx.x alone the compiler treats it - and every address formed
  //  with it, i.e. all of this net's weights and images - as lane-varying, in VGPR pairs)
  const int wave_b = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int usub = upb > 1 ? wave_b / k : 0;                 // this wave's unit within the workgroup (wave-uniform)
  const int wave = wave_b - usub * k;
  const int tid = (int)threadIdx.x - usub * (64 * k), lane_in = tid & 63;
  const int nthreads = upb > 1 ? 64 * k : (int)blockDim.x, nw = nthreads >> 6;
  const int net = wave;
  const int64_t ublock = (int64_t)blockIdx.x * upb + usub;   // what blockIdx.x is with one unit per workgroup
  // transfer-operator mode (x_lag != NULL), two launch forms:
  //   PAIRED (launch bit 8): the block runs unit u of the frames and then, with the same waves, unit u of their lagged
  //     partners, so that y and y' of the same 16 frame indices meet in one
  //     block and wave 0 can form the unit's row of the TIME-LAGGED batch sums (sum w (y' - y)^2 pairs a frame with its
  //     partner); cvf_ef16_finish then adds the rows as in generator mode (was: cvf_ef_stats, two launches, 15 us).  The
  //     launch is one round of units_x blocks doing two units each instead of two rounds of 2 units_x blocks.
  //   unpaired: the units of x, then the units of the lagged frames, one per block.
  // In both the lagged frames' tiles follow the tiles of x in every tiled output, and a pass stops after y and the hand-off.
  const bool paired = kTransfer && x_lag != nullptr && ((launch >> 8) & 1) != 0;   // (uniform)
  // ISOTROPIC metric (launch bit 9, generator instances; wave-uniform, in an SGPR): the caller vouches that the three coefficients
  // of every record atom are equal, a[3b] == a[3b+1] == a[3b+2].  Then R a_b R^T = a_b I and q = J A J^T g is formed in the ALIGNED
  // frame, from the features alone (see the passes behind CVF_STAMP(26)): no rotation, no centroid and no coordinates are read.
  const bool iso = !kTransfer && ((launch >> 9) & 1) != 0;
  const int nc = pp.n_coord, nal = pp.n_align, N = pp.n_rec;
  const int stride = x_tile_stride(nc);
  const Front16Lds Lo = front16_lds(nc, nal, k);   // (the transfer instance is launched with Lo.g + 16 floats per unit: no g images)
  float* lds = lds_all + usub * (kTransfer ? Lo.g + 16 : Lo.total);
  // units past the last one (the last workgroup of a launch whose unit count is not a multiple of upb) repeat the last unit: the
  // same values into the same places, and every wave meets the workgroup's barriers
  const int64_t n_ublock = (kTransfer && !paired) ? 2 * units_x : units_x;
  const int64_t ub = ublock < n_ublock ? ublock : n_ublock - 1;
  const float* const x_first = x;
  const float* const w_first = w;
  // one unit from its coordinates to y (transfer instance) / to the unit's row of batch sums (generator instances).  A lambda so that
  // a paired transfer block can run it twice as STRAIGHT-LINE code: written as a loop, the by-value descriptors stay in scalar
  // registers across the iterations, the scalar file overflows into vector lanes and the kernel spills (128 + 37 against 109)
  auto run_pass = [&](const int pass) __attribute__((always_inline)) {
  const int lane = lane_in;
  // ---- this net's weights (requested in every pass, behind the coordinates)
  const PackLayout L = pack_layout(H, NH, D);
  const URows pk = urows(packed + (int64_t)net * L.per_net, L.per_net, lane);   // this net's fragments (see URows)
  const int S = (D + 3) >> 2, CT = (D + 15) >> 4;
  float a0[SMAX][RT];
  float bias[NH][RT][4];
  const int q_ = lane >> 4;
  auto request_a0 = [&]() {
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      const int se = s < S ? s : S - 1;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) a0[s][rt] = pk.ld(L.f0() + (se * RT + rt) * 64);   // (k-steps past S are skipped below)
    }
  };
  auto request_bias0 = [&]() { load_hid_const_u<H>(urows(theta + mlp.b_off[net][0], H, q_), bias[0]); };
  auto request_layer0 = [&]() {
    request_a0();
    request_bias0();
  };
  const bool lagged = x_lag != nullptr && (paired ? pass == 1 : ub >= units_x);   // (wave-uniform)
  const int64_t unit = (lagged && !paired) ? ub - units_x : ub;   // unit within its frame set
  const int64_t tile = (unit >> 2) + (lagged ? (units_x >> 2) : 0);
  const int sub = (int)(unit & 3);
  x = lagged ? x_lag : x_first;
  w = lagged ? w_lag : w_first;
  float* xt = lds;
  float* refL = lds + Lo.ref;
  float* aL = lds + Lo.a;
  float* auxL = lds + Lo.aux;
  float* wL = (kTransfer && pass == 1) ? lds + Lo.g : lds + Lo.w;   // (second pass: the partners' weights behind the layout)
  float* rsL = lds + Lo.rs;
  float* yL = lds + Lo.y + (kTransfer ? pass * (k * kU) : 0);   // (second pass: y' goes where the generator instance keeps E)
  float* eL = lds + Lo.e;
  float* featI = lds + Lo.feat;
  float* gI = lds + Lo.g + net * (kU * kImgP);
  const int f = lane >> 2, p = lane & 3;       // four-lanes-per-frame phases: frame f of the unit, part p
  const int col = lane & 15, q = lane >> 4;    // matrix-core phases: frame col of the unit, k-slot / row group q

  CVF_STAMP(20);
  float bf0[SMAX];   // ROWS: layer 0's B operand
  if constexpr (ROWS) {
    // ---- ROWS: EVERYTHING the pass reads from global memory in front of its first matrix instruction is requested here, before
    //      anything is waited for - ONE round trip at the head of the block (the staging loops below, kept for the solving twins,
    //      wait per iteration: coordinates, second piece, tables, weights = four in a row).  Clamped indices and selected
    //      addresses, no branch around a load; at this launch's sizes a thread holds at most two 16-byte pieces of the records,
    //      two of the coordinates and one table entry, larger layers finish in the counted loops behind the stores.
    //      The staged data first, then layer 0's operand (feature 4 s + q of frame col, from the batch's tile) and the first
    //      layer's fragments: vector memory returns in issue order, so the LDS stores do not wait for the fragments.
    constexpr int n4r = kRowsUnit / 4;
    const float4* rsrc = reinterpret_cast<const float4*>(rows + unit * (int64_t)kRowsUnit);
    const float4 row_a = rsrc[tid < n4r ? tid : n4r - 1];
    const float4 row_b = rsrc[tid + nthreads < n4r ? tid + nthreads : n4r - 1];
    const float rs_in = rows[units_x * (int64_t)kRowsUnit + (tid < 3 ? tid : 2)];
    // the unit as it lies in memory (see the solving twins' stager below); otherwise the general stager, behind the stores
    const bool plain = stride == nc && (unit + 1) * kU <= B && (reinterpret_cast<uintptr_t>(x) & 15) == 0;   // (uniform)
    const int n4 = (kU * nc) >> 2;
    const float4* xsrc = reinterpret_cast<const float4*>(x + unit * (int64_t)(kU * nc));
    const float4* xs = plain ? xsrc : rsrc;   // (not plain: any readable piece, dropped)
    const int nx = plain ? n4 : 1;
    float4 cx0 = {0.0f, 0.0f, 0.0f, 0.0f}, cx1 = cx0;
    if (!iso) {   // (uniform; isotropic: the passes read the features, and the head requests no coordinates at all)
      cx0 = xs[tid < nx ? tid : nx - 1];
      cx1 = xs[tid + nthreads < nx ? tid + nthreads : nx - 1];
    }
    const int nt = 3 * nal + nc, jt = tid < nt ? tid : nt - 1;   // refL | aL
    const bool in_a = jt >= 3 * nal && a != nullptr;
    const float tv_ld = *(in_a ? a + (jt - 3 * nal) : pp.ref_c + (jt < 3 * nal ? jt : 0));
    const float tv = (jt < 3 * nal || in_a) ? tv_ld : 0.0f;
    const int64_t frame = unit * kU + (tid < kU ? tid : kU - 1);
    const float wv_ld = *(w != nullptr ? w + (frame < B ? frame : B - 1) : rows);
    const float wv = (w != nullptr && frame < B) ? wv_ld : 0.0f;   // frames past the batch replicate the last one with weight 0
    {
      const float* ft = feat_tiled + tile * (int64_t)D * CVF_TILE + kU * sub + col;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        const int kf = 4 * (s < S ? s : S - 1) + q;
        bf0[s] = ft[(kf < D ? kf : D - 1) * CVF_TILE];   // rows past D meet zero weights
      }
    }
    request_a0();
    // ---- the stores of what was staged (no barrier behind them: this wave's forward and d chains read no LDS but its own
    //      image - the block's barrier stands in front of CVF_STAMP(26))
    float4* adst = reinterpret_cast<float4*>(auxL);
    if (tid < n4r) adst[tid] = row_a;
    if (tid + nthreads < n4r) adst[tid + nthreads] = row_b;
    if (tid < 3) rsL[tid] = rs_in;
    if (iso) {
      // (nothing: the unit's features go from bf0 into the LDS image beside layer 0, below)
    } else if (plain) {
      float4* dst = reinterpret_cast<float4*>(xt);
      if (tid < n4) dst[tid] = cx0;
      if (tid + nthreads < n4) dst[tid + nthreads] = cx1;
      for (int v = tid + 2 * nthreads; v < n4; v += nthreads) dst[v] = xsrc[v];
    } else {
      load_x_tile<3, true>(x, B, nc, unit, xt, tid, nthreads, kU);   // (behind the requests above: see kPlainRagged)
    }
    if (tid < nt) refL[tid] = tv;
    for (int j = tid + nthreads; j < nt; j += nthreads) refL[j] = j < 3 * nal ? pp.ref_c[j] : (a != nullptr ? a[j - 3 * nal] : 0.0f);
    if (tid < kU) wL[tid] = wv;
    request_bias0();   // (behind the stores: its registers and the staged pieces' are not live together)
  } else {
  // ---- stage the unit's coordinates (16 x nc floats, one contiguous run), the tables and the weights
  if (stride == nc && (unit + 1) * kU <= B && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    // the unit as it lies in memory (3N = 2 mod 4: plain copy, 16 x 3N floats = a whole number of 16-byte pieces; at most two
    // per thread here) - the general stager's index arithmetic (integer divisions by 3N) was a tenth of this kernel's
    // vector instructions
    const float4* src = reinterpret_cast<const float4*>(x + unit * (int64_t)(kU * nc));
    float4* dst = reinterpret_cast<float4*>(xt);
    const int n4 = (kU * nc) >> 2;
    for (int v = tid; v < n4; v += nthreads) dst[v] = src[v];
  } else {
    load_x_tile<6>(x, B, nc, unit, xt, tid, nthreads, kU);
  }
  for (int j = tid; j < 3 * nal + nc; j += nthreads) refL[j] = j < 3 * nal ? pp.ref_c[j] : (a != nullptr ? a[j - 3 * nal] : 0.0f);   // refL | aL
  if (tid < kU) {
    const int64_t frame = unit * kU + tid;
    wL[tid] = (w != nullptr && frame < B) ? w[frame] : 0.0f;      // frames past the batch replicate the last one with weight 0
  }
  // ---- the first layer's weights are requested here, behind the coordinates and the tables (vector memory returns in issue
  //      order: in front of them they delayed the staging by 7 k cycles): their round trip runs beside the barrier and the
  //      alignment (requested after the alignment, layer 0 began with a wait of ~2 k cycles per wave)
  // (wave 0 asks after its alignment: the solve's fp64 state and these 36 + 8 registers do not fit 128 together, and
  //  a spilled fragment is stored behind a wait for ALL outstanding loads)
  if (wave != 0) request_layer0();   // (every pass: kept across wave 0's solve of the second pass they would spill)
  __syncthreads();
  }
  const float* my = xt + f * stride;
  CVF_STAMP(21);

  if constexpr (!ROWS) {
    // ---- wave 0: centroid, covariance (this lane's quarter of the align atoms, fp64) and the rotation of the 16 frames
    if (wave == 0) {
      ef16_align_unit<kTransfer>(my, refL, nal, lane, auxL, rsL);
      request_layer0();
    }
    lds_barrier();
  }
  CVF_STAMP(22);

  // ---- aligned positions = features: the block's waves split the atoms (lane p of wave v: atoms p + 4 v + 4 nw i)
  //      (ROWS: they are in the batch's tile)
  if constexpr (!ROWS) {
    float R[9];
    const float* ar = auxL + f * kAuxP;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ar[i];
    Centre c;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      c.hi[i] = ar[9 + i];
      c.lo[i] = ar[18 + i];
    }
    // (LDS only here: the tiled copy for the backward kernel leaves at the end of the kernel - vector-memory operations
    //  return in issue order, so global stores at this point would sit in front of every weight fragment requested above)
    for (int at = p + 4 * wave; at < N; at += 4 * nw) {
      const V3 al = ef16_feature(my, at, c, R);
      float* fi = featI + f * kImgP + 3 * at;
      fi[0] = al.x;
      fi[1] = al.y;
      fi[2] = al.z;
    }
    // (the rest of the frame's row up to the end of the last k-step, at most three floats: layer 0 reads rows 4 s + q without a
    //  clamp, and a row past D meets a zero weight AND a zero this block wrote)
    if (wave == 0 && D + p < 4 * S) featI[f * kImgP + D + p] = 0.0f;
    lds_barrier();
  }
  CVF_STAMP(23);

  // ---- forward chain of this wave's net on the matrix cores: h_l = tanh(W_l h_{l-1} + b_l), 16 frames = the MFMA's N
  Vec<H, 1> h[NH];
  auto set_bias = [&](Vec<H, 1>& X, const float (&b)[RT][4]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) X.v[rt][0][r] = b[rt][r];
  };
  set_bias(h[0], bias[0]);
  {
    float bf[SMAX];
    float* fr = featI + col * kImgP;
    static_assert(4 * (SMAX - 1) + 3 < kImgP, "the ROWS twins' feature copy stays inside a frame's row of the image");
    // ROWS + isotropic: the passes read the unit's features from the LDS image [frame][feature] the solving twins build in their
    // feature phase.  Every wave of the block holds the unit's features in bf0 (the matrix layout: feature 4 s + q of frame
    // col), so the waves split the k-steps - wave v takes s = v mod P, P the largest power of two <= the block's waves (a bit
    // per k-step in an SGPR: no division) - and write them beside layer 0's matrix instructions, in front of the block's barrier
    // at CVF_STAMP(26).  A row past D (4 s + q <= 71) lands in the padding of the frame's row (kImgP = 76), which nobody reads.
    unsigned own = 0u;
    if constexpr (ROWS) {
      if (iso) {
        const int P = nw >= 8 ? 8 : nw >= 4 ? 4 : nw >= 2 ? 2 : 1;
        own = (P == 8 ? 0x10101u : P == 4 ? 0x11111u : P == 2 ? 0x15555u : 0x3ffffu) << (wave & (P - 1));
      }
    }
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if constexpr (ROWS) bf[s] = bf0[s];
      else bf[s] = fr[q + 4 * s];   // (one address and immediate offsets; rows past D: zeros meet zero weights; steps past S: inside the frame's row, unused)
    }
    HFrag<H> hf[NH > 1 ? NH - 1 : 1];
#pragma unroll
    for (int l = 1; l < NH; ++l) {
      load_hfrag_u<H>(hf[l - 1], pk, L.fh(l));
      load_hid_const_u<H>(urows(theta + mlp.b_off[net][l], H, q), bias[l]);
    }
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < S) {   // wave-uniform
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) h[0].v[rt][0] = mfma4(a0[s][rt], bf[s], h[0].v[rt][0]);
        if constexpr (ROWS) {
          if ((own >> s) & 1u) fr[q + 4 * s] = bf[s];   // (wave-uniform; one address register and an immediate offset)
        }
      }
    }
    CVF_STAMP(24);
    tanh_inplace<H, 1>(h[0]);
#pragma unroll
    for (int l = 1; l < NH; ++l) {
      set_bias(h[l], bias[l]);
      hidden_mul<H, 1>(h[l], hf[l - 1], h[l - 1]);
      tanh_inplace<H, 1>(h[l]);
    }
  }
  float wl[RT][4];
  load_hid_const_u<H>(urows(theta + mlp.w_off[net][NH], H, q), wl);
  const float bL = theta[mlp.b_off[net][NH]];
  HFrag<H> tf[NH > 1 ? NH - 1 : 1];
#pragma unroll
  for (int l = 1; l < NH; ++l) load_hfrag_u<H>(tf[l - 1], pk, L.th(l));

  // hand-off to the backward kernel, per (tile, net): 2 NH vectors in the register layout both kernels use, as
  // [vector][group g][unit of the tile][lane] (every (vector, g, unit) one coalesced 256-byte row):
  //   h_1..h_NH | e_1..e_{NH-1} (e_l = W_{l+1}^T d_{l+1}: the d chain) | s = W_1 q (the tangent chain's first product)
  // (stored after g below: vector-memory operations return in issue order, and the fragment loads of the d chain and of g -
  //  which the compiler places just in time - must not queue behind 25 stores)
  const URows sv = urows(saved + (tile * k + net) * (int64_t)(kHand<NH>() * NG * 256) + sub * 64, kHand<NH>() * NG * 256 - sub * 64, lane);
  {
    float part = 0.0f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) part = fmaf(wl[rt][r], h[NH - 1].v[rt][0][r], part);
    const float yv = sum_over_q(part) + bL;
    // (all four q groups hold the same value and store it to the same place: no lane-divergent branch around a store,
    //  behind which the compiler could no longer count the outstanding memory operations and would drain them all)
    yL[net * kU + col] = yv;
    urows(y_tiled + (tile * k + net) * CVF_TILE + kU * sub, kU, col).st(0, yv);   // (the unit's 16 values of this net: a uniform base and the lane's column)
  }
  CVF_STAMP(25);
  if constexpr (kTransfer) {   // transfer-operator mode: y, h_1..h_NH and the feature tile are all the backward pass needs
#pragma unroll
    for (int l = 0; l < NH; ++l)
#pragma unroll
      for (int g = 0; g < NG; ++g) sv.st((l * NG + g) * 256, h[l].v[g >> 2][0][g & 3]);
    float* ft = feat_tiled + tile * (int64_t)D * CVF_TILE + kU * sub + f;
    const float* fi = featI + f * kImgP;
#pragma unroll 1
    for (int j = p + 4 * wave; j < D; j += 4 * nw) ft[j * CVF_TILE] = fi[j];
    return;
  } else {

  // ---- d chain and g = W_1^T d_1 -> this wave's image [frame][feature]
  {
    // (requested behind the hand-off stores of h - vector-memory operations return in issue order - but the d chain below
    //  runs on fragments requested before them and covers that)
    float t0[CTMAX][NG];
#pragma unroll
    for (int rt = 0; rt < CTMAX; ++rt)
#pragma unroll
      for (int s = 0; s < NG; ++s) t0[rt][s] = pk.ld(L.t0() + ((rt < CT ? rt : CT - 1) * NG + s) * 64);
    Vec<H, 1> d;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float hv = h[NH - 1].v[rt][0][r];
        d.v[rt][0][r] = wl[rt][r] * (1.0f - hv * hv);
      }
    Vec<H, 1> ev[NH > 1 ? NH - 1 : 1];
#pragma unroll
    for (int l = NH - 1; l >= 1; --l) {
      init_bias<H, 1>(ev[l - 1], nullptr, q);
      hidden_mul<H, 1>(ev[l - 1], tf[l - 1], d);
      tangent_of<H, 1>(d, h[l - 1], ev[l - 1]);
    }
#pragma unroll
    for (int rt = 0; rt < CTMAX; ++rt) {
      if (rt < CT) {   // wave-uniform
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < NG; ++s) acc = mfma4(t0[rt][s], d.v[s >> 2][0][s & 3], acc);
        // rows 16 rt + 4 q .. + 3 of column col: four consecutive features of one frame = one 16-byte write
        if (16 * rt + 4 * q < D) *reinterpret_cast<float4*>(gI + col * kImgP + 16 * rt + 4 * q) = float4{acc[0], acc[1], acc[2], acc[3]};
      }
    }
    // the hand-off rows h_1..h_NH and e_1..e_{NH-1}
#pragma unroll
    for (int l = 0; l < NH; ++l)
#pragma unroll
      for (int g = 0; g < NG; ++g) sv.st((l * NG + g) * 256, h[l].v[g >> 2][0][g & 3]);
#pragma unroll
    for (int l = 1; l < NH; ++l)
#pragma unroll
      for (int g = 0; g < NG; ++g) sv.st(((NH + l - 1) * NG + g) * 256, ev[l - 1].v[g >> 2][0][g & 3]);
  }
  // ROWS: the block's barrier for the staged coordinates, records and tables - from here on a wave reads what others staged
  // (LDS alone: every wave stored what it staged behind its own wait for the loads; the hand-off stores above stay in flight)
  if constexpr (ROWS) lds_barrier();
  CVF_STAMP(26);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the image is this wave's own: LDS keeps a wave's accesses in order

  float f0b[SMAX][RT];   // the first layer's fragments once more, for s = W_1 q after the passes
  // ---- q = J A J^T g and E with four lanes per frame (the three passes of cvf_metric.hpp; lane p of a frame takes the atoms
  // p, p + 4, ..).  NIT = ceil(N / 4) rounded up to 2 / 4 / 6 is a template parameter: the lane's g rows and centred
  // coordinates are read from LDS ONCE into registers (clamped index + mask for the ragged end, no branches), u = a .* G
  // replaces g in those registers and q is formed from them - one LDS round trip for the three passes instead of three.
  {
    const float* ar = auxL + f * kAuxP;
    float* Ul = gI + f * kImgP;
    V3 gv[NIT];
    if (iso) {
    // ---- ISOTROPIC metric (wave-uniform branch): a_b the one coefficient of atom b, f_b its feature = its aligned position (the LDS
    // image), r_b its reference position (zero off the align atoms).  With u = a .* G = R (a_b G') the lab-frame passes below
    // become, in the aligned frame,
    //   pass 1: gbar = sum_b g_b / n_align, tau = sum_b g_b x f_b (the axial vector of R^T M), s = K^-1 tau
    //   pass 2: G'_b = g_b + m_b (s x r_b - gbar)  (Z ref = R (s x ref)),  u'_b = a_b G'_b,  E = sum_b u'_b . G'_b,
    //           om = K^-1 (sum_align r_b x u'_b - rsum x ubar')  (the axial vector of R^T dH)
    //   pass 3: q_b = u'_b - ubar' + f_b x om  ((x - c) dR = f [om]x)
    // - cross products instead of 3x3 products, 6 quad sums instead of 24, and neither R nor the centroid nor a coordinate.
    // The lane, duplicate-atom and mask conventions are those of the general passes.
    const float* Fl = featI + f * kImgP;
    V3 gsum = v3(0.0f, 0.0f, 0.0f), tau = v3(0.0f, 0.0f, 0.0f);
    int pb = p;
    asm volatile("" : "+v"(pb));   // (opaque, once per pass: the pass's addresses are formed here, not hoisted and kept across the passes)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const AtomSlot sl = atom_slot<NIT>(pb, it, N);
      const bool last = it == NIT - 1;
      const int i3 = sl.i3;
      const float lv = sl.lv;
      gv[it] = v3(Ul[i3], Ul[i3 + 1], Ul[i3 + 2]);
      const V3 fb = v3(Fl[i3], Fl[i3 + 1], Fl[i3 + 2]);
      const V3 gm = last ? lv * gv[it] : gv[it];
      gsum = gsum + gm;
      tau.x = fmaf(gm.y, fb.z, fmaf(-gm.z, fb.y, tau.x));
      tau.y = fmaf(gm.z, fb.x, fmaf(-gm.x, fb.z, tau.y));
      tau.z = fmaf(gm.x, fb.y, fmaf(-gm.y, fb.x, tau.z));
    }
    CVF_STAMP(27);
    gsum = v3(quad_sumf16(gsum.x), quad_sumf16(gsum.y), quad_sumf16(gsum.z));
    tau = v3(quad_sumf16(tau.x), quad_sumf16(tau.y), quad_sumf16(tau.z));
    float Kinv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) Kinv[i] = ar[12 + i];
    const V3 s = sym_times(Kinv, tau);
    const float inv_nal = 1.0f / (float)nal;
    const V3 gbar = inv_nal * gsum;
    float E = 0.0f;
    V3 usum = v3(0.0f, 0.0f, 0.0f), tau2 = v3(0.0f, 0.0f, 0.0f);
    pb = p;
    asm volatile("" : "+v"(pb));
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const AtomSlot sl = atom_slot<NIT>(pb, it, N);
      const bool last = it == NIT - 1;
      const int ac = sl.ac;
      const float lv = sl.lv;                                        // alive (not a duplicate): counts in the sums
      const float ma = ALLAL ? 1.0f : (ac < nal ? 1.0f : 0.0f);      // align atom
      const int r3 = ALLAL ? sl.i3 : (ac < nal ? sl.i3 : 0);
      V3 rf = v3(refL[r3], refL[r3 + 1], refL[r3 + 2]);
      if (!ALLAL) rf = ma * rf;
      const V3 sh = ALLAL ? gbar : ma * gbar;
      V3 G;
      G.x = fmaf(s.y, rf.z, fmaf(-s.z, rf.y, gv[it].x - sh.x));
      G.y = fmaf(s.z, rf.x, fmaf(-s.x, rf.z, gv[it].y - sh.y));
      G.z = fmaf(s.x, rf.y, fmaf(-s.y, rf.x, gv[it].z - sh.z));
      const V3 u = aL[sl.i3] * G;
      gv[it] = u;
      const bool masked = last || !ALLAL;                            // (compile-time)
      const V3 ue = last ? lv * u : u;
      E = fmaf(ue.x, G.x, fmaf(ue.y, G.y, fmaf(ue.z, G.z, E)));
      const V3 um = masked ? (ma * lv) * u : u;
      usum = usum + um;
      tau2.x = fmaf(rf.y, um.z, fmaf(-rf.z, um.y, tau2.x));
      tau2.y = fmaf(rf.z, um.x, fmaf(-rf.x, um.z, tau2.y));
      tau2.z = fmaf(rf.x, um.y, fmaf(-rf.y, um.x, tau2.z));
    }
    CVF_STAMP(28);
    E = quad_sumf16(E);
    usum = v3(quad_sumf16(usum.x), quad_sumf16(usum.y), quad_sumf16(usum.z));
    tau2 = v3(quad_sumf16(tau2.x), quad_sumf16(tau2.y), quad_sumf16(tau2.z));
    const V3 rsum = v3(rsL[0], rsL[1], rsL[2]);   // sum of the reference over the align atoms (the fp32 residue of its centring)
    eL[net * kU + f] = E;   // (the four lanes of a frame hold the same sum and store it to the same place)
    urows(e_tiled + (tile * k + net) * CVF_TILE + kU * sub, kU, f).st(0, E);
    const V3 ubar = inv_nal * usum;
    tau2.x = fmaf(-rsum.y, ubar.z, fmaf(rsum.z, ubar.y, tau2.x));
    tau2.y = fmaf(-rsum.z, ubar.x, fmaf(rsum.x, ubar.z, tau2.y));
    tau2.z = fmaf(-rsum.x, ubar.y, fmaf(rsum.y, ubar.x, tau2.z));
    const V3 om = sym_times(Kinv, tau2);
    CVF_STAMP(31);
    pb = p;
    asm volatile("" : "+v"(pb));
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i3 = atom_slot<NIT>(pb, it, N).i3;
      const V3 fb = v3(Fl[i3], Fl[i3 + 1], Fl[i3 + 2]);
      V3 qv;
      qv.x = fmaf(fb.y, om.z, fmaf(-fb.z, om.y, gv[it].x - ubar.x));
      qv.y = fmaf(fb.z, om.x, fmaf(-fb.x, om.z, gv[it].y - ubar.y));
      qv.z = fmaf(fb.x, om.y, fmaf(-fb.y, om.x, gv[it].z - ubar.z));
      gv[it] = qv;   // (kept: q leaves for global memory at the very end, behind every load of this kernel)
      Ul[i3] = qv.x;
      Ul[i3 + 1] = qv.y;
      Ul[i3 + 2] = qv.z;
    }
    } else {
    float R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ar[i];
    const Centre c = centre_of(ar[9], ar[10], ar[11]);
    // pass 1: sum_b g_b and M = sum_b (x_b - c) (x) g_b
    V3 gsum = v3(0.0f, 0.0f, 0.0f);
    Outer3 Mo = {{{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}}, {0.0f, 0.0f, 0.0f}};
    int pb = p;
    asm volatile("" : "+v"(pb));   // (opaque, once per pass: the pass's addresses are formed here, not hoisted and kept across the passes)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const AtomSlot sl = atom_slot<NIT>(pb, it, N);
      const bool last = it == NIT - 1;           // (compile-time: the only iteration that can run past the last atom)
      const int i3 = sl.i3;
      const float lv = sl.lv;
      // (a lane past the last atom works on a DUPLICATE of atom N - 1 - masked out of every sum, but carried through so that
      //  it computes and stores the same u and q as that atom's owner: no lane-divergent branch around the stores)
      gv[it] = v3(Ul[i3], Ul[i3 + 1], Ul[i3 + 2]);
      const V3 gm = last ? lv * gv[it] : gv[it];
      gsum = gsum + gm;
      outer_acc(Mo, centred(my + i3, 0, c), gm);
    }
    CVF_STAMP(27);
    gsum = v3(quad_sumf16(gsum.x), quad_sumf16(gsum.y), quad_sumf16(gsum.z));
    const V3 sump = mat_times(R, gsum);   // sum_b R g_b
    float M[9];
    outer_to_array(Mo, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = quad_sumf16(M[i]);
    float T[9], Z[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) T[3 * i + j] = R[i] * M[j] + R[3 + i] * M[3 + j] + R[6 + i] * M[6 + j];
    float Kinv[6];   // (read where it is used, twice: six registers less across the atom loops)
#pragma unroll
    for (int i = 0; i < 6; ++i) Kinv[i] = ar[12 + i];
    const V3 s = sym_times(Kinv, v3(T[7] - T[5], T[2] - T[6], T[3] - T[1]));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Z[3 * i + 0] = R[3 * i + 1] * s.z - R[3 * i + 2] * s.y;
      Z[3 * i + 1] = -R[3 * i + 0] * s.z + R[3 * i + 2] * s.x;
      Z[3 * i + 2] = R[3 * i + 0] * s.y - R[3 * i + 1] * s.x;
    }
    const float inv_nal = 1.0f / (float)nal;
    const V3 shift = inv_nal * sump;
    // pass 2: G = R g (+ Z ref - shift on the align atoms), u = a .* G, E = u . G; u replaces g in the registers
    const MatCols Rc = mat_cols(R), Zc = mat_cols(Z);
    f2 E2 = {0.0f, 0.0f};
    float Ez = 0.0f;
    f2 usum_xy = {0.0f, 0.0f};
    float usum_z = 0.0f;
    Outer3 dHo = {{{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}}, {0.0f, 0.0f, 0.0f}};
    pb = p;
    asm volatile("" : "+v"(pb));
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const AtomSlot sl = atom_slot<NIT>(pb, it, N);
      const bool last = it == NIT - 1;
      const int ac = sl.ac, i3 = sl.i3;
      const float lv = sl.lv;                                        // alive (not a duplicate): counts in the sums
      const float ma = ALLAL ? 1.0f : (ac < nal ? 1.0f : 0.0f);      // align atom: carries the rotation's and the centroid's derivative
      const int r3 = ALLAL ? i3 : (ac < nal ? i3 : 0);
      V3 rf = v3(refL[r3], refL[r3 + 1], refL[r3 + 2]);
      if (!ALLAL) rf = ma * rf;
      f2 Gxy = ALLAL ? f2{-shift.x, -shift.y} : f2{-ma * shift.x, -ma * shift.y};
      float Gz = ALLAL ? -shift.z : -ma * shift.z;
      mat_times_acc(Rc, gv[it], Gxy, Gz);
      mat_times_acc(Zc, rf, Gxy, Gz);
      asm volatile("");   // (the coefficients' reads behind G: see atom_slot)
      const f2 uxy = f2{aL[i3], aL[i3 + 1]} * Gxy;
      const float uz = aL[i3 + 2] * Gz;
      gv[it] = v3(uxy.x, uxy.y, uz);
      const bool masked = last || !ALLAL;                            // (compile-time)
      const float m = ma * lv;
      const f2 uxm = masked ? m * uxy : uxy;
      const float uzm = masked ? m * uz : uz;
      E2 = fma2(last ? lv * uxy : uxy, Gxy, E2);
      Ez = fmaf(last ? lv * uz : uz, Gz, Ez);
      usum_xy += uxm; usum_z += uzm;
      outer_acc(dHo, v3(uxm.x, uxm.y, uzm), rf);
    }
    CVF_STAMP(28);
    const float E = quad_sumf16((E2.x + E2.y) + Ez);
    const V3 usum = v3(quad_sumf16(usum_xy.x), quad_sumf16(usum_xy.y), quad_sumf16(usum_z));
    const V3 rsum = v3(rsL[0], rsL[1], rsL[2]);   // sum of the reference over the align atoms (the fp32 residue of its centring)
    float dH[9];
    outer_to_array(dHo, dH);
#pragma unroll
    for (int i = 0; i < 9; ++i) dH[i] = quad_sumf16(dH[i]);
    eL[net * kU + f] = E;   // (the four lanes of a frame hold the same sum and store it to the same place)
    urows(e_tiled + (tile * k + net) * CVF_TILE + kU * sub, kU, f).st(0, E);
    const V3 ubar = inv_nal * usum;
    dH[0] -= ubar.x * rsum.x; dH[1] -= ubar.x * rsum.y; dH[2] -= ubar.x * rsum.z;
    dH[3] -= ubar.y * rsum.x; dH[4] -= ubar.y * rsum.y; dH[5] -= ubar.y * rsum.z;
    dH[6] -= ubar.z * rsum.x; dH[7] -= ubar.z * rsum.y; dH[8] -= ubar.z * rsum.z;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) T[3 * i + j] = R[i] * dH[j] + R[3 + i] * dH[3 + j] + R[6 + i] * dH[6 + j];
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 6; ++i) Kinv[i] = ar[12 + i];
    const V3 om = sym_times(Kinv, v3(T[7] - T[5], T[2] - T[6], T[3] - T[1]));
    float dR[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      dR[3 * i + 0] = R[3 * i + 1] * om.z - R[3 * i + 2] * om.y;
      dR[3 * i + 1] = -R[3 * i + 0] * om.z + R[3 * i + 2] * om.x;
      dR[3 * i + 2] = R[3 * i + 0] * om.y - R[3 * i + 1] * om.x;
    }
    // pass 3: q_b = (u_b - ubar) R + (x_b - c) dR  -> in place of g, this wave's image (the B operand of s = W_1 q below)
    CVF_STAMP(31);
    const MatRows Rr = mat_rows(R), dRr = mat_rows(dR);
    pb = p;
    asm volatile("" : "+v"(pb));
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i3 = atom_slot<NIT>(pb, it, N).i3;
      f2 qxy = {0.0f, 0.0f};
      float qz = 0.0f;
      row_times_acc(Rr, gv[it] - ubar, qxy, qz);
      row_times_acc(dRr, centred(my + i3, 0, c), qxy, qz);
      gv[it] = v3(qxy.x, qxy.y, qz);   // (kept: q leaves for global memory at the very end, behind every load of this kernel)
      Ul[i3] = qxy.x;
      Ul[i3 + 1] = qxy.y;
      Ul[i3 + 2] = qz;
    }
    }   // (general metric)
    CVF_STAMP(32);
    asm volatile("" ::: "memory");   // (not earlier: 36 more live registers during the passes spill, and a spill's reload
                                     //  drains every outstanding store)
    // (S opaque from here on: the row offsets of the fragments and the k-step tests below are scalar arithmetic of their own.  Shared
    //  with the head's request of the same rows and with layer 0's loop, the 36 offsets and the `s < S` masks were formed once,
    //  kept across the whole kernel and spilled into lanes of a vector register - a v_readlane and its wait states per use)
    int Sq = S;
    asm volatile("" : "+s"(Sq));
#pragma unroll
    for (int s_ = 0; s_ < SMAX; ++s_) {
      const int se = s_ < Sq ? s_ : Sq - 1;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) f0b[s_][rt] = pk.ld(L.f0() + (se * RT + rt) * 64);
    }
    // ---- s = W_1 q (what the backward kernel's tangent chain starts from, up to the per-frame factor 2 w dL/dE it only
    // knows after the batch sums are reduced): the first layer's fragments once more, q from this wave's image
    {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      Vec<H, 1> sv0;
      init_bias<H, 1>(sv0, nullptr, q);
      // (one address and the k-step as the read's immediate offset, no clamp: a row past D of the last k-step, 4 s + q <= 4 S - 1,
      //  holds what this wave's g tile put there above - the 16-byte writes cover the row up to 4 S - 1, the passes replace
      //  what lies below D only - and meets a zero weight, as the clamped row did.  That value is a zero because the rows past D
      //  of the T0 fragments are zero, like those of F0: cvf_ef_pack clears the packed buffer before it scatters, and so must
      //  whoever else fills it - a NaN there would reach s through 0 x NaN)
      const float* qr = gI + col * kImgP + q;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        if (s < Sq) {   // wave-uniform
          const float b = qr[4 * s];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) sv0.v[rt][0] = mfma4(f0b[s][rt], b, sv0.v[rt][0]);
        }
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) sv.st(((2 * NH - 1) * NG + g) * 256, sv0.v[g >> 2][0][g & 3]);
    }
    CVF_STAMP(33);
    // ---- q -> the tiled hand-off (the first layer's weight-gradient operand of the backward kernel)
    //      (as the hand-off rows: a buffer resource on this (tile, net, unit)'s columns, ONE lane offset - row 3 p, frame f - and
    //       the rows of the lane's further atoms as scalar offsets; the clamped last atom has a lane offset of its own.  With
    //       pointers every store formed a 64-bit address in a register pair)
    const int q_floats = D * CVF_TILE - kU * sub;
    const __amdgpu_buffer_rsrc_t qres =
        __builtin_amdgcn_make_buffer_rsrc(q_tiled + (tile * k + net) * (int64_t)D * CVF_TILE + kU * sub, 0, q_floats * 4, 0x00020000);
    int pb = p;
    asm volatile("" : "+v"(pb));
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const bool last = it == NIT - 1;
      const URows qt{qres, ((last ? atom_slot<NIT>(pb, it, N).i3 : 3 * pb) * CVF_TILE + f) * 4};
      const int row = last ? 0 : 12 * it;
      qt.st(row * CVF_TILE, gv[it].x);
      qt.st((row + 1) * CVF_TILE, gv[it].y);
      qt.st((row + 2) * CVF_TILE, gv[it].z);
    }
  }
  CVF_STAMP(34);
  // ---- the feature tile for the backward kernel (the first layer's weight-gradient operand), from the LDS image
  //      (ROWS: the batch's tile is already what the backward kernel reads)
  if constexpr (!ROWS) {
    float* ft = feat_tiled + tile * (int64_t)D * CVF_TILE + kU * sub + f;
    const float* fi = featI + f * kImgP;
    // (a plain counted loop: left to itself the compiler unrolls and vectorises this run-time trip count into ~200 vector
    //  instructions with three remainder paths and spills an address across them - each reload behind a wait for ALL stores)
#pragma unroll 1
    for (int j = p + 4 * wave; j < D; j += 4 * nw) ft[j * CVF_TILE] = fi[j];
  }
  CVF_STAMP(29);
  if (partial == nullptr) return;   // (uniform) large batches: the caller reduces y / E with cvf_ef_stats
  // wave 0: where its registers of the two matrix results below go in the unit's row - the byte offset of statistic t of this unit,
  // t * G + unit (G = the launch's units, its rows; at most kMaxRows16 where the launch is given `partial`, and t < 170: 32 bits
  // and 24-bit products), or an offset past the end of the rows for a register that holds nothing: the buffer store drops it, as the
  // backward launch's dead tile entries are dropped - no lane-divergent branch around a store.  They depend on the lane, k and the launch alone and are
  // formed HERE, in front of the barrier at which the wave waits for the others anyway; behind the matrix instructions they
  // were the tail of every block (64-bit products and adds per store, after the other waves had left).
  //   D1 (row ri, column cj): (0, 0) -> W; (0, j) -> S1_j; (i, j), 1 <= i <= j <= k -> S2 pair (i-1, j-1) in row-major i <= j order
  //   D2: (ri < k, 0) -> E_ri
  constexpr int kDeadRow = 0x7fff0000;   // (positive, and far past 170 rows of at most 16 384 doubles)
  int o1[4], o2[4];
  if (wave == 0) {
    const int cj = lane & 15, G = (int)units_x, u = (int)unit;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ri = (lane >> 4) + 4 * r, a_ = ri - 1;
      const int t = ri == 0 ? cj : 1 + k + __mul24(a_, k) - (__mul24(a_, a_ - 1) >> 1) + (cj - ri);
      o1[r] = (ri <= cj && cj <= k) ? (__mul24(t, G) + u) * 8 : kDeadRow;
      o2[r] = (cj == 0 && ri < k) ? (__mul24(1 + k + CVF_NPAIR(k) + ri, G) + u) * 8 : kDeadRow;
    }
  }
  lds_barrier();                    // y and E of every net are in LDS

  // ---- wave 0: this unit's row of the batch sums [W | S1(k) | S2(i<=j) | E(k)] in fp64 on the matrix cores: with the frames
  // as the contraction index (four k-steps of four frames), D1 = [1, y_1..y_k] x [w, w y_1..w y_k] holds W (0,0), S1_j (0,j)
  // and S2_ij (i,j), D2 = [E_1..E_k] x [w, ..] holds E_i in column 0 - eight v_mfma_f64_16x16x4_f64 instead of the 13
  // statistic-by-statistic DPP scans (~570 vector instructions, 3-4 k cycles at the end of every block).  Products of two
  // floats are exact in fp64 and the hardware adds the k-steps in a fixed order: bitwise reproducible, as before.
  // cvf_ef_stats_finish adds the units' rows.
  if (wave == 0) {
    typedef double f64x4 __attribute__((ext_vector_type(4)));
    const int np = CVF_NPAIR(k);
    const int i = lane & 15, kq = lane >> 4;   // operand row / column, k-slot
    f64x4 d1 = {0.0, 0.0, 0.0, 0.0}, d2 = {0.0, 0.0, 0.0, 0.0};
    // (yL and eL are adjacent: rows 1..k of the A operand are y, the same index k rows further is E)
    const float* yrow = yL + (i >= 1 && i <= k ? i - 1 : 0) * kU;
    const float* erow = eL + (i < k ? i : 0) * kU;
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) {
      const int fr = 4 * s_ + kq;
      const double wb = (double)wL[fr];
      const double yv = (double)yrow[fr];
      const double a1 = i == 0 ? 1.0 : (i <= k ? yv : 0.0);
      const double b = i == 0 ? wb : (i <= k ? wb * yv : 0.0);
      const double a2 = i < k ? (double)erow[fr] : 0.0;
      d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, d1, 0, 0, 0);
      d2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b, d2, 0, 0, 0);
    }
    // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 r - to the offsets formed in front of the barrier
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const __amdgpu_buffer_rsrc_t pres = __builtin_amdgcn_make_buffer_rsrc(partial, 0, __mul24(1 + 2 * k + np, (int)units_x) * 8, 0x00020000);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v1 = d1[r], v2 = d2[r];   // (by value: bit casts of vector elements)
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v1), pres, o1[r], 0, 0);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v2), pres, o2[r], 0, 0);
    }
  }
  CVF_STAMP(30);
  }   // (generator instance)
  };  // run_pass
  run_pass(0);
  if constexpr (kTransfer) {
    if (!paired) return;                         // (uniform)
    run_pass(1);                                 // the same waves, the lagged partners of these 16 frames
    if (partial == nullptr) return;              // (uniform)
    const int lane = lane_in;
    const int64_t unit = ub;
    lds_barrier();                               // y and y' of every net are in LDS
    // ---- wave 0: this unit's row of the time-lagged batch sums [W | S1 | S2(i<=j) | W' | S1' | S2'_ii | T] (cvf_ef_nstats, lag > 0)
    // in fp64 on the matrix cores, the 16 frames as the contraction index: D1 = [1, y] x [w, w y] holds W, S1_j, S2_ij;
    // D2 = [1, y'] x [w', w' y'] holds W', S1'_j and S2'_jj on its diagonal; D3 = [y' - y] x [w (y' - y)] holds T_i = sum w (y'_i - y_i)^2
    // on its diagonal (core.py:412-416, 428).  Products of two floats are exact in fp64, the k-steps add in a fixed order.
    if (wave == 0) {
      typedef double f64x4 __attribute__((ext_vector_type(4)));
      const int np = CVF_NPAIR(k);
      const int i = lane & 15, kq = lane >> 4;
      const float* y0 = lds + Lo.y;                  // y of the frames | y' of the partners (the two passes' yL)
      const float* y1 = y0 + k * kU;
      const float* w0 = lds + Lo.w;
      const float* w1 = lds + Lo.g;
      f64x4 d1 = {0.0, 0.0, 0.0, 0.0}, d2 = {0.0, 0.0, 0.0, 0.0}, d3 = {0.0, 0.0, 0.0, 0.0};
      const int yi = (i >= 1 && i <= k ? i - 1 : 0) * kU, ti = (i < k ? i : 0) * kU;
#pragma unroll
      for (int s_ = 0; s_ < 4; ++s_) {
        const int fr = 4 * s_ + kq;
        const double wb = (double)w0[fr], wl_ = (double)w1[fr];
        const double yv = (double)y0[yi + fr], ylv = (double)y1[yi + fr];
        const double a1 = i == 0 ? 1.0 : (i <= k ? yv : 0.0), b1 = i == 0 ? wb : (i <= k ? wb * yv : 0.0);
        const double a2 = i == 0 ? 1.0 : (i <= k ? ylv : 0.0), b2 = i == 0 ? wl_ : (i <= k ? wl_ * ylv : 0.0);
        const double df = i < k ? (double)y1[ti + fr] - (double)y0[ti + fr] : 0.0;
        d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, d1, 0, 0, 0);
        d2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, d2, 0, 0, 0);
        d3 = __builtin_amdgcn_mfma_f64_16x16x4f64(df, wb * df, d3, 0, 0, 0);
      }
      const int cj = lane & 15, o = 1 + k + np;
      const int64_t G = units_x;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ri = (lane >> 4) + 4 * r;
        int t = -1;
        if (ri == 0 && cj <= k) t = cj;
        else if (ri >= 1 && ri <= cj && cj <= k) {
          const int a_ = ri - 1, b_ = cj - 1;
          t = 1 + k + a_ * k - (a_ * (a_ - 1)) / 2 + (b_ - a_);
        }
        if (t >= 0) partial[t * G + unit] = d1[r];
        if (ri == 0 && cj <= k) partial[(o + cj) * G + unit] = d2[r];                             // W', S1'_j
        if (ri >= 1 && ri == cj && cj <= k) partial[(o + 1 + k + (cj - 1)) * G + unit] = d2[r];   // S2'_jj
        if (ri == cj && cj < k) partial[(o + 1 + 2 * k + cj) * G + unit] = d3[r];                 // T_i
      }
    }
  }
}
}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// host side shared by cvf_ef16_front (ROWS = false) and cvf_ef16_front_rows (ROWS = true)
// ------------------------------------------------------------------------------------------------------------------
int cvf_ef_stats_finish_impl(const cvf_ef_cfg* cfg, int n_rows, int stat_major, const double* partial, double* stats,
                             double* loss_vec, double* coef, hipStream_t s);
int cvf_ef_stats_finish_ll(const cvf_ef_cfg* cfg, int n_rows, int stat_major, const double* partial, double* stats,
                           double* loss_vec, double* coef, hipStream_t s, const P2PLL* ll);

// Units per workgroup of a front launch (see the kernel).  ONE by default.  Several (CVF_EF16_UPB = 2..5, a developer switch, results
// bit for bit those of one: tools/upb_check.py) were built on the observation that the 1250 one-unit workgroups of a 20 000-frame
// batch reach their first stamp over 4.4 us - and measured SLOWER: 37.2 us per launch with five units per workgroup against 34.6
// (two or three: 47-49 us, a second round under the 16-waves-per-CU limit).  tools/dispatch_probe.hip settled why: starting 1250
// workgroups of 3 waves costs the same as 250 of 15 (2.5-2.8 us per empty launch, identical with work inside), so the spread of
// the first stamps is the cold instruction cache and kernel-argument fetch, which every wave pays wherever it sits; what the
// large workgroup adds is five units waiting at each other's barriers (two of the five alignment solves share a SIMD).
static int ef16_units_per_wg(int64_t units, int k, size_t lds_unit_bytes) {
  int cap = 16 / k;
  if (cap > 5) cap = 5;
  while (cap > 1 && (size_t)cap * lds_unit_bytes > 150 * 1024) --cap;
  if (cap < 1) cap = 1;
  int upb = 1;
  (void)units;
  if (const char* e = getenv("CVF_EF16_UPB")) {
    const int v = atoi(e);
    if (v >= 1 && v <= cap) upb = v;
  }
  return upb;
}

// argument checks, instance dispatch and launch of the generator-mode front kernel (+ the finishing launch when stats != NULL).
// iso (the _iso entry points) or cfg->iso_metric: the caller vouches for a[3b] == a[3b+1] == a[3b+2] on every record atom (launch bit 9: the aligned-frame passes) - a
// run-time switch of the same instances, not a template parameter: the branch is wave-uniform and taken once per block, and a
// second set of instances would double the two longest compilations of the build.
template <bool ROWS>
static int ef16_front_go(const char* what, const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                         const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, float* y_tiled, float* saved, float* q_tiled,
                         float* e_tiled, const cvf_ef_cfg* cfg, const float* w, double* scratch, double* stats, double* loss_vec,
                         double* coef, const float* align_rows, void* stream, bool iso = false) {
  CVF_REQUIRE(pp && pp->mode != CVF_PP_FACTORED, "%s: takes coordinates, not CVF_PP_FACTORED records", what);
  CVF_REQUIRE(cvf_ef16_supported(mlp, pp), "%s: shape not covered (cvf_ef16_supported() == 0)", what);
  CVF_REQUIRE(theta && packed && feat_tiled && x && a && y_tiled && saved && q_tiled && e_tiled && cfg && w && scratch && B > 0,
              "%s: bad argument", what);
  CVF_REQUIRE(stats != nullptr || cvf_ef16_rows(B) > 0, "%s: stats == NULL (rows left for cvf_ef16_finish) needs cvf_ef16_rows(B) > 0", what);
  CVF_REQUIRE(cfg->k == mlp->n_nets && cfg->lag_idx == 0, "%s: generator mode only, cfg.k must equal the number of nets", what);
  CVF_REQUIRE(loss_vec == nullptr || coef != nullptr, "%s: loss_vec without coef", what);
  int H, NH;
  ef16_shape(mlp, &H, &NH);
  const int k = mlp->n_nets;
  const int64_t T = cvf_ntiles(B), units = 4 * T;
  const int ns = cvf_ef_nstats(k, 0);
  const bool rows = units <= kMaxRows16;
  const size_t lds1 = (size_t)front16_lds(pp->n_coord, pp->n_align, k).total * sizeof(float);
  const int upb = ef16_units_per_wg(units, k, lds1);
  const size_t lds = lds1 * upb;
  (void)ns;
  ef16_dispatch(H, NH, [&](auto h_, auto nh_) {
    constexpr int kH = decltype(h_)::value, kNH = decltype(nh_)::value;
    auto go = [&](auto kernel) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)((units + upb - 1) / upb)), dim3(64 * k * upb), lds, (hipStream_t)stream, *mlp, theta, packed, *pp,
                         x, B, a, w, feat_tiled, y_tiled, saved, q_tiled, e_tiled, rows ? scratch : nullptr, upb | (iso || cfg->iso_metric != 0 ? 512 : 0), (const float*)nullptr, units,
                         (const float*)nullptr, align_rows);
    };
    const int nit = (pp->n_rec + 3) / 4;   // atoms per lane in the four-lanes-per-frame passes (1..6: d_r <= 72)
    const bool allal = pp->n_align == pp->n_rec;
#define EF16_GO(NIT_)                                                  \
    case NIT_:                                                          \
      if (allal) go(ef16_front_kernel<kH, kNH, NIT_, true, ROWS>);      \
      else go(ef16_front_kernel<kH, kNH, NIT_, false, ROWS>);           \
      break;
    switch (nit) {
#ifndef CVF_DEV_SHAPES
      EF16_GO(1) EF16_GO(2) EF16_GO(3) EF16_GO(4) EF16_GO(5)
#endif
      default:
        if (allal) go(ef16_front_kernel<kH, kNH, 6, true, ROWS>);
#ifndef CVF_DEV_SHAPES
        else go(ef16_front_kernel<kH, kNH, 6, false, ROWS>);
#endif
    }
#undef EF16_GO
  });
  int rc = cvf_check_launch("ef16_front_kernel");
  if (rc || stats == nullptr) return rc;   // stats == NULL: the caller adds the units' rows itself (cvf_ef16_finish)
  if (rows) return cvf_ef_stats_finish_impl(cfg, (int)units, 1, scratch, stats, loss_vec, coef, (hipStream_t)stream);
  return cvf_ef_stats(cfg, B, w, y_tiled, e_tiled, nullptr, nullptr, scratch, stats, loss_vec, coef, stream);
}


