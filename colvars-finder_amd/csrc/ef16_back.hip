// The backward kernel of the 16-frames-per-wave step (see ef16_front.hip for the decomposition and the hand-off layout).
#include "ef16_common.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// back: parameter gradient of the loss given the coefficients d loss / d sums (what loss.backward() does at core.py:517).
// Block = (64-frame tile, net), four waves; wave w owns the unit w of the tile (frames 16 w .. 16 w + 15) for the
// register-resident chains and a share of every weight-gradient product, whose K dimension is the tile's 64 frames
// (operands transposed through LDS images [feature][frame], as in ef_bwd_mfma_kernel).
// Against that kernel: the forward chain, the d chain AND the first product of the tangent chain arrive from the front
// kernel (30 coalesced 256-byte rows per wave), every weight fragment and the first layer's feature / q operands are
// requested before the first matrix instruction - no global round trip is left inside the dependent chain, which at these
// batch sizes was two thirds of the old kernel's time (tools/ef16_probe.hip: d + tangent chains 32 k, reverse l=0 19 k
// of 69 k cycles per wave with just-in-time loads).
// ------------------------------------------------------------------------------------------------------------------
struct Back16Args {
  int k;
  int64_t B;
  int64_t n_tiles;
  int64_t T;              // transfer-operator mode: tiles 0..T-1 hold the frames, T..2T-1 their lagged partners
  const float* w_lag;     // ... and the partners' weights
};
// What the kernel reads of cvf_mlp_desc (by value the descriptor is 1 KB of kernel arguments whose offset tables are loaded
// piecemeal into a scalar file that is too small for them).  The host has checked that every net is laid out the regular way -
// per layer the weight [out, in], then the bias, layer after layer - so that an offset inside a net is a constant of (H, NH)
// plus H * D, and a block needs ONE scalar of the record's table: its own net's base.
struct Back16Nets {
  int D;                       // dims[0]
  int n_params;
  int base[CVF_MAX_NETS];      // w_off[net][0]
};
// offsets of layer l = 0..NH (NH: the 1 x H output layer) from the net's base; hd = H * D
template <int H, int NH>
__host__ __device__ constexpr int net_w_off(int l, int hd) { return l == 0 ? 0 : hd + H + (l - 1) * (H * H + H); }
template <int H, int NH>
__host__ __device__ constexpr int net_b_off(int l, int hd) { return net_w_off<H, NH>(l, hd) + (l == 0 ? hd : l == NH ? H : H * H); }

// GEN: generator mode (tangent chain, second operands).  !GEN: transfer-operator mode - the plain backward pass of y and y'
// with the coefficients of the time-lagged loss (as ef_bwd_mfma_kernel's lag_idx > 0 branch), no tangent chain.
template <int H, int NH, bool MULTI, bool GEN>
__global__ __launch_bounds__(256, 4) void ef16_back_kernel(Back16Args args, Back16Nets nets, const float* __restrict__ theta,
                                                            const float* __restrict__ packed, const float* __restrict__ w,
                                                            const float* __restrict__ feat, const float* __restrict__ y_tiled,
                                                            const float* __restrict__ q_tiled, const double* __restrict__ coef,
                                                            float* __restrict__ slab, int32_t* __restrict__ step,
                                                            const float* __restrict__ saved) {
  constexpr int RT = Hid<H>::RT, NG = Hid<H>::NG;
  constexpr int RTO = (H + 15) / 16;      // row tiles of an H-row image (natural order)
  constexpr int CTH = (H + 1 + 15) / 16;  // column tiles of [h ; 1]
  constexpr int NT = 256, WPB = 4;
  // a second row tile with 1..4 useful rows (H = 20 among the instances) goes to the matrix cores as 4x4x1 blocks, which have no
  // padding rows and cost a quarter of a 16x16x4 instruction each; every other instance compiles to what it was
  constexpr bool TAIL4 = RTO == 2 && H % 16 >= 1 && H % 16 <= 4;
  constexpr int kRows = 2 * H + 2 * (H + 1) + 16;   // packed images: reads past an image's rows meet finite values whose products are discarded
  __shared__ __attribute__((aligned(16))) float IMG[kRows * kPitch];
  __shared__ float PART[4 * (H + 1)];   // the last layer's gradient, one partial row per wave (strip_rows, ef16_common.hpp)
  extern __shared__ float GI[];  // MULTI (a block walks several tiles): its partial gradient of `net`, flat parameter order
  float* SA1 = IMG;
  float* SA2 = SA1 + H * kPitch;
  float* SB1 = SA2 + H * kPitch;
  float* SB2 = SB1 + (H + 1) * kPitch;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform values in SGPRs (see the front kernel)
  int lane = tid & 63, col, q, row16, r0, fo, rowf;
  auto derive_lane = [&]() {
    col = lane & 15, q = lane >> 4, row16 = col, r0 = 4 * q;
    fo = 16 * wave + col;   // this lane's frame of the tile
    rowf = 4 * col + q;     // the row whose strip sum this lane keeps (strip_rows: hid_feature(col >> 2, col & 3, q))
  };
  derive_lane();
  static_assert(H % 4 == 0, "a lane's four rows of a gradient tile are inside the layer together (emit_tile)");
  const int net = blockIdx.y;
  int k = args.k;
  // What follows from D.  A last column tile of the first layer [f ; 1] with 1..4 useful columns (D = 66: features 64, 65 and the
  // bias) does not go to the matrix cores: its columns are `ncol` strips of H sums over the frames (strip_rows).  CTM column tiles
  // stay matrix tiles.  (Not const: the multi-tile form derives them again for every tile, see the tile loop.)
  int D = nets.D, HD, c0, nfeat, ncol, CTM;   // c0, nfeat, ncol: the last tile's first column, its features, its columns
  bool strip;
  PackLayout L;
  auto derive = [&]() {
    const int CT1 = (D + 1 + 15) / 16;
    HD = H * D;
    c0 = 16 * (CT1 - 1), nfeat = D - c0, ncol = nfeat + 1;
    strip = ncol <= 4;
    CTM = strip ? CT1 - 1 : CT1;
    L = pack_layout(H, NH, D);
  };
  derive();
  const int gbase = nets.base[net];
  const int gspan = net_b_off<H, NH>(NH, HD) + 1;
  float* out = slab + (int64_t)blockIdx.x * nets.n_params + gbase;   // this block's slab row, this net's span

  {   // (16-byte LDS writes: kRows * kPitch is a multiple of 4)
    static_assert((kRows * kPitch) % 4 == 0, "IMG is zeroed in 16-byte pieces");
    float4* img4 = reinterpret_cast<float4*>(IMG);
    for (int i = tid; i < kRows * kPitch / 4; i += NT) img4[i] = float4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  if (MULTI)
    for (int i = tid; i < gspan; i += NT) GI[i] = 0.0f;
  // (LDS only: __syncthreads() would also wait for every global load requested so far - a whole global round trip at the head of
  //  every block before the tile's own requests go out; stamped prologue 4.4 k cycles)
  lds_barrier();
  if (tid < 64) SB1[H * kPitch + tid] = 1.0f;  // bias column of [h ; 1]  (row H of SB2 stays 0)

  const URows pk = urows(packed + (int64_t)net * L.per_net, L.per_net, lane);   // this net's fragments (see URows)
  float wl[RT][4];
  load_hid_const_u<H>(urows(theta + gbase + net_w_off<H, NH>(NH, HD), H, q), wl);
  const float one[1] = {1.0f};

  // a finished 16x16 tile of layer `l` (rows = outputs, columns = inputs + bias).  Every tile of the gradient is produced
  // by exactly one wave, so a block that handles ONE tile of frames stores it straight into its slab row; a block that
  // walks several accumulates in the LDS image and flushes at the end.
  // (direct stores go through a buffer descriptor of the row's span: entries outside the layer get an offset past its end and
  //  are dropped by the hardware - no lane-divergent branch around the stores, so the compiler can count them when it waits
  //  for the weight fragments requested before them instead of waiting for everything; and the row offset is made opaque, or
  //  the four offsets of every call site are hoisted out of the layer loops, spilled, and reloaded behind a wait for ALL
  //  outstanding memory operations - i.e. for the previous store's completion, eight times per tile)
  const __amdgpu_buffer_rsrc_t out_rs = __builtin_amdgcn_make_buffer_rsrc(out, 0, gspan * 4, 0x00020000);
  // A lane's four entries of a tile are rows ob .. ob + 3 of ONE column: they are inside the layer together (H % 4 == 0) and a constant
  // stride apart - a row of the weights, or one float in the bias column.  So a tile costs one offset and one stride, not four of each.
  constexpr int kDead = 0x7fff0000;   // (+ 3 strides stays positive)
  auto emit_tile = [&](int l, int n_in, int rt, int ct, const f32x4& acc) {
    const int wo = net_w_off<H, NH>(l, HD), bo = net_b_off<H, NH>(l, HD);
    const int i = 16 * ct + row16;
    int ob = 16 * rt + r0;
    asm volatile("" : "+v"(ob));
    const bool isb = i == n_in, live = ob < H && i <= n_in;
    const int idx0 = isb ? bo + ob : wo + ob * n_in + i, stride = isb ? 1 : n_in;
    const int off0 = live ? idx0 * 4 : kDead;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float av = acc[r];   // (by value: __builtin_bit_cast applied to the vector-element lvalue acc[r] read element 0 four times)
      if (MULTI) {
        if (live) GI[idx0 + r * stride] += av;
      } else {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, av), out_rs, off0 + r * stride * 4, 0, 0);
      }
    }
  };
  // one 16x16 tile of  A1 B1^T + A2 B2^T  over the tile's 64 frames, operands in LDS images (eight 16-byte reads at a time)
  auto outer2 = [&](const float* A1, const float* B1, const float* A2, const float* B2, int rt, int ct) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    acc = outer_half(A1, B1, rt, ct, lane, acc);
    if constexpr (GEN) acc = outer_half(A2, B2, rt, ct, lane, acc);
    return acc;
  };

  // a strip entry: stored like a tile's (no lane-divergent branch around the store, dead lanes get an offset past the span)
  auto emit_entry = [&](bool live, int idx, float v) {
    if (MULTI) {
      if (live) GI[idx] += v;
    } else {
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), out_rs, live ? idx * 4 : kDead, 0, 0);
    }
  };
  // the last layer's H weights and bias from the four waves' partials in PART (one wave; behind a block barrier)
  auto emit_last = [&]() {
    if (wave == WPB - 1) {   // wave-uniform
      int i = lane;
      asm volatile("" : "+v"(i));
      const bool live = i <= H;
      const float v = strip_total(PART + (live ? i : H), H + 1);
      emit_entry(live, i < H ? net_w_off<H, NH>(NH, HD) + i : net_b_off<H, NH>(NH, HD), v);
    }
  };
  // the first layer's strip columns from the partials in SB1 ([wave][row][4 columns]; behind a block barrier)
  auto emit_strip = [&]() {
    if (strip && 64 * wave < 4 * H) {   // wave-uniform
      int e = tid;
      asm volatile("" : "+v"(e));
      const int o = e >> 2, c = e & 3;
      const bool live = o < H && c < ncol;
      const float v = strip_total(SB1 + (o < H ? e : 0), 4 * H);
      emit_entry(live, c < nfeat ? o * D + c0 + c : HD + o, v);
    }
  };

  // (a block of the one-tile form runs this ONCE, and as straight-line code: around a loop the compiler computes every uniform value
  //  of the body - some eighty fragment and hand-off row offsets among them - in front of it, and with a hundred scalar registers
  //  that means a lane write into a spill register there and a lane read back at the use, for values that are one scalar add.
  //  gridDim.x <= n_tiles, so a block's first tile always exists.)
  // The multi-tile form keeps the loop, with D, k and the lane opaque inside it: what the body derives from them then depends on the
  // iteration and stays in the body (uniform values in scalar registers, per-lane offsets in vector registers that are free again).
  int64_t tile = blockIdx.x;
  do {
    if constexpr (MULTI) {
      asm volatile("" : "+s"(D), "+s"(k));
      derive();
      asm volatile("" : "+v"(lane));
      derive_lane();
    }
    CVF_STAMP(8);
    // ---- everything the chains need from memory is requested here
    // the block's coefficients in one go: its row of the k x k block (entries past k repeat the last one and are not used) and its
    // entries of the k-vectors, one wait for all of them in front of `alpha` instead of a load and a wait per j
    double crow[CVF_MAX_NETS];
#pragma unroll
    for (int j = 0; j < CVF_MAX_NETS; ++j) crow[j] = coef[k + net * k + (j < k ? j : k - 1)];
    double gS1n = coef[net], gEtn = coef[k + k * k + net];
    double gS1ln = GEN ? 0.0 : coef[2 * k + k * k + net], gS2ln = GEN ? 0.0 : coef[3 * k + k * k + net];
    __builtin_amdgcn_sched_barrier(0);   // (requested HERE, ahead of the vector requests below: the scheduler otherwise sinks them to the pins)
    const bool lagged = !GEN && tile >= args.T;              // (uniform) a tile of lagged partners
    const int64_t t0 = lagged ? tile - args.T : tile;        // the tile of the frames themselves
    const int64_t frame = t0 * CVF_TILE + fo;
    const bool valid = frame < args.B;
    const float wraw = w[valid ? frame : args.B - 1];
    // the frame's y of the k nets that exist: a buffer resource on the tile's k rows, the lane's frame as the one lane offset and the
    // row as the instruction's offset - a row past k lies outside the resource, reads 0 without a request to memory and is not used
    // (with pointers: eight 64-bit vector addresses, and for j >= k the last row requested again)
    float yb[CVF_MAX_NETS];
    if constexpr (MULTI) {   // (the multi-tile form as it was: the resource's four scalar registers, live in its loop, cost it spills)
#pragma unroll
      for (int j = 0; j < CVF_MAX_NETS; ++j) yb[j] = y_tiled[(t0 * k + (j < k ? j : k - 1)) * CVF_TILE + fo];
    } else {
      const URows yrows = urows(y_tiled + t0 * k * CVF_TILE, k * CVF_TILE, fo);
#pragma unroll
      for (int j = 0; j < CVF_MAX_NETS; ++j) yb[j] = yrows.ld(j * CVF_TILE);
    }
    float ylag = 0.0f, wlraw = 0.0f;
    if constexpr (!GEN) {
      ylag = y_tiled[((args.T + t0) * k + net) * CVF_TILE + fo];
      wlraw = args.w_lag[valid ? frame : args.B - 1];
    }
    const URows sv = urows(saved + (tile * k + net) * (int64_t)(kHand<NH>() * NG * 256) + wave * 64, kHand<NH>() * NG * 256 - wave * 64, lane);
    Vec<H, 1> h[NH], e[NH > 1 ? NH - 1 : 1], t[NH];
#pragma unroll
    for (int l = 0; l < NH; ++l) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) h[l].v[rt][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int g = 0; g < NG; ++g) h[l].v[g >> 2][0][g & 3] = sv.ld((l * NG + g) * 256);
    }
    if constexpr (GEN) {
#pragma unroll
      for (int l = 0; l + 1 < NH; ++l) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) e[l].v[rt][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int g = 0; g < NG; ++g) e[l].v[g >> 2][0][g & 3] = sv.ld(((NH + l) * NG + g) * 256);
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) t[0].v[rt][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int g = 0; g < NG; ++g) t[0].v[g >> 2][0][g & 3] = sv.ld(((2 * NH - 1) * NG + g) * 256);
    }
    // the tangent chain's weight fragments W_l, l = 2..NH, with the same round trip (the hbar chain's W_l^T are requested at
    // the top of each reverse step, a phase of outer products ahead of their use)
    HFrag<H> ffr[NH > 1 ? NH - 1 : 1];
    if constexpr (GEN) {
#pragma unroll
      for (int l = 1; l < NH; ++l) load_hfrag_u<H>(ffr[l - 1], pk, L.fh(l));
    }
    const float* f_tile = feat + tile * (int64_t)D * CVF_TILE;
    const float* q_tile = GEN ? q_tiled + (tile * k + net) * (int64_t)D * CVF_TILE : nullptr;
    // ---- per-frame coefficients
    const float wb = valid ? wraw : 0.0f;
    float alpha, gamma = 0.0f;
    float ynet = 0.0f;   // this net's y of the frame (selected, not indexed: yb[] lives in registers)
#pragma unroll
    for (int j = 0; j < CVF_MAX_NETS; ++j)
      if (j == net) ynet = yb[j];
    // (pinned: all of them are in scalar registers here, or each load sinks to its use behind the branch on j < k)
#pragma unroll
    for (int j = 0; j < CVF_MAX_NETS; ++j) asm volatile("" : "+s"(crow[j]));
    asm volatile("" : "+s"(gS1n), "+s"(gEtn));
    if constexpr (!GEN) asm volatile("" : "+s"(gS1ln), "+s"(gS2ln));
    if (GEN || !lagged) {
      double a = gS1n;
#pragma unroll
      for (int j = 0; j < CVF_MAX_NETS; ++j)
        if (j < k) a += (j == net ? 2.0 : 1.0) * crow[j] * (double)yb[j];
      alpha = (float)((double)wb * a);
      if constexpr (GEN) gamma = (float)(2.0 * (double)wb * gEtn);
      else alpha = (float)((double)wb * a - 2.0 * (double)wb * gEtn * ((double)ylag - (double)ynet));   // ... and d/dy of gT sum w (y' - y)^2
    } else {   // a lagged partner: d/dy' of the primed sums and of gT sum w (y' - y)^2
      const double wlg = valid ? (double)wlraw : 0.0;
      alpha = (float)(wlg * (gS1ln + 2.0 * gS2ln * (double)ylag) + 2.0 * (double)wb * gEtn * ((double)ylag - (double)ynet));
    }
    CVF_STAMP(9);
    if constexpr (GEN) {
      // ---- tangent chain: t_1 = gamma s, t_l = W_l tdot_{l-1}
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) t[0].v[rt][0][r] *= gamma;
#pragma unroll
      for (int l = 1; l < NH; ++l) {
        Vec<H, 1> td;
        tangent_of<H, 1>(td, h[l - 1], t[l - 1]);
        init_bias<H, 1>(t[l], nullptr, q);
        hidden_mul<H, 1>(t[l], ffr[l - 1], td);
      }
    }
    CVF_STAMP(11);
    // ---- last layer (1 x H):  W_L += sum alpha h_{NH} + tdot_{NH} ; b_L += sum alpha.  One useful row: no matrix tile - every wave
    // sums its 16 frames in registers and leaves H + 1 partials in PART; they are added and stored behind the first barrier of
    // the reverse sweep (emit_last).
    {
      const float pick = strip_rows<H>([&](int rt, int r) {
        const float hv = h[NH - 1].v[rt][0][r];
        if constexpr (GEN) return fmaf(alpha, hv, (1.0f - hv * hv) * t[NH - 1].v[rt][0][r]);
        else return alpha * hv;
      }, col);
      const float sa = row_sumf16(alpha);
      if (col < NG && rowf < H) PART[wave * (H + 1) + rowf] = pick;
      if (lane == 0) PART[wave * (H + 1) + H] = sa;
    }
    CVF_STAMP(12);
    // ---- reverse sweep
    Vec<H, 1> hbar;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) hbar.v[rt][0][r] = alpha * wl[rt][r];
    // Every step's operands from memory (the transposed weights of a hidden layer; the feature / q rows of the first) are
    // requested one step ahead, BEFORE the step's slab stores: vector memory returns in issue order, and requests issued
    // behind the stores (at the top of the next step) waited for the stores' acknowledgements first.
    HFrag<H> tfl;
    float4 bA[4], bB[4];
    float xs[3] = {0.0f, 0.0f, 0.0f}, qs[3] = {0.0f, 0.0f, 0.0f};   // the frame's features of the strip columns, and its q
    auto request = [&](float4 (&dst)[4], const float* src_tile, int ct) {
      const int i = 16 * ct + row16;
      const float4* p = reinterpret_cast<const float4*>(src_tile + (int64_t)(i < D ? i : D - 1) * CVF_TILE + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[j] = p[4 * j];
    };
    auto request_step = [&](int l) {   // l: compile-time after unrolling
      if (l > 0) {
        load_hfrag_u<H>(tfl, pk, L.th(l));
      } else {
        // (the strip's values first: they are used ahead of bA / bB, and with those eight requests behind them the wait for them
        //  cannot fall on the acknowledgements of the previous step's stores - a wave without a tile there issues none)
        if (strip) {   // wave-uniform
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if (c < nfeat) {
              xs[c] = f_tile[(int64_t)(c0 + c) * CVF_TILE + fo];
              if constexpr (GEN) qs[c] = q_tile[(int64_t)(c0 + c) * CVF_TILE + fo];
            }
        }
        request(bA, f_tile, wave);
        if constexpr (GEN) request(bB, q_tile, wave);
      }
    };
    request_step(NH - 1);
#pragma unroll
    for (int l = NH - 1; l >= 0; --l) {
      CVF_STAMP(13 + (NH - 1 - l));
      // the first layer's B operands come straight from memory (the feature tile + ones row, then q): wave w owns column
      // tile w; k-slot kq of k-step (j, c) is frame 16 j + 4 kq + c, so a lane's sixteen values of one operand row are four
      // 16-byte loads.  The [f ; 1] rows are requested here, q's after the barrier, behind the matrix instructions of the first half.
      Vec<H, 1> zbar, dl;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float hv = h[l].v[rt][0][r];
          const float om = 1.0f - hv * hv;
          if constexpr (GEN) {
            const float ev = (l == NH - 1) ? wl[rt][r] : e[l < NH - 1 ? l : 0].v[rt][0][r];
            const float hb = fmaf(-2.0f * hv * t[l].v[rt][0][r], ev, hbar.v[rt][0][r]);
            dl.v[rt][0][r] = ev * om;
            zbar.v[rt][0][r] = om * hb;
          } else {
            zbar.v[rt][0][r] = om * hbar.v[rt][0][r];
          }
        }
      store_image<H, 1, false>(SA1, zbar, one, lane, fo);
      if constexpr (GEN) {
        const float sc[1] = {l == 0 ? gamma : 1.0f};
        store_image<H, 1, true>(SA2, dl, sc, lane, fo);
      }
      if (l > 0) {
        store_image<H, 1, false>(SB1, h[l - 1], one, lane, fo);
        if constexpr (GEN) {
          Vec<H, 1> td;
          tangent_of<H, 1>(td, h[l - 1], t[l - 1]);
          store_image<H, 1, false>(SB2, td, one, lane, fo);
        }
        __syncthreads();
        // hbar_{l-1} = W_l^T zbar_l  (registers), then the next step's requests, then this step's tiles
        init_bias<H, 1>(hbar, nullptr, q);
        hidden_mul<H, 1>(hbar, tfl, zbar);
        request_step(l - 1);
        if constexpr (TAIL4) {
          // Only tile (0, 0) is full.  The rest of the H x (H + 1) gradient is four jobs of sixteen 4x4x1 blocks each (outer_half44):
          //   R1  rows 16.. x columns 0..15      R2  rows 16.. x columns 16..23 (column groups 16.., 20..; half the blocks idle)
          //   R3a rows 0..15 x columns 16..19    R3b rows 0..15 x columns 20..23 (the bias column and three dead ones)
          // i.e. 32 + 4 x 8 quarter-cost instructions per half instead of 4 x 16.  Role 0 has the full tile, role 1 R1 and R2,
          // role 2 R3a, role 3 R3b; the roles move by two waves from layer to layer, so that over two layers no wave (and no
          // SIMD, if wave w of every resident block sits on the same one) has the full tile twice.
          const int role = (wave + 2 * (l & 1)) & 3;   // wave-uniform
          if (role == 0) {
            emit_tile(l, H, 0, 0, outer2(SA1, SB1, SA2, SB2, 0, 0));
          } else {
            const int g = col >> 2, m = lane & 3;
            const int wo = net_w_off<H, NH>(l, HD), bo = net_b_off<H, NH>(l, HD);
            // one job: the lane's rows of the A and B images -> entry (o, i) in the lanes of DPP row q (rows_sum_scatter)
            auto job = [&](int arow, int brow, int o, int i, bool live) {
              f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
              acc = outer_half44(SA1, arow, SB1, brow, lane, acc);
              if constexpr (GEN) acc = outer_half44(SA2, arow, SB2, brow, lane, acc);
              const float v = rows_sum_scatter(acc);
              asm volatile("" : "+v"(o));   // (opaque, as emit_tile's row)
              live = live && o < H && i <= H;
              emit_entry(live, i < H ? wo + o * H + i : bo + o, v);
            };
            const bool low = role == 1;                       // rows 16.. (R1, then R2) or rows 0..15 (R3a / R3b)
            const int cb = role == 3 ? 20 : 16;               // R3's first column
            job(low ? 16 + m : 4 * g + m, low ? 4 * g + m : cb + m, low ? 16 + q : 4 * g + q, low ? 4 * g + m : cb + m, true);
            if (low) job(16 + m, 16 + 4 * (g & 1) + m, 16 + q, 16 + 4 * (g & 1) + m, g < 2);
          }
        } else {
          for (int pr = wave; pr < RTO * CTH; pr += WPB) {
            const int rt = pr / CTH, ct = pr - rt * CTH;
            emit_tile(l, H, rt, ct, outer2(SA1, SB1, SA2, SB2, rt, ct));
          }
        }
        if (l == NH - 1) emit_last();
        __syncthreads();
      } else {
        // the strip columns (see `strip`): column c of row o is  sum_f zbar[o] x_c (+ gamma dl[o] q_c), the bias column  sum_f zbar[o].
        // SB1's rows below H are free in this step (the B operands are in registers): the waves' partials go there.
        // (unrolled, a wave-uniform branch per column: the wait for x_c / q_c counts the previous step's stores issued behind their
        //  requests instead of waiting for those stores' acknowledgements, which a loop over c made it do)
        if (strip) {   // wave-uniform
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (c < ncol) {   // wave-uniform
              const float xv = c == nfeat ? 1.0f : xs[c < 3 ? c : 2];
              const float qv = c == nfeat ? 0.0f : gamma * qs[c < 3 ? c : 2];
              const float pick = strip_rows<H>([&](int rt, int r) {
                if constexpr (GEN) return fmaf(zbar.v[rt][0][r], xv, dl.v[rt][0][r] * qv);
                else return zbar.v[rt][0][r] * xv;
              }, col);
              if (col < NG && rowf < H) SB1[(wave * H + rowf) * 4 + c] = pick;
            }
          }
        }
        __syncthreads();
        // one half of the contraction of column tile `ct` for the row tiles rt0, rt0 + rstep, ..: A rows from the LDS image
        // `SA`, B rows in registers; columns: features, then the ones (bias) column when `ones`, zeros past it
        // (no MFMA under lane-divergent control flow: operand values are selected per lane, the MFMAs are uniform)
        // The rows of a column tile past D - zeros, and the ones (bias) column at D when `ones` - are put into the operand registers
        // ONCE, when the operand is first used, and only where there are any: a tile that lies below D whole (every tile but the
        // last; wave-uniform) is used as it was loaded.  (Selected inside half0 / tail0 the choice `i < D ? b : pad` was made per
        // matrix instruction: 16 selects per row tile and half.)
        auto pad_rows = [&](float4 (&b)[4], int ct, bool ones) {
          if (!MULTI && 16 * ct + 16 <= D) return;   // wave-uniform (the multi-tile form selects on every tile: the branch costs its loop two spilled scalar registers)
          const int i = 16 * ct + row16;
          const float pad = (ones && i == D) ? 1.0f : 0.0f;
#pragma unroll
          for (int j = 0; j < 4; ++j) b[j] = float4{i < D ? b[j].x : pad, i < D ? b[j].y : pad, i < D ? b[j].z : pad, i < D ? b[j].w : pad};
        };
        auto half0 = [&](f32x4 (&acc)[RTO], const float* SA, const float4 (&b)[4], int rt0, int rstep) {
#pragma unroll
          for (int rt = 0; rt < RTO; ++rt) {
            if (rt >= rt0 && (rt - rt0) % rstep == 0) {
              const float4* a1 = reinterpret_cast<const float4*>(SA + (16 * rt + row16) * kPitch + 4 * q);
              float4 av[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) av[j] = a1[4 * j];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                acc[rt] = mfma4(av[j].x, b[j].x, acc[rt]);
                acc[rt] = mfma4(av[j].y, b[j].y, acc[rt]);
                acc[rt] = mfma4(av[j].z, b[j].z, acc[rt]);
                acc[rt] = mfma4(av[j].w, b[j].w, acc[rt]);
              }
            }
          }
        };
        // matrix column tiles beyond the first four are dealt by (column tile, row tile) pairs: pair p -> wave p % 4
        const int extra = (CTM - WPB) * RTO;
        f32x4 acc[RTO];
#pragma unroll
        for (int rt = 0; rt < RTO; ++rt) acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // TAIL4: the same half for the 1..4 useful rows of row tile 1 as sixteen 4x4x1 blocks (rows_sum_scatter, ef16_common.hpp).
        // The B registers are read as they are: lane (c, q) holds feature 16 ct + c at frames 16 j + 4 q + e, i.e. column lane & 3
        // of block (q, c >> 2); the A operand of that block is rows 16 + (lane & 3) at the same frames.
        auto tail0 = [&](f32x4& tacc, const float* SA, const float4 (&b)[4]) {
          const float4* a1 = reinterpret_cast<const float4*>(SA + (16 + (lane & 3)) * kPitch + 4 * q);
          float4 av[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) av[j] = a1[4 * j];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            tacc = mfma1(av[j].x, b[j].x, tacc);
            tacc = mfma1(av[j].y, b[j].y, tacc);
            tacc = mfma1(av[j].z, b[j].z, tacc);
            tacc = mfma1(av[j].w, b[j].w, tacc);
          }
        };
        if (wave < CTM) {   // wave-uniform
          f32x4 tacc = {0.0f, 0.0f, 0.0f, 0.0f};
          pad_rows(bA, wave, true);
          half0(acc, SA1, bA, 0, TAIL4 ? RTO : 1);
          if constexpr (TAIL4) tail0(tacc, SA1, bA);
          if (wave < extra) request(bA, f_tile, WPB + wave / RTO);   // the extra pair's rows, behind the second half
          if constexpr (GEN) {
            pad_rows(bB, wave, false);
            half0(acc, SA2, bB, 0, TAIL4 ? RTO : 1);
            if constexpr (TAIL4) tail0(tacc, SA2, bB);
          }
#pragma unroll
          for (int rt = 0; rt < (TAIL4 ? 1 : RTO); ++rt) emit_tile(0, D, rt, wave, acc[rt]);
          if constexpr (TAIL4) {   // DPP row q holds row 16 + q of the lane's column
            const float v = rows_sum_scatter(tacc);
            int o = 16 + q;
            asm volatile("" : "+v"(o));
            const int i = 16 * wave + row16;
            const bool isw = o < H && i < D, isb = o < H && i == D;
            emit_entry(isw || isb, isw ? o * D + i : HD + (o < H ? o : 0), v);
          }
        }
        for (int pr = wave; pr < extra; pr += WPB) {
          const int ct = WPB + pr / RTO, rt = pr % RTO;
          if (pr != wave || wave >= CTM) request(bA, f_tile, ct);
          if constexpr (GEN) request(bB, q_tile, ct);
#pragma unroll
          for (int r_ = 0; r_ < RTO; ++r_) acc[r_] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          pad_rows(bA, ct, true);
          half0(acc, SA1, bA, rt, RTO);
          if constexpr (GEN) {
            pad_rows(bB, ct, false);
            half0(acc, SA2, bB, rt, RTO);
          }
#pragma unroll
          for (int r_ = 0; r_ < RTO; ++r_)
            if (r_ == rt) emit_tile(0, D, r_, ct, acc[r_]);
        }
        emit_strip();
        if (NH == 1) emit_last();
        __syncthreads();
      }
    }
    tile += gridDim.x;
  } while (MULTI && tile < args.n_tiles);
  CVF_STAMP(17);
  if (MULTI) {   // flush this block's partial gradient of `net` into its slab row
    __syncthreads();
    for (int i = tid; i < gspan; i += NT) out[i] = GI[i];
  }
  // one gradient per optimiser step: advance the step counter read by the Adam that follows
  if (step != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *step += 1;
  CVF_STAMP(18);
}

}  // namespace

extern "C" int64_t cvf_ef16_backward_slab_rows(int64_t n_tiles) { return n_tiles < 1024 ? n_tiles : 1024; }

static int ef16_backward_impl(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, const float* packed,
                              int64_t B, const float* w, const float* w_lag, const float* feat_tiled, const float* y_tiled,
                              const float* q_tiled, const double* coef, float* slab, int32_t* step_count, const float* saved,
                              void* stream) {
  const bool transfer = cfg != nullptr && cfg->lag_idx > 0;
  CVF_REQUIRE(cfg && mlp && theta && packed && w && feat_tiled && y_tiled && (transfer ? w_lag != nullptr : q_tiled != nullptr) && coef &&
              slab && saved && B > 0, "cvf_ef16_backward: bad argument");
  CVF_REQUIRE(cfg->k == mlp->n_nets, "cvf_ef16_backward: cfg.k must equal the number of nets");
  int H, NH;
  CVF_REQUIRE(ef16_shape(mlp, &H, &NH), "cvf_ef16_backward: unsupported net shape");
  CVF_REQUIRE(mlp->dims[0] <= 8 * 16 - 1, "cvf_ef16_backward: first layer wider than the column-tile schedule covers");
  // the LDS gradient image relies on each net's parameters being one contiguous run of the flat buffer
  const int span = mlp->b_off[0][NH] + 1 - mlp->w_off[0][0];
  int covered = 0;
  for (int n = 0; n < mlp->n_nets; ++n) {
    CVF_REQUIRE(mlp->b_off[n][NH] + 1 - mlp->w_off[n][0] == span, "cvf_ef16_backward: nets are not laid out contiguously");
    for (int l = 0; l <= NH; ++l)
      CVF_REQUIRE(mlp->w_off[n][l] >= mlp->w_off[n][0] && mlp->b_off[n][l] < mlp->w_off[n][0] + span,
                  "cvf_ef16_backward: nets are not laid out contiguously");
    covered += span;
  }
  CVF_REQUIRE(covered == mlp->n_params, "cvf_ef16_backward: flat buffer holds parameters outside the nets");
  // ... and the kernel derives a layer's offsets from its net's base: per layer the weight, then the bias, layer after layer (the order
  // of model.parameters(), which is what every caller passes)
  for (int n = 0; n < mlp->n_nets; ++n)
    for (int l = 0; l <= NH; ++l) {
      CVF_REQUIRE(mlp->b_off[n][l] == mlp->w_off[n][l] + mlp->dims[l] * mlp->dims[l + 1],
                  "cvf_ef16_backward: net %d, layer %d: the bias does not follow the weight", n, l);
      CVF_REQUIRE(l == NH || mlp->w_off[n][l + 1] == mlp->b_off[n][l] + mlp->dims[l + 1],
                  "cvf_ef16_backward: net %d: layer %d does not follow layer %d", n, l + 1, l);
    }
  Back16Nets nets;
  nets.D = mlp->dims[0];
  nets.n_params = mlp->n_params;
  for (int n = 0; n < CVF_MAX_NETS; ++n) nets.base[n] = n < mlp->n_nets ? mlp->w_off[n][0] : 0;
  Back16Args a;
  a.k = cfg->k;
  a.B = B;
  a.T = cvf_ntiles(B);
  a.n_tiles = transfer ? 2 * a.T : a.T;
  a.w_lag = w_lag;
  const int64_t G = cvf_ef16_backward_slab_rows(a.n_tiles);
  const bool launched = ef16_dispatch(H, NH, [&](auto h_, auto nh_) {
    constexpr int kH = decltype(h_)::value, kNH = decltype(nh_)::value;
    auto go = [&](auto kernel, size_t lds) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)G, cfg->k), dim3(256), lds, (hipStream_t)stream, a, nets, theta, packed, w, feat_tiled,
                         y_tiled, q_tiled, coef, slab, step_count, saved);
    };
    const size_t gi = (size_t)span * sizeof(float);
    // a.n_tiles > G: blocks walk several tiles (partial gradient in LDS, flushed once); else one tile per block, every
    // gradient tile goes straight to the block's slab row
    if (transfer) {
      if (a.n_tiles > G) go(ef16_back_kernel<kH, kNH, true, false>, gi);
      else go(ef16_back_kernel<kH, kNH, false, false>, 0);
    } else {
      if (a.n_tiles > G) go(ef16_back_kernel<kH, kNH, true, true>, gi);
      else go(ef16_back_kernel<kH, kNH, false, true>, 0);
    }
  });
  CVF_REQUIRE(launched, "cvf_ef16_backward: no kernel instance for hidden width %d x %d layers", H, NH);
  return cvf_check_launch("ef16_back_kernel");
}

extern "C" int cvf_ef16_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, const float* packed,
                                 int64_t B, const float* w, const float* feat_tiled, const float* y_tiled, const float* q_tiled,
                                 const double* coef, float* slab, int32_t* step_count, const float* saved, void* stream) {
  CVF_REQUIRE(cfg && cfg->lag_idx == 0, "cvf_ef16_backward: generator mode (transfer-operator mode: cvf_ef16_backward_transfer)");
  return ef16_backward_impl(cfg, mlp, theta, packed, B, w, nullptr, feat_tiled, y_tiled, q_tiled, coef, slab, step_count, saved, stream);
}


extern "C" int cvf_ef16_backward_transfer(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, const float* packed,
                                          int64_t B, const float* w, const float* w_lag, const float* feat_tiled,
                                          const float* y_tiled, const double* coef, float* slab, int32_t* step_count,
                                          const float* saved, void* stream) {
  CVF_REQUIRE(cfg && cfg->lag_idx > 0, "cvf_ef16_backward_transfer: transfer-operator mode (cfg.lag_idx > 0)");
  return ef16_backward_impl(cfg, mlp, theta, packed, B, w, w_lag, feat_tiled, y_tiled, nullptr, coef, slab, step_count, saved, stream);
}