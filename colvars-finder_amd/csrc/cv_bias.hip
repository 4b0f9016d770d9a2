// Bias energy and forces along a trained CV in ONE launch, in the MD engine's own arrays (cvf_cv_*_bias_*).
// The two one-launch kernels of csrc/cv_frame_kernel.hpp (one wave per frame) and csrc/cv_frame_large_kernel.hpp (one workgroup per
// frame) under another IO policy - their arithmetic from the coordinates in LDS to the gradient image is the namesakes', text for
// text:
//
//   frame   atom a of replica b from x_all[b x_frame_stride + atom_index[a] atom_stride + c] (cvf_md_layout; NULL: dense)
//   seed    once xi is in LDS, lane i < k sums its terms' U_t(xi_i) and U_t'(xi_i) in term order (cvf_bias.hpp; of a joint grid
//           term on (cv, cv2) lane cv takes U and dU/dxi_cv, lane cv2 dU/dxi_cv2: DESIGN.md section 4.19), writes du_rows,
//           stores -du_i and its share of U to 2 k LDS floats; behind a barrier thread 0 adds the k shares in index order into
//           u_rows, and the contracted sweep (coef form: one cotangent row) reads its seed from the LDS row instead of a global coef
//   force   f_all[b f_frame_stride + atom_index[a] atom_stride + c] += the row, each element by the one thread that owns it
//
// No atomics, no scratch, no aux; the bias table is read at launch time.
//
// Periodic cells (cvf_cv_*_bias_*_cell_eval, cvf_md_make_whole; the rule: csrc/cvf_cell.hpp): the same two
// bodies under IO policies with kCell set - the wrapped atoms are made whole along the CV's atom order before anything reads them
// (wave kernel: in place on the frame in LDS, the image counts through a wave scan; workgroup kernel: a prologue leaves every atom's
// summed image triple as one LDS word, applied where an atom is read), and the virial sum_a r_a (x) f_a is taken from the whole
// positions and the force row just before it is stored, in a fixed order.
#include "cv_frame_kernel.hpp"
#include "cv_frame_large_kernel.hpp"
#include "cvf_bias.hpp"
#include "cvf_cell.hpp"

namespace {

// the engine's arrays, as the kernels take them (a NULL cvf_md_layout: stride 3, frame strides n_coord, no index)
struct MdArgs {
  const float* x_all;
  float* f_all;
  const int32_t* atom_index;
  int64_t x_frame_stride, f_frame_stride;
  int32_t atom_stride;
  float* u_rows;
  float* du_rows;
};

__device__ __forceinline__ int64_t md_atom(const MdArgs& md, int a) {
  return (int64_t)(md.atom_index != nullptr ? md.atom_index[a] : a) * md.atom_stride;
}

// the seed row of the frame in spare[0..k) (spare holds 2 k floats), u_rows and du_rows written; every thread of the frame calls it
__device__ __forceinline__ const float* bias_seeds(const cvf_bias_desc& bias, const MdArgs& md, float* spare, const float* top,
                                                   int64_t frame, int k, int idx) {
  if (idx < k) {
    float u, du;
    cvf_bias_cv_eval(bias, idx, top, &u, &du);   // (the whole row: a joint grid term reads two of its k values)
    spare[idx] = -du;
    spare[k + idx] = u;
    if (md.du_rows != nullptr) md.du_rows[frame * k + idx] = du;
  }
  lds_barrier();
  if (idx == 0) {
    float U = spare[k];
    for (int i = 1; i < k; ++i) U += spare[k + i];
    md.u_rows[frame] = U;
  }
  return spare;
}

// the cell and the virial rows, as the cell kernels take them (cvf_md_cell)
struct CellArgs {
  const float* cell;
  int64_t cell_stride;
  float* virial;
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_movi(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
// inclusive scan over the wave's 64 lanes on the DPP path of wave_sum (cvf_common.hpp): a scan inside each row of 16 lanes, then
// row_bcast:15 and row_bcast:31 add the totals of the rows before.  Integers: exact in any association.
__device__ __forceinline__ int wave_scan_i(int v) {
  v += dpp_movi<0x111, 0xf>(v);
  v += dpp_movi<0x112, 0xf>(v);
  v += dpp_movi<0x114, 0xf>(v);
  v += dpp_movi<0x118, 0xf>(v);
  v += dpp_movi<0x142, 0xa>(v);
  v += dpp_movi<0x143, 0xc>(v);
  return v;
}

// The summed image triple N_a of every atom of a frame, 256 threads: chunks of kThreads atoms with a carried total; in a chunk the
// wave scan, the four waves' totals through `red` (12 ints) in index order.  at(a): the wrapped atom a (three floats);
// emit(a, word): N_a packed (cvf_cell_pack), called once per atom by the thread that owns it.  Every thread of the workgroup calls it.
// The atoms of kCellUnroll chunks are read together, unconditionally (an index clamped into the frame): a chunk's reads are two
// dependent global loads (atom_index, then the position), and behind a chunk's barriers they would be paid once per chunk, in series.
constexpr int kCellUnroll = 4;
template <class At, class Emit>
__device__ __forceinline__ void cell_group_scan(const CvfCell& c, int n_atoms, int tid, int* red, At at, Emit emit) {
  const int lane = tid & 63, wave = tid >> 6;
  int carry[3] = {0, 0, 0};
  for (int a0 = 0; a0 < n_atoms; a0 += kCellUnroll * cvfl::kThreads) {
    float d[kCellUnroll][3];
#pragma unroll
    for (int u = 0; u < kCellUnroll; ++u) {
      const int a = a0 + u * cvfl::kThreads + tid;
      const int ac = a < n_atoms ? a : n_atoms - 1, ap = ac > 0 ? ac - 1 : 0;
      const float* p = at(ac);
      const float* q = at(ap);
      d[u][0] = p[0] - q[0];
      d[u][1] = p[1] - q[1];
      d[u][2] = p[2] - q[2];
    }
#pragma unroll
    for (int u = 0; u < kCellUnroll; ++u) {
      const int a = a0 + u * cvfl::kThreads + tid;
      if (a0 + u * cvfl::kThreads >= n_atoms) break;   // (uniform)
      const bool on = a < n_atoms;
      int n[3] = {0, 0, 0};
      if (on && a > 0) cvf_cell_image(c, d[u][0], d[u][1], d[u][2], &n[0], &n[1], &n[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        n[i] = wave_scan_i(n[i]);
        if (lane == 63) red[wave * 3 + i] = n[i];
      }
      lds_barrier();
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < cvfl::kWaves; ++w) {
          const int t = red[w * 3 + i];
          before += w < wave ? t : 0;
          total += t;
        }
        n[i] += carry[i] + before;
        carry[i] += total;
      }
      if (on) emit(a, cvf_cell_pack(n[0], n[1], n[2]));
      lds_barrier();   // (the next chunk overwrites red)
    }
  }
}

struct WaveIO {
  const cvf_bias_desc& bias;
  const MdArgs& md;
  static constexpr bool kCell = false;
  __device__ __forceinline__ float load(int64_t frame, int, int j) const {
    const int a = j / 3;
    return md.x_all[frame * md.x_frame_stride + md_atom(md, a) + (j - 3 * a)];
  }
  __device__ __forceinline__ const float* seeds(float* spare, const float* top, int64_t frame, int k, int lane) const {
    return bias_seeds(bias, md, spare, top, frame, k, lane);
  }
  __device__ __forceinline__ void store(int64_t frame, int, int, int e, float v) const {   // (one row: e is the coordinate)
    const int a = e / 3;
    md.f_all[frame * md.f_frame_stride + md_atom(md, a) + (e - 3 * a)] += v;
  }
};

struct WaveCellIO : WaveIO {
  const CellArgs& cl;
  static constexpr bool kCell = true;
  __device__ __forceinline__ WaveCellIO(const cvf_bias_desc& b, const MdArgs& m, const CellArgs& c) : WaveIO{b, m}, cl(c) {}
  // the staged frame made whole in place: lane = atom, chunks of 64 atoms with a carried total (a CVF_PP_IDENTITY frame may hold more)
  __device__ __forceinline__ void whole(float* xs, int nc, int64_t frame, int lane) const {
    if (cl.cell == nullptr) return;
    CvfCell c = cvf_cell_load(cl.cell + frame * cl.cell_stride);
    // (uniform values, kept in vector registers: the body around this hook is what runs out of scalar ones)
    asm volatile("" : "+v"(c.ax), "+v"(c.bx), "+v"(c.by), "+v"(c.cx), "+v"(c.cy), "+v"(c.cz));
    const int na = nc / 3;
    int carry[3] = {0, 0, 0};
    float last[3] = {0.0f, 0.0f, 0.0f};   // the wrapped last atom of the chunk before
    for (int a0 = 0; a0 < na; a0 += CVF_WAVE) {
      const int a = a0 + lane;
      const bool on = a < na;
      float x[3] = {0.0f, 0.0f, 0.0f}, q[3] = {last[0], last[1], last[2]};
      if (on) {
        x[0] = xs[3 * a]; x[1] = xs[3 * a + 1]; x[2] = xs[3 * a + 2];
        if (lane > 0) { q[0] = xs[3 * a - 3]; q[1] = xs[3 * a - 2]; q[2] = xs[3 * a - 1]; }
      }
      int n[3] = {0, 0, 0};
      if (on && a > 0) cvf_cell_image(c, x[0] - q[0], x[1] - q[1], x[2] - q[2], &n[0], &n[1], &n[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        n[i] = carry[i] + wave_scan_i(n[i]);
        carry[i] = __builtin_amdgcn_readlane(n[i], 63);
        last[i] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x[i]), 63));
      }
      if (on) {   // (every lane has read its neighbour above: one wave, LDS in program order)
        float w[3];
        cvf_cell_whole(c, cvf_cell_pack(n[0], n[1], n[2]), x, w);
        xs[3 * a] = w[0]; xs[3 * a + 1] = w[1]; xs[3 * a + 2] = w[2];
      }
    }
  }
  // the virial of the frame from the whole positions in xs and the force row about to be added: lane = atom, then wave_sumf
  __device__ __forceinline__ void finish(const float* xs, const float* grad, int nc, int64_t frame, int lane) const {
    if (cl.virial == nullptr) return;
    float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = lane; a < nc / 3; a += CVF_WAVE) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[3 * i + j] = fmaf(xs[3 * a + i], grad[3 * a + j], v[3 * i + j]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float t = wave_sumf(v[i]);
      if (lane == 0) cl.virial[frame * 9 + i] = t;
    }
  }
};

template <bool SHARED>
__global__ __launch_bounds__(64) void cv_frame_bias_cell_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, cvfr::FrLayout lay, cvf_bias_desc bias,
                                                                 MdArgs md, CellArgs cl, const float* __restrict__ theta,
                                                                 float* __restrict__ xi_rows) {
  // (the three words of cl are used at the two ends of the body: as vector registers they leave its scalar ones alone)
  asm volatile("" : "+v"(cl.cell), "+v"(cl.cell_stride), "+v"(cl.virial));
  cvfr::cv_frame_body<SHARED>(mlp, pp, lay, theta, xi_rows, true, WaveCellIO(bias, md, cl));
}

template <bool SHARED>
__global__ __launch_bounds__(64) void cv_frame_bias_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, cvfr::FrLayout lay, cvf_bias_desc bias,
                                                            MdArgs md, const float* __restrict__ theta, float* __restrict__ xi_rows) {
  cvfr::cv_frame_body<SHARED>(mlp, pp, lay, theta, xi_rows, true, WaveIO{bias, md});
}

struct GroupIO {
  const cvf_bias_desc& bias;
  const MdArgs& md;
  __device__ __forceinline__ const float* atom(int64_t frame, int a) const { return md.x_all + frame * md.x_frame_stride + md_atom(md, a); }
  __device__ __forceinline__ const float* seeds(float* spare, const float* top, int64_t frame, int k, int tid) const {
    return bias_seeds(bias, md, spare, top, frame, k, tid);
  }
  __device__ __forceinline__ float* out(int64_t frame, int, int) const { return md.f_all + frame * md.f_frame_stride; }
  static constexpr bool kCell = false;
  static constexpr bool kByAtom = true;   // (an engine's atom is three adjacent floats: one index load, three accumulations in flight)
  __device__ __forceinline__ void put_atom(float* rows, int, int, int A, V3 v) const {   // (one row)
    float* p = rows + md_atom(md, A);
    const float f0 = p[0], f1 = p[1], f2 = p[2];
    p[0] = f0 + v.x;
    p[1] = f1 + v.y;
    p[2] = f2 + v.z;
  }
};

struct GroupCellIO : GroupIO {
  const CellArgs& cl;
  static constexpr bool kCell = true;
  // per thread: the frame's cell (uniform), the image words, the partial virial of the atoms this thread stores
  mutable CvfCell c;
  mutable const uint32_t* words;
  mutable float vir[9];
  __device__ __forceinline__ GroupCellIO(const cvf_bias_desc& b, const MdArgs& m, const CellArgs& a)
      : GroupIO{b, m}, cl(a), c{}, words(nullptr), vir{0, 0, 0, 0, 0, 0, 0, 0, 0} {}
  __device__ __forceinline__ void prologue(uint32_t* w, float* red, int64_t frame, int n_atoms, int tid) const {
    words = w;
    if (cl.cell == nullptr) return;
    c = cvf_cell_load(cl.cell + frame * cl.cell_stride);
    cell_group_scan(c, n_atoms, tid, reinterpret_cast<int*>(red), [&](int a) { return atom(frame, a); },
                    [&](int a, uint32_t word) { w[a] = word; });
  }
  __device__ __forceinline__ V3 whole(const uint32_t* w, int64_t frame, int a) const {
    const float* p = atom(frame, a);
    if (cl.cell == nullptr) return v3(p[0], p[1], p[2]);
    const float x[3] = {p[0], p[1], p[2]};
    float o[3];
    cvf_cell_whole(c, w[a], x, o);
    return v3(o[0], o[1], o[2]);
  }
  // The virial relies on the contracted launch: ONE row (kk == 1) and so one pass, one put_atom per atom and one finish per frame.  A
  // policy with k rows would have to keep the rows' partial sums apart and write once, behind the last pass.  The atom is read again
  // (an L2 hit) rather than carried from the body, which does not hold it at this point; the frame is the workgroup's, blockIdx.x,
  // as in the body (put_atom is not passed it).
  __device__ __forceinline__ void put_atom(float* rows, int nc, int ii, int A, V3 v) const {   // (one row)
    GroupIO::put_atom(rows, nc, ii, A, v);
    if (cl.virial == nullptr) return;
    const V3 r = whole(words, (int64_t)blockIdx.x, A);
    vir[0] = fmaf(r.x, v.x, vir[0]); vir[1] = fmaf(r.x, v.y, vir[1]); vir[2] = fmaf(r.x, v.z, vir[2]);
    vir[3] = fmaf(r.y, v.x, vir[3]); vir[4] = fmaf(r.y, v.y, vir[4]); vir[5] = fmaf(r.y, v.z, vir[5]);
    vir[6] = fmaf(r.z, v.x, vir[6]); vir[7] = fmaf(r.z, v.y, vir[7]); vir[8] = fmaf(r.z, v.z, vir[8]);
  }
  // the threads' partial virials: wave_sumf, then the four waves in index order through red ([wave][12] floats)
  __device__ __forceinline__ void finish(float* red, int64_t frame, int tid) const {
    if (cl.virial == nullptr) return;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float t = wave_sumf(vir[i]);
      if (lane == 0) red[wave * 12 + i] = t;
    }
    lds_barrier();
    if (tid < 9) {
      float t = red[tid];
#pragma unroll
      for (int w = 1; w < cvfl::kWaves; ++w) t += red[w * 12 + tid];
      cl.virial[frame * 9 + tid] = t;
    }
  }
};

template <int MODE, bool SHARED>
__global__ __launch_bounds__(cvfl::kThreads) void cv_frame_large_bias_cell_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, cvfl::LgLayout lay,
                                                                                  cvf_bias_desc bias, MdArgs md, CellArgs cl,
                                                                                  const float* __restrict__ theta, float* __restrict__ xi_rows) {
  cvfl::cv_frame_large_body<false, MODE, SHARED>(mlp, pp, lay, theta, xi_rows, true, GroupCellIO(bias, md, cl));
}

// cvf_md_make_whole: one workgroup per frame, the gather through the layout and the chain of csrc/cvf_cell.hpp in one launch
__global__ __launch_bounds__(cvfl::kThreads) void md_make_whole_kernel(MdArgs md, CellArgs cl, int n_atoms, float* __restrict__ x_whole) {
  __shared__ int red[cvfl::kWaves * 3];
  const int64_t frame = blockIdx.x;
  const CvfCell c = cvf_cell_load(cl.cell + frame * cl.cell_stride);
  const float* xf = md.x_all + frame * md.x_frame_stride;
  float* out = x_whole + frame * 3 * (int64_t)n_atoms;
  cell_group_scan(c, n_atoms, threadIdx.x, red, [&](int a) { return xf + md_atom(md, a); },
                  [&](int a, uint32_t word) {
                    const float* p = xf + md_atom(md, a);
                    const float x[3] = {p[0], p[1], p[2]};
                    float o[3];
                    cvf_cell_whole(c, word, x, o);
                    out[3 * (int64_t)a] = o[0];
                    out[3 * (int64_t)a + 1] = o[1];
                    out[3 * (int64_t)a + 2] = o[2];
                  });
}

template <int MODE, bool SHARED>
__global__ __launch_bounds__(cvfl::kThreads) void cv_frame_large_bias_kernel(cvf_mlp_desc mlp, cvf_pp_desc pp, cvfl::LgLayout lay,
                                                                             cvf_bias_desc bias, MdArgs md, const float* __restrict__ theta,
                                                                             float* __restrict__ xi_rows) {
  cvfl::cv_frame_large_body<false, MODE, SHARED>(mlp, pp, lay, theta, xi_rows, true, GroupIO{bias, md});
}

// nullptr and *md filled, or why the call is refused (the model's own check has passed: k CVs, pp is a coordinate mode)
const char* md_why(const cvf_pp_desc* pp, int k, const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* theta, const float* x_all,
                   int64_t B, float* xi_rows, float* u_rows, float* du_rows, float* f_all, MdArgs* md) {
  static thread_local char buf[240];
  const char* why = cvf_bias_why(bias, k, buf, sizeof buf);
  if (why != nullptr) return why;
#define CVFB_NO(...)                       \
  do {                                     \
    snprintf(buf, sizeof buf, __VA_ARGS__); \
    return buf;                            \
  } while (0)
  if (B < 0 || B > 0x7fffffff) CVFB_NO("B = %lld frames (one call takes 0 to 2^31 - 1)", (long long)B);
  const int nc = pp->n_coord;
  MdArgs m = {x_all, f_all, nullptr, nc, nc, 3, u_rows, du_rows};
  if (layout != nullptr) {
    if (layout->atom_stride < 3) CVFB_NO("layout.atom_stride = %d: an atom has at least 3 floats", layout->atom_stride);
    if (layout->x_frame_stride < 0 || layout->f_frame_stride < 0)
      CVFB_NO("layout.x_frame_stride = %lld, layout.f_frame_stride = %lld: negative", (long long)layout->x_frame_stride, (long long)layout->f_frame_stride);
    if (layout->atom_index != nullptr && nc % 3 != 0)
      CVFB_NO("layout.atom_index with n_coord = %d%s: an atom index needs frames of whole atoms (n_coord %% 3 == 0)", nc,
              pp->mode == CVF_PP_IDENTITY ? " (CVF_PP_IDENTITY)" : "");
    if (B > 1) {
      // Two frames' force elements must not coincide: each is accumulated by one thread of its own workgroup.  n_coord / 3 distinct
      // atoms reach at least atom n_coord / 3 - 1, so a frame of forces spans at least `extent` floats (exactly that without an
      // index; with one the true extent is the caller's knowledge).  x_all is only read: frames may overlap or repeat there.
      const int64_t extent = (int64_t)((nc + 2) / 3 - 1) * layout->atom_stride + (nc % 3 == 0 ? 3 : nc % 3);
      if (layout->f_frame_stride < extent)
        CVFB_NO("layout.f_frame_stride = %lld with B = %lld: the force frames of the batch overlap (one frame spans at least %lld floats)",
                (long long)layout->f_frame_stride, (long long)B, (long long)extent);
    }
    m.atom_index = layout->atom_index;
    m.atom_stride = layout->atom_stride;
    m.x_frame_stride = layout->x_frame_stride;
    m.f_frame_stride = layout->f_frame_stride;
  }
  if (B > 0 && !(theta && x_all && xi_rows && u_rows && f_all)) CVFB_NO("null argument");
#undef CVFB_NO
  *md = m;
  return nullptr;
}

// floats of LDS that a cell launch of the workgroup kernel keeps for the image counts
int64_t cell_words(const cvf_pp_desc* pp) { return pp->n_coord > 0 ? pp->n_coord / 3 : 0; }

// nullptr, or why a model's frames cannot go with a cell or a virial (the model's own check has passed)
const char* whole_atoms_why(const cvf_pp_desc* pp) {
  static thread_local char buf[200];
  if (pp->n_coord % 3 == 0) return nullptr;
  snprintf(buf, sizeof buf, "cvf_md_cell with n_coord = %d%s: a cell and a virial need frames of whole atoms (n_coord %% 3 == 0)", pp->n_coord,
           pp->mode == CVF_PP_IDENTITY ? " (CVF_PP_IDENTITY)" : "");
  return buf;
}

// nullptr and *cl filled, or why the cell call is refused (cell == nullptr: the plain call, *cl empty)
const char* cell_why(const cvf_pp_desc* pp, const cvf_md_cell* cell, CellArgs* cl) {
  static thread_local char buf[200];
  *cl = CellArgs{nullptr, 0, nullptr};
  if (cell == nullptr) return nullptr;
  const char* atoms = whole_atoms_why(pp);
  if (atoms != nullptr) return atoms;
  if (cell->cell_frame_stride < 0) {
    snprintf(buf, sizeof buf, "cell.cell_frame_stride = %lld: negative", (long long)cell->cell_frame_stride);
    return buf;
  }
  if (cell->cell == nullptr && cell->virial_rows == nullptr) return "cell.cell and cell.virial_rows are both NULL: take the call without a cell";
  *cl = CellArgs{cell->cell, cell->cell_frame_stride, cell->virial_rows};
  return nullptr;
}

template <bool SHARED>
int wave_eval(const char* name, const cvf_mlp_desc* mlp, const float* theta, int cut, const cvf_pp_desc* pp, const cvf_bias_desc* bias,
              const cvf_md_layout* layout, const float* x_all, int64_t B, float* xi_rows, float* u_rows, float* du_rows, float* f_all,
              void* stream, const cvf_md_cell* cell = nullptr, bool with_cell = false) {
  CVF_REQUIRE(!with_cell || cell != nullptr, "%s: cell is NULL (the call without a cell is %s)", name, SHARED ? "cvf_cv_frame_bias_shared_eval" : "cvf_cv_frame_bias_eval");
  cvfr::FrLayout lay;
  const char* why = SHARED ? cvfr::cvfr_shared_why(mlp, cut, pp, &lay, "cvf_cv_frame_bias_eval", 2) : cvfr::cvfr_why(mlp, cut, pp, &lay, 0, 2);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  MdArgs md;
  why = md_why(pp, lay.k, bias, layout, theta, x_all, B, xi_rows, u_rows, du_rows, f_all, &md);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  CellArgs cl;
  why = cell_why(pp, cell, &cl);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  if (B == 0) return 0;
  const size_t lds = ((size_t)lay.total + 2 * (size_t)lay.k) * sizeof(float);
  if (cell != nullptr) {
    if (lds > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void*)cv_frame_bias_cell_kernel<SHARED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      CVF_REQUIRE(e == hipSuccess, "%s: %zu bytes of dynamic LDS: %s", name, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(cv_frame_bias_cell_kernel<SHARED>, dim3((unsigned)B), dim3(CVF_WAVE), lds, (hipStream_t)stream, *mlp, *pp, lay, *bias, md,
                       cl, theta, xi_rows);
    return cvf_check_launch("cv_frame_bias_cell_kernel");
  }
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)cv_frame_bias_kernel<SHARED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    CVF_REQUIRE(e == hipSuccess, "%s: %zu bytes of dynamic LDS: %s", name, lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(cv_frame_bias_kernel<SHARED>, dim3((unsigned)B), dim3(CVF_WAVE), lds, (hipStream_t)stream, *mlp, *pp, lay, *bias, md,
                     theta, xi_rows);
  return cvf_check_launch("cv_frame_bias_kernel");
}

template <bool SHARED>
int group_eval(const char* name, const cvf_mlp_desc* mlp, const float* theta, int cut, const cvf_pp_desc* pp, const cvf_bias_desc* bias,
               const cvf_md_layout* layout, const float* x_all, int64_t B, float* xi_rows, float* u_rows, float* du_rows, float* f_all,
               void* stream, const cvf_md_cell* cell = nullptr, bool with_cell = false) {
  CVF_REQUIRE(!with_cell || cell != nullptr, "%s: cell is NULL (the call without a cell is %s)", name,
              SHARED ? "cvf_cv_frame_large_bias_shared_eval" : "cvf_cv_frame_large_bias_eval");
  cvfl::LgLayout lay;
  const int64_t words = cell != nullptr && pp != nullptr ? cell_words(pp) : 0;   // the image counts' LDS: one word per atom
  const char* why = SHARED ? cvfl::cvfl_shared_why(mlp, cut, pp, &lay, "cvf_cv_frame_large_bias_eval", words) : cvfl::cvfl_why(mlp, cut, pp, &lay, 0, words);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  MdArgs md;
  why = md_why(pp, lay.k, bias, layout, theta, x_all, B, xi_rows, u_rows, du_rows, f_all, &md);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  CellArgs cl;
  why = cell_why(pp, cell, &cl);
  CVF_REQUIRE(why == nullptr, "%s: %s", name, why);
  if (B == 0) return 0;
  const size_t lds = ((size_t)lay.rows + 3 * (size_t)pp->n_ref + (size_t)words) * sizeof(float);   // one cotangent row (the seeds sit in the moments' LDS)
  const int mode = pp->mode != CVF_PP_ALIGN ? 0 : (pp->align_w == nullptr ? 1 : 2);
  if (cell != nullptr) {
    const auto ck = mode == 0 ? cv_frame_large_bias_cell_kernel<0, SHARED> : mode == 1 ? cv_frame_large_bias_cell_kernel<1, SHARED> : cv_frame_large_bias_cell_kernel<2, SHARED>;
    if (lds > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void*)ck, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      CVF_REQUIRE(e == hipSuccess, "%s: %zu bytes of dynamic LDS: %s", name, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(ck, dim3((unsigned)B), dim3(cvfl::kThreads), lds, (hipStream_t)stream, *mlp, *pp, lay, *bias, md, cl, theta, xi_rows);
    return cvf_check_launch("cv_frame_large_bias_cell_kernel");
  }
  const auto kernel = mode == 0 ? cv_frame_large_bias_kernel<0, SHARED> : mode == 1 ? cv_frame_large_bias_kernel<1, SHARED> : cv_frame_large_bias_kernel<2, SHARED>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    CVF_REQUIRE(e == hipSuccess, "%s: %zu bytes of dynamic LDS: %s", name, lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(cvfl::kThreads), lds, (hipStream_t)stream, *mlp, *pp, lay, *bias, md, theta, xi_rows);
  return cvf_check_launch("cv_frame_large_bias_kernel");
}

int answer(const char* name, const char* why) {
  if (why != nullptr) {
    cvf_set_error("%s: %s", name, why);
    return 0;
  }
  return 1;
}

}  // namespace

extern "C" int cvf_cv_bias_check(const cvf_bias_desc* bias, int k) {
  char buf[240];
  return answer("cvf_cv_bias_check", cvf_bias_why(bias, k, buf, sizeof buf));
}

extern "C" int cvf_cv_frame_bias_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_bias", cvfr::cvfr_why(mlp, upto_layer, pp, nullptr, 0, 2));
}

extern "C" int cvf_cv_frame_bias_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_bias_shared", cvfr::cvfr_shared_why(mlp, n_shared, pp, nullptr, "cvf_cv_frame_bias_eval", 2));
}

extern "C" int cvf_cv_frame_large_bias_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_large_bias", cvfl::cvfl_why(mlp, upto_layer, pp, nullptr));
}

extern "C" int cvf_cv_frame_large_bias_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  return answer("cvf_cv_frame_large_bias_shared", cvfl::cvfl_shared_why(mlp, n_shared, pp, nullptr, "cvf_cv_frame_large_bias_eval"));
}

extern "C" int cvf_cv_frame_bias_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                      const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                      float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return wave_eval<false>("cvf_cv_frame_bias_eval", mlp, theta, upto_layer, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all, stream);
}

extern "C" int cvf_cv_frame_bias_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                             const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                             float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return wave_eval<true>("cvf_cv_frame_bias_shared_eval", mlp, theta, n_shared, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all,
                         stream);
}

extern "C" int cvf_cv_frame_large_bias_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                            const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                            float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return group_eval<false>("cvf_cv_frame_large_bias_eval", mlp, theta, upto_layer, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all,
                           stream);
}

extern "C" int cvf_cv_frame_large_bias_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                                   const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                                   float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream) {
  return group_eval<true>("cvf_cv_frame_large_bias_shared_eval", mlp, theta, n_shared, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows,
                          f_all, stream);
}

// ---- periodic cells
extern "C" int cvf_cv_frame_bias_cell_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  const char* why = cvfr::cvfr_why(mlp, upto_layer, pp, nullptr, 0, 2);
  return answer("cvf_cv_frame_bias_cell", why != nullptr ? why : whole_atoms_why(pp));
}

extern "C" int cvf_cv_frame_bias_shared_cell_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  const char* why = cvfr::cvfr_shared_why(mlp, n_shared, pp, nullptr, "cvf_cv_frame_bias_eval", 2);
  return answer("cvf_cv_frame_bias_shared_cell", why != nullptr ? why : whole_atoms_why(pp));
}

extern "C" int cvf_cv_frame_large_bias_cell_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp) {
  const char* why = cvfl::cvfl_why(mlp, upto_layer, pp, nullptr, 0, pp != nullptr ? cell_words(pp) : 0);
  return answer("cvf_cv_frame_large_bias_cell", why != nullptr ? why : whole_atoms_why(pp));
}

extern "C" int cvf_cv_frame_large_bias_shared_cell_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp) {
  const char* why = cvfl::cvfl_shared_why(mlp, n_shared, pp, nullptr, "cvf_cv_frame_large_bias_eval", pp != nullptr ? cell_words(pp) : 0);
  return answer("cvf_cv_frame_large_bias_shared_cell", why != nullptr ? why : whole_atoms_why(pp));
}

extern "C" int cvf_cv_frame_bias_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                           const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                           float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream, const cvf_md_cell* cell) {
  return wave_eval<false>("cvf_cv_frame_bias_cell_eval", mlp, theta, upto_layer, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all, stream,
                          cell, true);
}

extern "C" int cvf_cv_frame_bias_shared_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                                  const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                                  float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream,
                                                  const cvf_md_cell* cell) {
  return wave_eval<true>("cvf_cv_frame_bias_shared_cell_eval", mlp, theta, n_shared, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows, f_all,
                         stream, cell, true);
}

extern "C" int cvf_cv_frame_large_bias_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                                 const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                                 float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream,
                                                 const cvf_md_cell* cell) {
  return group_eval<false>("cvf_cv_frame_large_bias_cell_eval", mlp, theta, upto_layer, pp, bias, layout, x_all, B, xi_rows, u_rows, du_rows,
                           f_all, stream, cell, true);
}

extern "C" int cvf_cv_frame_large_bias_shared_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                                        const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                                        float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream,
                                                        const cvf_md_cell* cell) {
  return group_eval<true>("cvf_cv_frame_large_bias_shared_cell_eval", mlp, theta, n_shared, pp, bias, layout, x_all, B, xi_rows, u_rows,
                          du_rows, f_all, stream, cell, true);
}

extern "C" int cvf_md_make_whole(const cvf_md_layout* layout, const cvf_md_cell* cell, const float* x_all, int64_t n_atoms, int64_t B,
                                 float* x_whole, void* stream) {
  const char* name = "cvf_md_make_whole";
  CVF_REQUIRE(n_atoms >= 1 && n_atoms <= 0x7fffffff / 3, "%s: n_atoms = %lld (1 to %d)", name, (long long)n_atoms, 0x7fffffff / 3);
  CVF_REQUIRE(B >= 0 && B <= 0x7fffffff, "%s: B = %lld frames (one call takes 0 to 2^31 - 1)", name, (long long)B);
  CVF_REQUIRE(cell != nullptr && cell->cell != nullptr, "%s: no cell", name);
  CVF_REQUIRE(cell->cell_frame_stride >= 0, "%s: cell.cell_frame_stride = %lld: negative", name, (long long)cell->cell_frame_stride);
  MdArgs md = {x_all, nullptr, nullptr, 3 * n_atoms, 0, 3, nullptr, nullptr};
  if (layout != nullptr) {
    CVF_REQUIRE(layout->atom_stride >= 3, "%s: layout.atom_stride = %d: an atom has at least 3 floats", name, layout->atom_stride);
    CVF_REQUIRE(layout->x_frame_stride >= 0, "%s: layout.x_frame_stride = %lld: negative", name, (long long)layout->x_frame_stride);
    md.atom_index = layout->atom_index;
    md.atom_stride = layout->atom_stride;
    md.x_frame_stride = layout->x_frame_stride;
  }
  if (B == 0) return 0;
  CVF_REQUIRE(x_all && x_whole, "%s: null argument", name);
  const CellArgs cl = {cell->cell, cell->cell_frame_stride, nullptr};
  hipLaunchKernelGGL(md_make_whole_kernel, dim3((unsigned)B), dim3(cvfl::kThreads), 0, (hipStream_t)stream, md, cl, (int)n_atoms, x_whole);
  return cvf_check_launch("md_make_whole_kernel");
}
