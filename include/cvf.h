/* cvf.h - C ABI of libcvf_hip.so, the MI355X (gfx950) hot path of colvarsfinder.
 *
 * The reference (zwpku/colvars-finder v0.1.14) exposes NO FFI for this path: it is
 * plain PyTorch behind Python objects.  This header is therefore
 * the boundary the reference's Python layer would bind with ctypes; every entry point
 * names the reference code it replaces (file:line under the reference checkout).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - every function is stream-ordered on `stream` (a hipStream_t passed as void*),
 *     never synchronises the host, never allocates, never frees: the caller owns all
 *     buffers (sizes are returned by the cvf_*_size helpers);
 *   - return value: 0 on success, negative on error (cvf_last_error() has the text);
 *   - "tiled" tensors are laid out [tile][row][64]: frame b lives in tile b/64, lane
 *     b%64; rows are features / nets / auxiliary slots.  Tail tiles are padded with
 *     copies of the last frame whose weight is forced to 0.
 *   - theta / grad / adam moments are flat fp32 buffers in torch's parameters() order
 *     (per Linear: weight [out,in] row-major, then bias [out]); cvf_mlp_desc holds the
 *     offsets.
 */
#ifndef CVF_H
#define CVF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVF_TILE 64
#define CVF_MAX_NETS 8
#define CVF_MAX_LAYERS 12
#define CVF_AUX_ROWS 18 /* R (9, row-major), centroid (3), Kinv (6: 00 01 02 11 12 22) */

/* feature record types: molann's ids (examples/dipeptide/main.ipynb:306-307 prints
 * "position ... type_id 3") */
enum { CVF_FEAT_ANGLE = 0, CVF_FEAT_BOND = 1, CVF_FEAT_DIHEDRAL = 2, CVF_FEAT_POSITION = 3 };
/* CVF_PP_FACTORED: r(x) is any torch module, evaluated on the host once per frame (colvarsfinder/pp.py: FactoredMetric).  A
 * "frame" is then one fp32 RECORD [r(x) (d_r) | L (d_r x rho, row-major)] with L L^T = J A J^T (J = dr/dx, A = diag(diag_coeff)):
 * n_coord = d_r * (1 + rho), 1 <= rho <= d_r, d_r * rho <= 65536; every other descriptor field is ignored.
 * cvf_align_feature_fwd copies r(x) out of the records; cvf_metric_apply[_stats] computes t = L^T g, q = L t, E = |t|^2 from them
 * (csrc/metric_factor.hip; `a` and `aux_tiled` are ignored: diag_coeff is folded into L).  The fused and 16-frame launches
 * (cvf_ef16_*, cvf_ef_[align_]fwd_metric_*, cvf_ef_align_fwd) take coordinates and refuse this mode; their predicates answer 0. */
enum { CVF_PP_IDENTITY = 0, CVF_PP_ALIGN = 1, CVF_PP_FACTORED = 2, CVF_PP_FEATURES = 3 };
/* CVF_PP_FEATURES: the features of the RAW coordinates - molann's PreprocessingANN(None, feature_layer): no centroid, no rotation; a
 * position record copies x[atom] bit for bit (csrc/k1_features.hip).  The descriptor carries n_coord = 3 N, n_rec, rec, d_r,
 * use_angle_value, has_position, the slot tables (atom_slot, slot_atom, rec_slot, n_slot, n_rec_slot) and, for the derivative entry
 * points, mrec / slot_row / n_mrec / n_ref; n_align = 0 and align_idx, ref_c, align_w, atom_align, flags are not read.  aux_tiled,
 * scratch, slot_xyz and dense are ignored wherever they are arguments (NULL is fine) and cvf_align_feature_scratch_bytes answers 0.
 * Taken by cvf_align_feature_fwd, cvf_align_feature_vjp[_rows] and cvf_metric_apply[_stats] (the batch sums by cvf_ef_stats'
 * two-stage tail); the fused and 16-frame launches refuse the mode and their predicates answer 0.  One design serves every atom
 * count - only the feature atoms of a frame are read (12 bytes each), never the frame - so what bounds a launch is the feature list:
 * beyond the two limits below the entry points return a negative code whose message names the limit, before any launch. */
#define CVF_FEATURES_MAX_SLOT 4096 /* n_slot: distinct atoms the features read */
#define CVF_FEATURES_MAX_REF 6144  /* n_ref: (record, atom) pairs = contribution rows of the derivative kernels (vjp, metric) */
/* cvf_mlp_desc.act[l]: what follows Linear layer l (nn.py:29-59 takes any torch activation module).  The chain kernels
 * (cvf_ae_*, cvf_regae_*, cvf_mlp_eval_rows) and the eigenfunction kernels on 64-frame tiles (cvf_ef_*: they use the
 * activation's first TWO derivatives, expressed through its output) take all of these, one code for every hidden layer of a
 * net; the 16-frames-per-wave kernels (cvf_ef16_*) take CVF_ACT_TANH only - cvf_ef16_supported() answers 0 otherwise. */
enum {
  CVF_ACT_NONE = 0,
  CVF_ACT_TANH = 1,
  CVF_ACT_SIGMOID = 2,
  CVF_ACT_RELU = 3,
  CVF_ACT_ELU = 4,        /* alpha = 1 */
  CVF_ACT_LEAKY_RELU = 5, /* negative_slope = 0.01 */
  CVF_ACT_SOFTPLUS = 6    /* beta = 1, threshold = 20 */
};
/* cvf_pp_desc.flags: structure of the tables, enabling kernels whose LDS addresses are affine in the atom index */
enum {
  CVF_PP_ALIGN_CONTIG = 1,   /* align_idx[b] == b for all b (the align atoms are the first n_align frame atoms) */
  CVF_PP_PURE_POSITION = 2,  /* record r is {POSITION, atom r, out 3r}: n_rec atoms emit their aligned positions in order */
  CVF_PP_SLOT_BATCHED = 4    /* rec_slot holds n_rec_slot entries in batches of 64 of ONE feature type (one entry per lane of a wave),
                              * entries of type -1 are padding */
};

/* The preprocessing layer r(x): torch.nn.Identity (examples/2d/2d.ipynb:485) or the
 * Kabsch alignment + feature map the reference gets from molann
 * (examples/dipeptide/main.ipynb:333-348; consumed at core.py:403,414,635). */
typedef struct cvf_pp_desc {
  int32_t mode;            /* CVF_PP_* */
  int32_t n_coord;         /* floats per frame: 3*N (align), d (identity) or d_r*(1+rho) (factored record) */
  int32_t n_align;         /* number of align atoms */
  int32_t n_rec;           /* number of feature records */
  int32_t d_r;             /* output dimension */
  int32_t use_angle_value; /* 0: angle->cos, dihedral->(cos,sin); 1: radians */
  int32_t has_position;    /* any CVF_FEAT_POSITION record */
  int32_t flags;           /* CVF_PP_* hints the caller vouches for (0 is always valid) */
  const int32_t* align_idx; /* [n_align] atom indices into the frame */
  const float* ref_c;       /* [n_align*3] reference positions minus their centroid */
  const int32_t* rec;       /* [n_rec*6]: type, a0, a1, a2, a3, out_offset (one record per
                               position ATOM: a0 = atom, 3 outputs) */
  /* optional (large molecules): per-atom tables that let the streaming kernel copy the atoms the features
   * use ("slots") to LDS while the frame goes by, instead of gathering them from HBM afterwards */
  const int32_t* atom_align; /* [N]: index b of the atom in align_idx / ref_c, or -1 */
  const int32_t* atom_slot;  /* [N] (16-byte aligned): slot of the atom, or -1 when no feature uses it */
  const int32_t* rec_slot;   /* [n_rec_slot*6]: rec with the atom fields replaced by slots; any order (best grouped by type) */
  const int32_t* slot_atom;  /* [n_slot]: atom of each slot */
  int32_t n_slot;
  int32_t n_rec_slot;        /* entries of rec_slot (0: n_rec, unbatched) */
  /* optional per-atom alignment weights ("weighted Kabsch": the rotation and translation minimise
   * sum_b w_b |(x_b - c) R - ref_b|^2, c = sum_b w_b x_b / sum_b w_b).  NULL = uniform weights.  When set:
   *   align_w[b] = n_align * w_b / sum w   (mean 1), and ref_c[b] = align_w[b] * (ref_b - weighted centroid of ref).
   *   n_coord <= 192 (the lane-per-frame kernels): flags must be 0 (the layouts built for speed assume uniform weights).
   *   n_coord  > 192 (the streaming kernels, csrc/k1_large.hip): accepted with any combination of CVF_PP_ALIGN_CONTIG /
   *     CVF_PP_SLOT_BATCHED - the flags describe the tables, not the weights - by cvf_align_feature_fwd,
   *     cvf_align_feature_vjp[_rows], cvf_metric_apply[_stats] and cvf_metric_dense_tensors.  The vectorised instances of the
   *     streaming kernels read four weights per 16-byte load: align_w must then be 16-byte aligned like ref_c and atom_slot,
   *     otherwise the launch takes a scalar instance (cvf_align_feature_route tells which).
   * The fused and 16-frame launches (cvf_ef16_*, cvf_ef_[align_]fwd_metric_*) do not take weights; their predicates answer 0. */
  const float* align_w;      /* [n_align] or NULL */
  /* large molecules, derivative kernel (cvf_metric_apply; csrc/metric_large.hip): the scatter J^T g -> feature atoms as a table
   * of rows.  Every (record, atom position) pair owns one row; the rows of one slot are contiguous:
   *   slot_row[t] .. slot_row[t+1]-1 (slot_row[n_slot] = n_ref = total number of pairs, < 65536).
   * mrec[r] = { (type + 1) | out_offset << 3, slot[0] | slot[1] << 16, slot[2] | slot[3] << 16, urow[0] | urow[1] << 16,
   *             urow[2] | urow[3] << 16, off[0] | off[1] << 8 | off[2] << 16 | off[3] << 24, 0, 0 }   (16-byte aligned)
   * with urow[p] = slot_row[slot[p]] and urow[p] + off[p] = the row of atom p of record r (off < 256; unused positions 0;
   * n_slot, n_ref < 65536); records of one type side by side keep a wave on one code path. */
  const int32_t* mrec;       /* [n_mrec*8] */
  const int32_t* slot_row;   /* [n_slot+1] */
  int32_t n_mrec;
  int32_t n_ref;
} cvf_pp_desc;

/* k identical feed-forward nets (colvarsfinder.nn.EigenFunctions, nn.py:242-293) or one
 * chain (AutoEncoder = encoder followed by decoder, nn.py:61-114). */
typedef struct cvf_mlp_desc {
  int32_t n_nets;
  int32_t n_layers;                      /* Linear layers per net */
  int32_t dims[CVF_MAX_LAYERS + 1];      /* widths d0..dL */
  int32_t act[CVF_MAX_LAYERS];           /* 1: tanh after this Linear (nn.py:55-57) */
  int32_t w_off[CVF_MAX_NETS][CVF_MAX_LAYERS];
  int32_t b_off[CVF_MAX_NETS][CVF_MAX_LAYERS];
  int32_t n_params;
} cvf_mlp_desc;

/* Scalars of EigenFunctionTask (core.py:293-354). */
typedef struct cvf_ef_cfg {
  int32_t k;
  int32_t lag_idx;       /* 0: generator (core.py:418-426,438); >0: transfer operator (428,440) */
  int32_t sort_eigvals;  /* core.py:430-434 */
  int32_t iso_metric;    /* generator mode, the 16-frame front launches (cvf_ef16_front, cvf_ef16_front_rows): 1 = the caller vouches for an
                          * ISOTROPIC metric, a[3b] == a[3b+1] == a[3b+2] for every record atom b, and q = J A J^T g is formed in the
                          * aligned frame; 0 = the general passes.  (Was padding: zero in every earlier caller.)  Not read elsewhere. */
  double alpha;          /* core.py:455 */
  double beta;           /* core.py:426,438 */
  double dt;             /* core.py:428,440 */
  double eig_w[CVF_MAX_NETS];
} cvf_ef_cfg;

/* layout of the fp64 statistics vector (collective #1) */
#define CVF_NPAIR(k) ((k) * ((k) + 1) / 2)
/* generator: [W, S1(k), S2(k(k+1)/2, i<=j row-major), E(k)]
 * transfer : [W, S1(k), S2(...), W', S1'(k), S2'_ii(k), T(k)] */
int cvf_ef_nstats(int k, int lag_idx);
/* loss vector written by cvf_ef_loss: [loss, npl, pen, eig_sorted(k), cvec(k) as doubles] */
#define CVF_LOSS_LEN(k) (3 + 2 * (k))
/* coefficient vector written by cvf_ef_loss and read by cvf_ef_backward:
 * [gS1(k), gS2(k*k symmetric full), gE_or_gT(k), gS1'(k), gS2'_ii(k)]
 * Each entry is the partial derivative of the loss with respect to the sum of that name, eigenvalues and cvec held constant.
 * gS2 is [i][j] row-major and symmetric by convention: gS2[i][j] = gS2[j][i] = d loss / d S2(min(i,j), max(i,j)), the derivative
 * with respect to the ONE stored sum, in both places (not halved).  gS1' and gS2'_ii are 0 in generator mode.  W and W' have no
 * entry (the weights do not depend on the parameters). */
#define CVF_COEF_LEN(k) (4 * (k) + (k) * (k))

/* Adam scalars + state for the fused "reduce the gradient and update" calls (single-process runs, where no
 * cross-rank all-reduce sits between the gradient and the update).  torch.optim.Adam as built at core.py:164. */
typedef struct cvf_adam_args {
  float* theta;
  float* m;
  float* v;
  double lr, beta1, beta2, eps;
  const int32_t* step_count;   /* device: number t >= 1 of the current step */
  const cvf_mlp_desc* mlp;     /* with `packed`: the nets whose fragment copy is refreshed, else NULL */
  float* packed;
  const float* lr_dev;         /* device scalar that overrides `lr` when non-NULL: a captured hipGraph of the step then follows
                                * a learning rate the host changes between replays (scheduler, manual decay) */
} cvf_adam_args;

int cvf_version(void);
const char* cvf_last_error(void);

/* --- K1: alignment + features, forward.  Replaces pp_layer(X) at core.py:403,414,635.
 * x [B, n_coord] row-major fp32.  feat_tiled [T][d_r][64] and/or feat_rows [B][d_r]
 * (either may be NULL); aux_tiled [T][18][64] (may be NULL; identity mode ignores it).
 * Frames of thousands of atoms take the streaming path (groups of 8 frames; large batches with a tiled output run the resident
 * role-split kernel of csrc/k1_large.hip - same numbers, bit for bit - which writes every tiled row of 32 consecutive frames as one
 * 128-byte line: feat_tiled / aux_tiled / scratch must cover the padded frame count, ceil(B / 64) * 64, as documented).
 * `scratch` (may be NULL; cvf_align_feature_scratch_bytes() bytes): on the streaming path it receives the compact
 * copy [padded frames / 8][n_slot*3][8] (coordinate rows of groups of eight frames) of the atoms the features use, which
 * cvf_metric_apply consumes as `slot_xyz`. */
int64_t cvf_align_feature_scratch_bytes(const cvf_pp_desc* pp, int64_t B); /* 0 for small molecules */
int cvf_align_feature_fwd(const cvf_pp_desc* pp, const float* x, int64_t B, float* feat_tiled, float* feat_rows,
                          float* aux_tiled, void* scratch, void* stream);
/* Which kernel cvf_align_feature_fwd launches for a CVF_PP_ALIGN descriptor, a batch size and a set of outputs (has_* != 0: that
 * buffer is passed; has_scratch counts only where cvf_align_feature_scratch_bytes() > 0).  Host arithmetic only, no launch;
 * cvf_align_feature_fwd decides by the same function, and the developer environment switches it reads (CVF_K1_NOSLICE, CVF_K1_NOPIPE,
 * CVF_K1_PIPE_MIN_GROUPS) are honoured here too.  `x` and `feat_rows` are taken to be 16-byte aligned (torch allocations are); a
 * misaligned `x` takes the scalar capture / gather instances instead.  Per-atom weights (align_w) have their own instances of the
 * gather, capture and slice kernels and never take the pipelined kernel.  Returns one of the codes below, or a negative value (and
 * cvf_last_error()) for a descriptor cvf_align_feature_fwd refuses. */
enum {
  CVF_K1_ROUTE_SMALL = 0,         /* n_coord <= 192: the lane-per-frame kernels (csrc/k1_align.hip) */
  CVF_K1_ROUTE_GATHER_CONTIG = 1, /* k1_large_gather_kernel<CONTIG = true>: feature atoms re-read after the streaming pass */
  CVF_K1_ROUTE_GATHER = 2,        /* k1_large_gather_kernel<CONTIG = false> */
  CVF_K1_ROUTE_CAPTURE_VEC4 = 3,  /* k1_large_capture_kernel<VEC4 = true>: one wave per frame, 16-byte loads */
  CVF_K1_ROUTE_CAPTURE = 4,       /* k1_large_capture_kernel<VEC4 = false>: 4-byte loads, any align set */
  CVF_K1_ROUTE_SLICE = 10,        /* + NI = 11..14: k1_large_slice_kernel<NI> (NI = ceil(N / 2048) groups of four atoms per lane) */
  CVF_K1_ROUTE_PIPE = 20          /* + NI = 21..23: k1_large_pipe_kernel<NI> (uniform weights only) */
};
int cvf_align_feature_route(const cvf_pp_desc* pp, int64_t B, int has_tiled, int has_rows, int has_aux, int has_scratch);

/* --- VJP of K1: dL/dx of the alignment + feature map, gx_rows[b] = J(x_b)^T g_rows[b] (csrc/k1_vjp.hip).  What autograd
 * computes through pp_layer when the reference differentiates a loss or a CV with respect to the coordinates (core.py:418-426).
 * x [B, n_coord] and aux_tiled [T][18][64] exactly as passed to / written by cvf_align_feature_fwd for the same frames;
 * g_rows [B][d_r]; gx_rows [B][n_coord], fully written (0 for atoms no feature reads and the alignment does not use).
 *   CVF_PP_ALIGN: every descriptor cvf_align_feature_fwd takes (any flags, partial alignment sets, all feature types, both
 *     use_angle_value modes, align_w); frames of more than 192 coordinates also need the slot tables and mrec / slot_row, with
 *     n_ref * 12 bytes within the LDS.  CVF_PP_FEATURES: aux_tiled is ignored (may be NULL); gx_rows is 0 on every atom no feature
 *     reads; n_slot <= CVF_FEATURES_MAX_SLOT, n_ref <= CVF_FEATURES_MAX_REF.  CVF_PP_IDENTITY: a copy.  CVF_PP_FACTORED: refused (the records come from a torch
 *     module, which has its own autograd).
 * No atomics: two calls on the same inputs give the same bits. */
int cvf_align_feature_vjp(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled,
                          const float* g_rows, float* gx_rows, void* stream);
/* k cotangents per frame in one launch, 1 <= k <= CVF_MAX_NETS: gx_rows[b][i] = J(x_b)^T g_rows[b][i]  (g_rows [B][k][d_r],
 * gx_rows [B][k][n_coord]; the Jacobian of a k-vector CV when g_rows holds d xi_i / d r).  Same descriptors, inputs and
 * refusals as cvf_align_feature_vjp; row i equals cvf_align_feature_vjp on g_rows[:, i] bit for bit.  The x tile / gathers,
 * the tables, the aux rows and every record's geometry are taken once per frame, not once per row.  No atomics. */
int cvf_align_feature_vjp_rows(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled, int k,
                               const float* g_rows, float* gx_rows, void* stream);

/* --- JVP of K1 (csrc/k1_jvp.hip; CVF_PP_FEATURES: csrc/k1_features.hip).
 * q_rows[b] = J(x_b) u_rows[b]: the directional derivative of r(x) (cvf_align_feature_fwd) along u.
 * u_rows [B][n_coord], q_rows [B][d_r], aux_tiled as written by cvf_align_feature_fwd for the same x
 * (NULL for CVF_PP_IDENTITY / CVF_PP_FEATURES).  The transpose of cvf_align_feature_vjp: same descriptors (frames of more than
 * 192 coordinates need slot_atom and mrec), same CVF_FEATURES_MAX_SLOT / CVF_FEATURES_MAX_REF limits, CVF_PP_IDENTITY a copy,
 * CVF_PP_FACTORED refused.  Of x and u only the align atoms and the atoms some feature reads are loaded into the arithmetic:
 * whatever u holds elsewhere (NaN included) does not reach q.  With ubar = sum_b w_b u_b / n_align, dH = sum_b (u_b - ubar) (x) ref_b
 * and dR = R [Kinv ax(R^T dH)]x, a position record gives (u_a - ubar) R + (x_a - c) dR and a bond / angle / dihedral record the
 * sum of its gradient vectors times its atoms' tangents.  What forward-mode differentiation through the layer computes, and the
 * derivative of cvf_align_feature_vjp in its cotangent (the map g -> J^T g is linear).
 * No allocation, no host synchronisation, no atomics: two calls give the same bits.  B == 0 returns 0; only rows < B are written. */
int cvf_align_feature_jvp(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled,
                          const float* u_rows, float* q_rows, void* stream);

/* --- Hessian-vector product of K1 (csrc/k1_hvp.hip).
 * h_rows[b] = d/dx <g_rows[b], J(x_b) u_rows[b]> = (sum_i g_i Hess r_i(x_b)) u_rows[b]: the derivative along u of
 * cvf_align_feature_vjp's result, symmetric in u - the curvature term of a double backward through the layer.
 * g_rows [B][d_r], u_rows [B][n_coord], h_rows [B][n_coord], fully written; aux_tiled as written by cvf_align_feature_fwd for the
 * same x (NULL for CVF_PP_IDENTITY / CVF_PP_FEATURES).  Same descriptors as cvf_align_feature_vjp (frames of more than 192
 * coordinates need the slot and contribution-row tables, n_ref * 12 bytes within the LDS), same CVF_FEATURES_MAX_SLOT /
 * CVF_FEATURES_MAX_REF limits; CVF_PP_IDENTITY writes zeros (its Hessian is 0), CVF_PP_FACTORED is refused.  Position records
 * contribute the derivative along u of R g_a and of Z ref_b - w_b shift (the rotation's and the centroid's second derivative, on
 * the aux rows and the covariance sum_b (x_b - c) (x) ref_b recomputed over the align atoms); bond / angle / dihedral records the
 * derivative along u of their gradient vectors times their adjoint.  Of x and u only the align atoms and the atoms some feature
 * reads are loaded into the arithmetic: whatever u holds elsewhere (NaN included) does not reach h, and h is exactly 0 there.
 * No allocation, no host synchronisation, no atomics: two calls give the same bits.  B == 0 returns 0 and writes nothing. */
int cvf_align_feature_hvp(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled,
                          const float* g_rows, const float* u_rows, float* h_rows, void* stream);

/* Which kernel instance a cvf_align_feature_vjp / _vjp_rows / _jvp / _hvp call on B frames launches, with its LDS, grid and row
 * grouping, by the very function the four calls launch by (host arithmetic; no pointer of the descriptor is read but align_w, and
 * that only for NULL, so a descriptor that carries its counts and flags is enough).  k: the cotangents of _vjp_rows (ignored by the
 * other three).  out_aligned16: whether gx_rows / h_rows is 16-byte aligned - with n_coord % 4 == 0 it selects the 16-byte stores of
 * the kernels for frames of more than 192 coordinates.  Returns 0 and fills *plan, or a negative value (and cvf_last_error()) for a
 * descriptor, a batch or a k the call refuses.  Fields that do not apply to the family are 0.  For CVF_PP_FEATURES descriptors two
 * more values of `which` answer for the launches of cvf_align_feature_fwd and cvf_metric_apply (k nets) in csrc/k1_features.hip. */
enum { CVF_DERIV_VJP = 0, CVF_DERIV_VJP_ROWS = 1, CVF_DERIV_JVP = 2, CVF_DERIV_HVP = 3,
       CVF_DERIV_FEATURES_FWD = 4, CVF_DERIV_FEATURES_METRIC = 5 /* CVF_PP_FEATURES only */ };
enum {
  CVF_DERIV_ROUTE_IDENTITY = 0, /* a copy (vjp, vjp_rows, jvp) or a zero fill (hvp): no kernel of these files */
  CVF_DERIV_ROUTE_FEATURES = 1, /* features_{vjp,jvp,hvp,fwd,metric}_kernel: CVF_PP_FEATURES, 1 << lg frames per workgroup */
  CVF_DERIV_ROUTE_SMALL = 2,    /* {vjp_align,vjp_rows_small,hvp_align}_kernel<tables_lds>, jvp_align_kernel<tables_lds, q_lds>: n_coord <= 192 */
  CVF_DERIV_ROUTE_LARGE = 3     /* {vjp,vjp_rows}_[weighted_]large_kernel<vec4>, {jvp,hvp}_large_kernel<weighted>: n_coord > 192 */
};
typedef struct {
  int32_t family;          /* CVF_DERIV_ROUTE_* */
  int32_t tables_lds;      /* small: rec, align_idx and ref_c are copied to LDS */
  int32_t q_lds;           /* small jvp: the [64][d_r | 1] result image is in LDS */
  int32_t u_lds;           /* features hvp: the feature atoms of u are staged in LDS */
  int32_t weighted;        /* align_w != NULL */
  int32_t vec4;            /* large vjp, vjp_rows, hvp: 16-byte stores of the dense row */
  int32_t lg;              /* features: log2 frames per workgroup */
  int32_t rows_per_launch; /* vjp_rows: rows whose images share the LDS (kg); features metric: nets per pass; else 1 */
  int32_t launches;        /* vjp_rows on large frames: ceil(k / kg); else 1 */
  int32_t reserved;
  int64_t lds_bytes, grid; /* dynamic LDS and workgroups of the first launch (identity: 0) */
} cvf_deriv_plan;
int cvf_align_feature_deriv_route(const cvf_pp_desc* pp, int64_t B, int which, int k, int out_aligned16, cvf_deriv_plan* plan);

/* --- K2+K3: per frame and net, q = J A J^T g and E = g^T J A J^T g with J the Jacobian
 * of r at the frame and A = diag(a).  Replaces the k autograd.grad calls through
 * pp_layer at core.py:424 and the a-weighted square sums at core.py:426,438; the
 * [B,3N,k] gradient tensor is never materialised.
 * g_tiled, q_tiled [T][k][d_r][64]; e_tiled [T][k][64]; a [n_coord]. */
int cvf_metric_apply(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled, const float* a,
                     int k, const float* g_tiled, float* q_tiled, float* e_tiled, const float* slot_xyz,
                     const double* dense, void* stream);
/* Which kernel a cvf_metric_apply (with_stats = 0) or cvf_metric_apply_stats (with_stats = 1) call on B frames and k nets launches,
 * by the very function the two calls launch by (host arithmetic; no pointer of the descriptor is read, so a descriptor that carries only
 * its counts and flags is enough).  Returns 0 and fills *plan, or a negative value (and cvf_last_error()) for a descriptor or a batch the
 * calls refuse.  Fields that do not apply to the family are 0.  CVF_METRIC_ROUTE_FEATURES: the launch of csrc/k1_features.hip (frames per
 * workgroup, nets per pass, LDS, grid) is answered by cvf_align_feature_deriv_route(pp, B, CVF_DERIV_FEATURES_METRIC, k, 0, &plan) above,
 * beside the other launches of that file. */
enum {
  CVF_METRIC_ROUTE_IDENTITY = 0, /* metric_identity_kernel */
  CVF_METRIC_ROUTE_FACTORED = 1, /* csrc/metric_factor.hip */
  CVF_METRIC_ROUTE_FEATURES = 2, /* csrc/k1_features.hip */
  CVF_METRIC_ROUTE_ALIGN = 3,    /* metric_align_kernel: n_coord <= 192, any feature list, weighted or not */
  CVF_METRIC_ROUTE_PURE = 4,     /* metric_pure_kernel: n_coord <= 192, CVF_PP_ALIGN_CONTIG | CVF_PP_PURE_POSITION, n_align <= n_rec */
  CVF_METRIC_ROUTE_ROWS = 5      /* metric_rows_kernel<F, waves, geo_pre, multi>: n_coord > 192 (csrc/metric_large.hip) */
};
typedef struct {
  int32_t family;      /* CVF_METRIC_ROUTE_* */
  int32_t F;           /* rows: frames per workgroup, 16 | 8 | 4 */
  int32_t waves;       /* rows: 8 | 16;  pure: nets_per_wg;  align, identity: 1 */
  int32_t geo_pre;     /* rows: records per lane group whose geometry stays in registers */
  int32_t multi;       /* rows: the instance that walks npb nets per workgroup */
  int32_t npb;         /* rows: nets per workgroup (a divisor of k; CVF_METRIC_NPB is read on every call) */
  int32_t nets_per_wg; /* pure: k (all nets share one staged coordinate tile) or 1;  rows: npb;  else 1 */
  int32_t fused;       /* with_stats: the launch also writes the first stage of the batch sums */
  int32_t fused_rows;  /* rows of partial sums it writes: pure - tiles; rows - frame groups of F; 0 when not fused */
  int32_t reserved;
  int64_t lds_bytes;   /* dynamic LDS of the launch */
  int64_t grid;        /* workgroups */
} cvf_metric_plan;
int cvf_metric_route(const cvf_pp_desc* pp, int64_t B, int k, int with_stats, cvf_metric_plan* plan);
/* The same launch with the first stage of K5 (cvf_ef_stats in generator mode, below) folded in: every block reduces its
 * tile's share of the batch sums, one short launch adds the tiles in a fixed order and, when loss_vec != NULL,
 * evaluates cvf_ef_loss.  Shapes the fused stage does not cover run cvf_metric_apply and cvf_ef_stats back to back -
 * the results agree to fp64 summation order.  scratch: cvf_metric_stats_scratch_doubles() doubles. */
int64_t cvf_metric_stats_scratch_doubles(int64_t B, int k);
int cvf_metric_apply_stats(const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled, const float* a,
                           int k, const float* g_tiled, float* q_tiled, float* e_tiled, const float* slot_xyz,
                           const double* dense, const cvf_ef_cfg* cfg, const float* w, const float* y_tiled,
                           double* scratch, double* stats, double* loss_vec, double* coef, void* stream);
/* large molecules only (slot_xyz / dense may be NULL otherwise): dense[cvf_metric_dense_doubles(pp)], prepared once per (pp, a):
 * dense[0..41] = moments of (a, ref) over the align atoms, T0[c] = sum a_bc, T1[c][j] = sum a_bc ref_bj,
 * T2[c][j][k] = sum a_bc ref_bj ref_bk, R1[j] = sum ref_bj (fp64); behind them n_slot x 8 floats of per-slot constants
 * (a, ref, align flag, rows of the slot) for the derivative kernel.
 * With per-atom weights (w = align_w, 1 when NULL; ref = ref_c as stored, i.e. pre-weighted) the moments are
 *   T0[c] = sum a_bc w_b^2,  T1[c][j] = sum a_bc w_b ref_bj,  T2[c][j][k] = sum a_bc ref_bj ref_bk,  R1[j] = sum ref_bj
 * and column 6 of the per-slot constants holds w_b (0 off the align set) instead of 1 / 0: with d_b = Z ref_b - w_b shift and the
 * centroid's tangent dc = sum_b w_b u_b / n_align the closed forms of csrc/metric_large.hip keep their shape.  align_w = NULL gives the
 * bits of align_w = all ones. */
int64_t cvf_metric_dense_doubles(const cvf_pp_desc* pp);
int cvf_metric_dense_tensors(const cvf_pp_desc* pp, const float* a, double* dense, void* stream);
/* The CV metric tensor per frame from cvf_metric_apply's input and output: m_rows[b][i][j] = g_i . q_j = (J A J^T)_ij in CV
 * space (g_tiled, q_tiled [T][k][d_r][64] as cvf_metric_apply takes / writes them; m_rows [B][k][k]).  Each sum over the d_r
 * features runs in order for i <= j; the lower triangle mirrors it, so M is exactly symmetric.  1 <= k <= CVF_MAX_NETS. */
int cvf_metric_gram(int k, int64_t B, int d_r, const float* g_tiled, const float* q_tiled, float* m_rows, void* stream);

/* --- packed MFMA weight fragments of the nets (a second copy of the weights in the order the
 * matrix-core kernels consume them; see csrc/cvf_pack.hpp).  cvf_ef_pack rebuilds it from theta;
 * cvf_adam_step / cvf_sgd_step keep it in step when given the buffer. */
int64_t cvf_ef_pack_floats(const cvf_mlp_desc* mlp);
int cvf_ef_pack(const cvf_mlp_desc* mlp, const float* theta, float* packed, void* stream);

/* --- K4a: k nets forward (+ gradient of each output w.r.t. the features).
 * Replaces self.model(...) at core.py:403,414 (nn.py:293).
 * y_tiled [T][k][64]; g_tiled [T][k][d0][64] or NULL. */
int cvf_ef_mlp_fwd(const cvf_mlp_desc* mlp, const float* theta, const float* packed, const float* feat_tiled,
                   int64_t n_tiles, float* y_tiled, float* g_tiled, float* saved, void* stream);
/* `saved` (may be NULL): cvf_ef_saved_floats() floats in which the forward kernel leaves the hidden activations (and
 * the back-propagated output sensitivities) of every (tile, net) for cvf_ef_backward, which then skips recomputing
 * them; for first layers wider than 128 inputs the buffer also has room for the tangent chain's first product, which
 * cvf_ef_backward computes with a launch of its own ahead of its main kernel).  Opaque layout; 0 floats = this shape has no
 * hand-off, pass NULL to both calls. */
int64_t cvf_ef_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles);

/* --- K4a + K2/K3 + K5 in one go for the fast layout (pure position features on a contiguous align set, d_r <= 72):
 * cvf_ef_mlp_fwd, cvf_metric_apply_stats fused per tile - g = dy/dfeat never leaves the chip.  Same outputs (y, saved,
 * q, e, stats[, loss_vec, coef]) up to summation order; g_tiled is not produced.  Check cvf_ef_fwd_metric_supported()
 * first; otherwise make the two calls.  scratch as for cvf_metric_apply_stats. */
int cvf_ef_fwd_metric_supported(const cvf_mlp_desc* mlp, const cvf_pp_desc* pp);
int cvf_ef_fwd_metric_stats(const cvf_mlp_desc* mlp, const float* theta, const float* packed, const float* feat_tiled,
                            const cvf_pp_desc* pp, const float* x, int64_t B, const float* aux_tiled, const float* a,
                            float* y_tiled, float* saved, float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg,
                            const float* w, double* scratch, double* stats, double* loss_vec, double* coef, void* stream);

/* With stats == NULL the fused launches stop after leaving cvf_ef_fused_stats_rows() (> 0 required) rows of per-tile
 * sums in `scratch`; cvf_ef_stats_finish_rows adds them in a fixed order (and evaluates cvf_ef_loss when loss_vec != NULL).
 * Rows read by cvf_ef_stats_finish_rows: partial [n_rows][cvf_ef_nstats(k, lag_idx)] doubles, row-major (statistic i of row r at
 * partial[r * ns + i]), each row in the layout of the statistics vector above.  With loss_vec == NULL neither loss_vec nor coef
 * is touched. */
/* Transfer-operator mode (lag_tau > 0; core.py:403,414): alignment + features + nets forward in one launch for the frames x
 * and their lagged partners x_lag (may be NULL: T tiles only) -> feat_tiled [2T][d_r][64] (tiles T.. = lagged), y_tiled
 * [2T][k][64], saved (cvf_ef_saved_floats(mlp, 2T); may be NULL).  Same shapes as cvf_ef_align_fwd_metric_supported().
 * Follow with cvf_ef_stats (lag_idx > 0) and cvf_ef_backward as after cvf_align_feature_fwd x 2 + cvf_ef_mlp_fwd. */
int cvf_ef_align_fwd(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                     const cvf_pp_desc* pp, const float* x, const float* x_lag, int64_t B, float* y_tiled, float* saved,
                     void* stream);
int64_t cvf_ef_fused_stats_rows(const cvf_mlp_desc* mlp, const cvf_pp_desc* pp, int64_t B, int with_align);
int cvf_ef_stats_finish_rows(const cvf_ef_cfg* cfg, int64_t n_rows, const double* partial, double* stats, double* loss_vec,
                             double* coef, void* stream);
/* The same with K1 folded in: from the coordinates to q, E and the batch sums in one launch (feat_tiled and aux_tiled
 * become outputs; aux_tiled may be NULL).  Replaces cvf_align_feature_fwd + cvf_ef_fwd_metric_stats. */
int cvf_ef_align_fwd_metric_supported(const cvf_mlp_desc* mlp, const cvf_pp_desc* pp);
int cvf_ef_align_fwd_metric_stats(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                  const cvf_pp_desc* pp, const float* x, int64_t B, float* aux_tiled, const float* a,
                                  float* y_tiled, float* saved, float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg,
                                  const float* w, double* scratch, double* stats, double* loss_vec, double* coef,
                                  void* stream);

/* --- The generator-mode step with SIXTEEN frames per wave (csrc/ef16_front.hip, ef16_back.hip), for the shapes of cvf_ef16_supported(): pure position
 * features on a contiguous align set, d_r <= 72 (the dipeptide-sized configurations 3 and 4).  Same mathematics and the same
 * outputs as cvf_ef_align_fwd_metric_stats + cvf_ef_backward; what differs is the decomposition: a wave owns 16 frames (the
 * matrix instruction's N), so the launch has four times the waves of a quarter of the dependent chain each, 3-5 waves per SIMD.
 *  cvf_ef16_front   : x [B][n_coord] -> feat_tiled [T][d_r][64], y_tiled [T][k][64], saved (cvf_ef16_saved_floats(); opaque
 *                     hand-off of the hidden activations), q_tiled [T][k][d_r][64], e_tiled [T][k][64], stats (+ loss_vec, coef
 *                     when non-NULL: cvf_ef_loss in the same call).  Replaces pp_layer(X), model(...), the k autograd.grad calls
 *                     and the batch sums of core.py:403-452.  scratch: cvf_ef16_scratch_doubles(B, k) doubles.
 *  cvf_ef16_backward: flat parameter gradient as slab rows, as cvf_ef_backward (core.py:517); follow with cvf_slab_reduce.
 *                     Every net must be one run of the flat buffer in the order of model.parameters() - per layer the weight, then
 *                     the bias, layer after layer: the kernel derives a layer's offsets from w_off[net][0].  Any other order
 *                     inside a net is refused (cvf_ef16_backward_transfer alike). */
int cvf_ef16_supported(const cvf_mlp_desc* mlp, const cvf_pp_desc* pp);
int64_t cvf_ef16_scratch_doubles(int64_t B, int k);
int64_t cvf_ef16_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles);
/* With stats == NULL cvf_ef16_front stops after leaving cvf_ef16_rows(B) (> 0 required) rows of per-unit batch sums in `scratch`;
 * cvf_ef16_finish adds them in a fixed order (and evaluates cvf_ef_loss when loss_vec != NULL).  Two calls = two launches that
 * can be timed apart; one call with stats != NULL does both.
 * Rows read by cvf_ef16_finish: statistic-major, scratch [cvf_ef_nstats(k, lag_idx)][cvf_ef16_rows(B)] doubles (statistic i of
 * unit r at scratch[i * rows + r]); rows = 4 * ceil(B / 64), at most 16384 (cvf_ef16_rows returns 0 above, and the call is
 * refused).  With loss_vec == NULL neither loss_vec nor coef is touched. */
int64_t cvf_ef16_rows(int64_t B);
int cvf_ef16_finish(const cvf_ef_cfg* cfg, int64_t B, const double* scratch, double* stats, double* loss_vec, double* coef,
                    void* stream);
int cvf_ef16_front(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled, const cvf_pp_desc* pp,
                   const float* x, int64_t B, const float* a, float* y_tiled, float* saved, float* q_tiled, float* e_tiled,
                   const cvf_ef_cfg* cfg, const float* w, double* scratch, double* stats, double* loss_vec, double* coef,
                   void* stream);
int cvf_ef16_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, const float* packed, int64_t B,
                      const float* w, const float* feat_tiled, const float* y_tiled, const float* q_tiled, const double* coef,
                      float* slab, int32_t* step_count, const float* saved, void* stream);
/* A RESIDENT batch (csrc/ef16_front_rows.hip): the per-frame alignment records cvf_ef16_front solves for (rotation, centroid,
 * K^-1) depend on the coordinates and the layer only, not on the parameters, so a loop that visits the same frames again - the
 * static batches of core.py:472-481 - computes them once:
 *  cvf_ef16_align_rows : x [B][n_coord] -> rows (cvf_ef16_align_rows_floats(B) floats, 16-byte aligned; opaque: per unit of 16
 *                        frames the 16 x 21 floats the front kernel keeps on the chip, then the sum of the centred reference).
 *  cvf_ef16_align_rows_tile : the same launch also leaves the batch's FEATURE TILE - feat_tiled [T][d_r][64], T = cvf_ntiles(B), the
 *                        aligned positions exactly as cvf_ef16_front writes them (every unit of 4 T, frames past B as replicas of
 *                        the last one) - which depends on the coordinates and the layer only as well.
 *  cvf_ef16_front_rows : cvf_ef16_front (same arguments, same outputs BIT FOR BIT) starting from `rows` and the tile instead of
 *                        solving.  In this form `feat_tiled` is READ, NOT WRITTEN (layer 0's operand comes from it): it must be
 *                        the tile cvf_ef16_align_rows_tile left for the same `x`, and it is the `feat_tiled` cvf_ef16_backward
 *                        takes afterwards.  The caller answers for `rows` and the tile being those of exactly these B frames of
 *                        `x` under this `pp`. */
int64_t cvf_ef16_align_rows_floats(int64_t B);
int cvf_ef16_align_rows(const cvf_pp_desc* pp, const float* x, int64_t B, float* rows, void* stream);
int cvf_ef16_align_rows_tile(const cvf_pp_desc* pp, const float* x, int64_t B, float* rows, float* feat_tiled, void* stream);
int cvf_ef16_front_rows(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled, const cvf_pp_desc* pp,
                        const float* x, int64_t B, const float* a, float* y_tiled, float* saved, float* q_tiled, float* e_tiled,
                        const cvf_ef_cfg* cfg, const float* w, double* scratch, double* stats, double* loss_vec, double* coef,
                        const float* rows, void* stream);
/* ISOTROPIC metric: both front calls once more (same arguments, same outputs) for an `a` that holds ONE coefficient per record
 * atom, a[3b] == a[3b+1] == a[3b+2] for b < n_rec - ones, or 1 / mass.  Then R a_b R^T = a_b I, and q = J A J^T g and E are formed in
 * the aligned frame from the features alone: cross products instead of 3x3 products, no rotation, centroid or coordinate read
 * behind the alignment (the _rows_ form reads no coordinates at all).  The result is that of the general call up to fp32
 * reassociation; cvf_ef16_front_rows_iso and cvf_ef16_front_iso agree bit for bit.  The library cannot look at `a` (device memory):
 * the caller answers for the premise, and with an anisotropic `a` the result is wrong.  cvf_ef16_front / cvf_ef16_front_rows with
 * cfg->iso_metric = 1 are the same launches (what EigenFunctionTask sets); with 0, as in every earlier caller, they keep the general passes. */
int cvf_ef16_front_iso(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled, const cvf_pp_desc* pp,
                       const float* x, int64_t B, const float* a, float* y_tiled, float* saved, float* q_tiled, float* e_tiled,
                       const cvf_ef_cfg* cfg, const float* w, double* scratch, double* stats, double* loss_vec, double* coef,
                       void* stream);
int cvf_ef16_front_rows_iso(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                            const cvf_pp_desc* pp, const float* x, int64_t B, const float* a, float* y_tiled, float* saved,
                            float* q_tiled, float* e_tiled, const cvf_ef_cfg* cfg, const float* w, double* scratch, double* stats,
                            double* loss_vec, double* coef, const float* rows, void* stream);
/* Transfer-operator mode (lag_tau > 0; core.py:403,414: y = model(pp_layer(X)) on the frames and on their lagged partners, then
 * core.py:420-431,440 and loss.backward()) on the same kernels:
 *  cvf_ef16_front_transfer   : x, x_lag [B][n_coord] -> feat_tiled [2T][d_r][64], y_tiled [2T][k][64] (the partners' tiles follow
 *                              the frames'), saved (cvf_ef16_saved_floats(mlp, 2T)).  Follow with cvf_ef_stats (transfer mode).
 *  cvf_ef16_backward_transfer: slab rows of the parameter gradient from both passes; follow with cvf_slab_reduce. */
int cvf_ef16_front_transfer(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                            const cvf_pp_desc* pp, const float* x, const float* x_lag, int64_t B, float* y_tiled, float* saved,
                            void* stream);
/* ... and, for k <= 4 (cvf_ef16_transfer_rows(B, k) > 0), the units' rows of the TIME-LAGGED batch sums in the same launch: a block
 * takes a unit of the frames AND the same unit of their lagged partners, so that sum w (y' - y)^2 (core.py:428) is formed where both
 * values are; w, w_lag [B]; scratch as cvf_ef16_scratch_doubles.  Follow with cvf_ef16_finish / cvf_ef16_finish_dp (cfg.lag_idx > 0)
 * instead of cvf_ef_stats (two launches). */
int64_t cvf_ef16_transfer_rows(int64_t B, int k);
int cvf_ef16_front_transfer_rows(const cvf_mlp_desc* mlp, const float* theta, const float* packed, float* feat_tiled,
                                 const cvf_pp_desc* pp, const float* x, const float* x_lag, int64_t B, float* y_tiled, float* saved,
                                 const float* w, const float* w_lag, double* scratch, void* stream);
int cvf_ef16_backward_transfer(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, const float* packed, int64_t B,
                               const float* w, const float* w_lag, const float* feat_tiled, const float* y_tiled,
                               const double* coef, float* slab, int32_t* step_count, const float* saved, void* stream);

/* --- K5: batch statistics (core.py:406-416,426,428,446-452), fp64, fixed-order two
 * stage reduction.  w [B]; y_tiled [T][k][64]; generator: e_tiled [T][k][64];
 * transfer: y_lag_tiled, w_lag.  scratch: cvf_ef_stats_scratch_doubles() doubles. */
int64_t cvf_ef_stats_scratch_doubles(int k, int lag_idx);
int cvf_ef_stats(const cvf_ef_cfg* cfg, int64_t B, const float* w, const float* y_tiled, const float* e_tiled,
                 const float* w_lag, const float* y_lag_tiled, double* scratch, double* stats, double* loss_vec,
                 double* coef, void* stream); /* loss_vec/coef non-NULL: also run cvf_ef_loss in the same launch */

/* --- loss, eigenvalues, ordering and the partial derivatives d loss / d stat
 * (core.py:426-457 after the sums).  One wave; runs after the cross-rank all-reduce of
 * `stats` when there is one. */
int cvf_ef_loss(const cvf_ef_cfg* cfg, const double* stats, double* loss_vec, double* coef, void* stream);

/* --- K4b: parameter gradient of the loss given the coefficients (what loss.backward()
 * does at core.py:517): reverse mode over the nets and, in generator mode, over their
 * directional derivative along q.  Each block writes its partial sum to one row of
 * `slab` [cvf_ef_backward_slab_rows(n_tiles)][n_params]; cvf_slab_reduce then sums the rows
 * in fixed order into grad [n_params] (bitwise reproducible, no atomics).
 * transfer mode: feat/y hold 2T tiles (frames then their lagged partners); n_tiles = 2T. */
int64_t cvf_ef_backward_slab_rows(int64_t n_tiles);
int cvf_ef_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, const float* packed, int64_t B,
                    const float* w, const float* w_lag, const float* feat_tiled, const float* y_tiled,
                    const float* q_tiled, const double* coef, float* slab, int32_t* step_count, float* saved,
                    void* stream);
                    /* step_count (may be NULL): the optimiser's device step counter, advanced by one.  saved: the hand-off buffer of
                     * cvf_ef_mlp_fwd, cvf_ef_saved_floats(mlp, n_tiles) floats - NOT const: for first layers wider than 128 inputs
                     * the call writes t0 = W0 q behind the activations (the extra vector per (tile, net) that size includes). */
int cvf_slab_reduce(const float* slab, int64_t n_rows, int64_t n_params, float* grad, const cvf_adam_args* adam,
                    void* stream); /* adam (may be NULL): apply the update in the same launch */

/* --- K4a / K4b for nets of ANY shape (csrc/ef_general.hip; the reference takes any layer_dims, nn.py:29-59,242-293): one
 * launch per layer and pass over all tiles and nets instead of a compiled chain per (width, depth) - 1 to CVF_MAX_LAYERS - 1
 * hidden layers of 1 to 4096 units each (widths free to differ), d0 <= 65536, any act code of this header after each hidden
 * layer, scalar output, 1 <= n_nets <= CVF_MAX_NETS, nets that fill the flat buffer.  Same inputs and outputs as
 * cvf_ef_mlp_fwd / cvf_ef_backward (no fragment copy); `saved` is required and holds the activations, the backward sweep of g,
 * the tangent chain and the adjoints (opaque layout).  No atomics: the same inputs give the same gradient bit for bit.
 *  cvf_ef_general_supported   : 1, or 0 with the reason in cvf_last_error().
 *  cvf_ef_general_slab_rows   : rows of the gradient slab [rows][n_params] (128 MiB at most unless one row is larger).
 *  cvf_ef_general_saved_floats: floats of `saved`; n_tiles = T (lag_idx == 0) or 2T (transfer mode), as the two calls take.
 *  cvf_ef_general_fwd         : replaces self.model(...) at core.py:403,414 and the autograd.grad of core.py:424: y_tiled
 *                               [n_tiles][k][64] and, when g_tiled != NULL (generator mode), g_tiled [n_tiles][k][d0][64].
 *  cvf_ef_general_backward    : replaces loss.backward() at core.py:517: slab rows of the flat gradient (follow with
 *                               cvf_slab_reduce); step_count as cvf_ef_backward. */
int cvf_ef_general_supported(const cvf_mlp_desc* mlp);
int64_t cvf_ef_general_slab_rows(const cvf_mlp_desc* mlp, int64_t n_tiles);
int64_t cvf_ef_general_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles, int lag_idx);
int cvf_ef_general_fwd(const cvf_mlp_desc* mlp, const float* theta, const float* feat_tiled, int64_t n_tiles, float* y_tiled,
                       float* g_tiled, float* saved, void* stream);
int cvf_ef_general_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, const float* theta, int64_t B, const float* w,
                            const float* w_lag, const float* feat_tiled, const float* y_tiled, const float* q_tiled,
                            const double* coef, float* slab, int32_t* step_count, float* saved, void* stream);

/* --- The same for k nets that SHARE their first n_shared Linear layers (csrc/ef_general.hip), generator
 * mode only: the chains reg_i o encoder of RegAutoEncoderTask's regulariser (core.py:990,1008-1022: every reg_i reads the one
 * encoder) and the k components of the encoder in its gradient-norm penalty (core.py:896-910).  The sharing is stated by the
 * description: for l < n_shared, w_off[i][l] and b_off[i][l] are the same for every net i, and n_params counts those blocks
 * once; every other block is disjoint from all the rest, and the blocks fill the flat buffer.  0 <= n_shared <= n_layers - 1
 * (the hidden layers); shapes and limits as cvf_ef_general_supported.  The shared layers run forward once (one image of h_l for
 * all nets), their weights are read in place, and their gradient - the sum over the nets - is formed inside one launch, the
 * nets walked in the order 0..k-1: no atomics, the same inputs give the same bits.  n_shared = 0 is the launch list of the
 * calls above (and then takes any description those take whose blocks do not overlap).
 *  cvf_ef_general_shared_supported   : 1, or 0 with the reason in cvf_last_error().
 *  cvf_ef_general_shared_slab_rows   : as cvf_ef_general_slab_rows (which refuses a description with shared blocks).
 *  cvf_ef_general_shared_saved_floats: floats of `saved` for n_tiles = T tiles: the h_l of the shared layers once, everything
 *                                      else per net.
 *  cvf_ef_general_shared_fwd         : replaces self.model(...) at core.py:996 and the autograd.grad of core.py:1009 (and
 *                                      core.py:899,903 of the penalty): y_tiled [n_tiles][k][64], g_tiled [n_tiles][k][d0][64]
 *                                      (required: without it the call would be the transfer-mode step, which has entries of its own, below).
 *  cvf_ef_general_shared_backward    : replaces loss.backward() at core.py:1102 for these terms: slab rows of the flat gradient
 *                                      [rows][n_params], each shared entry written once (follow with cvf_slab_reduce).  A cfg
 *                                      with lag_idx != 0 is refused by name.
 * The four calls return a negative code (0 for the sizes), with the reason in cvf_last_error(), before any launch. */
int cvf_ef_general_shared_supported(const cvf_mlp_desc* mlp, int n_shared);
int64_t cvf_ef_general_shared_slab_rows(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared);
int64_t cvf_ef_general_shared_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared);
int cvf_ef_general_shared_fwd(const cvf_mlp_desc* mlp, int n_shared, const float* theta, const float* feat_tiled, int64_t n_tiles,
                              float* y_tiled, float* g_tiled, float* saved, void* stream);
int cvf_ef_general_shared_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, int n_shared, const float* theta, int64_t B,
                                   const float* w, const float* feat_tiled, const float* y_tiled, const float* q_tiled,
                                   const double* coef, float* slab, int32_t* step_count, float* saved, void* stream);

/* --- The shared trunk in TRANSFER mode (csrc/ef_general.hip): colvarsfinder.nn.SharedEigenFunctions under
 * EigenFunctionTask(lag_tau > 0) - the loss of core.py:403-457 on one trunk with k heads.  The description and its limits are those
 * of cvf_ef_general_shared_supported; n_tiles = 2T (the frames' tiles, then their lagged partners'), as on the plain general route.
 * Transfer mode has no tangent chain and no gamma term, so the adjoint that enters the trunk is the sum over the nets: the heads
 * run per net down to layer n_shared, ONE launch sums sigma'(h_{ns-1}) .* sum_i W_{ns,i}^T zbar_{ns,i} (the nets walked in the order
 * 0..k-1 into one accumulator; n_shared = n_layers - 1: sigma' .* sum_i alpha_i W_{NH,i}^T in the top step), the trunk
 * back-propagates once, and every weight gradient of a shared layer is one product from the summed adjoint, written once at the
 * shared offset of the slab row.  No atomics: the same inputs give the same bits.  n_shared = 0 is, launch for launch,
 * cvf_ef_general_fwd (g_tiled = NULL) / cvf_ef_general_backward (lag_idx != 0).
 *  cvf_ef_general_shared_transfer_supported   : 1, or 0 with the reason in cvf_last_error().
 *  cvf_ef_general_shared_transfer_slab_rows   : as cvf_ef_general_slab_rows.
 *  cvf_ef_general_shared_transfer_saved_floats: floats of `saved` = 64 n_tiles (sum_{l<ns} d_l + k (sum_{l>=ns} d_l + 2 max_l d_l + 1))
 *                                               over the hidden widths d_l: the trunk's h_l once (not k times), the heads' h_l per
 *                                               net, two ping-pong images of the adjoint, alpha.
 *  cvf_ef_general_shared_transfer_fwd         : replaces self.model(...) at core.py:403,414: y_tiled [n_tiles][k][64].
 *  cvf_ef_general_shared_transfer_backward    : replaces loss.backward() at core.py:517 (cvf_ef_stats between the two calls, follow
 *                                               with cvf_slab_reduce); step_count as cvf_ef_backward.  Refused by name: a
 *                                               generator-mode cfg (lag_idx == 0), a missing w_lag.
 * The calls return a negative code (0 for the sizes), with the reason in cvf_last_error(), before any launch. */
int cvf_ef_general_shared_transfer_supported(const cvf_mlp_desc* mlp, int n_shared);
int64_t cvf_ef_general_shared_transfer_slab_rows(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared);
int64_t cvf_ef_general_shared_transfer_saved_floats(const cvf_mlp_desc* mlp, int64_t n_tiles, int n_shared);
int cvf_ef_general_shared_transfer_fwd(const cvf_mlp_desc* mlp, int n_shared, const float* theta, const float* feat_tiled,
                                       int64_t n_tiles, float* y_tiled, float* saved, void* stream);
int cvf_ef_general_shared_transfer_backward(const cvf_ef_cfg* cfg, const cvf_mlp_desc* mlp, int n_shared, const float* theta,
                                            int64_t B, const float* w, const float* w_lag, const float* feat_tiled,
                                            const float* y_tiled, const double* coef, float* slab, int32_t* step_count,
                                            float* saved, void* stream);

/* --- AutoEncoder: weighted reconstruction loss and its parameter gradient in one pass
 * (core.py:664-666,708).  feat_rows [n][d0] row-major (the precomputed feature
 * trajectory of core.py:635); idx NULL or [B] frame indices into it; w [B]; inv_wsum =
 * 1/sum(w) (host-known: batches are static).  out2 [3] doubles: {sum w*err, sum w, their ratio = the loss}.
 * grad may be NULL (test pass, core.py:725-735). */
int64_t cvf_ae_scratch_floats(const cvf_mlp_desc* mlp, int64_t B);
int cvf_ae_step(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                const float* w, double inv_wsum, float* scratch, double* out2, float* grad, int32_t* step_count,
                const cvf_adam_args* adam, void* stream);
                /* step_count (may be NULL) is advanced by one when grad != NULL; adam (may be NULL): update in the same call */
/* The kernel cvf_ae_step launches for (mlp, theta, grad != NULL) - host arithmetic only, no launch: 0 = the register-resident
 * chain (ae16_kernel: tanh chains of d0 <= 80, hidden widths <= 32, at most 80 KiB of LDS, a 16-byte aligned theta, CVF_NO_AE16
 * unset in the environment), 1 / 2 = the general kernel (ae_mfma_kernel) on its roomy / tight LDS layout, negative = refused
 * (more than 160 KiB of LDS; cvf_last_error()).  lds_bytes (may be NULL): the launch's dynamic LDS.  cvf_ae_step itself decides
 * by this function.  CVF_NO_AE16 is consulted with getenv() on EVERY call of either function, so it can be set and cleared
 * while the process runs - by the thread that makes the calls: getenv is not safe against a concurrent setenv. */
int cvf_ae_step_route(const cvf_mlp_desc* mlp, const void* theta, int with_grad, int64_t* lds_bytes);

/* --- AutoEncoder chains of ANY width (csrc/ae_general.hip): the step for the chains cvf_ae_step_route
 * refuses - one launch per layer and pass over all 64-frame tiles, the activations handed over through `scratch`, instead of a
 * chain resident in LDS.  One chain (n_nets == 1, dims[0] == dims[n_layers]) of 1 to CVF_MAX_LAYERS layers, hidden widths 1 to
 * 4096, d0 <= 65536, at most 65535 blocks of 64 x 64 weights in a layer (d0 = 65536 beside a layer wider than 4032 passes it),
 * any act code of this header, parameters that fill the flat buffer; theta needs no alignment.  No atomics:
 * the same inputs give the same bits.
 *  cvf_ae_general_supported     : 1, or 0 with the reason in cvf_last_error().
 *  cvf_ae_general_scratch_floats: floats of `scratch` (8-byte aligned) for a batch of B frames, T = ceil(B / 64) tiles:
 *                                 64 T (d0 + sum of the hidden widths + 2 max(dims[1..n_layers])) for the tiled input, the saved
 *                                 activations and two adjoint images, R n_params slab rows with R = min(T, 256, 128 MiB /
 *                                 (4 n_params)) >= 1, rounded up to even, + 4 T for the tiles' loss pairs; 0 for a refused chain.
 *  cvf_ae_general_step          : the arguments, outputs and conventions of cvf_ae_step (out2, grad, step_count, adam). */
int cvf_ae_general_supported(const cvf_mlp_desc* mlp);
int64_t cvf_ae_general_scratch_floats(const cvf_mlp_desc* mlp, int64_t B);
int cvf_ae_general_step(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                        const float* w, double inv_wsum, float* scratch, double* out2, float* grad, int32_t* step_count,
                        const cvf_adam_args* adam, void* stream);

/* --- RegAutoEncoderTask (core.py:746-1217): time-lagged reconstruction loss
 * (weighted_MSE_loss, core.py:883-885) + transfer-operator eigenfunction regulariser (reg_eigen_loss with
 * lag_tau_reg > 0, core.py:973-1036) + the variance / covariance penalties on the latent vector (reg_enc_norm_loss,
 * reg_enc_orthognal_loss, core.py:912-971) + backward + optimizer step (core.py:1117,1128).  `mlp` is ONE chain: the
 * encoder's n_enc_layers layers, then the decoder and the K regulariser nets side by side as block-structured layers (built
 * by the host, colvarsfinder/core.py:_RegFlatParams), so that its last layer is [reconstruction (d_0 rows) | y_1..y_K].
 * feat_rows [n][d_0]: the feature trajectory; idx [B] (or NULL: 0..B-1): the batch's rows; rows idx + lag_target are
 * the reconstruction targets, rows idx + lag_input the lagged arguments of the regularisers (the generator-mode
 * regulariser and the gradient-norm penalty eta_0 of the reference are not built).
 *  cvf_regae_forward : y_tiled [2 T][K][64] (tiles 0..T-1: y on the rows idx, T..2T-1: on the lagged rows), enc_tiled
 *                      [T][k][64] (latent vector on the rows idx; NULL: not wanted) and out2 [3] = {sum w |dec(enc(f)) -
 *                      f_target|^2, sum w, their ratio}.  Then cvf_ef_stats (lag_idx > 0, k = K) on y_tiled gives the eigenfunction
 *                      terms and `coef`; cvf_ef_stats (lag_idx = 0, zero e_tiled) on enc_tiled + cvf_regae_enc_loss the
 *                      latent penalties and `enc_coef`.
 *  cvf_regae_backward: flat gradient of  mse_scale * sum w |..|^2 + head_scale * (npl + cfg.alpha * pen) + eta_1 norm +
 *                      eta_2 orth  in the chain's own parameter order (mse_scale = alpha / sum w, head_scale = gamma_0,
 *                      cfg.alpha = gamma_1 / gamma_0; coef / enc_coef NULL: that part is off), times `mask` (may be NULL;
 *                      zeros at the structural zeros of the block layers and at frozen parameters), + the Adam update
 *                      when adam != NULL; step_count as cvf_ae_step. */
int64_t cvf_regae_scratch_floats(const cvf_mlp_desc* mlp, int64_t B);
int cvf_regae_forward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                      int64_t lag_target, int64_t lag_input, int K, const float* w, float* scratch, float* y_tiled,
                      int n_enc_layers, float* enc_tiled, double* out2, void* stream);
int cvf_regae_backward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                       int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                       double head_scale, const float* y_tiled, const double* coef, int n_enc_layers, const double* enc_coef,
                       float* scratch, float* grad, const float* mask, int32_t* step_count, const cvf_adam_args* adam,
                       void* stream);
/* The two passes of ONE step on the same (theta, rows, lags): _keep leaves every tile's activations in `scratch`, _reuse reads
 * them instead of running the chain forward again (same arguments as the plain calls). */
int cvf_regae_forward_keep(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                      int64_t lag_target, int64_t lag_input, int K, const float* w, float* scratch, float* y_tiled,
                      int n_enc_layers, float* enc_tiled, double* out2, void* stream);
int cvf_regae_backward_reuse(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                       int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                       double head_scale, const float* y_tiled, const double* coef, int n_enc_layers, const double* enc_coef,
                       float* scratch, float* grad, const float* mask, int32_t* step_count, const cvf_adam_args* adam,
                       void* stream);
/* The LDS layout cvf_regae_forward / cvf_regae_backward take for (mlp, with_grad) - host arithmetic only, no launch: 1 / 2 = the
 * chain kernel (ae_mfma_kernel) on its roomy / tight layout, negative = refused (more than 160 KiB of LDS; cvf_last_error()).
 * lds_bytes (may be NULL): the launch's dynamic LDS.  The four calls above decide by this function. */
int cvf_regae_route(const cvf_mlp_desc* mlp, int with_grad, int64_t* lds_bytes);

/* --- RegAutoEncoderTask chains of ANY width (csrc/regae_general.hip): the calls for the merged chains
 * cvf_regae_route refuses - one launch per layer and pass over all 64-frame tiles (the kernels of cvf_ae_general_step), the
 * activations handed over through `scratch`.  One chain of 2 to CVF_MAX_LAYERS layers with dims[n_layers] == dims[0] + K,
 * 0 <= K <= CVF_MAX_NETS, inner widths 1 to 4096, d0 <= 65536, at most 65535 blocks of 64 x 64 weights in a layer, any act code
 * of this header, parameters that fill the flat buffer (the merged layers are dense: theta holds zeros off their blocks, `mask`
 * keeps them zero), 1 <= n_enc_layers < n_layers, no activation on the encoder's last layer, a latent vector of at most
 * CVF_MAX_NETS entries.  No atomics: the same inputs give the same bits.
 *  cvf_regae_general_supported     : 1, or 0 with the reason in cvf_last_error().
 *  cvf_regae_general_scratch_floats: floats of `scratch` (8-byte aligned) for a batch of B frames, T = ceil(B / 64): always laid
 *                                    out for 2 T tiles - 128 T (sum of dims[0..n_layers-1] + 2 max(dims[1..n_layers])), R n_params
 *                                    slab rows with R = min(2 T, 256, 128 MiB / (4 n_params)) >= 1, rounded up to even, + 4 T for
 *                                    the base tiles' loss pairs; 0 for a chain whose sizes are refused.
 *  cvf_regae_general_forward       : arguments and outputs of cvf_regae_forward; it always leaves its activation images in
 *                                    `scratch` (there is no _keep twin).
 *  cvf_regae_general_backward      : arguments and outputs of cvf_regae_backward; runs the chain forward again.
 *  cvf_regae_general_backward_reuse: the same from the images cvf_regae_general_forward left in `scratch` on the same (theta,
 *                                    rows, lags, K) - once: the call consumes them. */
int cvf_regae_general_supported(const cvf_mlp_desc* mlp, int K, int n_enc_layers);
int64_t cvf_regae_general_scratch_floats(const cvf_mlp_desc* mlp, int64_t B);
int cvf_regae_general_forward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                      int64_t lag_target, int64_t lag_input, int K, const float* w, float* scratch, float* y_tiled,
                      int n_enc_layers, float* enc_tiled, double* out2, void* stream);
int cvf_regae_general_backward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                       int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                       double head_scale, const float* y_tiled, const double* coef, int n_enc_layers, const double* enc_coef,
                       float* scratch, float* grad, const float* mask, int32_t* step_count, const cvf_adam_args* adam,
                       void* stream);
int cvf_regae_general_backward_reuse(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                       int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                       double head_scale, const float* y_tiled, const double* coef, int n_enc_layers, const double* enc_coef,
                       float* scratch, float* grad, const float* mask, int32_t* step_count, const cvf_adam_args* adam,
                       void* stream);
/* --- RegAutoEncoderTask with decoder and regulariser nets of DIFFERENT depths (csrc/regae_general.hip; DESIGN.md section 4.11;
 * core.py:884-897, 975-1034, 1066-1128): the calls above for a chain of n_enc_layers + max(n_dec_layers, n_reg_layers) layers,
 * n_dec_layers != n_reg_layers, both >= 1, 1 <= K <= CVF_MAX_NETS.  Behind the encoder every merged layer holds the rows of the
 * groups still alive, the deeper group's first.  With ls = n_enc_layers + min(n_dec_layers, n_reg_layers), the last `fin` of the
 * dims[ls] outputs of layer ls - 1 are the shallower group's outputs (fin = K heads when the decoder is deeper, else dims[0]
 * reconstruction rows): they take no activation, and layer ls reads the other dims[ls] - fin >= 1, so its matrix is dense
 * [dims[ls + 1]][dims[ls] - fin]; every other W_l is [dims[l + 1]][dims[l]].  dims[n_layers] is dims[0] (decoder deeper) or K.
 * The parameters fill the flat buffer; the other limits, the arguments, outputs, scratch formula (with this n_params) and
 * hand-off are those of the cvf_regae_general_* twin, which takes the equal depths these calls refuse.  No atomics. */
int cvf_regae_ragged_supported(const cvf_mlp_desc* mlp, int K, int n_enc_layers, int n_dec_layers, int n_reg_layers);
int64_t cvf_regae_ragged_scratch_floats(const cvf_mlp_desc* mlp, int64_t B, int K, int n_enc_layers, int n_dec_layers,
                                        int n_reg_layers);
int cvf_regae_ragged_forward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                      int64_t lag_target, int64_t lag_input, int K, const float* w, float* scratch, float* y_tiled,
                      int n_enc_layers, int n_dec_layers, int n_reg_layers, float* enc_tiled, double* out2, void* stream);
int cvf_regae_ragged_backward(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                       int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                       double head_scale, const float* y_tiled, const double* coef, int n_enc_layers, int n_dec_layers,
                       int n_reg_layers, const double* enc_coef, float* scratch, float* grad, const float* mask,
                       int32_t* step_count, const cvf_adam_args* adam, void* stream);
int cvf_regae_ragged_backward_reuse(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, const int64_t* idx, int64_t B,
                       int64_t lag_target, int64_t lag_input, int K, const float* w, const float* w_lag, double mse_scale,
                       double head_scale, const float* y_tiled, const double* coef, int n_enc_layers, int n_dec_layers,
                       int n_reg_layers, const double* enc_coef, float* scratch, float* grad, const float* mask,
                       int32_t* step_count, const cvf_adam_args* adam, void* stream);
/* latent penalties from the latent vector's batch sums (cvf_ef_stats layout [W, S1(k), S2(i<=j), ..]):
 * terms = {sum_j (var_j - 1)^2, sum_{i<j} cov_ij^2} (core.py:934, 966); enc_coef [k + k*k] for cvf_regae_backward */
int cvf_regae_enc_loss(const double* stats, int k, double eta1, double eta2, double* terms, double* enc_coef, void* stream);
/* row [7 + K] of the task's loss list (core.py:1112-1124): [loss, ae, npl, pen, eig_1..K, 0 (gradient-norm term), norm, orth]
 * with loss = alpha ae + gamma_0 npl + gamma_1 pen + eta_1 norm + eta_2 orth; from out2 (cvf_regae_forward), loss_vec
 * (cvf_ef_stats; NULL: regulariser off), enc_terms (cvf_regae_enc_loss; NULL: off); alpha = 0 leaves ae = 0 (core.py:1090). */
int cvf_regae_loss_row(const double* out2, const double* loss_vec, double alpha, double gamma0, double gamma1, int K,
                       const double* enc_terms, double eta1, double eta2, double* row, void* stream);

/* --- nets forward on row-major features (inference: colvar_model(), core.py:372-382,
 * 640-647).  out [B][n_out] where n_out = n_nets * d_L; upto_layer < n_layers stops a
 * single chain early (AutoEncoder encoder).  The chain stays in LDS: chains past 160 KiB are refused - wide chains, and
 * callers that also want d xi / d r, take cvf_cv_nets_eval below. */
int cvf_mlp_eval_rows(const cvf_mlp_desc* mlp, const float* theta, const float* feat_rows, int64_t B, int upto_layer,
                      float* out, void* stream);

/* --- a trained CV and its derivative in the features (csrc/cv_nets.hip): xi = nets(r) and
 * G = d xi / d r per frame, what self.model(...) and autograd through it give the callers of colvar_model() (core.py:372-382,
 * 640-647, 855-863).  One launch per layer and pass over all 64-frame tiles, activations handed over through `scratch`.  With
 * cvf_align_feature_fwd before it and cvf_align_feature_vjp_rows behind it, a C caller gets xi(x) and d xi / d x.
 * The model, read from cvf_mlp_desc (offsets may point anywhere inside theta; n_params is not read):
 *   form A  n_nets = k >= 2 scalar chains side by side (EigenFunctions), upto_layer = n_layers; weights per net;
 *   form B  n_nets = 1: the first upto_layer layers of one chain, k = dims[upto_layer] (the encoder of an AutoEncoder /
 *           RegAutoEncoder flat layout, or a bare chain; one Linear layer is legal).  The trunk runs once, not k times.
 * 1 to CVF_MAX_LAYERS layers, dims[0] from 1 to 65536, inner widths 1 to 4096, any act code of this header after any layer;
 * k <= CVF_MAX_NETS when g_rows or g_tiled is asked for (want_g), k <= 4096 for values alone.
 *  cvf_cv_nets_supported     : 1, or 0 with the reason in cvf_last_error(); the two calls below refuse the same models, before
 *                              any launch.
 *  cvf_cv_nets_scratch_floats: floats of `scratch` for B frames, T = ceil(B / 64): 64 T (dims[0] + c sum of dims[1..upto_layer]),
 *                              c = n_nets chains, + with want_g 128 T k max(dims[1..upto_layer-2]) (chains of three layers or
 *                              more); 0 for a refused model.
 *  cvf_cv_nets_eval          : exactly one of feat_rows [B][d_r] and feat_tiled [T][d_r][64] (as cvf_align_feature_fwd writes
 *                              it) -> xi_rows [B][k] and, each unless NULL, g_rows [B][k][d_r] (what cvf_align_feature_vjp_rows
 *                              reads) and g_tiled [T][k][d_r][64] (what cvf_metric_apply / cvf_metric_gram read; lanes of padded
 *                              frames hold exactly 0).  g_rows and g_tiled hold the same bits.
 * No atomics.  A frame's xi and g depend on its features and theta only - not on B, nor on the tile or lane the frame sits in.
 * Nothing is read from scratch or the outputs that the same call did not write. */
int cvf_cv_nets_supported(const cvf_mlp_desc* mlp, int upto_layer, int want_g);
int64_t cvf_cv_nets_scratch_floats(const cvf_mlp_desc* mlp, int upto_layer, int64_t B, int want_g);
int cvf_cv_nets_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const float* feat_rows,
                     const float* feat_tiled, int64_t B, float* xi_rows, float* g_rows, float* g_tiled, float* scratch,
                     void* stream);

/* --- xi(x) and d xi / d x per frame in ONE launch, one wave per frame (csrc/cv_frame.hip): the
 * deployment form of the three calls cvf_align_feature_fwd -> cvf_cv_nets_eval -> cvf_align_feature_vjp_rows for an MD engine
 * that biases along a learned CV and evaluates one frame (or a handful of replicas) per step.  The alignment, the features, the
 * nets' forward pass, their sweep and the coordinate part all stay in the LDS of the frame's workgroup (64 threads, grid B).
 *   x [B][n_coord] -> xi_rows [B][k] and
 *     coef == NULL : gx_rows [B][k][n_coord], row i = d xi_i / d x (the layout of cvf_align_feature_vjp_rows);
 *     coef [B][k]  : gx_rows [B][n_coord] = sum_i coef[b][i] d xi_i / d x (the bias force up to sign); the sum is taken at the
 *                    feature level, g = sum_i coef_i d xi_i / d r, so the coordinate part runs once, not k times.
 * The model is described as for cvf_cv_nets_eval (form A: n_nets = k scalar chains, upto_layer = n_layers; form B: the first
 * upto_layer layers of one chain, k = dims[upto_layer], the trunk forward once); any act code after any layer.
 *  cvf_cv_frame_supported: 1, or 0 with the reason in cvf_last_error() - it names the three-call recipe, which takes every shape
 *    this launch declines.  Accepted: CVF_PP_ALIGN and CVF_PP_FEATURES with n_coord <= 192 (align_w honoured, n_align <= 64;
 *    flags are ignored: only rec, align_idx, ref_c and align_w are read), CVF_PP_IDENTITY with n_coord <= 512; dims[0] == d_r <= 512,
 *    inner widths <= 256, 1 to CVF_MAX_LAYERS layers, k <= CVF_MAX_NETS; a workgroup LDS total (the frame, every layer's
 *    activations, two sweep vectors, k rows of d xi / d r, of per-record contributions and of the gradient image) of at most
 *    64 KiB.  CVF_PP_FACTORED is refused.
 *  cvf_cv_frame_eval: no aux, no scratch, no allocation, no host synchronisation, no atomics.  Every refusal happens before any
 *    launch (negative code, cvf_last_error()); B == 0 returns 0 and writes nothing.  xi_rows and gx_rows are fully written for
 *    rows < B; the gradient is exactly 0 on atoms that are neither aligned nor read by a feature.  Every dot product of the nets
 *    is a sequential sum in index order inside one lane, every sum over lanes a fixed tree: a frame's result depends on its own
 *    coordinates and theta only - not on B, nor on its place in the batch - and two calls give the same bits.
 * Large batches (the launch keeps one wave per frame busy with work a 64-frame tile shares), large molecules and wide nets
 * belong to the three-call recipe. */
int cvf_cv_frame_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp);
int cvf_cv_frame_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp, const float* x,
                      int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream);

/* --- the same for frames of ANY size: one launch, one WORKGROUP of 256 threads per frame, grid B (csrc/cv_frame_large.hip;
 * DESIGN.md section 4.16).  What a caller of colvar_model() (core.py:372-382) or of the scripted CV (save_model, core.py:205-226)
 * gets from autograd through the alignment + feature layer and the nets (examples/dipeptide/main.ipynb:333-348), for molecules past
 * the 64 atoms of cvf_cv_frame_eval.  Arguments, outputs and the meaning of coef are those of cvf_cv_frame_eval exactly; the two
 * kernels are independent (shapes below 64 atoms are accepted here too).  The frame stays in global memory; the features, the
 * nets' activations, d xi / d r and the table of contribution rows (n_ref * 12 bytes per cotangent row) live in the workgroup's
 * dynamic LDS, and the coordinate part walks the cotangent rows in passes of rows_per_pass.
 *  cvf_cv_frame_large_supported: 1, or 0 with the reason in cvf_last_error(), which names the limit and the three-call recipe.
 *    Accepted: CVF_PP_ALIGN (any n_align >= 3, align_w honoured) and CVF_PP_FEATURES with n_coord any positive multiple of 3;
 *    the nets' limits of cvf_cv_frame_eval (dims[0] == d_r <= 512, inner widths <= 256, 1 to CVF_MAX_LAYERS layers,
 *    k <= CVF_MAX_NETS, both forms); n_slot <= CVF_FEATURES_MAX_SLOT, n_ref <= CVF_FEATURES_MAX_REF; the tables mrec (n_mrec > 0),
 *    slot_row, slot_atom, atom_slot and, for CVF_PP_ALIGN, atom_align; an LDS total within 160 KiB with rows_per_pass >= 1.
 *    CVF_PP_IDENTITY (cvf_cv_frame_eval takes it) and CVF_PP_FACTORED are refused.
 *  cvf_cv_frame_large_lds_bytes: the dynamic LDS of one frame for coef == NULL, in bytes, and through rows_per_pass (may be NULL)
 *    the cotangent rows per pass, min(k, what fits) - or a negative code for a model the predicate refuses.
 *  cvf_cv_frame_large_eval: no aux, no scratch, no allocation, no host synchronisation, no atomics.  Every refusal happens before
 *    any launch (negative code, cvf_last_error()) and leaves the outputs untouched; B == 0 returns 0 and writes nothing.  Every
 *    element of xi_rows and gx_rows of rows < B is written exactly once; the gradient is exactly 0 on atoms that are neither
 *    aligned nor read by a feature.  Every sum has a fixed order (a thread's own terms in index order, wave_sum inside a wave,
 *    the four waves in index order), and a row's arithmetic does not depend on the pass it falls in: a frame's result depends on
 *    its own coordinates and theta only - not on B, nor on its place in the batch - and two calls give the same bits. */
int cvf_cv_frame_large_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp);
int64_t cvf_cv_frame_large_lds_bytes(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp, int32_t* rows_per_pass);
int cvf_cv_frame_large_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp, const float* x,
                            int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream);

/* --- a trained CV as ONE self-contained file, and its binder (csrc/cv_file.hip; parser and validator: csrc/cvf_cv_file.hpp, host
 * C++ without a HIP include).  colvarsfinder.export.save_cv_file writes it; a C caller reads the bytes, asks for the size of the
 * device buffer, allocates it and binds:
 *   cvf_cv_file_device_bytes(blob, nbytes)  -> bytes of dev_buf (> 0), or a negative code and a message naming the offending field;
 *   cvf_cv_file_bind(blob, nbytes, dev_buf, dev_bytes, &model, stream) -> model.mlp / model.pp / model.theta point into dev_buf
 *     (16-byte aligned, at least the size above), ready for cvf_cv_frame_eval - or, for shapes cvf_cv_frame_supported declines,
 *     for the three-call recipe: the file holds ALL tables of the layer, not only those the one-launch kernel reads.
 * `blob` is HOST memory (unlike the rest of this header).  cvf_cv_file_bind is a SET-UP call: it copies the table region in one
 * host-to-device copy on `stream` and SYNCHRONISES the stream before it returns (the blob may be freed right away); it does not
 * allocate.  cvf_cv_file_device_bytes touches no device.
 * Layout, little-endian, int32 unless noted:
 *   0    magic "CVF1", format version (1), CVF_MAX_NETS, CVF_MAX_LAYERS as written
 *   16   the cvf_mlp_desc fields in struct order (n_nets, n_layers, dims, act, w_off, b_off, n_params)
 *   896  mode, n_coord, n_align, n_rec, d_r, use_angle_value, has_position, flags, n_slot, n_rec_slot, n_mrec, n_ref
 *   944  upto_layer, k, number of directory entries, n_shared (0: forms A and B, as every file written before form C has it;
 *        > 0: form C below - theta holds the trunk once, and the offsets of its layers are the same for every net)
 *   960  directory: per table { name id, element type (0 int32, 1 float32), int64 count, int64 byte offset in the file }, one
 *        entry for EVERY id below (count 0 = the layer has no such table: the descriptor's pointer is NULL)
 *   then the tables, each 16-byte aligned, in the order of their offsets.
 * A file that is truncated, carries counts that disagree with the scalar fields, an atom index >= n_coord / 3, an output offset
 * past d_r, a parameter offset past theta, an unknown act code, type id or table id is refused before any pointer is formed. */
enum {
  CVF_FILE_ALIGN_IDX = 1, CVF_FILE_REF_C = 2, CVF_FILE_REC = 3, CVF_FILE_ALIGN_W = 4, CVF_FILE_ATOM_ALIGN = 5,
  CVF_FILE_ATOM_SLOT = 6, CVF_FILE_REC_SLOT = 7, CVF_FILE_SLOT_ATOM = 8, CVF_FILE_MREC = 9, CVF_FILE_SLOT_ROW = 10,
  CVF_FILE_THETA = 11, CVF_FILE_N_TABLES = 11
};
#define CVF_FILE_VERSION 1
typedef struct cvf_cv_model {
  cvf_mlp_desc mlp;
  cvf_pp_desc pp;
  const float* theta;   /* device, cvf_mlp_desc.n_params floats */
  int32_t upto_layer, k;
} cvf_cv_model;
int64_t cvf_cv_file_device_bytes(const void* blob_host, int64_t nbytes);
int cvf_cv_file_bind(const void* blob_host, int64_t nbytes, void* dev_buf, int64_t dev_bytes, cvf_cv_model* out, void* stream);

/* --- form C: k scalar chains on ONE trunk (csrc/cvf_cv_shared.hpp).  What nn.SharedEigenFunctions is,
 * and what RegAutoEncoderTask.reg_model() returns (reference nn.py:205-240: RegModel, the encoder followed by the K regulariser
 * nets in the order cvec; core.py:870-877: reg_model()) - the eigenfunctions that task learns.  Form C is form A plus n_shared:
 *   n_nets = k >= 1 scalar chains of one architecture, evaluated whole (k = 1 is legal);
 *   1 <= n_shared <= n_layers - 1: the chains' first n_shared layers are one set of tensors,
 *   w_off[i][l] == w_off[0][l] and b_off[i][l] == b_off[0][l] for every l < n_shared and every net i (the convention of
 *   cvf_ef_general_shared_*); a description that breaks it is refused before any launch, with the net and the layer named.
 * Any act code after any layer, CVF_ACT_NONE at the boundary included (a RegModel's encoder ends in a bare Linear layer).
 * The trunk runs ONCE per frame, forward.  In the sweep the k head sweeps stop at layer n_shared; below it the Jacobian rows
 * carry k vectors through the shared weights, and the coef form contracts at the boundary, v = sum_i coef_i v_i, and carries one.
 * Every entry point mirrors its namesake without _shared - arguments, outputs, limits and guarantees - with n_shared where that
 * one takes upto_layer; n_shared == 0 is refused with a message that names the namesake, B == 0 returns 0 and writes nothing.
 * With coef == NULL a row's arithmetic is that of form A on the same (aliased) description: xi and every gradient row hold the
 * same bits.  The coef form sums in another order (at the boundary, not at the features).
 *  cvf_cv_nets_shared_scratch_floats: 64 T (dims[0] + sum of dims[1..n_shared] + k sum of dims[n_shared+1..n_layers]), + with
 *    want_g 128 T k max(dims[1..n_layers-2]): the trunk's images once.
 *  cvf_cv_frame_shared_supported / cvf_cv_frame_large_shared_supported: the limits of their namesakes with the LDS total of form
 *    C - the trunk's activations once, plus two images of k max(dims[1..n_shared]) floats for the trunk's sweep.
 *  cvf_cv_file_n_shared: the word at byte 956 of a file cvf_cv_file_device_bytes accepts (0: call the entry points without
 *    _shared with model.upto_layer; > 0: call the _shared ones with it), or that call's negative code.  cvf_cv_model keeps its
 *    size and fields. */
int cvf_cv_nets_shared_supported(const cvf_mlp_desc* mlp, int n_shared, int want_g);
int64_t cvf_cv_nets_shared_scratch_floats(const cvf_mlp_desc* mlp, int n_shared, int64_t B, int want_g);
int cvf_cv_nets_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const float* feat_rows,
                            const float* feat_tiled, int64_t B, float* xi_rows, float* g_rows, float* g_tiled, float* scratch,
                            void* stream);
int cvf_cv_frame_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp);
int cvf_cv_frame_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp, const float* x,
                             int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream);
int cvf_cv_frame_large_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp);
int64_t cvf_cv_frame_large_shared_lds_bytes(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp, int32_t* rows_per_pass);
int cvf_cv_frame_large_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp, const float* x,
                                   int64_t B, const float* coef, float* xi_rows, float* gx_rows, void* stream);
int cvf_cv_file_n_shared(const void* blob_host, int64_t nbytes);

/* --- bias energy and forces along the CV in ONE launch, in the MD engine's own arrays (csrc/cv_bias.hip; the term formulas:
 * csrc/cvf_bias.hpp, host and device from one text).  The coefficient of a bias force is -dU/dxi_i(xi(x)):
 * it depends on the xi the launch is computing, so with cvf_cv_frame_eval an engine launches twice around a host round trip, or
 * takes all k gradient rows.  Here lanes i < k evaluate the bias on the xi in LDS, and the contracted sweep is seeded from there.
 *   U(xi) = sum over term[0 .. n_terms) of U_t(xi[cv_t]); several terms may name one CV (a restraint plus two walls); the sums
 *   over terms run in term order inside one lane.
 *     CVF_BIAS_HARMONIC    kappa (xi - center)^2 / 2
 *     CVF_BIAS_UPPER_WALL  kappa (xi - center)^2 / 2 for xi > center, else 0
 *     CVF_BIAS_LOWER_WALL  kappa (xi - center)^2 / 2 for xi < center, else 0
 *     CVF_BIAS_LINEAR      kappa xi
 *     CVF_BIAS_TABLE       a uniform 1-D grid: nodes j = 0 .. n_nodes - 1 at lo + j / inv_h, the pair (U_j, U'_j) at
 *                          table[tab_off + 2 j]; cubic Hermite interpolation - U is C1 and the force is the exact derivative of
 *                          the interpolated U; xi on the last node belongs to the last interval; below lo and above the last node
 *                          U continues linearly with the end node's value and slope.  `table` (device, n_table floats) is read
 *                          AT LAUNCH TIME: metadynamics or ABF update it in place between launches, a captured graph stays valid.
 *   cvf_cv_bias_check(bias, k): 1, or 0 with the reason - which names the field - in cvf_last_error(): a known kind, 0 <= cv < k,
 *     finite kappa, center and lo, and for a table inv_h > 0, n_nodes >= 2, tab_off >= 0 and even, tab_off + 2 n_nodes <= n_table,
 *     table != NULL; 0 <= n_terms <= CVF_BIAS_MAX_TERMS.  Host arithmetic; every eval below refuses what it refuses.
 * cvf_md_layout: atom a (0 .. n_coord / 3) of replica b is read from x_all[b x_frame_stride + atom_index[a] atom_stride + c],
 * c = 0, 1, 2, and the force is ACCUMULATED at the same place of f_all with its own frame stride:
 *     f_all[...] += - sum_t U_t'(xi) d xi / d x
 *   atom_index (device, n_coord / 3 entries WITHOUT REPEATS - the caller vouches for it) or NULL for the identity; atom_stride >= 3
 *   floats per atom.  Each element is touched by exactly one thread; elements of other atoms, the padding floats of a 4-float atom
 *   and the gaps between frames are neither read nor written.  The three floats of EVERY atom of the CV's group are read and
 *   written, those whose gradient is an exact 0 included (a -0.0f there becomes +0.0f).  x_all is only read: its frames may
 *   overlap or repeat (x_frame_stride = 0 broadcasts one frame).  The force frames of a batch must not overlap: with B > 1 the
 *   caller vouches that f_frame_stride is past the last float of a frame's atoms, as it vouches for "no repeats"; a stride below
 *   (n_coord / 3 - 1) atom_stride + 3, which no index can fit in, is refused.  A NULL layout pointer means the dense
 *   [B][n_coord] arrays of cvf_cv_frame_eval (still +=).  With atom_index n_coord must be a multiple of 3 (a CVF_PP_IDENTITY model with another n_coord
 *   is refused by name).
 * The four evals take forms A, B and C (_shared) as their namesakes cvf_cv_frame[_large][_shared]_eval do, under the same limits
 * (the wave kernel keeps 2 k more floats of LDS inside its 64 KiB; the workgroup kernel reuses the alignment's):
 *   xi_rows [B][k]; u_rows [B] = U; du_rows [B][k] (may be NULL), du_rows[b][i] = sum_{t: cv_t = i} U_t'(xi_i) - minus the
 *   coefficient the launch used (ABF-style estimators want it); f_all accumulated as above.
 * One launch; no aux, no scratch, no allocation, no host synchronisation, no atomics; fixed summation orders; a frame's bits do
 * not depend on B nor on its place in the batch; xi_rows holds the bits of the namesake's, and the force added to a zero-filled
 * dense f_all those of the namesake's coef form with coef = -du_rows.  Every refusal (the namesake's, the bias check, the layout)
 * happens before any launch and leaves the outputs untouched; B == 0 returns 0 and writes nothing. */
#define CVF_BIAS_MAX_TERMS 16
enum { CVF_BIAS_HARMONIC = 0, CVF_BIAS_UPPER_WALL = 1, CVF_BIAS_LOWER_WALL = 2, CVF_BIAS_LINEAR = 3, CVF_BIAS_TABLE = 4 };
typedef struct cvf_bias_term {
  int32_t kind;     /* CVF_BIAS_* */
  int32_t cv;       /* the CV the term acts on, 0 .. k - 1 */
  float kappa;      /* not CVF_BIAS_TABLE */
  float center;     /* harmonic and walls */
  int32_t tab_off;  /* CVF_BIAS_TABLE: node j's (U_j, U'_j) at table[tab_off + 2 j] */
  int32_t n_nodes;
  float lo;         /* position of node 0 */
  float inv_h;      /* 1 / node spacing */
  int32_t cv2;      /* CVF_BIAS_TABLE with n_nodes2 >= 2: the second CV of a joint grid (below), 0 .. k - 1 and not cv */
  int32_t n_nodes2; /* 0: the 1-D table, whatever cv2, lo2 and inv_h2 hold; >= 2: nodes along cv2 */
  float lo2;        /* position of node 0 along cv2 */
  float inv_h2;     /* 1 / node spacing along cv2 */
} cvf_bias_term;
typedef struct cvf_bias_desc {
  int32_t n_terms;
  int32_t n_table;      /* floats behind `table` */
  cvf_bias_term term[CVF_BIAS_MAX_TERMS];
  const float* table;   /* device; NULL when no term is a table */
} cvf_bias_desc;
typedef struct cvf_md_layout {
  const int32_t* atom_index;   /* device [n_coord / 3], or NULL: atom a is the engine's atom a */
  int32_t atom_stride;         /* floats per atom, >= 3 */
  int32_t reserved;            /* 0 */
  int64_t x_frame_stride;      /* floats between the replicas of x_all */
  int64_t f_frame_stride;      /* floats between the replicas of f_all */
} cvf_md_layout;
int cvf_cv_bias_check(const cvf_bias_desc* bias, int k);
int cvf_cv_frame_bias_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp);
int cvf_cv_frame_bias_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                           const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B, float* xi_rows,
                           float* u_rows, float* du_rows, float* f_all, void* stream);
int cvf_cv_frame_bias_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp);
int cvf_cv_frame_bias_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                  const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                  float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream);
int cvf_cv_frame_large_bias_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp);
int cvf_cv_frame_large_bias_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                 const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B, float* xi_rows,
                                 float* u_rows, float* du_rows, float* f_all, void* stream);
int cvf_cv_frame_large_bias_shared_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp);
int cvf_cv_frame_large_bias_shared_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                        const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                        float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream);

/* --- periodic cells in the bias launches: whole molecules and the virial (csrc/cv_bias.hip; the rule: csrc/cvf_cell.hpp, host and
 * device from one text).  An MD engine keeps its atoms wrapped into the periodic cell, so a molecule that
 * crosses a cell face arrives torn.  The four _cell_eval calls take the arguments of their namesakes plus a cvf_md_cell and make the
 * CV's atoms whole INSIDE the launch, before the alignment or any feature reads them; the namesakes are unchanged.
 *   cell: 9 floats per frame, the lattice vectors as rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz) (the reduced
 *     lower-triangular form of OpenMM, GROMACS and LAMMPS), device memory read AT LAUNCH TIME - a barostat rescales it in place and a
 *     captured graph stays valid; frame b's cell is cell + b cell_frame_stride (0: one cell for all replicas).  An axis whose
 *     diagonal entry is 0, negative or not finite is not periodic (a slab: cz = 0); the upper triangle is never read.
 *   rule: atom 0 of the CV's atom order (the order of atom_index) stays where the engine has it; atom j takes the periodic image
 *     nearest to the whole atom j - 1 (PLUMED's WHOLEMOLECULES), the minimum image taken axis by axis in the order z, y, x with
 *     n = rint(d / diagonal).  The image counts are summed as integers, so the result does not depend on how the launch associates
 *     them; the subtraction x_j - (N.x a + N.y b + N.z c) has one form (csrc/cvf_cell.hpp), shared by every kernel and the host; an
 *     atom whose count is 0 keeps its bits.  Counts saturate at +-511 images per axis.
 *   precondition: consecutive atoms of the CV lie closer than half the shortest cell height; frames are whole atoms.
 *   forces: the shift is piecewise constant, so f_all gets the gradient at the whole positions, at the engine's own atom slots.
 *   virial_rows (optional, [B][9]): virial_rows[b][3 i + j] = sum_a r_a[i] f_a[j], r the whole position the launch used and f the
 *     force it adds to f_all; a fixed summation order, no atomics, a frame's 9 floats do not depend on B.  The caller applies its
 *     engine's sign and factor.  virial_rows is also taken with cell == NULL inside the struct: the virial of positions that the
 *     engine keeps whole, the forces then the namesake's bit for bit.
 *   refused before any launch, outputs untouched: what the namesake refuses; a NULL cvf_md_cell pointer; n_coord % 3 != 0; a negative
 *     cell_frame_stride; cell == NULL and virial_rows == NULL together.
 *   limits: those of the namesakes; the workgroup kernel keeps 4 more bytes of LDS per atom (the summed image counts), which the
 *     _cell_supported predicates count.
 * xi_rows, u_rows, du_rows and the force are, bit for bit, those of the namesake on the dense output of cvf_md_make_whole.
 * cvf_md_make_whole: the same rule stand-alone, one workgroup per frame, any n_atoms: atom a of frame b is read through `layout`
 *   (NULL: dense [B][3 n_atoms]; f_frame_stride is not used) and written whole to x_whole[b][3 a ..], dense.  cell->cell is needed,
 *   cell->virial_rows is not used. */
typedef struct cvf_md_cell {
  const float* cell;          /* device, 9 floats per frame (lower-triangular rows), or NULL: positions are whole already */
  int64_t cell_frame_stride;  /* floats between the replicas' cells; 0: one cell for all */
  float* virial_rows;         /* device [B][9], or NULL */
} cvf_md_cell;
int cvf_cv_frame_bias_cell_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp);
int cvf_cv_frame_bias_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B, float* xi_rows,
                                float* u_rows, float* du_rows, float* f_all, void* stream, const cvf_md_cell* cell);
int cvf_cv_frame_bias_shared_cell_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp);
int cvf_cv_frame_bias_shared_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                       const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                       float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream,
                                       const cvf_md_cell* cell);
int cvf_cv_frame_large_bias_cell_supported(const cvf_mlp_desc* mlp, int upto_layer, const cvf_pp_desc* pp);
int cvf_cv_frame_large_bias_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int upto_layer, const cvf_pp_desc* pp,
                                      const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                      float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream,
                                      const cvf_md_cell* cell);
int cvf_cv_frame_large_bias_shared_cell_supported(const cvf_mlp_desc* mlp, int n_shared, const cvf_pp_desc* pp);
int cvf_cv_frame_large_bias_shared_cell_eval(const cvf_mlp_desc* mlp, const float* theta, int n_shared, const cvf_pp_desc* pp,
                                             const cvf_bias_desc* bias, const cvf_md_layout* layout, const float* x_all, int64_t B,
                                             float* xi_rows, float* u_rows, float* du_rows, float* f_all, void* stream,
                                             const cvf_md_cell* cell);
int cvf_md_make_whole(const cvf_md_layout* layout, const cvf_md_cell* cell, const float* x_all, int64_t n_atoms, int64_t B,
                      float* x_whole, void* stream);

/* --- metadynamics along the CV: joint 2-D grid terms and hill deposition on the device (csrc/cvf_bias.hpp, csrc/cv_bias_hills.hip;
 * DESIGN.md section 4.19).
 * A CVF_BIAS_TABLE term with n_nodes2 >= 2 is a joint grid U(xi_cv, xi_cv2) (n_nodes2 == 0: the 1-D table above, bit for bit):
 *   node (j1, j2), j2 fastest, at (lo + j1 / inv_h, lo2 + j2 / inv_h2) holds the four floats (U, d1 U, d2 U, d12 U) at
 *   table[tab_off + 4 (j1 n_nodes2 + j2)]; tab_off is a multiple of 4 and `table` 16-byte aligned (a node is one 16-byte access).
 *   Inside the grid U is the bicubic Hermite interpolant of the cell - the tensor product of the 1-D basis, d_a U scaled by h_a and
 *   d12 U by h1 h2 - so U is C1 and the two gradient components are the exact gradient of that polynomial.  Outside, with P = xi
 *   clamped to the grid per axis and d = xi - P:
 *     U = U(P) + d1U(P) d_1 + d2U(P) d_2 + d12U(P) d_1 d_2,   d1 U = d1U(P) + d12U(P) d_2,   d2 U = d2U(P) + d12U(P) d_1
 *   (the 1-D rule per axis: C1 across every edge and corner, the force stays the exact gradient).  NaN takes the "below" branch; xi
 *   on the last node line belongs to the last cell; on a node the node's values come back bit for bit.
 *   In the launches above lane i < k sums in term order: its 1-D terms; for a 2-D term with cv == i its U and dU/dxi_cv; for a 2-D
 *   term with cv2 == i only dU/dxi_cv2.  du_rows[b][i] is that sum; u_rows, the sweep and the force are as before.
 *   cvf_cv_bias_check additionally refuses, naming the field: n_nodes2 == 1 or negative, cv2 outside 0 .. k - 1 or equal to cv, a
 *   non-finite lo2, inv_h2 not positive and finite, tab_off % 4 != 0, tab_off + 4 n_nodes n_nodes2 > n_table (in 64 bits), a table
 *   that is not 16-byte aligned.
 * cvf_cv_bias_deposit adds B Gaussian hills to ONE table term (1-D or 2-D) of `bias`, in place, centred on the xi_rows [B][k] a bias
 * launch wrote (device):  hill b has the centre c = (xi_b[cv], xi_b[cv2]) and the height
 *     w_b = height exp(-V_b inv_kdt),   V_b = the TARGET TERM's own U at c (not the whole bias), read through the interpolation above
 *                                             from the table as it is BEFORE any hill of this call (inv_kdt == 0: w_b = height)
 *   hills [B][4] (device, written) = (c_1, c_2 (0 in 1-D), w_b, V_b): the caller's HILLS log and reweighting input.  A non-finite
 *   centre, or a w_b that is not finite (exp overflows on a very negative V_b), gives w_b = 0 and the hill is skipped: no node
 *   receives NaN.  Every node, at x = lo + (float)j / inv_h per axis in fp32,
 *   with delta = x - c and G = exp(-(delta_1^2 / sigma^2 + delta_2^2 / sigma2^2) / 2), takes
 *     U += w G,  d1 U += -w G delta_1 / sigma^2,  d2 U += -w G delta_2 / sigma2^2,  d12 U += w G delta_1 delta_2 / (sigma^2 sigma2^2)
 *   (1-D: the first two).  Full Gaussians, no cut-off: values and slopes stay the exact derivatives of one smooth function.
 *   Two launches on `stream` - the heights (one thread per hill), then the nodes (one thread per node: read once, the hills added in
 *   order b = 0 .. B - 1 in registers, staged through LDS CVF_HILL_CHUNK at a time, written once) - because every height must see the
 *   table before any workgroup has written to it.  No atomics, no allocation, no host synchronisation; graph-capturable on one stream
 *   behind the launch that writes xi_rows; the bits do not depend on the launch geometry, and with inv_kdt == 0 one call of B hills
 *   gives the bits of B calls of one hill each.  Refused before any launch, table and hills untouched: what cvf_cv_bias_check refuses;
 *   term out of range or no CVF_BIAS_TABLE; height, sigma or (2-D) sigma2 not positive and finite, or so small that 1 / sigma^2
 *   overflows fp32; inv_kdt negative or not finite;
 *   table != bias->table; NULL pointers; B < 0.  B == 0 returns 0 and writes nothing. */
#define CVF_HILL_CHUNK 64
typedef struct cvf_hill_desc {
  int32_t term;         /* index of the CVF_BIAS_TABLE term (1-D or 2-D) that receives the hills */
  int32_t reserved;     /* 0 */
  float height;         /* w0 > 0 */
  float sigma, sigma2;  /* widths along cv and cv2 (sigma2 unused in 1-D), > 0 */
  float inv_kdt;        /* well-tempered: 1 / (k_B dT) = 1 / ((gamma - 1) k_B T) in the units of U; 0 = plain metadynamics */
} cvf_hill_desc;
int cvf_cv_bias_deposit(const cvf_bias_desc* bias, int k, const cvf_hill_desc* hill, const float* xi_rows, int64_t B, float* table,
                        float* hills, void* stream);

/* --- K6: Adam (torch.optim.Adam defaults as constructed at core.py:164: betas
 * (0.9,0.999), eps 1e-8, no weight decay, no amsgrad), one launch over the flat buffer.
 * step_count is a device int32 holding the number t of the CURRENT step (>= 1): it is advanced by the
 * gradient-producing call of the step (cvf_slab_reduce / cvf_ae_step), so a captured step replays
 * correctly without host involvement. */
int cvf_adam_step(float* theta, const float* grad, float* m, float* v, int64_t n, double lr, const float* lr_dev,
                  double beta1, double beta2, double eps, int32_t* step_count, const cvf_mlp_desc* mlp, float* packed,
                  void* stream);   /* lr_dev (may be NULL): device scalar overriding lr, as in cvf_adam_args */
int cvf_sgd_step(float* theta, const float* grad, int64_t n, double lr, const float* lr_dev, const cvf_mlp_desc* mlp,
                 float* packed, void* stream); /* mlp/packed: NULL, or the nets' desc + fragment buffer to refresh */

/* --- cross-rank sums of the data-parallel step (the reference has no multi-GPU path): RCCL all-reduces
 * (in place, SUM) issued on `stream`, for hosts that bind this library without PyTorch - one process per GPU, the caller's
 * current HIP device at cvf_comm_init is the rank's GPU.  Collective #1 = the fp64 batch sums between cvf_ef16_front /
 * cvf_ef_stats (loss_vec == NULL) and cvf_ef_loss; collective #2 = the fp32 flat gradient between cvf_slab_reduce
 * (adam == NULL) and cvf_adam_step.  Rank 0 calls cvf_comm_unique_id and hands the cvf_comm_unique_id_bytes() bytes to the
 * other ranks by any means (the shipped Python host: torch.distributed broadcast); RCCL is located at run time. */
int cvf_comm_unique_id_bytes(void);
int cvf_comm_unique_id(void* id_host);
int cvf_comm_init(void** comm, int rank, int world, const void* id_host);
int cvf_comm_allreduce_f64(void* comm, double* buf, int64_t n, void* stream);
int cvf_comm_allreduce_f32(void* comm, float* buf, int64_t n, void* stream);
int cvf_comm_destroy(void* comm);

/* --- the same two sums as a ONE-SHOT peer-to-peer reduce (csrc/p2p.hip): every rank writes its vector
 * into a slot of every peer's window (fine-grained device memory shared through HIP IPC handles: one xGMI hop, all links at once),
 * raises a flag there, waits for the `world` flags in its own window and adds the slots in RANK ORDER - every rank forms the same
 * sum bit for bit, whatever the arrival order.  One process per GPU.  Unlike the rest of this header cvf_p2p_create allocates (the
 * window, as a communicator does).  Sequence: every rank cvf_p2p_create -> exchange the cvf_p2p_handle_bytes()-byte handles by any
 * means, rank-major -> cvf_p2p_connect -> cvf_p2p_allreduce_* on a stream (in place, SUM; n * sizeof <= max_bytes; capturable:
 * the epoch lives on the device; all launches on one communicator must be ordered on ONE stream).  A peer whose data does not
 * arrive within the time-out (20 s; environment CVF_P2P_TIMEOUT_MS) does not hang the GPU: the kernel fills the result with NaN and
 * sets the communicator's error word, which cvf_p2p_error() returns (0 = none; a host-visible word - no device call, no
 * synchronisation: it reports what the kernels finished so far have found).  A host must read it wherever it reads results back
 * and treat a non-zero value as fatal for the communicator (the shipped host raises). */
int cvf_p2p_handle_bytes(void);
int cvf_p2p_create(void** comm, int rank, int world, int64_t max_bytes, void* handle_out_host);
int cvf_p2p_connect(void* comm, const void* all_handles_host);
int cvf_p2p_allreduce_f64(void* comm, double* buf, int64_t n, void* stream);
int cvf_p2p_allreduce_f32(void* comm, float* buf, int64_t n, void* stream);
int cvf_p2p_error(void* comm);
int cvf_p2p_destroy(void* comm);

/* --- the data-parallel step in FOUR launches (front, finish, backward, slab reduction - as the single-process step): the two
 * cross-rank sums folded into the launches on either side of them, over the same windows in their low-latency form (every 4-byte
 * payload travels as one 8-byte {payload, exchange number} word that the receiver polls: no flag, no fence, one xGMI hop;
 * csrc/cvf_p2p.hpp).  `p2p_comm`: a connected cvf_p2p communicator (max_bytes >= 4 * n_params).  Parallelises core.py:498-522.
 *  cvf_ef16_finish_dp : cvf_ef16_finish + collective #1 + cvf_ef_loss: the units' rows -> this rank's sums -> sum over ranks in
 *                       rank order (`stats`) -> loss_vec, coef; identical on every rank bit for bit.
 *  cvf_ef_stats_dp    : cvf_ef_stats + collective #1 + cvf_ef_loss (transfer-operator mode / shapes outside the fast layout).
 *  cvf_ef_loss_dp     : collective #1 + cvf_ef_loss on sums another launch left in `stats` (in place).
 *  cvf_slab_reduce_dp : cvf_slab_reduce + collective #2 + the optimiser step (adam != NULL) - every workgroup exchanges the
 *                       entries it has just summed and applies the identical Adam update; `grad` receives the global gradient.
 *                       Must follow one of the three calls above (or cvf_p2p_exchange_f64) of the same step: it carries that
 *                       exchange's number; a repeat without one in between sets the error word (bit 30).
 *  cvf_p2p_exchange_f64: any fp64 vector of at most 80 entries, in place, by the same low-latency exchange. */
int cvf_ef16_finish_dp(const cvf_ef_cfg* cfg, int64_t B, const double* scratch, double* stats, double* loss_vec, double* coef,
                       void* p2p_comm, void* stream);
int cvf_ef_stats_dp(const cvf_ef_cfg* cfg, int64_t B, const float* w, const float* y_tiled, const float* e_tiled,
                    const float* w_lag, const float* y_lag_tiled, double* scratch, double* stats, double* loss_vec,
                    double* coef, void* p2p_comm, void* stream);
int cvf_ef_loss_dp(const cvf_ef_cfg* cfg, double* stats, double* loss_vec, double* coef, void* p2p_comm, void* stream);
int cvf_slab_reduce_dp(const float* slab, int64_t n_rows, int64_t n_params, float* grad, const cvf_adam_args* adam,
                       void* p2p_comm, void* stream);
int cvf_p2p_exchange_f64(void* comm, double* buf, int64_t n, void* stream);

/* --- measurement aid (no reference counterpart): plain streaming on this device, timed by bench.py in the same loop as
 * cvf_align_feature_fwd so that the alignment kernel's HBM fraction can be read against what the box delivers at that moment.
 * mode 0: dst <- src, one 16-byte piece per thread; mode 1: read-only sweep (dst receives one float per 2048 pieces).
 * dst holds cvf_probe_stream_out_floats(mode, n_float4) floats. */
int64_t cvf_probe_stream_out_floats(int mode, int64_t n_float4);
int cvf_probe_stream(int mode, float* dst, const float* src, int64_t n_float4, void* stream);

#ifdef __cplusplus
}
#endif
#endif
