// The model file of a trained CV (include/cvf.h: cvf_cv_file_*): parser and validator.  Host C++ only - no HIP include - so
// that the very source the library binds with also builds into a stand-alone checker (tests/cv_file_check_main.cpp) under the
// host sanitizers.  Nothing here forms a pointer into the blob, or reads a table, before the sizes that bound it have been
// checked against `nbytes`; every multi-byte value is read with memcpy (the blob need not be aligned).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "cvf.h"

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "the CV model file is little-endian and is read in place"
#endif

namespace cvf_file {

constexpr int64_t kMlpOff = 16, kMlpBytes = 4 * (2 + (CVF_MAX_LAYERS + 1) + CVF_MAX_LAYERS + 2 * CVF_MAX_NETS * CVF_MAX_LAYERS + 1);
constexpr int64_t kPpOff = kMlpOff + kMlpBytes, kPpInts = 12;
constexpr int64_t kTailOff = kPpOff + 4 * kPpInts;   // upto_layer, k, n_entries, n_shared
constexpr int64_t kDirOff = kTailOff + 16, kEntryBytes = 24;
static_assert(kMlpBytes == (int64_t)sizeof(cvf_mlp_desc), "the file stores cvf_mlp_desc in struct order");
static_assert(kDirOff == 960, "documented in include/cvf.h");

enum { kInt32 = 0, kFloat32 = 1 };

struct Table {
  const unsigned char* p;   // into the blob (unaligned); nullptr when count == 0
  int64_t count, offset;
};

struct View {
  cvf_mlp_desc mlp;
  int32_t mode, n_coord, n_align, n_rec, d_r, use_angle_value, has_position, flags, n_slot, n_rec_slot, n_mrec, n_ref;
  int32_t upto_layer, k;
  int32_t n_shared;                 // form C: the chains' first n_shared layers are one set of tensors (0: forms A and B)
  Table t[CVF_FILE_N_TABLES + 1];   // by name id
  int64_t data_off, data_end;       // the table region [data_off, data_end) of the blob, what the binder copies
};

inline int32_t rd32(const unsigned char* p, int64_t i) {
  int32_t v;
  memcpy(&v, p + 4 * i, 4);
  return v;
}
inline int64_t rd64(const unsigned char* p) {
  int64_t v;
  memcpy(&v, p, 8);
  return v;
}

inline const char* table_name(int id) {
  static const char* const names[] = {"?", "align_idx", "ref_c", "rec", "align_w", "atom_align", "atom_slot", "rec_slot",
                                      "slot_atom", "mrec", "slot_row", "theta"};
  return id >= 1 && id <= CVF_FILE_N_TABLES ? names[id] : "?";
}

#define CVF_FILE_FAIL(code, ...)          \
  do {                                    \
    snprintf(err, errlen, __VA_ARGS__);   \
    return code;                          \
  } while (0)

// atoms a record of this type reads / outputs it writes; 0 for an unknown type
inline int rec_atoms(int type) {
  return type == CVF_FEAT_POSITION ? 1 : type == CVF_FEAT_BOND ? 2 : type == CVF_FEAT_ANGLE ? 3 : type == CVF_FEAT_DIHEDRAL ? 4 : 0;
}
inline int rec_outputs(int type, int angle_value) {
  return type == CVF_FEAT_POSITION ? 3 : (type == CVF_FEAT_DIHEDRAL && !angle_value) ? 2 : 1;
}

// 0 and *v filled, or a negative code and the reason (naming the field) in err.
inline int parse(const void* blob, int64_t nbytes, View* v, char* err, size_t errlen) {
  if (blob == nullptr || v == nullptr) CVF_FILE_FAIL(-1, "cv file: null argument");
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  if (nbytes < 4) CVF_FILE_FAIL(-2, "cv file: truncated inside the magic (%lld bytes)", (long long)nbytes);
  if (memcmp(b, "CVF1", 4) != 0) CVF_FILE_FAIL(-3, "cv file: wrong magic (not a CVF1 file)");
  if (nbytes < kDirOff) CVF_FILE_FAIL(-2, "cv file: truncated inside the header (%lld bytes, the header has %lld)", (long long)nbytes, (long long)kDirOff);
  if (rd32(b, 1) != CVF_FILE_VERSION) CVF_FILE_FAIL(-4, "cv file: format version %d, this library reads version %d", rd32(b, 1), CVF_FILE_VERSION);
  if (rd32(b, 2) != CVF_MAX_NETS || rd32(b, 3) != CVF_MAX_LAYERS)
    CVF_FILE_FAIL(-4, "cv file: written for CVF_MAX_NETS = %d, CVF_MAX_LAYERS = %d; this library has %d, %d", rd32(b, 2), rd32(b, 3), CVF_MAX_NETS, CVF_MAX_LAYERS);
  memset(v, 0, sizeof *v);
  memcpy(&v->mlp, b + kMlpOff, kMlpBytes);
  const unsigned char* q = b + kPpOff;
  v->mode = rd32(q, 0); v->n_coord = rd32(q, 1); v->n_align = rd32(q, 2); v->n_rec = rd32(q, 3); v->d_r = rd32(q, 4);
  v->use_angle_value = rd32(q, 5); v->has_position = rd32(q, 6); v->flags = rd32(q, 7); v->n_slot = rd32(q, 8);
  v->n_rec_slot = rd32(q, 9); v->n_mrec = rd32(q, 10); v->n_ref = rd32(q, 11);
  v->upto_layer = rd32(b + kTailOff, 0);
  v->k = rd32(b + kTailOff, 1);
  const int32_t n_entries = rd32(b + kTailOff, 2);
  v->n_shared = rd32(b + kTailOff, 3);

  // ---- the nets' description
  const cvf_mlp_desc& m = v->mlp;
  if (m.n_nets < 1 || m.n_nets > CVF_MAX_NETS) CVF_FILE_FAIL(-5, "cv file: n_nets = %d outside 1..%d", m.n_nets, CVF_MAX_NETS);
  if (m.n_layers < 1 || m.n_layers > CVF_MAX_LAYERS) CVF_FILE_FAIL(-5, "cv file: n_layers = %d outside 1..%d", m.n_layers, CVF_MAX_LAYERS);
  for (int l = 0; l <= m.n_layers; ++l)
    if (m.dims[l] < 1 || m.dims[l] > 65536) CVF_FILE_FAIL(-5, "cv file: dims[%d] = %d outside 1..65536", l, m.dims[l]);
  for (int l = 0; l < m.n_layers; ++l)
    if (m.act[l] < CVF_ACT_NONE || m.act[l] > CVF_ACT_SOFTPLUS) CVF_FILE_FAIL(-5, "cv file: act[%d] = %d is no activation code", l, m.act[l]);
  if (m.n_params < 0) CVF_FILE_FAIL(-5, "cv file: n_params = %d", m.n_params);
  if (v->upto_layer < 1 || v->upto_layer > m.n_layers) CVF_FILE_FAIL(-5, "cv file: upto_layer = %d outside 1..%d", v->upto_layer, m.n_layers);
  if (m.n_nets > 1 && (v->upto_layer != m.n_layers || m.dims[m.n_layers] != 1))
    CVF_FILE_FAIL(-5, "cv file: %d nets side by side must be scalar and whole (upto_layer = %d of %d, %d outputs)", m.n_nets, v->upto_layer, m.n_layers, m.dims[m.n_layers]);
  if (v->k != (m.n_nets > 1 ? m.n_nets : m.dims[v->upto_layer])) CVF_FILE_FAIL(-5, "cv file: k = %d disagrees with the nets' description", v->k);
  if (v->n_shared < 0 || v->n_shared > m.n_layers - 1) CVF_FILE_FAIL(-5, "cv file: n_shared = %d outside 0..%d (n_layers - 1)", v->n_shared, m.n_layers - 1);
  if (v->n_shared > 0) {   // form C: scalar chains, whole, the trunk's tensors once
    if (v->upto_layer != m.n_layers || m.dims[m.n_layers] != 1)
      CVF_FILE_FAIL(-5, "cv file: n_shared = %d needs scalar chains evaluated whole (upto_layer = %d of %d, %d outputs)", v->n_shared, v->upto_layer, m.n_layers, m.dims[m.n_layers]);
    for (int i = 1; i < m.n_nets; ++i)
      for (int l = 0; l < v->n_shared; ++l)
        if (m.w_off[i][l] != m.w_off[0][l] || m.b_off[i][l] != m.b_off[0][l])
          CVF_FILE_FAIL(-5, "cv file: n_shared = %d, but net %d does not share layer %d (w_off %d / %d, b_off %d / %d)", v->n_shared, i, l,
                        m.w_off[i][l], m.w_off[0][l], m.b_off[i][l], m.b_off[0][l]);
  }

  // ---- the layer's scalars
  if (v->mode != CVF_PP_IDENTITY && v->mode != CVF_PP_ALIGN && v->mode != CVF_PP_FEATURES)
    CVF_FILE_FAIL(-6, "cv file: mode = %d (a file holds an Identity layer or an alignment + feature layer)", v->mode);
  if (v->n_coord < 1) CVF_FILE_FAIL(-6, "cv file: n_coord = %d", v->n_coord);
  if (v->n_align < 0 || v->n_rec < 0 || v->d_r < 1 || v->n_slot < 0 || v->n_rec_slot < 0 || v->n_mrec < 0 || v->n_ref < 0)
    CVF_FILE_FAIL(-6, "cv file: a negative count (n_align %d n_rec %d d_r %d n_slot %d n_rec_slot %d n_mrec %d n_ref %d)", v->n_align,
                  v->n_rec, v->d_r, v->n_slot, v->n_rec_slot, v->n_mrec, v->n_ref);
  const bool identity = v->mode == CVF_PP_IDENTITY;
  if (identity && (v->d_r != v->n_coord || v->n_align || v->n_rec || v->n_slot || v->n_rec_slot || v->n_mrec || v->n_ref))
    CVF_FILE_FAIL(-6, "cv file: an Identity layer has d_r == n_coord and no tables");
  if (!identity && v->n_coord % 3 != 0) CVF_FILE_FAIL(-6, "cv file: n_coord = %d is no multiple of 3", v->n_coord);
  if (v->mode == CVF_PP_ALIGN && v->n_align < 3) CVF_FILE_FAIL(-6, "cv file: n_align = %d, the alignment needs 3 atoms", v->n_align);
  if (v->mode == CVF_PP_FEATURES && v->n_align != 0) CVF_FILE_FAIL(-6, "cv file: n_align = %d on a layer without alignment", v->n_align);
  if (m.dims[0] != v->d_r) CVF_FILE_FAIL(-6, "cv file: dims[0] = %d, the layer gives d_r = %d features", m.dims[0], v->d_r);
  const int64_t N = identity ? 0 : v->n_coord / 3;

  // ---- the directory
  if (n_entries != CVF_FILE_N_TABLES) CVF_FILE_FAIL(-7, "cv file: %d directory entries, the format has %d", n_entries, CVF_FILE_N_TABLES);
  const int64_t dir_end = kDirOff + kEntryBytes * (int64_t)n_entries;
  if (nbytes < dir_end) CVF_FILE_FAIL(-2, "cv file: truncated inside the directory (%lld bytes, the directory ends at %lld)", (long long)nbytes, (long long)dir_end);
  v->data_off = (dir_end + 15) / 16 * 16;
  v->data_end = v->data_off;
  const int64_t want[CVF_FILE_N_TABLES + 1] = {0, v->n_align, 3 * (int64_t)v->n_align, 6 * (int64_t)v->n_rec, v->n_align, N, N,
                                               6 * (int64_t)v->n_rec_slot, v->n_slot, 8 * (int64_t)v->n_mrec, (int64_t)v->n_slot + 1, m.n_params};
  const char* const want_name[CVF_FILE_N_TABLES + 1] = {"", "n_align", "3 n_align", "6 n_rec", "n_align", "n_coord / 3", "n_coord / 3",
                                                        "6 n_rec_slot", "n_slot", "8 n_mrec", "n_slot + 1", "n_params"};
  bool seen[CVF_FILE_N_TABLES + 1] = {};
  for (int e = 0; e < n_entries; ++e) {
    const unsigned char* d = b + kDirOff + kEntryBytes * e;
    const int32_t id = rd32(d, 0), type = rd32(d, 1);
    const int64_t count = rd64(d + 8), off = rd64(d + 16);
    if (id < 1 || id > CVF_FILE_N_TABLES) CVF_FILE_FAIL(-7, "cv file: directory entry %d has unknown table id %d", e, id);
    if (seen[id]) CVF_FILE_FAIL(-7, "cv file: table %s is listed twice", table_name(id));
    seen[id] = true;
    const bool is_float = id == CVF_FILE_REF_C || id == CVF_FILE_ALIGN_W || id == CVF_FILE_THETA;
    if (type != (is_float ? kFloat32 : kInt32)) CVF_FILE_FAIL(-7, "cv file: table %s has element type %d", table_name(id), type);
    // optional tables may be absent: align_w (uniform weights), the per-atom and contribution-row tables
    const bool optional = id == CVF_FILE_ALIGN_W || id == CVF_FILE_ATOM_ALIGN || id == CVF_FILE_ATOM_SLOT || id == CVF_FILE_SLOT_ROW;
    if (count != want[id] && !(optional && count == 0))
      CVF_FILE_FAIL(-8, "cv file: table %s holds %lld elements, %s gives %lld", table_name(id), (long long)count, want_name[id], (long long)want[id]);
    if (count > 0) {
      if (off < v->data_off || off % 16 != 0) CVF_FILE_FAIL(-9, "cv file: table %s at offset %lld (tables are 16-byte aligned behind the directory)", table_name(id), (long long)off);
      if (off > nbytes || count > (nbytes - off) / 4)
        CVF_FILE_FAIL(-2, "cv file: table %s (offset %lld, %lld elements) reaches past the end of the file (%lld bytes)", table_name(id),
                      (long long)off, (long long)count, (long long)nbytes);
      v->t[id] = Table{b + off, count, off};
      if (off + 4 * count > v->data_end) v->data_end = off + 4 * count;
    } else {
      v->t[id] = Table{nullptr, 0, 0};
    }
  }
  // (n_entries == CVF_FILE_N_TABLES distinct known ids: every table is listed)
  if (v->n_mrec > 0 && v->t[CVF_FILE_SLOT_ROW].count == 0) CVF_FILE_FAIL(-8, "cv file: table slot_row is missing beside mrec");

  // ---- table contents: every index a kernel would follow
  const Table& rec = v->t[CVF_FILE_REC];
  int any_position = 0;
  for (int64_t r = 0; r < v->n_rec; ++r) {
    const int type = rd32(rec.p, 6 * r), out = rd32(rec.p, 6 * r + 5), na = rec_atoms(type);
    if (na == 0) CVF_FILE_FAIL(-10, "cv file: rec[%lld] has unknown feature type %d", (long long)r, type);
    for (int j = 0; j < na; ++j) {
      const int a = rd32(rec.p, 6 * r + 1 + j);
      if (a < 0 || a >= N) CVF_FILE_FAIL(-10, "cv file: rec[%lld] reads atom %d of %lld", (long long)r, a, (long long)N);
    }
    if (out < 0 || out + rec_outputs(type, v->use_angle_value) > v->d_r)
      CVF_FILE_FAIL(-10, "cv file: rec[%lld] writes output %d of d_r = %d", (long long)r, out, v->d_r);
    any_position |= type == CVF_FEAT_POSITION;
  }
  if (!identity && (v->has_position != 0) != (any_position != 0)) CVF_FILE_FAIL(-10, "cv file: has_position = %d disagrees with rec", v->has_position);
  for (int64_t i = 0; i < v->n_align; ++i) {
    const int a = rd32(v->t[CVF_FILE_ALIGN_IDX].p, i);
    if (a < 0 || a >= N) CVF_FILE_FAIL(-10, "cv file: align_idx[%lld] = %d of %lld atoms", (long long)i, a, (long long)N);
  }
  for (int64_t i = 0; i < v->n_slot; ++i) {
    const int a = rd32(v->t[CVF_FILE_SLOT_ATOM].p, i);
    if (a < 0 || a >= N) CVF_FILE_FAIL(-10, "cv file: slot_atom[%lld] = %d of %lld atoms", (long long)i, a, (long long)N);
  }
  for (int64_t i = 0; i < v->t[CVF_FILE_ATOM_ALIGN].count; ++i) {
    const int s = rd32(v->t[CVF_FILE_ATOM_ALIGN].p, i);
    if (s < -1 || s >= v->n_align) CVF_FILE_FAIL(-10, "cv file: atom_align[%lld] = %d of %d align atoms", (long long)i, s, v->n_align);
  }
  for (int64_t i = 0; i < v->t[CVF_FILE_ATOM_SLOT].count; ++i) {
    const int s = rd32(v->t[CVF_FILE_ATOM_SLOT].p, i);
    if (s < -1 || s >= v->n_slot) CVF_FILE_FAIL(-10, "cv file: atom_slot[%lld] = %d of %d slots", (long long)i, s, v->n_slot);
  }
  const Table& rs = v->t[CVF_FILE_REC_SLOT];
  for (int64_t r = 0; r < v->n_rec_slot; ++r) {
    const int type = rd32(rs.p, 6 * r), out = rd32(rs.p, 6 * r + 5), na = rec_atoms(type);
    if (type == -1) continue;   // padding of a batch (CVF_PP_SLOT_BATCHED)
    if (na == 0) CVF_FILE_FAIL(-10, "cv file: rec_slot[%lld] has unknown feature type %d", (long long)r, type);
    for (int j = 0; j < na; ++j) {
      const int s = rd32(rs.p, 6 * r + 1 + j);
      if (s < 0 || s >= v->n_slot) CVF_FILE_FAIL(-10, "cv file: rec_slot[%lld] reads slot %d of %d", (long long)r, s, v->n_slot);
    }
    if (out < 0 || out + rec_outputs(type, v->use_angle_value) > v->d_r)
      CVF_FILE_FAIL(-10, "cv file: rec_slot[%lld] writes output %d of d_r = %d", (long long)r, out, v->d_r);
  }
  const Table& sr = v->t[CVF_FILE_SLOT_ROW];
  if (sr.count > 0) {
    int prev = 0;
    for (int64_t i = 0; i <= v->n_slot; ++i) {
      const int row = rd32(sr.p, i);
      if (row < prev || row > v->n_ref || (i == 0 && row != 0)) CVF_FILE_FAIL(-10, "cv file: slot_row[%lld] = %d is out of order or past n_ref = %d", (long long)i, row, v->n_ref);
      prev = row;
    }
    if (prev != v->n_ref) CVF_FILE_FAIL(-10, "cv file: slot_row ends at %d, n_ref = %d", prev, v->n_ref);
  }
  const Table& mr = v->t[CVF_FILE_MREC];
  for (int64_t r = 0; r < v->n_mrec; ++r) {
    uint32_t w[6];
    for (int j = 0; j < 6; ++j) w[j] = (uint32_t)rd32(mr.p, 8 * r + j);
    const int type = (int)(w[0] & 7u) - 1, out = (int)(w[0] >> 3), na = rec_atoms(type);
    if (na == 0) CVF_FILE_FAIL(-10, "cv file: mrec[%lld] has unknown feature type %d", (long long)r, type);
    if (out + rec_outputs(type, v->use_angle_value) > v->d_r) CVF_FILE_FAIL(-10, "cv file: mrec[%lld] writes output %d of d_r = %d", (long long)r, out, v->d_r);
    for (int j = 0; j < na; ++j) {
      const uint32_t slot = (w[1 + j / 2] >> (16 * (j & 1))) & 0xffffu, urow = (w[3 + j / 2] >> (16 * (j & 1))) & 0xffffu;
      const uint32_t off = (w[5] >> (8 * j)) & 0xffu;
      if ((int64_t)slot >= v->n_slot) CVF_FILE_FAIL(-10, "cv file: mrec[%lld] reads slot %u of %d", (long long)r, slot, v->n_slot);
      if ((int64_t)urow + off >= v->n_ref) CVF_FILE_FAIL(-10, "cv file: mrec[%lld] writes row %u of n_ref = %d", (long long)r, urow + off, v->n_ref);
    }
  }
  // ---- the parameters: every block of every chain inside theta
  for (int i = 0; i < m.n_nets; ++i)
    for (int l = 0; l < m.n_layers; ++l) {
      const int64_t wn = (int64_t)m.dims[l] * m.dims[l + 1], bn = m.dims[l + 1];
      if (m.w_off[i][l] < 0 || m.w_off[i][l] + wn > m.n_params)
        CVF_FILE_FAIL(-11, "cv file: w_off[%d][%d] = %d (+ %lld) lies outside theta (%d parameters)", i, l, m.w_off[i][l], (long long)wn, m.n_params);
      if (m.b_off[i][l] < 0 || m.b_off[i][l] + bn > m.n_params)
        CVF_FILE_FAIL(-11, "cv file: b_off[%d][%d] = %d (+ %lld) lies outside theta (%d parameters)", i, l, m.b_off[i][l], (long long)bn, m.n_params);
    }
  if (v->data_end == v->data_off) CVF_FILE_FAIL(-8, "cv file: no table holds anything (theta is empty)");
  return 0;
}

// bytes of the device buffer the binder fills: the table region, rounded up to 16
inline int64_t device_bytes(const View& v) { return (v.data_end - v.data_off + 15) / 16 * 16; }

// the descriptors over a device copy of [data_off, data_end) at `base`
inline void fill_model(const View& v, const unsigned char* base, cvf_cv_model* out) {
  auto at = [&](int id) -> const void* { return v.t[id].count > 0 ? base + (v.t[id].offset - v.data_off) : nullptr; };
  memset(out, 0, sizeof *out);
  out->mlp = v.mlp;
  cvf_pp_desc& p = out->pp;
  p.mode = v.mode; p.n_coord = v.n_coord; p.n_align = v.n_align; p.n_rec = v.n_rec; p.d_r = v.d_r;
  p.use_angle_value = v.use_angle_value; p.has_position = v.has_position; p.flags = v.flags;
  p.n_slot = v.n_slot; p.n_rec_slot = v.n_rec_slot; p.n_mrec = v.n_mrec; p.n_ref = v.n_ref;
  p.align_idx = static_cast<const int32_t*>(at(CVF_FILE_ALIGN_IDX));
  p.ref_c = static_cast<const float*>(at(CVF_FILE_REF_C));
  p.rec = static_cast<const int32_t*>(at(CVF_FILE_REC));
  p.align_w = static_cast<const float*>(at(CVF_FILE_ALIGN_W));
  p.atom_align = static_cast<const int32_t*>(at(CVF_FILE_ATOM_ALIGN));
  p.atom_slot = static_cast<const int32_t*>(at(CVF_FILE_ATOM_SLOT));
  p.rec_slot = static_cast<const int32_t*>(at(CVF_FILE_REC_SLOT));
  p.slot_atom = static_cast<const int32_t*>(at(CVF_FILE_SLOT_ATOM));
  p.mrec = static_cast<const int32_t*>(at(CVF_FILE_MREC));
  p.slot_row = static_cast<const int32_t*>(at(CVF_FILE_SLOT_ROW));
  out->theta = static_cast<const float*>(at(CVF_FILE_THETA));
  out->upto_layer = v.upto_layer;
  out->k = v.k;
}

#undef CVF_FILE_FAIL
}  // namespace cvf_file
