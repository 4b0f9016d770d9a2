// The periodic cell of an MD engine and the rule that makes a wrapped molecule whole (include/cvf.h: cvf_md_cell,
// cvf_cv_*_bias_*_cell_eval, cvf_md_make_whole): the text ONCE, for the kernels of csrc/cv_bias.hip and for
// the host (tools/cell_host.cpp compiles this file into a stand-alone program that tests/test_cell_host.py checks against fp64).  No
// HIP include: plain C++ on either side.
//
// Cell: 9 floats, the lattice vectors as rows  a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz)  - the reduced lower-triangular
// form of OpenMM, GROMACS and LAMMPS.  The cell is device memory that the host never sees, so the rule is total: an axis whose
// diagonal entry is 0, negative or not finite is NOT periodic - its image count is 0 and its lattice vector is never used (a slab is
// cz = 0) - and the upper triangle (cell[1], cell[2], cell[5]) is never read.
//
// Minimum image of a difference d, the axes in the order z, y, x (each step leaves the later axes' components alone):
//   n_z = rint(d.z / cz), d -= n_z c;   n_y = rint(d.y / by), d -= n_y b;   n_x = rint(d.x / ax), d -= n_x a
// (a true fp32 division and round-half-even; d -= n v is fmaf(-n, v, d) per component).  A count is kept within +-CVF_CELL_NMAX
// (saturated; NaN counts 0).
//
// Chain, in the order of the CV's atoms (WHOLEMOLECULES): atom 0 stays, atom j takes the image nearest to the WHOLE atom j - 1.
// With n_j the image triple of x_j - x_{j-1} on the WRAPPED coordinates and N_j = sum_{i <= j} n_i the whole position is
//   x_j - (N_j.x a + N_j.y b + N_j.z c)
// - the sequential rule, as an integer prefix sum: exact, and the same however a wave or a workgroup associates it.  The subtraction
// has ONE form, cvf_cell_whole below: the lattice shift first, summed in the minimum image's order z, y, x with one fused multiply-add
// per further term, then ONE subtraction:
//   s.x = fmaf(N.x, ax, fmaf(N.y, bx, N.z * cx))      w.x = x.x - s.x
//   s.y =               fmaf(N.y, by, N.z * cy)       w.y = x.y - s.y
//   s.z =                             N.z * cz        w.z = x.z - s.z
// every fmaf written out and none left to a compiler's contraction (the function is compiled with contraction off: N.z * cz is a
// rounded product on the device as on the host), so the host and every kernel round alike.  Where the shift is exact in fp32 (an orthorhombic cell, or lattice entries that
// are short binary fractions) the result is fp32(x - N L), one rounding; else |error| <= 4 eps (|x| + sum_i |N_i| |h_i|) per coordinate.
// N_j = 0 returns x_j untouched, bit for bit.
// N_j travels as one 32-bit word, 10 bits per axis: +-511 images (saturated, never wrapped).
//
// Precondition (the caller's): consecutive atoms of the CV lie closer than half the shortest cell height, and frames are whole atoms
// (n_coord % 3 == 0).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CVF_CELL_HD __host__ __device__ inline
#else
#define CVF_CELL_HD inline
#endif

#define CVF_CELL_NMAX 511   /* images per axis that the packed word holds */

struct CvfCell {
  float ax, bx, by, cx, cy, cz;   // the lattice vectors; all entries of a non-periodic axis are 0
  int px, py, pz;                 // the axis is periodic
};

CVF_CELL_HD int cvf_cell_axis_ok(float diag) { return diag > 0.0f && diag <= 3.402823466e+38f; }   // (false for NaN and inf)

CVF_CELL_HD CvfCell cvf_cell_load(const float* cell) {
  CvfCell c;
  c.px = cvf_cell_axis_ok(cell[0]);
  c.py = cvf_cell_axis_ok(cell[4]);
  c.pz = cvf_cell_axis_ok(cell[8]);
  c.ax = c.px ? cell[0] : 0.0f;
  c.bx = c.py ? cell[3] : 0.0f;
  c.by = c.py ? cell[4] : 0.0f;
  c.cx = c.pz ? cell[6] : 0.0f;
  c.cy = c.pz ? cell[7] : 0.0f;
  c.cz = c.pz ? cell[8] : 0.0f;
  return c;
}

// rint(q) as an int within +-CVF_CELL_NMAX; NaN gives 0
CVF_CELL_HD int cvf_cell_count(float q) {
  if (!(q == q)) return 0;
  if (q >= (float)CVF_CELL_NMAX) return CVF_CELL_NMAX;
  if (q <= -(float)CVF_CELL_NMAX) return -CVF_CELL_NMAX;
  return (int)rintf(q);
}

// the image triple n of the difference (dx, dy, dz)
CVF_CELL_HD void cvf_cell_image(const CvfCell& c, float dx, float dy, float dz, int* nx, int* ny, int* nz) {
  int n = 0;
  if (c.pz) {
    n = cvf_cell_count(dz / c.cz);
    dx = fmaf(-(float)n, c.cx, dx);
    dy = fmaf(-(float)n, c.cy, dy);
  }
  *nz = n;
  n = 0;
  if (c.py) {
    n = cvf_cell_count(dy / c.by);
    dx = fmaf(-(float)n, c.bx, dx);
  }
  *ny = n;
  n = 0;
  if (c.px) n = cvf_cell_count(dx / c.ax);
  *nx = n;
}

CVF_CELL_HD int cvf_cell_sat(int n) { return n > CVF_CELL_NMAX ? CVF_CELL_NMAX : (n < -CVF_CELL_NMAX ? -CVF_CELL_NMAX : n); }

// N as one word: 10 bits per axis, offset 512, saturated at +-511 (0 is N = 0)
CVF_CELL_HD uint32_t cvf_cell_pack(int nx, int ny, int nz) {
  if ((nx | ny | nz) == 0) return 0u;
  return (uint32_t)(cvf_cell_sat(nx) + 512) | ((uint32_t)(cvf_cell_sat(ny) + 512) << 10) | ((uint32_t)(cvf_cell_sat(nz) + 512) << 20);
}
CVF_CELL_HD void cvf_cell_unpack(uint32_t w, int* nx, int* ny, int* nz) {
  if (w == 0u) {
    *nx = *ny = *nz = 0;
    return;
  }
  *nx = (int)(w & 1023u) - 512;
  *ny = (int)((w >> 10) & 1023u) - 512;
  *nz = (int)((w >> 20) & 1023u) - 512;
}

// the whole position of an atom at x whose summed image triple is the word w: THE form of the subtraction (above)
CVF_CELL_HD void cvf_cell_whole(const CvfCell& c, uint32_t w, const float x[3], float out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)   // (x.z - N.z * cz stays a product and a difference on the device as on the host)
#endif
  float x0 = x[0], x1 = x[1], x2 = x[2];
  if (w != 0u) {
    int nx, ny, nz;
    cvf_cell_unpack(w, &nx, &ny, &nz);
    const float fx = (float)nx, fy = (float)ny, fz = (float)nz;
    x0 = x0 - fmaf(fx, c.ax, fmaf(fy, c.bx, fz * c.cx));
    x1 = x1 - fmaf(fy, c.by, fz * c.cy);
    x2 = x2 - fz * c.cz;
  }
  out[0] = x0;
  out[1] = x1;
  out[2] = x2;
}
