// Stand-alone checker of the CV model file's n_shared field (colvars-finder_amd/csrc/cvf_cv_file.hpp; form C, DESIGN.md section
// 4.17), beside tests/cv_file_check_main.cpp: reads each file named on the command line into a heap buffer of exactly its size,
// runs the parser and, for a good file, re-checks on the parsed view what n_shared promises - the offsets of the first n_shared
// layers are those of net 0 - and follows every parameter offset to its last float inside theta.
// Built by tests/test_cv_shared_host.py with -fsanitize=address,undefined: a read outside the buffer ends the program.
// Prints one line per file: "<code> <device bytes or 0> <n_shared or 0> <message>".
#include <stdio.h>
#include <stdlib.h>

#include "cvf_cv_file.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (f == nullptr) {
      printf("-100 0 0 cannot open %s\n", argv[i]);
      return 2;
    }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char* buf = static_cast<unsigned char*>(malloc(n > 0 ? (size_t)n : 1));
    if (n > 0 && fread(buf, 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    cvf_file::View v;
    char err[320] = "ok";
    const int rc = cvf_file::parse(buf, n, &v, err, sizeof err);
    long long bytes = 0;
    int n_shared = 0;
    if (rc == 0) {
      bytes = cvf_file::device_bytes(v);
      n_shared = v.n_shared;
      const cvf_mlp_desc& m = v.mlp;
      if (n_shared < 0 || n_shared > m.n_layers - 1) return 3;
      const cvf_file::Table& th = v.t[CVF_FILE_THETA];
      double sum = 0.0;   // (the reads are the point: the sanitizer watches them)
      for (int net = 0; net < m.n_nets; ++net)
        for (int l = 0; l < m.n_layers; ++l) {
          if (l < n_shared && (m.w_off[net][l] != m.w_off[0][l] || m.b_off[net][l] != m.b_off[0][l])) return 4;
          const int64_t w_last = (int64_t)m.w_off[net][l] + (int64_t)m.dims[l] * m.dims[l + 1] - 1;
          const int64_t b_last = (int64_t)m.b_off[net][l] + m.dims[l + 1] - 1;
          if (w_last >= th.count || b_last >= th.count) return 5;
          float a, b;
          memcpy(&a, th.p + 4 * w_last, 4);
          memcpy(&b, th.p + 4 * b_last, 4);
          sum += (double)a + (double)b;
        }
      cvf_cv_model model;
      cvf_file::fill_model(v, reinterpret_cast<const unsigned char*>(0x1000), &model);   // (pointer arithmetic only, never followed)
      if (model.k != v.k || model.upto_layer != v.upto_layer) return 6;
      if (sum == 12345.678) fputs("", stderr);   // (keeps the reads alive)
    }
    printf("%d %lld %d %s\n", rc, bytes, n_shared, err);
    free(buf);
  }
  return 0;
}
