// Stand-alone checker of the CV model file's parser (colvars-finder_amd/csrc/cvf_cv_file.hpp): reads each file named on the
// command line into a heap buffer of exactly its size and runs the parser and, for a good file, the descriptor fill on it.
// Built by tests/test_cv_file_host.py with -fsanitize=address,undefined: a read outside the buffer ends the program.
// Prints one line per file: "<code> <device bytes or 0> <message>".
#include <stdio.h>
#include <stdlib.h>

#include "cvf_cv_file.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (f == nullptr) {
      printf("-100 0 cannot open %s\n", argv[i]);
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
    if (rc == 0) {
      bytes = cvf_file::device_bytes(v);
      cvf_cv_model m;
      cvf_file::fill_model(v, reinterpret_cast<const unsigned char*>(0x1000), &m);   // (pointer arithmetic only, never followed)
      if (m.k != v.k || (m.theta == nullptr) != (v.mlp.n_params == 0)) return 3;
    }
    printf("%d %lld %s\n", rc, bytes, err);
    free(buf);
  }
  return 0;
}
