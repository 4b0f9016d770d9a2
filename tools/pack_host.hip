// Test harness (not part of the library): the fragment scatter of csrc/cvf_pack.hpp (pack_tab_fill + pack_scatter, the very
// source the optimiser kernels and cvf_ef_pack inline) compiled in hipcc's HOST pass as a stand-alone program, so that
// tests/test_pack_host.py can check on the CPU where every parameter lands (no GPU needed).  Built with AddressSanitizer and
// UBSan: a slot outside the buffer ends the run.
// (host code only: the sanitizer options follow -Xarch_host)
//   hipcc -O1 -g -std=c++17 --cuda-host-only --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=all -Iinclude -Icolvars-finder_amd/csrc tools/pack_host.hip -o <out>
// stdin: lines "H NH D n_nets" (nets d0 = D -> H x NH -> 1 in torch's parameters() order, net after net).
// stdout, per line (binary): int32 {H, NH, D, n_nets, per_net, n_params, shared}, then n_nets * per_net floats: the zeroed
// fragment buffer after parameter p = 0 .. n_params-1 was scattered with value p + 1 (exact in fp32: n_params < 2^24).
// shared: slots that hold another value when the parameters are scattered in DESCENDING order - a slot two parameters write
// keeps the later writer, so it differs between the two orders; 0 means that every slot has one writer.
#include <stdio.h>
#include <vector>
#include "cvf_pack.hpp"

void cvf_set_error(const char*, ...) {}
int cvf_check_launch(const char*) { return 0; }

int main() {
  int H, NH, D, k;
  while (scanf("%d %d %d %d", &H, &NH, &D, &k) == 4) {
    if (H < 1 || D < 1 || NH < 1 || NH + 1 > CVF_MAX_LAYERS || k < 1 || k > CVF_MAX_NETS) {
      fprintf(stderr, "pack_host: bad case %d %d %d %d\n", H, NH, D, k);
      return 2;
    }
    cvf_mlp_desc mlp = {};
    mlp.n_nets = k;
    mlp.n_layers = NH + 1;
    mlp.dims[0] = D;
    for (int l = 1; l <= NH; ++l) mlp.dims[l] = H;
    mlp.dims[NH + 1] = 1;
    int pos = 0;
    for (int n = 0; n < k; ++n)
      for (int l = 0; l <= NH; ++l) {
        mlp.w_off[n][l] = pos;
        mlp.b_off[n][l] = pos + mlp.dims[l + 1] * mlp.dims[l];
        pos += mlp.dims[l + 1] * (mlp.dims[l] + 1);
      }
    mlp.n_params = pos;
    if (pos >= (1 << 24)) {
      fprintf(stderr, "pack_host: %d parameters are not exact in fp32\n", pos);
      return 2;
    }
    const PackLayout L = pack_layout(H, NH, D);
    PackTab tab;
    pack_tab_fill(tab, mlp);
    std::vector<float> packed((size_t)k * L.per_net, 0.0f);
    for (int p = 0; p < pos; ++p) pack_scatter(tab, p, (float)(p + 1), packed.data());
    std::vector<float> down((size_t)k * L.per_net, 0.0f);
    for (int p = pos - 1; p >= 0; --p) pack_scatter(tab, p, (float)(p + 1), down.data());
    int shared = 0;
    for (size_t i = 0; i < packed.size(); ++i) shared += packed[i] != down[i];
    const int32_t head[7] = {H, NH, D, k, L.per_net, pos, shared};
    if (fwrite(head, sizeof(head), 1, stdout) != 1 || fwrite(packed.data(), sizeof(float), packed.size(), stdout) != packed.size()) {
      fprintf(stderr, "pack_host: short write\n");
      return 3;
    }
  }
  return 0;
}
