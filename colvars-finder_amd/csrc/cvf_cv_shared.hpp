// Form C of a CV model description (include/cvf.h: cvf_cv_*_shared_*): n_nets = k scalar chains of one
// architecture whose first n_shared layers are ONE set of tensors, w_off[i][l] == w_off[0][l] and b_off[i][l] == b_off[0][l]
// for l < n_shared - the convention of cvf_ef_general_shared_* (csrc/ef_general.hip).  Host C++ only: the check the three
// evaluation routes (csrc/cv_nets.hip, csrc/cv_frame.hip, csrc/cv_frame_large.hip) make before anything else.
#pragma once
#include <stdio.h>

#include "cvf.h"

// NULL, or why `mlp` with `n_shared` is no form-C description (in buf).  `plain` names the entry point that takes a model without
// a shared trunk.  The widths, the act codes and the limits of a route are the route's own checks.
inline const char* cvf_form_c_why(const cvf_mlp_desc* mlp, int n_shared, const char* plain, char* buf, size_t n_buf) {
  if (mlp == nullptr) return "no model description";
  if (mlp->n_nets < 1 || mlp->n_nets > CVF_MAX_NETS) {
    snprintf(buf, n_buf, "%d nets: 1 to %d are supported", mlp->n_nets, CVF_MAX_NETS);
    return buf;
  }
  if (mlp->n_layers < 1 || mlp->n_layers > CVF_MAX_LAYERS) {
    snprintf(buf, n_buf, "%d layers: 1 to %d are supported", mlp->n_layers, CVF_MAX_LAYERS);
    return buf;
  }
  if (n_shared == 0) {
    snprintf(buf, n_buf, "n_shared = 0: a model without a shared trunk takes %s", plain);
    return buf;
  }
  if (n_shared < 1 || n_shared > mlp->n_layers - 1) {
    snprintf(buf, n_buf, "n_shared = %d out of range: the %d layers leave 1 to %d for the trunk and at least one for the heads", n_shared,
             mlp->n_layers, mlp->n_layers - 1);
    return buf;
  }
  if (mlp->dims[mlp->n_layers] != 1) {
    snprintf(buf, n_buf, "the heads of a shared trunk must be scalar (they have %d outputs each)", mlp->dims[mlp->n_layers]);
    return buf;
  }
  for (int i = 1; i < mlp->n_nets; ++i)
    for (int l = 0; l < n_shared; ++l) {
      if (mlp->w_off[i][l] != mlp->w_off[0][l]) {
        snprintf(buf, n_buf, "net %d does not share layer %d: w_off[%d][%d] = %d, w_off[0][%d] = %d", i, l, i, l, mlp->w_off[i][l], l,
                 mlp->w_off[0][l]);
        return buf;
      }
      if (mlp->b_off[i][l] != mlp->b_off[0][l]) {
        snprintf(buf, n_buf, "net %d does not share layer %d: b_off[%d][%d] = %d, b_off[0][%d] = %d", i, l, i, l, mlp->b_off[i][l], l,
                 mlp->b_off[0][l]);
        return buf;
      }
    }
  return nullptr;
}
