// The binder of the CV model file (include/cvf.h: cvf_cv_file_device_bytes, cvf_cv_file_bind, cvf_cv_file_n_shared; DESIGN.md
// sections 4.15 and 4.17).  All the reading and checking is cvf_cv_file.hpp's (host C++, shared with the stand-alone checkers);
// this file adds the one host-to-device copy of the table region and the descriptors over it.
#include "cvf_common.hpp"
#include "cvf_cv_file.hpp"

extern "C" int64_t cvf_cv_file_device_bytes(const void* blob_host, int64_t nbytes) {
  cvf_file::View v;
  char err[320];
  const int rc = cvf_file::parse(blob_host, nbytes, &v, err, sizeof err);
  if (rc != 0) {
    cvf_set_error("cvf_cv_file_device_bytes: %s", err);
    return rc;
  }
  return cvf_file::device_bytes(v);
}

extern "C" int cvf_cv_file_bind(const void* blob_host, int64_t nbytes, void* dev_buf, int64_t dev_bytes, cvf_cv_model* out,
                                void* stream) {
  cvf_file::View v;
  char err[320];
  const int rc = cvf_file::parse(blob_host, nbytes, &v, err, sizeof err);
  if (rc != 0) {
    cvf_set_error("cvf_cv_file_bind: %s", err);
    return rc;
  }
  CVF_REQUIRE(dev_buf != nullptr && out != nullptr, "cvf_cv_file_bind: null argument");
  CVF_REQUIRE(((uintptr_t)dev_buf & 15) == 0, "cvf_cv_file_bind: dev_buf must be 16-byte aligned");
  const int64_t need = cvf_file::device_bytes(v);
  CVF_REQUIRE(dev_bytes >= need, "cvf_cv_file_bind: dev_buf holds %lld bytes, the tables need %lld (cvf_cv_file_device_bytes)",
              (long long)dev_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(dev_buf, static_cast<const unsigned char*>(blob_host) + v.data_off, (size_t)(v.data_end - v.data_off),
                                hipMemcpyHostToDevice, s);
  CVF_REQUIRE(e == hipSuccess, "cvf_cv_file_bind: copy of the tables: %s", hipGetErrorString(e));
  e = hipStreamSynchronize(s);   // a set-up call: the caller may free the blob when it returns
  CVF_REQUIRE(e == hipSuccess, "cvf_cv_file_bind: %s", hipGetErrorString(e));
  cvf_file::fill_model(v, static_cast<const unsigned char*>(dev_buf), out);
  return 0;
}

extern "C" int cvf_cv_file_n_shared(const void* blob_host, int64_t nbytes) {
  cvf_file::View v;
  char err[320];
  const int rc = cvf_file::parse(blob_host, nbytes, &v, err, sizeof err);
  if (rc != 0) {
    cvf_set_error("cvf_cv_file_n_shared: %s", err);
    return rc;
  }
  return v.n_shared;
}
