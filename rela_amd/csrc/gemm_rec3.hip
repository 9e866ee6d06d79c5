// The three-part record GEMM (gemm_rec3.h) and its split kernels as a translation unit of their own, so that the compiler's
// account of the kernels can be checked by compiling this file alone (tests/test_lstm_in_rec3_plan_host.py).
// learner_r2d2.hip reaches them through the functions declared in learner_common.h.
#include "gemm_rec3.h"

#include "learner_common.h"

namespace rela_amd {

static_assert(kLstmRec3Bytes == rec3::REC, "record size");

int lstm_rec3_row_tile(bool small) { return small ? rec3::SBM : rec3::BM; }

void split_rows_rec3(const float* src, int64_t R, int K, uint8_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(rec3::split_rows_rec3, dim3(ceil_div(R * K / 8, 256)), dim3(256), 0, s, src, R, K, dst);
}
void split_cols_rec3(const float* src, int64_t R, int C, bool a3_order, uint8_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(rec3::split_cols_rec3, dim3(C / 64, ceil_div(R, 64)), dim3(256), 0, s, src, R, C, a3_order ? 1 : 0, dst);
}
int launch_rec3_nt_plain(const uint8_t* A, const uint8_t* B, int M, int N, int KC, float* out, hipStream_t s, const char* name) {
  return rec3::launch_rec3_nt(A, B, M, N, KC, gemm16::EpiPlain{out, N}, s, name);
}
int launch_rec3_nt_relu_mask(const uint8_t* A, const uint8_t* B, int M, int N, int KC, float* out, const float* act, hipStream_t s,
                             const char* name) {
  return rec3::launch_rec3_nt(A, B, M, N, KC, gemm16::EpiReluMask{out, act, N}, s, name);
}

}  // namespace rela_amd
