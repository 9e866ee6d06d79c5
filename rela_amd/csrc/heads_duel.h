// heads_duel.h -- the AtariFFNet's heads and the dueling combination in one launch, per Q table (heads_duel) or for the
// Ape-X learner's three tables at once (heads_duel_jobs).  Included by ffnet.hip only: the kernels live in
// rela_amd::(anonymous).
#pragma once
#include "ffnet_kern.h"
#include "prof.h"

namespace rela_amd {
namespace {

// Heads + dueling in ONE launch (AtariFFNet): [N, 512] x [512, 32] (fc_a in columns 0..A-1, fc_v in column 31) and
// q = v + a*legal - mean_A(a*legal) (net.py:33-39).  The two separate launches (a 4-block-wide GEMM and a
// one-thread-per-row kernel) cost 18 + 10 us at N = 6,400 and 17 + 9 us at N = 512 for 0.2 GFLOP: launch and latency,
// not work.  Block = 16 rows, 4 waves; wave w multiplies the k-slice [128w, 128w + 128) on v_mfma_f32_16x16x4_f32 (a
// lane reads 32 CONTIGUOUS floats of its row: k-step j of lane group g is k = 128w + 32g + j, the weights are packed
// in that order by pack_heads_perm_at, weight_pack.h), the four partial tiles meet in LDS, then 16 threads per row finish the row.
constexpr int kHeadRows = 16;
__device__ __forceinline__ void heads_duel_body(const float* __restrict__ h, const float* __restrict__ Bhp,
                                                const float* __restrict__ bias, const float* __restrict__ legal,
                                                float* __restrict__ ha, float* __restrict__ q, int N, int A, int bid) {
  __shared__ float part[4][kHeadRows][33];
  __shared__ float hs[kHeadRows][33];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int row0 = bid * kHeadRows;
  float av[32];
  {
    const int row = min(row0 + li, N - 1);
    const float4* hp = reinterpret_cast<const float4*>(h + (size_t)row * 512 + 128 * wave + 32 * g);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float4 v = hp[c];
      av[4 * c] = v.x, av[4 * c + 1] = v.y, av[4 * c + 2] = v.z, av[4 * c + 3] = v.w;
    }
  }
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const float* bp = Bhp + ((size_t)(ct * 4 + wave) * 32) * 64 + lane;
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bp[j * 64], acc[ct], 0, 0, 0);
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][4 * g + r][ct * 16 + li] = acc[ct][r];
  __syncthreads();
  const int r = tid >> 4, c = tid & 15, row = row0 + r;
#pragma unroll
  for (int hcol = 0; hcol < 2; ++hcol) {
    const int col = c + 16 * hcol;
    hs[r][col] = ((part[0][r][col] + part[1][r][col]) + (part[2][r][col] + part[3][r][col])) + bias[col];
  }
  __syncthreads();
  if (row >= N) return;
  if (ha) ha[(size_t)row * 32 + c] = hs[r][c], ha[(size_t)row * 32 + c + 16] = hs[r][c + 16];
  const float* lg = legal + (size_t)row * A;
  float sum = 0.f;  // in column order, as the one-thread-per-row kernel summed it
  for (int j = 0; j < A; ++j) sum += hs[r][j] * lg[j];
  const float mean = sum / (float)A, v = hs[r][31];
  if (c < A) q[(size_t)row * A + c] = (v + hs[r][c] * lg[c]) - mean;
  if (c + 16 < A) q[(size_t)row * A + c + 16] = (v + hs[r][c + 16] * lg[c + 16]) - mean;
}
__global__ __launch_bounds__(256) void heads_duel(const float* __restrict__ h, const float* __restrict__ Bhp,
                                                  const float* __restrict__ bias, const float* __restrict__ legal,
                                                  float* __restrict__ ha, float* __restrict__ q, int N, int A) {
  heads_duel_body(h, Bhp, bias, legal, ha, q, N, A, blockIdx.x);
}
// up to three head passes in one launch (the learner's three Q tables): segment j owns blocks [first[j], first[j + 1])
struct HeadJobs {
  const float *h[3], *Bhp[3], *bias[3], *legal[3];
  float *ha[3], *q[3];
  int N[3], first[4];
};
__global__ __launch_bounds__(256) void heads_duel_jobs(HeadJobs jb, int A) {
  int j = 0;
  while (j < 2 && (int)blockIdx.x >= jb.first[j + 1]) ++j;
  heads_duel_body(jb.h[j], jb.Bhp[j], jb.bias[j], jb.legal[j], jb.ha[j], jb.q[j], jb.N[j], A, (int)blockIdx.x - jb.first[j]);
}

// h [N][512] -> ha [N][32] (or NULL) and q [N][A]
inline void launch_heads_duel(const float* h, const float* Bhp, const float* bh, const float* legal, float* ha, float* q, int N,
                              int A, hipStream_t s) {
  note_launch("heads_duel");
  hipLaunchKernelGGL(heads_duel, dim3(ceil_div(N, kHeadRows)), dim3(256), 0, s, h, Bhp, bh, legal, ha, q, N, A);
}
inline void launch_heads_duel_jobs(const HeadJobs& jb, int A, hipStream_t s) {
  note_launch("heads_duel_jobs");
  hipLaunchKernelGGL(heads_duel_jobs, dim3(jb.first[3]), dim3(256), 0, s, jb, A);
}

}  // namespace
}  // namespace rela_amd
