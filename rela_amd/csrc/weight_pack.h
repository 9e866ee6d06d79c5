// weight_pack.h -- every kernel-layout copy of a net's weights is written by ONE kernel, weight_pack, over a list of
// segments: a segment is one layout (or one of the learners' operand copies) with its pack body, up to two source
// tensors in state_dict layout, the destination and two small integers.  A learner re-packs after every optimiser step,
// so a net's whole load is one launch (rela_ffnet_load / rela_lstmnet_load, csrc/ffnet.hip), and so is every pack on
// its own (the lazy BfT, pack_gate_x3, the learners' test taps): a list of one segment.
//
// Host side (every translation unit): PackList and launch_weight_pack.  Device side (csrc/ffnet.hip alone, which
// defines RELA_WEIGHT_PACK_KERNEL so that the library holds one copy of the kernel): the pack bodies with their layout
// comments, and the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rela_amd {

enum PackKind {
  kPackConv1x3,      // pack_conv1_bf16x3_at
  kPackFragsConv2,   // pack_frags_at, by mode; a0 = CT, a1 = KS
  kPackFragsConv3,
  kPackFragsFc,
  kPackFragsLstm,    // src2 = weight_hh_l0
  kPackFragsHeads,   // src = fc_a, src2 = fc_v, a0 = num_action
  kPackFcT,          // pack_fc_t_at
  kPackHeadsPerm,    // pack_heads_perm_at: src = fc_a, src2 = fc_v, a0 = num_action
  kPackBf16sConv2,   // pack_frags_bf16s_at, modes 1..3 in this order; a0 = CT, a1 = KS
  kPackBf16sConv3,
  kPackBf16sFc,
  kPackEmuConv2,     // f32emu::pack_f32emu_at, modes 1..4 in this order; a0 = NCG, a1 = KS
  kPackEmuConv3,
  kPackEmuFc,
  kPackEmuGatesPerm,
  kPackConv1I8,      // pack_conv1_i8_block: src = conv1 weight, src2 = conv1 bias; dst: digits | scales [32] | biases [32]
  kPackWihRec64,     // pack_wih_rec64_perm_at
  kPackCopy,         // dst[i] = src[i] (the biases)
  kPackHeadBias,     // src = fc_a bias, src2 = fc_v bias, a0 = num_action
  kPackLstmBias,     // src = bias_ih_l0, src2 = bias_hh_l0
  kPackPermute,      // permute_weight_at (ffnet_layout.h): a0 = kPermConv2 / kPermConv3 / kPermFc
};

constexpr int kPackMaxSegs = 24;
constexpr int kPackThreads = 256;
// head layouts: 32 columns (fc_a in 0..A-1, fc_v in 31) of K = 512 as [2][128][64] f32 fragments
constexpr int kHeadsCT = 2, kHeadsKS = 128;
constexpr int kConv1I8Weights = 32 * 256;  // conv1's weights, three int8 digits each: a block of 256 per output channel

struct PackSeg {
  const float *src, *src2;
  void* dst;
  int64_t elements;  // threads of pack work
  int kind, a0, a1;
};
struct PackList {  // passed to the kernel by value
  PackSeg seg[kPackMaxSegs];
  int first[kPackMaxSegs + 1] = {0};  // first block of segment j; first[n] = blocks of the launch
  int n = 0;
  bool overflow = false;
  // a segment of zero elements gets no blocks
  void add(int kind, const float* src, const float* src2, void* dst, int a0, int a1, int64_t elements) {
    if (n == kPackMaxSegs) {
      overflow = true;
      return;
    }
    seg[n] = PackSeg{src, src2, dst, elements, kind, a0, a1};
    first[n + 1] = first[n] + (int)((elements + kPackThreads - 1) / kPackThreads);
    ++n;
  }
};
static_assert(sizeof(PackList) <= 1280, "PackList travels as a kernel argument: keep it well under the 4 KB limit");

// one launch over the list (none if it has no blocks); defined in ffnet.hip
int launch_weight_pack(const PackList& list, hipStream_t s);
// a list of one segment
inline int pack_one(int kind, const float* src, const float* src2, void* dst, int a0, int a1, int64_t elements, hipStream_t s) {
  PackList one;
  one.add(kind, src, src2, dst, a0, a1, elements);
  return launch_weight_pack(one, s);
}

}  // namespace rela_amd

#ifdef RELA_WEIGHT_PACK_KERNEL
#include "common.h"
#include "ffnet_layout.h"
#include "gemm_bf16s.h"
#include "gemm_f32emu.h"

namespace rela_amd {
namespace {

using f32emu::bf16_bits_f32;
using f32emu::bf16_rne_bits;

// conv1 weights (32,4,8,8)/255 -> three bf16 planes in MFMA 16x16x32 fragment order, k running (c, kh, kw) linearly
// (conv1_bf16x3).  w == hi + mid + lo exactly for every finite fp32 weight (each residual is exact in fp32).
__device__ __forceinline__ void pack_conv1_bf16x3_at(int idx, const float* __restrict__ w, uint16_t* __restrict__ frag) {
  if (idx >= 2 * 8 * 64 * 8) return;
  const int j = idx & 7, lane = (idx >> 3) & 63, ks = (idx >> 9) & 7, ct = idx >> 12;
  const int k = ks * 32 + (lane >> 4) * 8 + j;
  const int oc = ct * 16 + (lane & 15);
  const float v = w[oc * 256 + k] / 255.0f;
  const uint16_t hi = bf16_rne_bits(v);
  const float r1 = v - bf16_bits_f32(hi);
  const uint16_t mid = bf16_rne_bits(r1);
  const float r2 = r1 - bf16_bits_f32(mid);
  const uint16_t lo = bf16_rne_bits(r2);
  const int plane = 2 * 8 * 64 * 8;
  frag[idx] = hi;
  frag[plane + idx] = mid;
  frag[2 * plane + idx] = lo;
}

// weights -> [ct][ks][hi, lo][lane] x 8 bf16 in MFMA 16x16x32 fragment order.  mode: 1 conv2 (k = tap*32 + c),
// 2 conv3 (k = tap*64 + c), 3 fc (k = pos*64 + c  <-  torch flatten c*49 + pos)
__device__ __forceinline__ void pack_frags_bf16s_at(int64_t idx, int mode, const float* __restrict__ w, uint16_t* __restrict__ frag, int CT, int KS) {
  if (idx >= (int64_t)CT * KS * 64 * 8) return;
  const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
  const int ks = (int)((idx >> 9) % KS), ct = (int)((idx >> 9) / KS);
  const int k = ks * 32 + (lane >> 4) * 8 + j;
  const int oc = ct * 16 + (lane & 15);
  float v;
  if (mode == 1) {  // conv2: (64,32,4,4)
    const int c = k & 31, tap = k >> 5;
    v = w[((oc * 32 + c) * 4 + (tap >> 2)) * 4 + (tap & 3)];
  } else if (mode == 2) {  // conv3: (64,64,3,3)
    const int c = k & 63, tap = k >> 6;
    v = w[((oc * 64 + c) * 3 + tap / 3) * 3 + tap % 3];
  } else {  // fc: (512,3136)
    const int c = k & 63, pos = k >> 6;
    v = w[(size_t)oc * 3136 + c * 49 + pos];
  }
  const uint16_t hi = bf16_rne_bits(v);
  const uint16_t lo = bf16_rne_bits(v - bf16_bits_f32(hi));
  const size_t base = (((size_t)ct * KS + ks) * 2) * 64 * 8;
  frag[base + (size_t)lane * 8 + j] = hi;
  frag[base + 64 * 8 + (size_t)lane * 8 + j] = lo;
}

// heads weights [ct 2][wave 4][j 32][lane 64] in the k order of heads_duel: k-step j of lane group g of wave w is
// k = 128w + 32g + j
__device__ __forceinline__ void pack_heads_perm_at(int idx, const float* __restrict__ a_w, const float* __restrict__ v_w, int A,
                                float* __restrict__ out) {
  if (idx >= 2 * 4 * 32 * 64) return;
  const int lane = idx & 63, j = (idx >> 6) & 31, w = (idx >> 11) & 3, ct = idx >> 13;
  const int k = 128 * w + 32 * (lane >> 4) + j, col = ct * 16 + (lane & 15);
  out[idx] = col < A ? a_w[(size_t)col * 512 + k] : (col == 31 ? v_w[k] : 0.f);
}

// wt[k = pos*64 + c][u] = linear.0.weight[u][c*49 + pos]   (net.py:49 flattens channel-first)
__device__ __forceinline__ void pack_fc_t_at(int idx, const float* __restrict__ w, float* __restrict__ wt) {
  if (idx >= 3136 * 512) return;
  const int k = idx >> 9, u = idx & 511;
  const int c = k & 63, pos = k >> 6;
  wt[idx] = w[(size_t)u * 3136 + c * 49 + pos];
}

// f32 weights -> [ct][ks][lane] fragments of the 16x16x4 f32 MFMA: lane holds column ct*16 + lane % 16 at k = ks*4 + lane / 16
enum FragsMode { kFragsConv2 = 1, kFragsConv3 = 2, kFragsFc = 3, kFragsHeads = 4, kFragsLstm = 5 };
__device__ __forceinline__ void pack_frags_at(int64_t idx, int mode, const float* __restrict__ w, const float* __restrict__ w2, int num_action,
                           float* __restrict__ frag, int CT, int KS) {
  const int64_t total = (int64_t)CT * KS * 64;
  if (idx >= total) return;
  const int lane = (int)(idx & 63);
  const int ks = (int)((idx >> 6) % KS);
  const int ct = (int)((idx >> 6) / KS);
  const int k = ks * 4 + (lane >> 4);
  const int oc = ct * 16 + (lane & 15);
  float v = 0.f;
  switch (mode) {
    case kFragsConv2: {  // k = (kh, kw, c)
      const int c = k & 31, kw = (k >> 5) & 3, kh = k >> 7;
      v = w[((oc * 32 + c) * 4 + kh) * 4 + kw];
      break;
    }
    case kFragsConv3: {  // k = (kh, kw, c)
      const int c = k & 63, r = k >> 6, kw = r % 3, kh = r / 3;
      v = w[((oc * 64 + c) * 3 + kh) * 3 + kw];
      break;
    }
    case kFragsFc: {  // k = pos*64 + c  <-  torch flatten c*49 + pos (net.py:49)
      const int c = k & 63, p = k >> 6;
      v = w[(size_t)oc * 3136 + c * 49 + p];
      break;
    }
    case kFragsLstm: {  // col' = 4*unit + gate  <-  row gate*512 + unit of weight_ih_l0 / weight_hh_l0
      const int row = (oc & 3) * 512 + (oc >> 2);
      if (k < 3136) {
        const int c = k & 63, p = k >> 6;  // k = pos*64 + c  <-  c*49 + pos (net.py:105-106)
        v = w[(size_t)row * 3136 + c * 49 + p];
      } else {
        v = w2[(size_t)row * 512 + (k - 3136)];
      }
      break;
    }
    case kFragsHeads:
      if (oc < num_action)
        v = w[oc * 512 + k];  // fc_a
      else if (oc == 31)
        v = w2[k];  // fc_v
      break;
  }
  frag[idx] = v;
}

// weight_ih_l0 [gate*512 + unit][c*49 + pos] -> rec64 rows in the gate GEMM's permuted column order:
// rec[col = 4*unit + gate][chunk = pos][64 hi | 64 lo] over c (the B operand of gemm16::gemm_rec64_nt for the x part)
__device__ __forceinline__ void pack_wih_rec64_perm_at(int64_t i, const float* __restrict__ wih, uint8_t* __restrict__ rec) {
  if (i >= (int64_t)2048 * 392) return;  // one thread per 8 channels
  const int col = (int)(i / 392), o = (int)(i - (int64_t)col * 392);
  const int pos = o >> 3, c0 = (o & 7) * 8;
  const float* w = wih + (size_t)((col & 3) * 512 + (col >> 2)) * 3136 + pos;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = w[(c0 + j) * 49];
  uint4 hi, lo;
  gemm16::split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), hi, lo);
  uint8_t* r = rec + ((size_t)col * 49 + pos) * 256 + (o & 7) * 16;
  *reinterpret_cast<uint4*>(r) = hi;
  *reinterpret_cast<uint4*>(r + 128) = lo;
}

// conv1 for conv12_i8: one block of 256 threads per output channel c (thread = weight k = p*64 + ky*8 + kx of
// state_dict's [32][4][8][8]).  s_c = max|w| / QMAX rounded UP to f32 (so that |w / s_c| <= QMAX), q = rint(w / s_c) in
// double, balanced base-256 digits; b' = b + 128 s_c sum q in double, rounded once.  Digit d of (c, k) is byte
// j = (ky % 4) * 4 + kx % 4 of lane (g = p) * 16 + c % 16 of fragment [d][c / 16][tap (ky / 4) * 2 + kx / 4].
constexpr int kConv1QMax = 127 * 65536 + 127 * 256 + 127;
__device__ __forceinline__ void pack_conv1_i8_block(int c, const float* __restrict__ w, const float* __restrict__ b,
                                                    uint8_t* __restrict__ W1d, float* __restrict__ s1q, float* __restrict__ b1q) {
  __shared__ float amax[256];
  __shared__ long long qsum[256];
  const int k = threadIdx.x;
  const float wv = w[c * 256 + k] / 255.0f;  // the s / 255 of net.py:46, folded as in the other conv1 packs
  amax[k] = fabsf(wv);
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (k < o) amax[k] = fmaxf(amax[k], amax[k + o]);
    __syncthreads();
  }
  const float mx = amax[0];
  float sc = 1.0f;
  if (mx > 0.f) {
    sc = (float)((double)mx / (double)kConv1QMax);
    if (sc <= 0.f || (double)mx / (double)sc > (double)kConv1QMax) sc = nextafterf(sc, INFINITY);
  }
  long long q = llrint((double)wv / (double)sc);
  q = q > kConv1QMax ? kConv1QMax : (q < -kConv1QMax ? -kConv1QMax : q);
  qsum[k] = q;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (k < o) qsum[k] += qsum[k + o];
    __syncthreads();
  }
  if (k == 0) {
    s1q[c] = sc;
    b1q[c] = (float)((double)b[c] + 128.0 * (double)sc * (double)qsum[0]);
  }
  // balanced digits: lo, mid in [-128, 127], hi = the rest (|hi| <= 127 by the bound on q)
  const int qi = (int)q;
  const int lo = ((qi + 128) & 255) - 128;
  const int q1 = (qi - lo) >> 8;
  const int mid = ((q1 + 128) & 255) - 128;
  const int hi = (q1 - mid) >> 8;
  const int pl = k >> 6, ky = (k >> 3) & 7, kx = k & 7;
  const int tap = (ky >> 2) * 2 + (kx >> 2), j = (ky & 3) * 4 + (kx & 3);
  const int lane = pl * 16 + (c & 15), ct = c >> 4;
  const int dig[3] = {hi, mid, lo};
#pragma unroll
  for (int d = 0; d < 3; ++d) W1d[((size_t)((d * 2 + ct) * 4 + tap) * 64 + lane) * 16 + j] = (uint8_t)(int8_t)dig[d];
}

// A block finds its segment in the table of first-block indices (block-uniform: kPackConv1I8 synchronises, one whole
// block per output channel); its threads are elements blockDim * (block within the segment) + thread, 64-bit.
__global__ __launch_bounds__(kPackThreads) void weight_pack(PackList a) {
  const int b = blockIdx.x;
  int j = 0;
  while (b >= a.first[j + 1]) ++j;
  const PackSeg& g = a.seg[j];
  const int seg_block = b - a.first[j];
  const int64_t idx = (int64_t)seg_block * kPackThreads + threadIdx.x;
  if (idx >= g.elements) return;  // (kPackConv1I8's blocks are whole)
  const float *w = g.src, *w2 = g.src2;
  float* f = static_cast<float*>(g.dst);
  uint16_t* h = static_cast<uint16_t*>(g.dst);
  uint8_t* u = static_cast<uint8_t*>(g.dst);
  const int a0 = g.a0, a1 = g.a1;
  switch (g.kind) {
    case kPackConv1x3: pack_conv1_bf16x3_at((int)idx, w, h); break;
    case kPackFragsConv2: pack_frags_at(idx, kFragsConv2, w, nullptr, 0, f, a0, a1); break;
    case kPackFragsConv3: pack_frags_at(idx, kFragsConv3, w, nullptr, 0, f, a0, a1); break;
    case kPackFragsFc: pack_frags_at(idx, kFragsFc, w, nullptr, 0, f, a0, a1); break;
    case kPackFragsLstm: pack_frags_at(idx, kFragsLstm, w, w2, 0, f, a0, a1); break;
    case kPackFragsHeads: pack_frags_at(idx, kFragsHeads, w, w2, a0, f, kHeadsCT, kHeadsKS); break;
    case kPackFcT: pack_fc_t_at((int)idx, w, f); break;
    case kPackHeadsPerm: pack_heads_perm_at((int)idx, w, w2, a0, f); break;
    case kPackBf16sConv2:
    case kPackBf16sConv3:
    case kPackBf16sFc: pack_frags_bf16s_at(idx, g.kind - kPackBf16sConv2 + 1, w, h, a0, a1); break;
    case kPackEmuConv2:
    case kPackEmuConv3:
    case kPackEmuFc:
    case kPackEmuGatesPerm: f32emu::pack_f32emu_at(idx, g.kind - kPackEmuConv2 + 1, w, h, a0, a1); break;
    case kPackConv1I8: {
      float* s1q = reinterpret_cast<float*>(u + kConv1I8Weights * 3);
      pack_conv1_i8_block(seg_block, w, w2, u, s1q, s1q + 32);
      break;
    }
    case kPackWihRec64: pack_wih_rec64_perm_at(idx, w, u); break;
    case kPackCopy: f[idx] = w[idx]; break;
    case kPackHeadBias: f[idx] = idx < a0 ? w[idx] : (idx == 31 ? w2[0] : 0.f); break;
    case kPackLstmBias: {  // col' = 4*unit + gate, as kFragsLstm
      const int row = ((int)idx & 3) * 512 + ((int)idx >> 2);
      f[idx] = w[row] + w2[row];
      break;
    }
    case kPackPermute: permute_weight_at(a0, (int)idx, w, f); break;
  }
}

}  // namespace

int launch_weight_pack(const PackList& list, hipStream_t s) {
  RELA_CHECK(!list.overflow, RELA_EINVAL, "launch_weight_pack: more than %d segments", kPackMaxSegs);
  if (list.first[list.n] > 0) hipLaunchKernelGGL(weight_pack, dim3(list.first[list.n]), dim3(kPackThreads), 0, s, list);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

}  // namespace rela_amd
#endif  // RELA_WEIGHT_PACK_KERNEL
