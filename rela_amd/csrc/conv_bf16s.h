// conv_bf16s.h -- the split-bf16 ("fast", bf16x2) arithmetic: its split records and conv_bf16s, the persistent convolution
// over them (conv3 as a kernel of its own; conv2 inside conv12_i8.h).  Included by ffnet.hip only: the kernels live in
// rela_amd::(anonymous).
#pragma once
#include "ffnet_kern.h"
#include "prof.h"

namespace rela_amd {
namespace {

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// =====================================================================================================
// Split-bf16 ("fast") path: conv2 / conv3 / fc on v_mfma_f32_16x16x32_bf16 (16x the f32 MFMA rate).
// Every activation and weight x is kept as TWO bf16 numbers, hi = bf16(x), lo = bf16(x - hi) (16 mantissa
// bits together), and a product is evaluated as  a_lo*b_hi + a_hi*b_lo + a_hi*b_hi  with f32 accumulation:
// the dropped terms (a_lo*b_lo and the residuals beyond 16 bits) are ~2^-16 of |a||b| per product, against
// 2^-24 for the exact f32 path, which stays the parity mode (rela_ffnet_set_precision).  Activations travel
// between the layers in "split records": per pixel, C channels of hi (2 B each) followed by C channels of
// lo -- the same 4 bytes per element as f32, so HBM traffic is unchanged while the MFMA work drops 5.3x.
// =====================================================================================================
// Four CONSECUTIVE channels of ONE pixel -> the hi and lo halves of its LDS record.  This is what a lane holds when the
// MFMA is issued with the operands swapped (weights as the A operand: D[channel 4g + r][pixel li]): ReLU, two packed
// RNE conversions per half and TWO 8-byte LDS stores for four values, where the pixel-major tile needed eight 2-byte
// stores (the epilogues' LDS stores were a fifth of the frame time).
__device__ __forceinline__ void split_store_lds4(uint8_t* rec, int C, int ch0, f32x4 v) {
  typedef float f32x2_ __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
  const f32x2_ a = {v[0] > 0.f ? v[0] : 0.f, v[1] > 0.f ? v[1] : 0.f}, b = {v[2] > 0.f ? v[2] : 0.f, v[3] > 0.f ? v[3] : 0.f};
  const bf16x2_ ha = __builtin_convertvector(a, bf16x2_), hb = __builtin_convertvector(b, bf16x2_);
  const bf16x2_ la = __builtin_convertvector(a - __builtin_convertvector(ha, f32x2_), bf16x2_);
  const bf16x2_ lb = __builtin_convertvector(b - __builtin_convertvector(hb, f32x2_), bf16x2_);
  *reinterpret_cast<uint2*>(rec + ch0 * 2) = make_uint2(__builtin_bit_cast(uint32_t, ha), __builtin_bit_cast(uint32_t, hb));
  *reinterpret_cast<uint2*>(rec + C * 2 + ch0 * 2) =
      make_uint2(__builtin_bit_cast(uint32_t, la), __builtin_bit_cast(uint32_t, lb));
}

// Makes the compiler treat a resident weight fragment as consumed HERE: its s_waitcnt for the load lands before
// the persistent loop instead of at the first use inside it, where on later rounds the same counter value
// would wait for the output stores and prefetches of the round before.
__device__ __forceinline__ void pin_loaded(bf16x8& f) {
  u32x4 t = __builtin_bit_cast(u32x4, f);
  asm volatile("" : "+v"(t));
  f = __builtin_bit_cast(bf16x8, t);
}

// Two values of one channel (rows r, r + 1 of an accumulator tile) -> the hi and lo halves of their LDS records:
// two packed RNE conversions (v_cvt_pk_bf16_f32) and four 2-byte LDS stores, no cross-lane exchange and no wait
// (pairing lanes through ds_bpermute costs an LDS round trip per value, which serialised the epilogues).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_store_lds2(uint8_t* rec0, uint8_t* rec1, int C, int col, float v0, float v1) {
  const f32x2 v = {v0, v1};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  const f32x2 hf = __builtin_convertvector(h, f32x2);
  const bf16x2 l = __builtin_convertvector(v - hf, bf16x2);
  const u16x2 hb = __builtin_bit_cast(u16x2, h), lb = __builtin_bit_cast(u16x2, l);
  *reinterpret_cast<uint16_t*>(rec0 + col * 2) = hb[0];
  *reinterpret_cast<uint16_t*>(rec1 + col * 2) = hb[1];
  *reinterpret_cast<uint16_t*>(rec0 + C * 2 + col * 2) = lb[0];
  *reinterpret_cast<uint16_t*>(rec1 + C * 2 + col * 2) = lb[1];
}

// conv on split records, weight-stationary and persistent (one block per CU walks over its sample groups with
// a double-buffered LDS tile).  k = (tap, c): one MFMA k-step = 32 channels of one input pixel, i.e. lane
// group g reads the 16 bytes of channels 8g..8g+7 from the hi part and from the lo part of the pixel record.
// LDS pixel / row / sample strides (in 16-byte units) are padded so that the 16 lanes ds_read_b128 services
// together hit 16 different 16-byte bank groups: unit(p, g) = 2p + g (mod 16) over output positions p.
template <int CIN_, int IH_, int IW_, int KH_, int KW_, int STRIDE_, int OH_, int OW_, int S_, int Q_, int RQ_, int SQ_>
struct ConvFastCfg {
  static constexpr int CIN = CIN_, IH = IH_, IW = IW_, KH = KH_, KW = KW_, STRIDE = STRIDE_, OH = OH_, OW = OW_, S = S_;
  static constexpr int OC = 64, CT = 4, RG = kWaves / CT;
  static constexpr int P = OH * OW, M = S * P, RT = (M + 15) / 16, RPW = (RT + RG - 1) / RG;
  static constexpr int KSUB = CIN / 32;              // k-steps per tap
  static constexpr int KS = KH * KW * KSUB;          // k-steps of 32
  static constexpr int REC = CIN * 4;                // bytes per input pixel record
  static constexpr int Q = Q_, RQ = RQ_, SQ = SQ_;   // pixel / row / sample stride in 16-byte units
  static constexpr int DEPTH = (CIN == 32) ? 4 : 3;  // A fragment pairs in flight per wave (register ring)
  static constexpr int LDS_BYTES = S * SQ * 16;      // one input buffer
  static constexpr int OROW = OC * 4 + 16;  // staged record stride: the 16 pixels of a store spread over the banks
  static constexpr int OUT_BYTES = S * OH * OW * OROW;  // output records of one group (staged for coalesced stores)
  static constexpr int LDS_TOTAL = 2 * LDS_BYTES + 2 * OUT_BYTES + OC * 4;  // + one spare record
  static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");
  static constexpr int IN_BYTES = IH * IW * REC;     // per sample in HBM
  static constexpr int V16 = S * IN_BYTES / 16;      // 16-byte chunks per group
  static constexpr int IT = (V16 + kThreads - 1) / kThreads, IT2 = (IT + 1) / 2;
  static_assert(REC / 16 <= Q, "pixel stride too small");
};
// conv2: 20x20x32 -> 9x9x64, stride 2: 2*Q = 2, 2*RQ = 18 = 2 (mod 16)
using Conv2F = ConvFastCfg<32, 20, 20, 4, 4, 2, 9, 9, 1, 9, 185, 20 * 185>;
// conv3: 9x9x64 -> 7x7x64, stride 1: Q = 2, RQ = 14 (7 positions per row), SQ = 98 = 2 (mod 16)
using Conv3F = ConvFastCfg<64, 9, 9, 3, 3, 1, 7, 7, 2, 18, 174, 1570>;

template <class C, bool STAMPS = false>
__device__ __forceinline__ void conv_bf16s_body(const uint8_t* __restrict__ in, const uint4* __restrict__ Bfrag,
                                                const float* __restrict__ bias, uint8_t* __restrict__ out, int N, int bid,
                                                int nblk, unsigned long long* stamps = nullptr) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  int stamp_frame = 0;
  auto stamp = [&](int point) {  // (diagnostic build only: rela_ffnet_debug_conv3_stamps)
    if constexpr (STAMPS) {
      if (bid == 0 && (threadIdx.x == 0 || threadIdx.x == 448) && stamp_frame < kStampFrames)
        stamps[((threadIdx.x == 0 ? 0 : 1) * kStampFrames + stamp_frame) * kStampPoints + point] = __builtin_amdgcn_s_memtime();
    }
  };
  const int wave = tid >> 6, lane = tid & 63;
  const int ct = wave % C::CT, rg = wave / C::CT;
  const int li = lane & 15, g = lane >> 4;
  const int ngroups = (N + C::S - 1) / C::S;

  // weights of this wave's 16 output channels: [ks][hi, lo] fragments, resident for the whole launch
  bf16x8 bh[C::KS], bl[C::KS];
  {
    const uint4* bp = Bfrag + (size_t)ct * C::KS * 2 * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      bh[ks] = __builtin_bit_cast(bf16x8, bp[(size_t)(ks * 2) * 64]);
      bl[ks] = __builtin_bit_cast(bf16x8, bp[(size_t)(ks * 2 + 1) * 64]);
    }
  }
  int abase[C::RPW];
#pragma unroll
  for (int t = 0; t < C::RPW; ++t) {
    const int m = (rg + t * C::RG) * 16 + li;
    const int mm = (m < C::M) ? m : 0;
    const int sm = mm / C::P, pos = mm - sm * C::P;
    const int oy = pos / C::OW, ox = pos - oy * C::OW;
    abase[t] = (sm * C::SQ + oy * C::STRIDE * C::RQ + ox * C::STRIDE * C::Q + g) * 16;
  }
  const int ch0 = ct * 16 + 4 * g;  // this lane's four output channels (operands swapped: channels are the tile rows)
  const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + ch0);

  uint4 v[C::IT2];
  auto stage_load = [&](int grp, int phase) {
    const int n0 = grp * C::S;
    const int ns = min(C::S, N - n0);
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)n0 * C::IN_BYTES);
#pragma unroll
    for (int j = 0; j < C::IT2; ++j) {
      const int i = tid + (phase * C::IT2 + j) * kThreads;
      v[j] = (i < ns * (C::IN_BYTES / 16)) ? src[i] : make_uint4(0, 0, 0, 0);
    }
  };
  auto stage_store = [&](int buf, int phase) {
    uint8_t* dst = smem + buf * C::LDS_BYTES;
    constexpr int UPP = C::REC / 16;  // 16-byte units per pixel record
#pragma unroll
    for (int j = 0; j < C::IT2; ++j) {
      const int i = tid + (phase * C::IT2 + j) * kThreads;
      if (i < C::V16) {
        const int pixel = i / UPP, u = i - pixel * UPP;
        const int sm = pixel / (C::IH * C::IW), pin = pixel - sm * (C::IH * C::IW);
        const int y = pin / C::IW, x = pin - y * C::IW;
        *reinterpret_cast<uint4*>(dst + (size_t)(sm * C::SQ + y * C::RQ + x * C::Q + u) * 16) = v[j];
      }
    }
  };

  int grp = bid;
  if (grp >= ngroups) return;
  stage_load(grp, 0);
  stage_store(0, 0);
  stage_load(grp, 1);
  stage_store(0, 1);
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
    pin_loaded(bh[ks]);
    pin_loaded(bl[ks]);
  }
  __syncthreads();
  constexpr int LO = C::CIN * 2;  // byte offset of the lo part inside a pixel record
  uint8_t* const obase = smem + 2 * C::LDS_BYTES;
  uint8_t* const spare = obase + 2 * C::OUT_BYTES;  // rows past the group's last pixel land here
  // A row group whose LAST tile lies wholly past the group's pixels (conv3: 98 pixels = 7 tiles over RG = 2 row groups
  // of RPW = 4) skips that tile's fragment reads and MFMAs (wave-uniform): the two waves of a SIMD belong to different
  // row groups, so the SIMD issues 7 tiles' MFMAs where it issued 8.
  constexpr int RT_REAL = (C::M + 15) / 16;
  static_assert(C::RPW >= 2 && (RT_REAL - (C::RG - 1) + C::RG - 1) / C::RG >= C::RPW - 1, "at most the last tile of a row group is empty");
  const bool full = (RT_REAL - __builtin_amdgcn_readfirstlane(rg) + C::RG - 1) / C::RG >= C::RPW;
  {
    constexpr int NT = C::RPW;
    int buf = 0;
    int prev_n0 = 0, prev_nv = 0;  // the group whose records wait in the other output buffer, its 16-byte chunks
    constexpr int OV = C::S * C::P * (C::OC * 4 / 16), OIT = (OV + kThreads - 1) / kThreads;
    static_assert(OIT <= 4, "named chunk registers below");
    uint4 oc0, oc1, oc2, oc3;
    // chunk j of the previous group's records: read from LDS behind pair RD(j), stored to HBM behind pair RD(j) + 2 --
    // in the shadow of this group's MFMAs (after the loop, on all eight waves at once, the copy took 8 % of a group)
    auto o_read = [&](int j) {
      const uint8_t* ot = obase + (buf ^ 1) * C::OUT_BYTES;
      const int i = min(tid + j * kThreads, OV - 1);
      return *reinterpret_cast<const uint4*>(ot + (i >> 4) * C::OROW + (i & 15) * 16);
    };
    auto o_write = [&](int j, const uint4& val) {
      const int i = tid + j * kThreads;
      if (i < prev_nv) reinterpret_cast<uint4*>(out + (size_t)prev_n0 * C::P * (C::OC * 4))[i] = val;
    };
    for (; grp < ngroups; grp += nblk) {
      const bool has_next = grp + nblk < ngroups;
      stamp(0);
      if (has_next) stage_load(grp + nblk, 0);
      const uint8_t* tile = smem + buf * C::LDS_BYTES;
      f32x4 acc[NT];  // starts at the bias
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = bv;
      // A fragments run D (hi, lo) pairs ahead of the MFMAs that consume them, in a register ring over the
      // flattened (k-step, row tile) sequence: with two waves per SIMD nothing else hides the LDS latency.
      constexpr int TOT = C::KS * NT, D = C::DEPTH;
      uint4 ah[D], al[D];
      auto a_issue = [&](int idx, int slot) {
        const int ks = idx / NT, t = idx - ks * NT;
        const int tap = ks / C::KSUB, sub = ks - tap * C::KSUB;
        const int kh = tap / C::KW, kw = tap - kh * C::KW;
        const uint8_t* ap = tile + abase[t] + (kh * C::RQ + kw * C::Q) * 16 + sub * 64;
        ah[slot] = *reinterpret_cast<const uint4*>(ap);
        al[slot] = *reinterpret_cast<const uint4*>(ap + LO);
      };
#pragma unroll
      for (int i = 0; i < D; ++i)
        if (i % NT < NT - 1 || full) a_issue(i, i);
      __builtin_amdgcn_sched_barrier(0);
      static_assert(3 + 4 * (OIT - 1) < TOT, "copy-out slots inside the loop");
      // (two loops of TOT / 2: as ONE loop the body is too large for the unroller's full-unroll budget, it unrolls by
      // half the trip count instead, k-steps become run-time indices and the resident fragments move to scratch memory)
      auto pair = [&](int idx) {
        const int ks = idx / NT, t = idx - ks * NT;
        const int slot = idx % D;
        if (t < NT - 1 || full) {
          const bf16x8 xh = __builtin_bit_cast(bf16x8, ah[slot]);
          const bf16x8 xl = __builtin_bit_cast(bf16x8, al[slot]);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ks], xl, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[ks], xh, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ks], xh, acc[t], 0, 0, 0);
        }
        if (idx + D < TOT && ((idx + D) % NT < NT - 1 || full)) a_issue(idx + D, slot);
        if (idx == 1) oc0 = o_read(0);
        if (idx == 3) o_write(0, oc0);
        if (OIT > 1 && idx == 5) oc1 = o_read(1);
        if (OIT > 1 && idx == 7) o_write(1, oc1);
        if (OIT > 2 && idx == 9) oc2 = o_read(2);
        if (OIT > 2 && idx == 11) o_write(2, oc2);
        if (OIT > 3 && idx == 13) oc3 = o_read(3);
        if (OIT > 3 && idx == 15) o_write(3, oc3);
        __builtin_amdgcn_sched_barrier(0);  // keep the reads where they are (the scheduler sinks them to their use)
        // the other buffer was last read one group ago (barrier since): fill it while this group computes
        if (has_next) {
          if (idx == TOT / 3) {
            stage_store(buf ^ 1, 0);
            stage_load(grp + nblk, 1);
          } else if (idx == (2 * TOT) / 3) {
            stage_store(buf ^ 1, 1);
          }
        }
      };
      static_assert(TOT % 2 == 0, "two halves");
#pragma unroll
      for (int idx = 0; idx < TOT / 2; ++idx) pair(idx);
#pragma unroll
      for (int idx = TOT / 2; idx < TOT; ++idx) pair(idx);
      // epilogue: bias + ReLU + hi/lo split into an LDS copy of the group's output records; they leave for HBM as
      // coalesced 16-byte-per-lane copies during the NEXT group's MFMA loop (a wave's own 16 channels are only 32
      // contiguous bytes per pixel).  The output tile is double buffered like the input, so ONE barrier per group
      // orders everything: it publishes this group's records and the next group's staged input, and the records of
      // two groups ago were read out before the barrier in between.
      stamp(1);
      uint8_t* otile = obase + buf * C::OUT_BYTES;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int m = (rg + t * C::RG) * 16 + li;  // this lane's pixel of the tile
        split_store_lds4((m < C::M) ? otile + (size_t)m * C::OROW : spare, C::OC, ch0, acc[t]);
      }
      stamp(2);
      __syncthreads();
      stamp(3);
      prev_n0 = grp * C::S;
      prev_nv = min(C::S, N - prev_n0) * C::P * (C::OC * 4 / 16);
      stamp(4);
      stamp_frame += 1;
      buf ^= 1;
    }
    {  // the last group's records
      const uint8_t* ot = obase + (buf ^ 1) * C::OUT_BYTES;
      uint4* dst = reinterpret_cast<uint4*>(out + (size_t)prev_n0 * C::P * (C::OC * 4));
      for (int i = tid; i < prev_nv; i += kThreads)
        dst[i] = *reinterpret_cast<const uint4*>(ot + (i >> 4) * C::OROW + (i & 15) * 16);
    }
  }
}

template <class C>
__global__ __launch_bounds__(kThreads) void conv_bf16s(const uint8_t* __restrict__ in, const uint4* __restrict__ Bfrag,
                                                       const float* __restrict__ bias, uint8_t* __restrict__ out,
                                                       int N) {
  conv_bf16s_body<C>(in, Bfrag, bias, out, N, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(kThreads) void conv3_bf16s_stamps(const uint8_t* __restrict__ in, const uint4* __restrict__ Bfrag,
                                                               const float* __restrict__ bias, uint8_t* __restrict__ out,
                                                               int N, unsigned long long* stamps) {
  conv_bf16s_body<Conv3F, true>(in, Bfrag, bias, out, N, blockIdx.x, gridDim.x, stamps);
}

// a3 split records -> f32 in place (per pixel: 64 x bf16 hi | 64 x bf16 lo  ->  64 x f32; hi + lo is exact in f32).
// One wave per pixel: all of its loads complete before its stores (same wave, program order).  Used where the trunk
// runs on split-bf16 MFMA but the batch is too small for fc_bf16s and fc goes through the f32 split-K GEMM.
__global__ void unsplit_records64(uint8_t* __restrict__ rec, int64_t pixels) {
  const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= pixels) return;
  const int c = threadIdx.x & 63;
  uint8_t* r = rec + p * 256;
  const uint16_t hi = reinterpret_cast<const uint16_t*>(r)[c], lo = reinterpret_cast<const uint16_t*>(r)[64 + c];
  const float v = bf16_to_f32(hi) + bf16_to_f32(lo);
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  reinterpret_cast<float*>(r)[c] = v;
}

// conv3 over a2's records [N][81][256 B] -> a3's records [N][49][256 B]
inline void launch_conv3_bf16s(const uint8_t* a2, const uint4* B3f, const float* b3, uint8_t* a3, int N, hipStream_t s) {
  note_launch("conv_bf16s<Conv3F>");
  hipLaunchKernelGGL(conv_bf16s<Conv3F>, dim3(persistent_blocks(ceil_div(N, Conv3F::S))), dim3(kThreads), Conv3F::LDS_TOTAL,
                     s, a2, B3f, b3, a3, N);
}
// rela_ffnet_debug_conv3_stamps: the diagnostic variant opts in on its first use
inline hipError_t opt_in_conv3_bf16s_stamps() {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_bf16s_stamps),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, Conv3F::LDS_TOTAL);
  return attr;
}
inline void launch_conv3_bf16s_stamps(const uint8_t* a2, const uint4* B3f, const float* b3, uint8_t* a3, int N,
                                      unsigned long long* stamps, hipStream_t s) {
  hipLaunchKernelGGL(conv3_bf16s_stamps, dim3(std::min(kNumCU, ceil_div(N, Conv3F::S))), dim3(kThreads), Conv3F::LDS_TOTAL, s,
                     a2, B3f, b3, a3, N, stamps);
}
inline void launch_unsplit_records64(uint8_t* records, int64_t pixels, hipStream_t s) {
  note_launch("unsplit_records64");
  hipLaunchKernelGGL(unsplit_records64, dim3(ceil_div(pixels, 4)), dim3(256), 0, s, records, pixels);
}

inline int opt_in_lds_conv_bf16s() {
  const LdsOptIn ks[] = {{reinterpret_cast<const void*>(&conv_bf16s<Conv3F>), Conv3F::LDS_TOTAL}};
  return opt_in(ks);
}

}  // namespace
}  // namespace rela_amd
