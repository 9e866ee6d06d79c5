// conv12_i8.h -- the front of the split-bf16 trunk (kTrunkBf16): conv1 on the int8 matrix cores fused per frame with conv2
// on split records (conv_bf16s.h), as one kernel per pass (conv12_i8), with shader-clock stamps (conv12_i8_stamps) and in
// the learners' job form (conv12_i8_jobs / conv3_bf16s_jobs: several passes per launch); unsplit_trunk_rows turns the
// records the learners keep back into f32.  Included by ffnet.hip only: the kernels live in rela_amd::(anonymous).
#pragma once
#include <type_traits>

#include "conv_bf16s.h"

namespace rela_amd {
namespace {

// ---- conv1 on the INT8 matrix cores, whole frame at a time (r3) ----------------------------------------------------
// The frames are u8, so conv1 needs no floating-point operand at all: the weights of an output channel c become
// 24-bit fixed point, w = s_c * q with |q| <= 127 * 65536 + 127 * 256 + 127 and q = 65536 d_hi + 256 d_mid + d_lo in
// balanced base-256 digits (int8 each), the pixels x - 128 (int8), and
//     conv1(x)[c] = s_c * (65536 S_hi + 256 S_mid + S_lo) + (b_c + 128 s_c sum_k q_k),   S_d = sum_k (x_k - 128) d_k
// with the three S exact in i32 (|S| <= 256 * 128 * 128 = 2^22).  v_mfma_i32_16x16x64_i8 runs at twice the bf16 rate:
// three digit products cost 0.75 of the two bf16 products (hi, mid) they replace -- and carry 24 bits of every weight
// relative to its channel's largest instead of 16, so conv1 of the split-bf16 mode is now within an f32 rounding or
// two of the exact mode and independent of summation order.  The float part is fixed (tests mirror it bit for bit):
//     u = f32(S_hi) * 65536 + f32(S_mid * 256 + S_lo);  y = u * s_c + b'_c      (the integer sum exact, no fused multiply-add)
//
// Layout.  K = 4 taps x 64: the 8 x 8 stride-4 kernel is a 2 x 2 stride-1 kernel over the 4 x 4 space-to-depth image
// (21 x 21 cells of [plane 4][yy 4][xx 4] bytes).  LDS holds the WHOLE frame as [plane][cell 441][16 B] (28 KB; the
// bf16 image of HALF a frame took 30): the B operand of tap (dy, dx) for output pixel (oy, ox) is one aligned
// ds_read_b128 at plane g, cell (oy + dy) * 21 + ox + dx -- 16 consecutive pixels of a tile read 16 consecutive cells,
// and the plane stride is 0 (mod 256), so the lanes a b128 pass serves ({li 0-3, 12-15 of g} + {li 4-11 of g + 1})
// cover the 64 banks once.  A thread stages a cell with four dword loads (rows 4 Y .. 4 Y + 3 of the plane; a wave
// reads 21-cell runs of 84 contiguous bytes), flips the sign bits and stores it with one ds_write_b128.
//
// Schedule (two barriers per frame where the half-frame kernel had five):
//   phase A  conv1: T1 -> T2 (conv2's padded input tile of split records); the previous frame's conv2 output tile O
//            leaves for HBM in the shadow of these MFMAs
//   phase B  conv2: T2 -> O; the next frame's cells are loaded at its start and stored into T1 in its second half
struct Conv12I {
  using C2 = Conv2F;
  static constexpr int GW = 21, NPIX = GW * GW, PLANE_ELEMS = 84 * 84, IN_ELEMS = 4 * PLANE_ELEMS;
  static constexpr int PLANE1 = 7168;  // 441 cells x 16 B, padded to a multiple of 256 B
  static_assert(PLANE1 >= NPIX * 16 && PLANE1 % 256 == 0, "plane stride");
  static constexpr int T1_BYTES = 4 * PLANE1, T2_BYTES = C2::LDS_BYTES, O_BYTES = C2::OUT_BYTES + 256;
  static constexpr int W1_UINT4 = 3 * 2 * 4 * 64;  // [digit hi, mid, lo][ct 2][tap 4][lane 64] x 16 int8
  static constexpr int LDS_TOTAL = T1_BYTES + T2_BYTES + O_BYTES + W1_UINT4 * 16;
  static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");
  static constexpr int CELLS = 4 * NPIX;
  static constexpr int IT = (CELLS + kThreads - 1) / kThreads;  // 4 cells per thread
  static constexpr int RT = 25, RG = 4, RPW = 7;  // 400 pixels = 25 tiles of 16; wave (ct, rg) owns tiles rg + 4 t
  static constexpr int G0 = 3, G1 = 2, G2 = 2;    // three passes over the taps (tiles 0..2, 3..4, 5..6): 12 accumulator registers per tile
  static constexpr int OV16 = C2::P * (C2::OC * 4 / 16);  // 16-byte chunks of an output tile
  static constexpr int OIT = (OV16 + kThreads - 1) / kThreads;
};
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <bool JOBS, bool STAMPS = false>
__device__ __forceinline__ void conv12i_body(const uint8_t* __restrict__ in, const uint8_t* __restrict__ in1, int n_in0,
                                             const uint4* __restrict__ W1d, const float* __restrict__ scale1,
                                             const float* __restrict__ bias1q, const uint4* __restrict__ B2frag,
                                             const float* __restrict__ bias2, uint8_t* __restrict__ out,
                                             uint8_t* __restrict__ a1_out, int a1_lo, int n_a1, int N, int bid, int nblk,
                                             unsigned long long* stamps = nullptr) {
  using F = Conv12I;
  using C2 = Conv2F;
  int stamp_frame = 0;
  auto stamp = [&](int point) {
    if constexpr (STAMPS) {
      if (bid == 0 && (threadIdx.x == 0 || threadIdx.x == 448) && stamp_frame < kStampFrames)
        stamps[((threadIdx.x == 0 ? 0 : 1) * kStampFrames + stamp_frame) * kStampPoints + point] = __builtin_amdgcn_s_memtime();
    }
  };
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* t1 = smem;
  uint8_t* t2 = smem + F::T1_BYTES;
  uint8_t* otile = t2 + F::T2_BYTES;
  uint8_t* spare = otile + C2::OUT_BYTES;  // 256 B: rows past the last pixel of either layer land here
  uint4* w1s = reinterpret_cast<uint4*>(otile + F::O_BYTES);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;

  // ---- residents ----
  for (int i = tid; i < F::W1_UINT4; i += kThreads) w1s[i] = W1d[i];
  const int ct1 = wave & 1, rg1 = wave >> 1;
  const int ct2 = wave % C2::CT, rg2 = wave / C2::CT;
  bf16x8 bh[C2::KS], bl[C2::KS];
  {
    const uint4* bp = B2frag + (size_t)ct2 * C2::KS * 2 * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < C2::KS; ++ks) {
      bh[ks] = __builtin_bit_cast(bf16x8, bp[(size_t)(ks * 2) * 64]);
      bl[ks] = __builtin_bit_cast(bf16x8, bp[(size_t)(ks * 2 + 1) * 64]);
    }
  }
  // operands swapped (weights as the A operand): a lane holds four consecutive channels of one pixel
  const int ch1 = ct1 * 16 + 4 * g, ch2 = ct2 * 16 + 4 * g;
  const f32x4 bv2 = *reinterpret_cast<const f32x4*>(bias2 + ch2);
  // conv1 B fragments: lane (li, g) reads plane g's cell of its pixel (+ the tap's cell offset)
  int a1base[F::RPW];
#pragma unroll
  for (int t = 0; t < F::RPW; ++t) {
    const int m = min((min(rg1 + t * F::RG, F::RT - 1)) * 16 + li, 399);
    const int oy = m / 20, ox = m - oy * 20;
    a1base[t] = g * F::PLANE1 + (oy * F::GW + ox) * 16;
  }
  int a2base[C2::RPW];
#pragma unroll
  for (int t = 0; t < C2::RPW; ++t) {
    const int m = (rg2 + t * C2::RG) * 16 + li;
    const int mm = (m < C2::M) ? m : 0;
    const int oy = mm / C2::OW, ox = mm - oy * C2::OW;
    a2base[t] = (oy * C2::STRIDE * C2::RQ + ox * C2::STRIDE * C2::Q + g) * 16;
  }

  // ---- staging of a frame's cells (unpredicated, clamped cell index) ----
  // (the cell addresses are derived per use from an opaque copy of tid: hoisted out of the frame loop they pin 8 registers)
  auto cell_of = [&](int j, int& goff, int& loff) {
    int tq = tid;
    asm volatile("" : "+v"(tq));
    const int c = min(tq + j * kThreads, F::CELLS - 1);
    const int pl = c / F::NPIX, P = c - pl * F::NPIX;
    const int Y = P / F::GW, X = P - Y * F::GW;
    goff = pl * F::PLANE_ELEMS + 4 * Y * 84 + 4 * X;
    loff = pl * F::PLANE1 + P * 16;
  };
  uint32_t st[F::IT][4];
  int st_loff[F::IT];  // (the cell's LDS address travels with its bytes from the load to the store)
  auto g_load1 = [&](int n, int j) {
    const uint8_t* src = (!JOBS || n < n_in0) ? in + (size_t)n * F::IN_ELEMS : in1 + (size_t)(n - n_in0) * F::IN_ELEMS;
    int goff;
    cell_of(j, goff, st_loff[j]);
#pragma unroll
    for (int r = 0; r < 4; ++r) st[j][r] = *reinterpret_cast<const uint32_t*>(src + goff + r * 84);
  };
  auto s_store = [&](int j) {  // x -> x - 128 as int8: flip the sign bits
    *reinterpret_cast<uint4*>(t1 + st_loff[j]) = make_uint4(st[j][0] ^ 0x80808080u, st[j][1] ^ 0x80808080u,
                                                            st[j][2] ^ 0x80808080u, st[j][3] ^ 0x80808080u);
  };

  // ---- conv1 over the tiles [T0, T0 + NT) of this wave: T1 -> split records in T2 ----
  // `hook(i)` runs after the MFMAs of pair i (the caller's copy-out slices)
  auto conv1_pass = [&](auto t0_tag, auto nt_tag, auto&& hook) {
    constexpr int T0 = decltype(t0_tag)::value, NT = decltype(nt_tag)::value;
    i32x4 s_hi[NT], s_mid[NT], s_lo[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) s_hi[t] = s_mid[t] = s_lo[t] = i32x4{0, 0, 0, 0};
    constexpr int TOT = 4 * NT, D = 4;
    uint4 x[D];
    auto a_issue = [&](int idx, int slot) {
      const int ks = idx / NT, t = T0 + idx - ks * NT;
      x[slot] = *reinterpret_cast<const uint4*>(t1 + a1base[t] + ((ks >> 1) * F::GW + (ks & 1)) * 16);
    };
    // this wave's digit fragments of the current tap: ONE register set (a second one spills: conv2's resident weights
    // hold 128 of the 256 registers); the next tap's are issued behind the last MFMAs that read these
    uint4 wd[3];
    auto w_issue = [&](int ks) {
#pragma unroll
      for (int d = 0; d < 3; ++d) wd[d] = w1s[((d * 2 + ct1) * 4 + ks) * 64 + lane];
    };
    w_issue(0);
#pragma unroll
    for (int i = 0; i < D; ++i) a_issue(i, i);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int idx = ks * NT + t, slot = idx % D;
        const i32x4 xv = __builtin_bit_cast(i32x4, x[slot]);
        s_hi[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, wd[0]), xv, s_hi[t], 0, 0, 0);
        s_mid[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, wd[1]), xv, s_mid[t], 0, 0, 0);
        s_lo[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, wd[2]), xv, s_lo[t], 0, 0, 0);
        if (idx + D < TOT) a_issue(idx + D, slot);
        if (t == NT - 1 && ks + 1 < 4) w_issue(ks + 1);
        hook(idx);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // (scale and bias come from L1 per pass: kept across the frame loop they would cost eight registers)
    int chq = ch1;
    asm volatile("" : "+v"(chq));
    const f32x4 sc1 = *reinterpret_cast<const f32x4*>(scale1 + chq), bv1 = *reinterpret_cast<const f32x4*>(bias1q + chq);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int rt = rg1 + (T0 + t) * F::RG;
      if (rt >= F::RT) continue;  // (wave-uniform: only the group rg = 0 has a seventh tile)
      const int m = rt * 16 + li;
      const int y = m / 20, xx = m - y * 20;
      const i32x4 ml = s_mid[t] * 256 + s_lo[t];  // exact: |S_mid * 256 + S_lo| < 2^31
      const f32x4 u = __builtin_convertvector(s_hi[t], f32x4) * 65536.0f + __builtin_convertvector(ml, f32x4);
      const f32x4 v = u * sc1 + bv1;
      split_store_lds4((m < 400) ? t2 + (size_t)(y * C2::RQ + xx * C2::Q) * 16 : spare, 32, ch1, v);
    }
  };

  int n = bid;
  if (n >= N) return;
#pragma unroll
  for (int j = 0; j < F::IT; ++j) g_load1(n, j);
#pragma unroll
  for (int j = 0; j < F::IT; ++j) s_store(j);
#pragma unroll
  for (int ks = 0; ks < C2::KS; ++ks) {
    pin_loaded(bh[ks]);
    pin_loaded(bl[ks]);
  }
  __syncthreads();
  constexpr int LO = C2::CIN * 2;
  int prev = -1;  // the frame whose conv2 output waits in O
  // the output tile of frame `prev` -> HBM: chunk j is read from O after pair RD(j) of conv1's first pass and stored
  // after pair RD(j) + 2 (first frame: the reads return stale bytes and the stores are skipped)
  static_assert(F::OIT == 3, "three named chunk registers below (an array indexed inside the hook stays in scratch)");
  uint4 oc0, oc1, oc2;
  auto o_read = [&](int j) {
    const int i = min(tid + j * kThreads, F::OV16 - 1);
    return *reinterpret_cast<const uint4*>(otile + (i >> 4) * C2::OROW + (i & 15) * 16);
  };
  auto o_write = [&](int j, const uint4& v) {
    const int i = min(tid + j * kThreads, F::OV16 - 1);
    if (prev >= 0) reinterpret_cast<uint4*>(out + (size_t)prev * C2::P * (C2::OC * 4))[i] = v;
  };
  auto copy_hook = [&](int idx) {
    if (idx == 1) oc0 = o_read(0);
    if (idx == 3) o_write(0, oc0);
    if (idx == 5) oc1 = o_read(1);
    if (idx == 7) o_write(1, oc1);
    if (idx == 9) oc2 = o_read(2);
    if (idx == 11) o_write(2, oc2);
  };
  static_assert(3 + 4 * (F::OIT - 1) < 4 * F::G0 && F::G0 + F::G1 + F::G2 == F::RPW, "copy-out slots inside the first pass");
  for (; n < N; n += nblk) {
    const int nn = (n + nblk < N) ? n + nblk : n;  // (the last round re-stages its own frame)
    stamp(0);
    conv1_pass(std::integral_constant<int, 0>{}, std::integral_constant<int, F::G0>{}, copy_hook);
    conv1_pass(std::integral_constant<int, F::G0>{}, std::integral_constant<int, F::G1>{}, [](int) {});
    conv1_pass(std::integral_constant<int, F::G0 + F::G1>{}, std::integral_constant<int, F::G2>{}, [](int) {});
    stamp(1);
    __syncthreads();  // T2 complete, T1 and O free
    stamp(2);
    if constexpr (JOBS) {
      if (a1_out && (unsigned)(n - a1_lo) < (unsigned)n_a1) {  // (block-uniform) conv1's records: [400 pixels][32 hi | 32 lo]
        uint4* dst = reinterpret_cast<uint4*>(a1_out + (size_t)n * (400 * 128));
        for (int i = tid; i < 400 * 8; i += kThreads) {
          const int px = i >> 3, u = i & 7;
          const int y = px / 20, x = px - y * 20;
          dst[i] = *reinterpret_cast<const uint4*>(t2 + (size_t)(y * C2::RQ + x * C2::Q + u) * 16);
        }
      }
    }
    // ---- conv2 from T2; the next frame's cells go into T1 in the second half ----
    {
      f32x4 acc[C2::RPW];
#pragma unroll
      for (int t = 0; t < C2::RPW; ++t) acc[t] = bv2;
      constexpr int TOT = C2::KS * C2::RPW, D = 3;
      uint4 ah[D], al[D];
      auto a_issue = [&](int idx, int slot) {
        const int ks = idx / C2::RPW, t = idx - ks * C2::RPW;
        const int kh = ks / C2::KW, kw = ks - kh * C2::KW;  // KSUB = 1: one k-step per tap
        const uint8_t* ap = t2 + a2base[t] + (kh * C2::RQ + kw * C2::Q) * 16;
        ah[slot] = *reinterpret_cast<const uint4*>(ap);
        al[slot] = *reinterpret_cast<const uint4*>(ap + LO);
      };
#pragma unroll
      for (int i = 0; i < D; ++i) a_issue(i, i);
      __builtin_amdgcn_sched_barrier(0);
      static_assert(TOT / 2 + 6 * (F::IT - 1) < TOT, "staging slots inside the loop");
#pragma unroll
      for (int idx = 0; idx < TOT; ++idx) {
        const int ks = idx / C2::RPW, t = idx - ks * C2::RPW;
        const int slot = idx % D;
        const bf16x8 xh = __builtin_bit_cast(bf16x8, ah[slot]);
        const bf16x8 xl = __builtin_bit_cast(bf16x8, al[slot]);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ks], xl, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[ks], xh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ks], xh, acc[t], 0, 0, 0);
        if (idx + D < TOT) a_issue(idx + D, slot);
        // the next frame's cells: loaded behind pairs 1, 4, 7, 10, stored (sign bits flipped) in the second half
#pragma unroll
        for (int j = 0; j < F::IT; ++j) {
          if (idx == 1 + 3 * j) g_load1(nn, j);
          if (idx == TOT / 2 + 6 * j) s_store(j);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      stamp(3);
#pragma unroll
      for (int t = 0; t < C2::RPW; ++t) {
        const int m = (rg2 + t * C2::RG) * 16 + li;
        split_store_lds4((m < C2::M) ? otile + (size_t)m * C2::OROW : spare, C2::OC, ch2, acc[t]);
      }
    }
    stamp(4);
    __syncthreads();  // O complete, T1 ready, T2 free
    stamp(5);
    stamp_frame += 1;
    prev = n;
  }
  {  // the last frame's output tile
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)prev * C2::P * (C2::OC * 4));
    for (int i = tid; i < F::OV16; i += kThreads)
      dst[i] = *reinterpret_cast<const uint4*>(otile + (i >> 4) * C2::OROW + (i & 15) * 16);
  }
}

__global__ __launch_bounds__(kThreads) void conv12_i8(const uint8_t* __restrict__ in, const uint4* __restrict__ W1d,
                                                      const float* __restrict__ scale1, const float* __restrict__ bias1q,
                                                      const uint4* __restrict__ B2frag, const float* __restrict__ bias2,
                                                      uint8_t* __restrict__ out, int N) {
  conv12i_body<false>(in, nullptr, N, W1d, scale1, bias1q, B2frag, bias2, out, nullptr, 0, 0, N, blockIdx.x, gridDim.x);
}

// Several trunk passes in one launch (the learner's three forwards: online over [s ; s'], target over s'): job j owns
// the blocks [block0, block0 + nblocks) and walks its own frames with its own weights.
struct TrunkJob {
  const uint8_t *in0, *in1;  // rows [0, n_in0) of in0, then rows of in1
  int n_in0;
  const uint4 *B2, *B3;  // conv2 / conv3 fragments of the job's net
  const float *b2, *b3;
  const uint4* W1d;  // conv1 for the int8 matrix cores (conv12_i8_jobs)
  const float *s1q, *b1q;
  uint8_t *a1_out;  // conv1's records [N][400][128 B], written for the rows [a1_lo, a1_lo + n_a1); or NULL
  int a1_lo, n_a1;
  uint8_t *a2, *a3;  // conv2's / conv3's split records [N][81][256 B] / [N][49][256 B]
  int N, block0, nblocks;
};
constexpr int kMaxTrunkJobs = 3;
struct TrunkJobs {
  TrunkJob j[kMaxTrunkJobs];
  int n;
};
inline TrunkJob trunk_job(const uint4* W1d, const float* s1q, const float* b1q, const uint4* B2, const float* b2, const uint4* B3,
                          const float* b3, const uint8_t* in0, const uint8_t* in1, int n_in0, uint8_t* a1_out, int a1_lo, int n_a1,
                          uint8_t* a2, uint8_t* a3, int N, int block0, int nblocks) {
  TrunkJob j{};
  j.in0 = in0, j.in1 = in1, j.n_in0 = n_in0;
  j.B2 = B2, j.B3 = B3, j.b2 = b2, j.b3 = b3;
  j.W1d = W1d, j.s1q = s1q, j.b1q = b1q;
  j.a1_out = a1_out, j.a1_lo = a1_lo, j.n_a1 = n_a1;
  j.a2 = a2, j.a3 = a3;
  j.N = N, j.block0 = block0, j.nblocks = nblocks;
  return j;
}
__global__ __launch_bounds__(kThreads) void conv12_i8_stamps(const uint8_t* __restrict__ in, const uint4* __restrict__ W1d,
                                                             const float* __restrict__ scale1, const float* __restrict__ bias1q,
                                                             const uint4* __restrict__ B2frag, const float* __restrict__ bias2,
                                                             uint8_t* __restrict__ out, int N, unsigned long long* stamps) {
  conv12i_body<false, true>(in, nullptr, N, W1d, scale1, bias1q, B2frag, bias2, out, nullptr, 0, 0, N, blockIdx.x, gridDim.x, stamps);
}
__global__ __launch_bounds__(kThreads) void conv12_i8_jobs(TrunkJobs jobs) {
  int k = 0;
  while (k + 1 < jobs.n && (int)blockIdx.x >= jobs.j[k + 1].block0) ++k;
  const TrunkJob& t = jobs.j[k];
  conv12i_body<true>(t.in0, t.in1, t.n_in0, t.W1d, t.s1q, t.b1q, t.B2, t.b2, t.a2, t.a1_out, t.a1_lo, t.n_a1, t.N,
                     (int)blockIdx.x - t.block0, t.nblocks);
}
__global__ __launch_bounds__(kThreads) void conv3_bf16s_jobs(TrunkJobs jobs) {
  int k = 0;
  while (k + 1 < jobs.n && (int)blockIdx.x >= jobs.j[k + 1].block0) ++k;
  const TrunkJob& t = jobs.j[k];
  conv_bf16s_body<Conv3F>(t.a2, t.B3, t.b3, t.a3, t.N, (int)blockIdx.x - t.block0, t.nblocks);
}

// split records -> f32, in place, for the rows the backward kernels read: a1 [rows][400] records of 32 channels
// (64 B hi | 64 B lo), a2 [rows][81] and a3 [rows][49] records of 64 channels (128 B hi | 128 B lo).  A record is read
// whole by the lanes that then overwrite it (one wave per 64-channel record, half a wave per 32-channel one).
__global__ void unsplit_trunk_rows(uint8_t* __restrict__ a1, uint8_t* __restrict__ a2, uint8_t* __restrict__ a3, int rows,
                                   int blocks1, int blocks2) {
  // a thread owns four channels of a record: 8 B of hi + 8 B of lo in, 16 B of f32 out; the 8 (a1) or 16 (a2, a3) lanes
  // of a record sit in one wave, which reads all its records before it overwrites any
  int b = blockIdx.x;
  const int t = threadIdx.x;
  int64_t rec;
  int q, C;
  uint8_t* base;
  bool ok;
  if (b < blocks1) {
    rec = (int64_t)b * 32 + (t >> 3), q = t & 7, C = 32, base = a1, ok = rec < (int64_t)rows * 400;
  } else {
    b -= blocks1;
    base = a2;
    int64_t pixels = (int64_t)rows * 81;
    if (b >= blocks2) b -= blocks2, base = a3, pixels = (int64_t)rows * 49;
    rec = (int64_t)b * 16 + (t >> 4), q = t & 15, C = 64, ok = rec < pixels;
  }
  uint8_t* r = base + (ok ? rec : 0) * (C * 4);
  const uint2 hi = *reinterpret_cast<const uint2*>(r + q * 8), lo = *reinterpret_cast<const uint2*>(r + C * 2 + q * 8);
  float4 v;
  v.x = __uint_as_float(hi.x << 16) + __uint_as_float(lo.x << 16);
  v.y = __uint_as_float(hi.x & 0xffff0000u) + __uint_as_float(lo.x & 0xffff0000u);
  v.z = __uint_as_float(hi.y << 16) + __uint_as_float(lo.y << 16);
  v.w = __uint_as_float(hi.y & 0xffff0000u) + __uint_as_float(lo.y & 0xffff0000u);
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (ok) *reinterpret_cast<float4*>(r + q * 16) = v;
}

// frames u8 [N][4][84][84] -> a2's records [N][81][256 B]
inline void launch_conv12_i8(const uint8_t* frames, const uint4* W1d, const float* s1q, const float* b1q, const uint4* B2f,
                             const float* b2, uint8_t* a2, int N, hipStream_t s) {
  note_launch("conv12_i8");
  hipLaunchKernelGGL(conv12_i8, dim3(persistent_blocks(N)), dim3(kThreads), Conv12I::LDS_TOTAL, s, frames, W1d, s1q, b1q, B2f, b2,
                     a2, N);
}
// rela_ffnet_debug_conv12_stamps: the diagnostic variant opts in on its first use
inline hipError_t opt_in_conv12_i8_stamps() {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv12_i8_stamps),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, Conv12I::LDS_TOTAL);
  return attr;
}
inline void launch_conv12_i8_stamps(const uint8_t* frames, const uint4* W1d, const float* s1q, const float* b1q, const uint4* B2f,
                                    const float* b2, uint8_t* a2, int N, unsigned long long* stamps, hipStream_t s) {
  hipLaunchKernelGGL(conv12_i8_stamps, dim3(std::min(kNumCU, N)), dim3(kThreads), Conv12I::LDS_TOTAL, s, frames, W1d, s1q, b1q,
                     B2f, b2, a2, N, stamps);
}
// A TrunkJobs pass over `blocks` blocks (the jobs' ranges together): conv1 -> conv2 of every job in one launch, then
// (label3 != NULL: the jobs have an a3) conv3 likewise.  conv3 walks groups of Conv3F::S frames over the same block
// ranges (a job's surplus blocks leave at once).
inline void launch_trunk_jobs(const TrunkJobs& jobs, int blocks, const char* label12, const char* label3, hipStream_t s) {
  {
    ProfScope prof(label12, s);
    note_launch("conv12_i8_jobs");
    hipLaunchKernelGGL(conv12_i8_jobs, dim3(blocks), dim3(kThreads), Conv12I::LDS_TOTAL, s, jobs);
  }
  if (!label3) return;
  ProfScope prof(label3, s);
  note_launch("conv3_bf16s_jobs");
  hipLaunchKernelGGL(conv3_bf16s_jobs, dim3(blocks), dim3(kThreads), Conv3F::LDS_TOTAL, s, jobs);
}
inline void launch_unsplit_trunk_rows(uint8_t* a1, uint8_t* a2, uint8_t* a3, int rows, hipStream_t s) {
  const int b1 = (int)ceil_div((int64_t)rows * 400, 32), b2 = (int)ceil_div((int64_t)rows * 81, 16),
            b3 = (int)ceil_div((int64_t)rows * 49, 16);
  note_launch("unsplit_trunk_rows");
  hipLaunchKernelGGL(unsplit_trunk_rows, dim3(b1 + b2 + b3), dim3(256), 0, s, a1, a2, a3, rows, b1, b2);
}

inline int opt_in_lds_conv12_i8() {
  const LdsOptIn ks[] = {{reinterpret_cast<const void*>(&conv12_i8), Conv12I::LDS_TOTAL},
                         {reinterpret_cast<const void*>(&conv12_i8_jobs), Conv12I::LDS_TOTAL}};
  return opt_in(ks);
}

}  // namespace
}  // namespace rela_amd
