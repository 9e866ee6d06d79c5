// conv12_s3.h -- conv1 -> conv2 of the AtariFFNet trunk (pyrela/net.py:20-25) FUSED per frame through LDS in the f32x3
// arithmetic: conv1's output a1 (400 pixels x 32 channels) never reaches HBM (r4: conv1_bf16x3 wrote 328 MB per 6,400
// frames and gemm_f32emu<conv2> read 395 MB back).
//
//   conv1  u8 frames x 24-bit fixed-point weights on the INT8 matrix cores, exactly as conv12_i8 (conv12_i8.h): the pixels
//          x - 128 as int8, every weight as three balanced base-256 digits relative to its channel's largest, three
//          exact i32 sums per output, one f32 scale + bias (pack_conv1_i8).  Whole frame in LDS as [plane][4x4 cell].
//   a1     ReLU, split into the three bf16 parts (split3 record, 192 B per pixel) in conv1's epilogue, stored into the
//          LDS image T2: pixel (y, x) at 16-byte unit y * RQ + x * Q with Q = 13 (12 + 1 pad), RQ = 261, so that the 16
//          consecutive OUTPUT pixels of a conv2 tile (stride 2) advance by 10 units mod 16: conflict-free ds_read_b128.
//   conv2  six products per operand pair on v_mfma_f32_16x16x32_bf16 (gemm_f32emu.h's arithmetic, small terms in their own
//          accumulator); a wave owns 16 output channels, its 16 k-steps x 3 parts of weights are RESIDENT (192 registers);
//          tile by tile (16 pixels), fragments three k-steps ahead in a register ring.  A frame runs FIVE tiles (pixels
//          0 .. 79); pixel 80's 16 input records go into an LDS ring of RING_S slots, and one more tile over the ring's
//          slots, when it is full and after the block's last frame, computes pixel 80 of up to RING_S frames at once.
//          Every output is one MFMA column fed by its own pixel's fragments in the same k order: the same bits as a
//          sixth tile per frame that held pixel 80 and fifteen copies of it.
//   a2     ReLU, split, staged in LDS as records and copied out whole (coalesced 16-byte stores) under the next frame's
//          conv1 (pixels 0 .. 79; pixel 80's three parts go from the ring's tile straight to HBM).
// One block of FOUR waves per CU (512 registers each: 240 hold weights), persistent over the frames b, b + grid, ...;
// two barriers per frame.  Registers by construction: conv2's 192 weight registers are pinned into the accumulator half
// of the file (MFMA A operands only) beside the sums; conv1's digits, every address and every staged byte live in the 256
// VGPRs: no scratch in either instantiation.  Per frame a thread stages two units of four cells by 16-byte row loads
// (uniform frame base + 32-bit offset + immediate row offset); the offsets that do not depend on the frame (T1 / T2 / O
// places of conv1's tiles, conv2's tiles and the copy-out chunks) are computed once before the frame loop.
// A1OUT (the learner's online(obs) pass): a1 is also written to HBM as f32 channel-last, what the backward kernels
// read.
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_s3.h"

namespace rela_amd {
namespace s3 {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // a frame's rows are 4-byte aligned only
// probe builds only (tools/ubench/s3_probe.hip): leave one part of the kernel out to see what it costs
#ifndef C12_ABLATE
#define C12_ABLATE 0
#endif

constexpr bool kNoCopyOut = C12_ABLATE == 1, kNoStage = C12_ABLATE == 2, kNoEpi1 = C12_ABLATE == 3, kNoEpi2 = C12_ABLATE == 4,
               kNoConv1 = C12_ABLATE == 5, kNoConv2 = C12_ABLATE == 6;
// (conv12_s3_copy2's pass-through, timing only: 7 loads its pieces and stores nothing, 8 stores registers it never loaded)
constexpr bool kNoPtStore = C12_ABLATE == 7, kNoPtLoad = C12_ABLATE == 8;

struct Conv12S {
  static constexpr int kT = 256;
  static constexpr int GW = 21, NPIX = GW * GW, PLANE_ELEMS = 84 * 84, IN_ELEMS = 4 * PLANE_ELEMS;
  static constexpr int PLANE1 = 7168;                 // 441 cells x 16 B, padded to a multiple of 256 B
  static constexpr int T1_BYTES = 4 * PLANE1;         // the frame as int8 cells
  static constexpr int Q = 13, RQ = 261;              // a1 image: pixel / row stride in 16-byte units
  static constexpr int T2_BYTES = 20 * RQ * 16;       // 83,520
  static constexpr int OROW = 400;                    // a2 record (384 B) + 16: the 16 pixels of a store spread over the banks
  // conv2's image is 9 x 9 = 81 pixels = five whole 16-pixel tiles + pixel 80.  The frame loop runs the five tiles; pixel
  // 80's input patch (the a1 records of rows 16 .. 19 x columns 16 .. 19, in tap order: 16 x 192 B) is copied into a ring
  // of RING_S slots, and ONE tile over the ring's slots -- lane li takes slot li -- yields pixel 80 of RING_S frames.
  // Slot stride 202 units (10 mod 16, as the pixel stride 2 Q of a tile inside T2): conflict-free ds_read_b128.
  static constexpr int C2TILES = 5, C2PIX = C2TILES * 16;
  static constexpr int O_BYTES = C2PIX * OROW;
  static constexpr int RING_S = 5;
  static constexpr int PATCH_UNITS = 16 * 12, SLOT_BYTES = 202 * 16;
  static constexpr int RING = T1_BYTES + T2_BYTES + O_BYTES;
  static constexpr int LDS_TOTAL = RING + RING_S * SLOT_BYTES;  // 160,352
  static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");
  static_assert(RING_S >= 1 && RING_S <= 16, "one slot per lane of a tile's column");
  static constexpr int OV16 = C2PIX * 24, OIT = (OV16 + kT - 1) / kT;  // 16-byte chunks of an output tile: 8 per thread
  // staging by 16-byte row loads: a unit = four cells side by side (X0 .. X0 + 3) of one plane, six units per cell row
  // (X0 = 0, 4, 8, 12, 16 and 17: the sixth unit, cells 17 .. 20, re-writes the cells 17 .. 19 with the same bytes)
  static constexpr int UNITS = 4 * GW * 6, UIT = (UNITS + kT - 1) / kT;  // 504: two units per thread
  static constexpr int KS2 = 16;
  // k-step -> tap in pack_f32emu_at's mode-1 order (f32emu::ProbConv2::tap), as byte offset inside the a1 image
  static constexpr int tap2(int ks) {
    const int c = ks >> 2, j = ks & 3;
    const int dh = j >> 1, dw = (j ^ (j >> 1)) & 1;
    return (((c >> 1) + 2 * dh) << 2) | ((c & 1) + 2 * dw);
  }
  static constexpr int koff2(int ks) { return ((tap2(ks) >> 2) * RQ + (tap2(ks) & 3) * Q) * 16; }
};

// W1d / scale1 / bias1q: pack_conv1_i8 ([digit][ct 2][tap 4][lane] x 16 int8); B2: pack_f32emu_at mode 1
// ([ks][u][part][lane] x 8 bf16); out: a2 records [N][81] x 384 B; A1OUT: a1 also as f32 [N][400][32] (a1_out).
// COPY (conv12_s3_copy, the Ape-X shard's target forward): every 16-byte row piece a thread stages is ALSO stored, from
// the registers it was loaded into, to the frame's row of a ring of frame rows: frame fr -> copy_dst + ((copy_first + fr)
// wrapped once at copy_ring) * IN_ELEMS.  The units cover all 84 bytes of all 84 rows of the 4 planes (bytes 68 .. 79 of a
// row and the clamped last unit twice, with the same values), so the row is the frame, byte for byte.
// COPY == 2 (conv12_s3_copy2: the same forward, which stores the insert's obs rows too): besides, frame fr of a SECOND
// source in2 (N frames, the stride of `in`) passes through to row (copy2_first + fr) wrapped once at copy_ring of copy2_dst.
// Its bytes take no part in the arithmetic: the thread's eight row pieces of the frame -- the same units, so again the whole
// frame -- are loaded behind conv1's later items and stored behind conv2's early ones, the frame the block is computing,
// through four rotating registers (pt): every piece has some 20 items of MFMAs between its load and its store, and every
// wait the compiler places for them is a counted vmcnt (nothing of the staging's own loads is outstanding behind them).
template <bool A1OUT, int COPY>
__device__ __forceinline__ void conv12_s3_body(const uint8_t* __restrict__ in, const uint4* __restrict__ W1d,
                                               const float* __restrict__ scale1, const float* __restrict__ bias1q,
                                               const uint4* __restrict__ B2, const float* __restrict__ bias2,
                                               uint8_t* __restrict__ out, float* __restrict__ a1_out, int N,
                                               uint8_t* __restrict__ copy_dst, int copy_first, int copy_ring,
                                               const uint8_t* __restrict__ in2, uint8_t* __restrict__ copy2_dst,
                                               int copy2_first) {
  using F = Conv12S;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_c12[];
  uint8_t* t1 = smem_c12;
  uint8_t* t2 = t1 + F::T1_BYTES;
  uint8_t* otile = t2 + F::T2_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bid = blockIdx.x, nblk = gridDim.x;
  int n = bid;
  if (n >= N) return;

  // ---- residents: conv2's weights (this wave's 16 channels), conv1's digits (this wave's column tile)
  const int ct1 = wave & 1, rg1 = wave >> 1;
  bf16x8 w2[F::KS2][3];
  {
    const uint4* bp = B2 + (size_t)wave * 3 * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < F::KS2; ++ks)
#pragma unroll
      for (int p = 0; p < 3; ++p) w2[ks][p] = __builtin_bit_cast(bf16x8, bp[(size_t)(ks * TN * 3 + p) * 64]);
  }
  i32x4 wd[4][3];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int d = 0; d < 3; ++d) wd[ks][d] = __builtin_bit_cast(i32x4, W1d[((d * 2 + ct1) * 4 + ks) * 64 + lane]);
  // registers by construction (the pins are empty statements: they only say where a value lives at that point).  conv2's
  // 192 weight registers are MFMA A operands only: they sit in the accumulator half of the register file, whose other 64
  // registers hold the sums (60 in conv1's five-tile pass, 8 in conv2).  conv1's 48 digit registers and everything VALU,
  // LDS and VMEM touch share the 256 architectural VGPRs: no spills, no copies between the halves but the sums' read-out.
  // (All 240 in the accumulator half leaves 16 for the sums: in the compiled loop conv1 then moves every sum
  // in and out around its MFMA.)
  auto pin_weights = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < F::KS2; ++ks)
#pragma unroll
      for (int p = 0; p < 3; ++p) asm volatile("" : "+a"(w2[ks][p]));
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int d = 0; d < 3; ++d) asm volatile("" : "+v"(wd[ks][d]));
  };
  pin_weights();
  const int ch1 = ct1 * 16 + 4 * g, ch2 = wave * 16 + 4 * g;
  const f32x4 sc1 = *reinterpret_cast<const f32x4*>(scale1 + ch1), bv1 = *reinterpret_cast<const f32x4*>(bias1q + ch1);
  const f32x4 bv2 = *reinterpret_cast<const f32x4*>(bias2 + ch2);

  // ---- staging of a frame by 16-byte row loads: unit u = rows 4Y .. 4Y + 3 x 16 bytes from cell X0 of one plane, i.e.
  // four cells side by side; which dword of which row goes to which cell is only a choice of registers (clamped unit index)
  u32x4_a4 sq[F::UIT][4];
  uint32_t ugoff[F::UIT], uloff[F::UIT];  // (frame-invariant: this thread's units in the frame and in T1)
#pragma unroll
  for (int j = 0; j < F::UIT; ++j) {
    const int u = min(tid + j * F::kT, F::UNITS - 1);
    const int pl = u / (F::GW * 6), rem = u - pl * (F::GW * 6);
    const int Y = rem / 6, qi = rem - Y * 6;
    const int X0 = qi < 5 ? 4 * qi : 17;
    ugoff[j] = (uint32_t)(pl * F::PLANE_ELEMS + 4 * Y * 84 + 4 * X0);
    uloff[j] = (uint32_t)(pl * F::PLANE1 + (Y * F::GW + X0) * 16);
  }
  auto g_load4 = [&](int fr, int j) __attribute__((always_inline)) {
    const uint8_t* fb = in + (size_t)fr * F::IN_ELEMS;  // uniform frame base + 32-bit offset + the row as immediate
#pragma unroll
    for (int r = 0; r < 4; ++r) sq[j][r] = *reinterpret_cast<const u32x4_a4*>(fb + (size_t)ugoff[j] + r * 84);
  };
  // COPY: frame fr's row of the destination ring (uniform: copy_first + fr < 2 copy_ring, one compare and subtract) ...
  auto copy_row = [&](int fr) __attribute__((always_inline)) -> uint8_t* {
    int sl = copy_first + fr;
    if (sl >= copy_ring) sl -= copy_ring;
    return copy_dst + (size_t)sl * F::IN_ELEMS;
  };
  // ... and row r of unit j into it, at the place it was loaded from (uniform base + the same 32-bit offset + immediate)
  auto g_copy4 = [&](uint8_t* cb, int j, int r) __attribute__((always_inline)) {
    *reinterpret_cast<u32x4_a4*>(cb + (size_t)ugoff[j] + r * 84) = sq[j][r];
  };
  // COPY == 2: piece P of the pass-through frame = row P & 3 of unit P >> 2, through register P & 3 (cb2: frame n's row)
  u32x4_a4 pt[4] = {};
  uint8_t* cb2 = nullptr;
  auto pt_load = [&](auto p_tag) __attribute__((always_inline)) {
    constexpr int P = decltype(p_tag)::value;
    const uint8_t* fb = in2 + (size_t)n * F::IN_ELEMS;
    if constexpr (!kNoPtLoad) pt[P & 3] = *reinterpret_cast<const u32x4_a4*>(fb + (size_t)ugoff[P >> 2] + (P & 3) * 84);
  };
  auto pt_store = [&](auto p_tag) __attribute__((always_inline)) {
    constexpr int P = decltype(p_tag)::value;
    const u32x4_a4 v = pt[P & 3];
    if constexpr (!kNoPtStore) *reinterpret_cast<u32x4_a4*>(cb2 + (size_t)ugoff[P >> 2] + (P & 3) * 84) = v;
    else asm volatile("" ::"v"(v));
  };
  auto s_store4 = [&](int j, int k) __attribute__((always_inline)) {  // cell X0 + k of unit j; x -> x - 128: flip the sign bits
    *reinterpret_cast<uint4*>(t1 + uloff[j] + k * 16) = make_uint4(sq[j][0][k] ^ 0x80808080u, sq[j][1][k] ^ 0x80808080u,
                                                                   sq[j][2][k] ^ 0x80808080u, sq[j][3][k] ^ 0x80808080u);
  };

  // ---- the output tile of the previous frame -> HBM, in slices behind conv1's MFMAs
  int prev = -1;
  static_assert(F::OIT == 8, "eight named chunk registers (an array indexed inside the hooks stays in scratch)");
  uint4 oc0, oc1, oc2, oc3, oc4, oc5, oc6, oc7;
  auto oc_at = [&](auto jt) -> uint4& {
    constexpr int j = decltype(jt)::value;
    if constexpr (j == 0) return oc0;
    else if constexpr (j == 1) return oc1;
    else if constexpr (j == 2) return oc2;
    else if constexpr (j == 3) return oc3;
    else if constexpr (j == 4) return oc4;
    else if constexpr (j == 5) return oc5;
    else if constexpr (j == 6) return oc6;
    else return oc7;
  };
  // (frame-invariant: chunk j of this thread inside O.  Its place in the frame's records, i * 16, is recomputed at each
  // store -- two VALU instructions; eight more live registers across the frame loop bring 20 / 28 B of scratch back)
  uint32_t oloff[F::OIT];
#pragma unroll
  for (int j = 0; j < F::OIT; ++j) {
    const int i = min(tid + j * F::kT, F::OV16 - 1);
    const int px = i / 24, u = i - px * 24;
    oloff[j] = (uint32_t)(px * F::OROW + u * 16);
  }
  auto o_read = [&](auto jt) __attribute__((always_inline)) {
    constexpr int j = decltype(jt)::value;
    oc_at(jt) = *reinterpret_cast<const uint4*>(otile + oloff[j]);
  };
  auto o_write = [&](auto jt) __attribute__((always_inline)) {
    constexpr int j = decltype(jt)::value;
    const int i = min(tid + j * F::kT, F::OV16 - 1);
    // (first frame: O holds nothing yet -- the bytes go to frame n's own rows, which its real tile overwrites later from
    // the same thread; no branch in conv1's instruction stream)
    uint8_t* ob = out + (size_t)(prev >= 0 ? prev : n) * (81 * 384);  // (uniform base + 32-bit offset)
    *reinterpret_cast<uint4*>(ob + (size_t)(uint32_t)(i * 16)) = oc_at(jt);
  };
  // conv1's per-tile offsets (frame-invariant): tile rt of this wave -> its pixels' cells in T1 and records in T2
  uint32_t c1src[13], c1dst[13];
#pragma unroll
  for (int t = 0; t < 13; ++t) {
    const int rt = min(rg1 + 2 * t, 24);
    const int m = rt * 16 + li;
    const int oy = m / 20, ox = m - oy * 20;
    c1src[t] = (uint32_t)(g * F::PLANE1 + (oy * F::GW + ox) * 16);
    c1dst[t] = (uint32_t)((oy * F::RQ + ox * F::Q) * 16 + ch1 * 2);
  }
  const uint32_t a1lane = (uint32_t)((li * 32 + ch1) * 4);

  // ---- conv1 over this wave's tiles [T0, T0 + NT): T1 -> split3 records in T2
  auto conv1_pass = [&](auto t0_tag, auto nt_tag, auto&& hook) {
    constexpr int T0 = decltype(t0_tag)::value, NT = decltype(nt_tag)::value;
    i32x4 s_hi[NT], s_mid[NT], s_lo[NT];
    int a1base[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s_hi[t] = s_mid[t] = s_lo[t] = i32x4{0, 0, 0, 0};
      a1base[t] = (int)c1src[T0 + t];
    }
    constexpr int TOT = 4 * NT, D = 4;
    uint4 x[D];
    auto a_issue = [&](auto idx_tag, int slot) {
      constexpr int IDX = decltype(idx_tag)::value, KS = IDX / NT, T = IDX - KS * NT;
      x[slot] = *reinterpret_cast<const uint4*>(t1 + a1base[T] + ((KS >> 1) * F::GW + (KS & 1)) * 16);
    };
    static_for<D>([&](auto i) { a_issue(i, decltype(i)::value); });
    __builtin_amdgcn_sched_barrier(0);
    static_for<TOT>([&](auto it) {
      constexpr int IDX = decltype(it)::value, KS = IDX / NT, T = IDX - KS * NT, SLOT = IDX % D;
      const i32x4 xv = __builtin_bit_cast(i32x4, x[SLOT]);
      if constexpr (!kNoConv1) {
        s_hi[T] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd[KS][0], xv, s_hi[T], 0, 0, 0);
        s_mid[T] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd[KS][1], xv, s_mid[T], 0, 0, 0);
        s_lo[T] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd[KS][2], xv, s_lo[T], 0, 0, 0);
      } else {
        asm volatile("" ::"v"(xv));
      }
      if constexpr (IDX + D < TOT) a_issue(IC<IDX + D>{}, SLOT);
      hook(IC<T0 * 4 + IDX>{});
      __builtin_amdgcn_sched_barrier(0);
    });
    // every sum of the pass stays in its own accumulator registers until the pass's last MFMA has issued: no MFMA is
    // followed by a read of its own result (the compiler otherwise sends each final MFMA through ONE register tuple and
    // waits out its latency 3 NT times)
#pragma unroll
    for (int t = 0; t < NT; ++t) asm volatile("" : "+a"(s_hi[t]), "+a"(s_mid[t]), "+a"(s_lo[t]));
#pragma unroll
    for (int t = 0; t < (kNoEpi1 ? 0 : NT); ++t) {
      // (the odd group's thirteenth tile is tile 24 again: the same values to the same addresses as the even group's)
      const int rt = min(rg1 + 2 * (T0 + t), 24);
      // the exact integer sum S_hi * 2^16 + S_mid * 2^8 + S_lo enters f32 in two halves (|S_mid * 256 + S_lo| < 2^31; the
      // product with 65536 is exact, so the fused form rounds once where mul + add rounded once too), then ONE rounding
      // for scale and bias (fused: the file is compiled -ffp-contract=off, so the fusion is spelled out)
      const i32x4 ml = s_mid[t] * 256 + s_lo[t];
      const f32x4 hf = __builtin_convertvector(s_hi[t], f32x4), lf = __builtin_convertvector(ml, f32x4);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float u = __builtin_fmaf(hf[r], 65536.0f, lf[r]);
        const float y = __builtin_fmaf(u, sc1[r], bv1[r]);
        v[r] = y > 0.f ? y : 0.f;
      }
      uint2 p0, p1, p2;
      split3_4(v, p0, p1, p2);
      uint8_t* rec = t2 + c1dst[T0 + t];
      *reinterpret_cast<uint2*>(rec) = p0;
      *reinterpret_cast<uint2*>(rec + 64) = p1;
      *reinterpret_cast<uint2*>(rec + 128) = p2;
      if constexpr (A1OUT) {  // the learner's copy: f32 channel-last
        // uniform base (frame and tile) + this lane's pixel and channels
        uint8_t* ab = reinterpret_cast<uint8_t*>(a1_out + ((size_t)n * 400 + rt * 16) * 32);
        *reinterpret_cast<f32x4*>(ab + (size_t)a1lane) = v;
      }
    }
  };

  // first frame into T1
#pragma unroll
  for (int j = 0; j < F::UIT; ++j) g_load4(n, j);
#pragma unroll
  for (int j = 0; j < F::UIT; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) s_store4(j, k);
  if constexpr (COPY != 0) {
    uint8_t* cb = copy_row(n);
#pragma unroll
    for (int j = 0; j < F::UIT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) g_copy4(cb, j, r);
  }
  __syncthreads();

  auto copy_hook = [&](auto idx_tag) {
    constexpr int IDX = decltype(idx_tag)::value;
    // copy-out slots: read chunk j from O behind conv1's item 2 j, store it behind item 2 j + 1 (first pass: 20 items)
    // (measured r5, same box: chunks spaced six items apart instead of one 302 us against 303; a conv1 ring of 8 instead of
    // 4 items 315)
    if constexpr (!kNoCopyOut && IDX < 2 * F::OIT) {
      if constexpr (IDX % 2 == 0) o_read(IC<IDX / 2>{});
      else o_write(IC<IDX / 2>{});
    }
  };
  // (conv1's second and third pass: nothing, but for) COPY == 2: the pass-through frame's pieces 0 .. 3 are loaded behind conv1's items 20, 28, 36 and 44 (second and third
  // pass; the first holds the copy-out), stored behind conv2's items 4, 8, 12 and 16; pieces 4 .. 7 are loaded behind
  // conv2's items 6, 10, 15 and 18 and stored behind 27, 31, 35 and 39, ahead of the staging's own stores (40 ..)
  auto pass_hook = [&](auto idx_tag) {
    constexpr int IDX = decltype(idx_tag)::value;
    if constexpr (COPY == 2 && IDX >= 20 && (IDX - 20) % 8 == 0 && !kNoStage) pt_load(IC<(IDX - 20) / 8>{});
  };
  constexpr int kPtStore[8] = {4, 8, 12, 16, 27, 31, 35, 39}, kPtLoad[8] = {-1, -1, -1, -1, 6, 10, 15, 18};
  static_assert(2 * F::OIT <= 20, "copy-out slots inside conv1's first pass");

  uint32_t xbh[F::C2TILES];  // conv2's per-tile offsets into the a1 image (frame-invariant)
#pragma unroll
  for (int t = 0; t < F::C2TILES; ++t) {
    const int m = t * 16 + li;
    const int oy = m / 9, ox = m - oy * 9;
    xbh[t] = (uint32_t)((2 * oy * F::RQ + 2 * ox * F::Q + g) * 16);
  }
  uint32_t o2dst[F::C2TILES];  // ... and into O
#pragma unroll
  for (int t = 0; t < F::C2TILES; ++t) o2dst[t] = (uint32_t)(F::T1_BYTES + F::T2_BYTES + (t * 16 + li) * F::OROW + ch2 * 2);
  // pixel 80's patch: thread t < 192 moves unit t % 12 of record t / 12 (tap order) from T2 into the ring (frame-invariant;
  // the fourth wave repeats thread 191's unit: the same bytes to the same place, no branch)
  uint32_t psrc, pdst;
  {
    const int t = min(tid, F::PATCH_UNITS - 1);
    const int r = t / 12, u = t - r * 12;
    psrc = (uint32_t)(((16 + (r >> 2)) * F::RQ + (16 + (r & 3)) * F::Q + u) * 16);
    pdst = (uint32_t)(F::RING + t * 16);
  }
  // ---- pixel 80 of the frames first, first + nblk, ... whose patches fill the ring's slots 0 .. cnt - 1: one conv2 tile,
  // the same k-steps, the same six products into the same acc / accs as any other pixel; a lane past cnt takes the last
  // slot and repeats its store.  The results go straight to HBM (part p of an a2 record at + 128 p).
  auto pixel80_tile = [&](int cnt, int first) {
    constexpr int D = 3;
    const int sl = min(li, cnt - 1);
    const uint8_t* rp = smem_c12 + F::RING + sl * F::SLOT_BYTES + g * 16;
    uint4 xr[D][3];
    auto a_issue = [&](auto ks_tag, int slot) {
      constexpr int KS = decltype(ks_tag)::value;
      const uint8_t* ap = rp + F::tap2(KS) * 192;
      xr[slot][0] = *reinterpret_cast<const uint4*>(ap);
      xr[slot][1] = *reinterpret_cast<const uint4*>(ap + 64);
      xr[slot][2] = *reinterpret_cast<const uint4*>(ap + 128);
    };
    static_for<D>([&](auto i) { a_issue(i, decltype(i)::value); });
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc = bv2, accs = {0.f, 0.f, 0.f, 0.f};
    static_for<F::KS2>([&](auto it) {
      constexpr int KS = decltype(it)::value, SLOT = KS % D;
      const bf16x8 x0 = __builtin_bit_cast(bf16x8, xr[SLOT][0]), x1 = __builtin_bit_cast(bf16x8, xr[SLOT][1]),
                   x2 = __builtin_bit_cast(bf16x8, xr[SLOT][2]);
      if constexpr (!kNoConv2) {
        accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][2], x0, accs, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][0], x2, accs, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][1], x1, accs, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][1], x0, accs, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][0], x1, accs, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][0], x0, acc, 0, 0, 0);
      } else {
        asm volatile("" ::"v"(x0), "v"(x1), "v"(x2));
      }
      if constexpr (KS + D < F::KS2) a_issue(IC<KS + D>{}, SLOT);
      __builtin_amdgcn_sched_barrier(0);
    });
    if constexpr (kNoEpi2) {
      asm volatile("" ::"v"(acc), "v"(accs));
    } else {
      f32x4 v = acc + accs;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
      uint2 p0, p1, p2;
      split3_4(v, p0, p1, p2);
      uint8_t* rec = out + (size_t)(first + sl * nblk) * (81 * 384) + (F::C2PIX * 384 + ch2 * 2);
      *reinterpret_cast<uint2*>(rec) = p0;
      *reinterpret_cast<uint2*>(rec + 128) = p1;
      *reinterpret_cast<uint2*>(rec + 256) = p2;
    }
  };
  int filled = 0;  // the ring's slots in use (uniform)
  for (; n < N; n += nblk) {
    const int nn = (n + nblk < N) ? n + nblk : n;  // (the last round re-stages its own frame)
    // (COPY: ... and stores it again, the same bytes to the same row; no branch inside conv2's instruction stream)
    uint8_t* cbn = nullptr;
    if constexpr (COPY != 0) cbn = copy_row(nn);
    if constexpr (COPY == 2) {
      int sl = copy2_first + n;
      if (sl >= copy_ring) sl -= copy_ring;
      cb2 = copy2_dst + (size_t)sl * F::IN_ELEMS;
    }
    pin_weights();
    conv1_pass(IC<0>{}, IC<5>{}, copy_hook);
    conv1_pass(IC<5>{}, IC<4>{}, pass_hook);
    conv1_pass(IC<9>{}, IC<4>{}, pass_hook);
    if constexpr (kNoEpi1) asm volatile("" ::"v"(sc1), "v"(bv1));
    __syncthreads();  // T2 complete, T1 and O free
    // ---- conv2 from T2, tile by tile; the next frame's cells go into T1 in the second half
    {
      constexpr int TOT = F::C2TILES * F::KS2, D = 3;
      // pixel 80's patch -> slot `filled` of the ring: read here, written behind item 2
      const uint4 patch = *reinterpret_cast<const uint4*>(t2 + psrc);
      uint4 xr[D][3];
      auto a_issue = [&](auto idx_tag, int slot) {
        constexpr int IDX = decltype(idx_tag)::value, T = IDX / F::KS2, KS = IDX - T * F::KS2;
        const uint8_t* ap = t2 + xbh[T] + F::koff2(KS);
        xr[slot][0] = *reinterpret_cast<const uint4*>(ap);
        xr[slot][1] = *reinterpret_cast<const uint4*>(ap + 64);
        xr[slot][2] = *reinterpret_cast<const uint4*>(ap + 128);
      };
      static_for<D>([&](auto i) { a_issue(i, decltype(i)::value); });
      __builtin_amdgcn_sched_barrier(0);
      f32x4 acc = bv2, accs = {0.f, 0.f, 0.f, 0.f};
      static_for<TOT>([&](auto it) {
        constexpr int IDX = decltype(it)::value, T = IDX / F::KS2, KS = IDX - T * F::KS2, SLOT = IDX % D;
        const bf16x8 x0 = __builtin_bit_cast(bf16x8, xr[SLOT][0]), x1 = __builtin_bit_cast(bf16x8, xr[SLOT][1]),
                     x2 = __builtin_bit_cast(bf16x8, xr[SLOT][2]);
        if constexpr (!kNoConv2) {
          accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][2], x0, accs, 0, 0, 0);
          accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][0], x2, accs, 0, 0, 0);
          accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][1], x1, accs, 0, 0, 0);
          accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][1], x0, accs, 0, 0, 0);
          accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][0], x1, accs, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[KS][0], x0, acc, 0, 0, 0);
        } else {
          asm volatile("" ::"v"(x0), "v"(x1), "v"(x2));
        }
        if constexpr (IDX + D < TOT) a_issue(IC<IDX + D>{}, SLOT);
        if constexpr (IDX == 2) *reinterpret_cast<uint4*>(smem_c12 + pdst + filled * F::SLOT_BYTES) = patch;
        // the next frame's two units: loaded behind items 1 and 13, their eight cells stored (sign bits flipped) behind
        // items 40, 44, ..., 68 (COPY: one of the unit's four rows goes to the destination row with each cell, so the
        // staged registers live exactly as long as before)
        static_for<4 * F::UIT>([&](auto jj) {
          constexpr int JJ = decltype(jj)::value;
          if constexpr (JJ < F::UIT && IDX == 1 + 12 * JJ && !kNoStage) g_load4(nn, JJ);
          if constexpr (IDX == TOT / 2 + 4 * JJ && !kNoStage) s_store4(JJ >> 2, JJ & 3);
          if constexpr (COPY != 0 && IDX == TOT / 2 + 4 * JJ && !kNoStage) g_copy4(cbn, JJ >> 2, JJ & 3);
          if constexpr (COPY == 2 && IDX == kPtStore[JJ] && !kNoStage) pt_store(IC<JJ>{});
          if constexpr (COPY == 2 && IDX == kPtLoad[JJ] && !kNoStage) pt_load(IC<JJ>{});
        });
        if constexpr (KS == F::KS2 - 1 && kNoEpi2) asm volatile("" ::"v"(acc), "v"(accs));
        if constexpr (KS == F::KS2 - 1 && !kNoEpi2) {  // tile T complete: ReLU, split, its record slice into O
          f32x4 v = acc + accs;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
          uint2 p0, p1, p2;
          split3_4(v, p0, p1, p2);
          uint8_t* rec = smem_c12 + o2dst[T];
          *reinterpret_cast<uint2*>(rec) = p0;
          *reinterpret_cast<uint2*>(rec + 128) = p1;
          *reinterpret_cast<uint2*>(rec + 256) = p2;
          acc = bv2, accs = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    __syncthreads();  // O complete, T1 ready, T2 free, the ring's slot written
    prev = n;
    // the ring is full, or this was the block's last frame: its pixels 80 now (uniform branch).  The next write into the
    // ring comes behind the next frame's first barrier, which every wave reaches only after this tile: no barrier here.
    if (++filled == F::RING_S || n + nblk >= N) {
      pixel80_tile(filled, n - (filled - 1) * nblk);
      filled = 0;
    }
  }
  {  // the last frame's output tile
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)prev * (81 * 384));
    for (int i = tid; i < F::OV16; i += F::kT) {
      const int px = i / 24, u = i - px * 24;
      dst[i] = *reinterpret_cast<const uint4*>(otile + px * F::OROW + u * 16);
    }
  }
}

template <bool A1OUT>
__global__ __launch_bounds__(256, 1) void conv12_s3(const uint8_t* __restrict__ in, const uint4* __restrict__ W1d,
                                                    const float* __restrict__ scale1, const float* __restrict__ bias1q,
                                                    const uint4* __restrict__ B2, const float* __restrict__ bias2,
                                                    uint8_t* __restrict__ out, float* __restrict__ a1_out, int N) {
  conv12_s3_body<A1OUT, 0>(in, W1d, scale1, bias1q, B2, bias2, out, a1_out, N, nullptr, 0, 0, nullptr, nullptr, 0);
}
// conv12_s3<false> that also stores frame fr to row (copy_first + fr) mod copy_ring of copy_dst (N <= copy_ring)
__global__ __launch_bounds__(256, 1) void conv12_s3_copy(const uint8_t* __restrict__ in, const uint4* __restrict__ W1d,
                                                         const float* __restrict__ scale1, const float* __restrict__ bias1q,
                                                         const uint4* __restrict__ B2, const float* __restrict__ bias2,
                                                         uint8_t* __restrict__ out, int N, uint8_t* __restrict__ copy_dst,
                                                         int copy_first, int copy_ring) {
  conv12_s3_body<false, 1>(in, W1d, scale1, bias1q, B2, bias2, out, nullptr, N, copy_dst, copy_first, copy_ring, nullptr, nullptr,
                           0);
}
// ... and frame fr of in2 to row (copy2_first + fr) mod copy_ring of copy2_dst (the two destinations do not overlap).
// Label and census name: conv12_s3_copy2.  The symbol is spelled conv12_s3_copies2 so that "conv12_s3_copy" keeps naming
// exactly one kernel of this file (tests/test_conv12_copy_resources_cpu.py and tools/trace_insert_tail.py find it so).
__global__ __launch_bounds__(256, 1) void conv12_s3_copies2(const uint8_t* __restrict__ in, const uint4* __restrict__ W1d,
                                                            const float* __restrict__ scale1, const float* __restrict__ bias1q,
                                                            const uint4* __restrict__ B2, const float* __restrict__ bias2,
                                                            uint8_t* __restrict__ out, int N, uint8_t* __restrict__ copy_dst,
                                                            int copy_first, int copy_ring, const uint8_t* __restrict__ in2,
                                                            uint8_t* __restrict__ copy2_dst, int copy2_first) {
  conv12_s3_body<false, 2>(in, W1d, scale1, bias1q, B2, bias2, out, nullptr, N, copy_dst, copy_first, copy_ring, in2, copy2_dst,
                           copy2_first);
}

// frames u8 [N][4][84][84] -> a2 as split3 records at rec2; a1 != NULL: a1 as channel-last f32 too (A1OUT)
inline void launch_conv12(const uint8_t* frames, const uint4* W1d, const float* s1q, const float* b1q, const uint4* B2e,
                          const float* b2, uint8_t* rec2, float* a1, int N, hipStream_t s, int blocks) {
  const auto kernel = a1 ? conv12_s3<true> : conv12_s3<false>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(Conv12S::kT), Conv12S::LDS_TOTAL, s, frames, W1d, s1q, b1q, B2e, b2, rec2, a1, N);
}
// ... and every frame to its row of the ring of frame rows at copy_dst (0 <= copy_first < copy_ring, N <= copy_ring)
inline void launch_conv12_copy(const uint8_t* frames, const uint4* W1d, const float* s1q, const float* b1q, const uint4* B2e,
                               const float* b2, uint8_t* rec2, int N, hipStream_t s, int blocks, uint8_t* copy_dst,
                               int copy_first, int copy_ring) {
  hipLaunchKernelGGL(conv12_s3_copy, dim3(blocks), dim3(Conv12S::kT), Conv12S::LDS_TOTAL, s, frames, W1d, s1q, b1q, B2e, b2, rec2,
                     N, copy_dst, copy_first, copy_ring);
}
// ... and the N frames at frames2 to their rows of the ring at copy2_dst (0 <= copy2_first < copy_ring, the same length)
inline void launch_conv12_copy2(const uint8_t* frames, const uint4* W1d, const float* s1q, const float* b1q, const uint4* B2e,
                                const float* b2, uint8_t* rec2, int N, hipStream_t s, int blocks, uint8_t* copy_dst,
                                int copy_first, int copy_ring, const uint8_t* frames2, uint8_t* copy2_dst, int copy2_first) {
  hipLaunchKernelGGL(conv12_s3_copies2, dim3(blocks), dim3(Conv12S::kT), Conv12S::LDS_TOTAL, s, frames, W1d, s1q, b1q, B2e, b2, rec2,
                     N, copy_dst, copy_first, copy_ring, frames2, copy2_dst, copy2_first);
}
// the four kernels' opt-in to their dynamic LDS (once per process, before the first launch)
inline int opt_in_lds_conv12() {
  for (const void* k : {reinterpret_cast<const void*>(&conv12_s3<false>), reinterpret_cast<const void*>(&conv12_s3<true>),
                        reinterpret_cast<const void*>(&conv12_s3_copy), reinterpret_cast<const void*>(&conv12_s3_copies2)})
    RELA_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, Conv12S::LDS_TOTAL));
  return RELA_OK;
}

}  // namespace s3
}  // namespace rela_amd
