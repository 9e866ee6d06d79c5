// ffnet.hip -- the host side of the AtariFFNet (pyrela/net.py:8-55) and AtariLSTMNet (net.py:58-163) forwards: the
// weight-layout table, create / load, the two nets' forwards with their debug taps, and the learners' entry points.
// This is the forward's one translation unit; its device code is in headers, one kernel family each, with a launcher per
// kernel that takes plain pointers.  A forward runs in one of three arithmetics (ffnet_plan.h decides which kernels):
//   exact f32    conv_f32.h (conv1_bf16x3, conv_mfma), gemm_f32.h (gemm_mfma: fc, LSTM gates + cell, the LSTM net's
//                heads; dueling_kernel; the small-batch fc through gemm_lds.h; fc_reduce, which every split-K fc ends in)
//   split-bf16   conv12_i8.h (conv1 on the int8 matrix cores -> conv2, per pass or as the learners' jobs), conv_bf16s.h
//                (the split records, conv3), fc_bf16s.h (fc, whole or split-K), gemm_bf16s.h (the LSTM gates' x part)
//   f32x3        conv12_s3.h, conv_img_s3.h, gemm_s3.h (fc, the gates' x part)
// and every AtariFFNet forward ends in heads_duel.h.  ffnet_kern.h holds what the families share.
// Besides the C ABI (include/rela_amd.h) this file defines the internal entry points that ffnet_layout.h declares: the
// ffnet_* ones for learner.hip (Ape-X), the lstmnet_*, gate_x3 and trunk_unsplit_rows ones for learner_r2d2.hip.
#include "common.h"
#include "gemm_bf16s.h"
#include "gemm_f32emu.h"
#include "gemm_s3.h"
#include "conv_img_s3.h"
#include "conv12_s3.h"
#include "ffnet_layout.h"
#include "ffnet_plan.h"
#include "conv_f32.h"
#include "gemm_f32.h"
#include "conv12_i8.h"
#include "fc_bf16s.h"
#include "heads_duel.h"
#include "param_layout.h"
#include "prof.h"
#define RELA_WEIGHT_PACK_KERNEL  // this translation unit holds the library's one pack kernel
#include "weight_pack.h"

namespace rela_amd {

struct FFNetDev {
  uint4* B1 = nullptr;                 // conv1 bf16 frags [piece 3][ct 2][ks 8][lane 64] x 8 bf16
  float* b1 = nullptr;                 // conv1 bias[32]
  float *B2 = nullptr, *b2 = nullptr;  // conv2 frags [4][128][64], bias[64]
  float *B3 = nullptr, *b3 = nullptr;  // conv3 frags [4][144][64], bias[64]
  float *Bf = nullptr, *bf = nullptr;  // fc    frags [32][784][64], bias[512]
  float* BfT = nullptr;                // fc    weights [3136 (k = pos*64+c)][512] for the small-batch split-K path
  float *Bh = nullptr, *bh = nullptr;  // heads frags [2][128][64], bias[32]  (cols 0..A-1 = fc_a, col 31 = fc_v)
  // split-bf16 fast path: [ct][ks][hi, lo][lane] x 8 bf16 (conv_bf16s.h)
  uint4 *B2f = nullptr, *B3f = nullptr, *Bff = nullptr;
  float* Bhp = nullptr;  // heads weights [ct 2][wave 4][j 32][lane 64] in the k order of heads_duel
  // conv1 for the int8 matrix cores (conv12_i8): digits [hi, mid, lo][ct 2][tap 4][lane 64] x 16 int8, then (the same
  // layout, s1q and b1q point into it) the channels' scales s_c and the biases b_c + 128 s_c sum_k q_k
  uint4* W1d = nullptr;
  float *s1q = nullptr, *b1q = nullptr;
  // f32-accurate mode on the bf16 matrix cores (gemm_f32emu.h): bf16 triples in fragment order [cg][ks][u][part][lane]
  uint4 *B2e = nullptr, *B3e = nullptr, *Bfe = nullptr;
  // AtariLSTMNet only
  float* Bl = nullptr;      // lstm frags [128][912][64]
  float* bl = nullptr;      // b_ih + b_hh, permuted [2048]
  uint8_t* Wrec = nullptr;  // weight_ih_l0 as rec64 rows in the permuted column order [2048][49][64 hi | 64 lo]
  uint4* Wx3 = nullptr;     // ... as three-part bf16 fragments in the same column order (gemm_s3.h; f32x3 mode)
};

// what rela_ffnet and rela_lstmnet both are
struct NetBase {
  int device = 0;
  int num_action = 0;
  FFNetDev d;      // the net's rows of the layout table ...
  DevBuffers mem;  // ... which it owns
  bool loaded = false;
  uint64_t version = 0;  // bumped by every load
  int precision = 0;     // 0 = exact f32 | 1 = split-bf16 | 2 = f32x3; what each net runs in them: at its struct
};

}  // namespace rela_amd

using namespace rela_amd;

namespace {
const char* const kProfActor[6] = {"conv1_bf16x3", "conv2_mfma", "conv3_mfma", "fc_mfma", "heads_mfma", "dueling"};
const char* const kProfLearner[6] = {"learner_fwd_conv1", "learner_fwd_conv2", "learner_fwd_conv3",
                                     "learner_fwd_fc",    "learner_fwd_heads", "learner_fwd_dueling"};

// ---- launch helpers shared by the AtariFFNet, the AtariLSTMNet and the learners' entry points -------------------------

// the split-K fcs' partial tiles: behind ha, 256-byte aligned within the workspace (float4 loads)
inline float* fc_part_ptr(const void* ws, float* ha, int N) {
  float* part = ha + kHA * N;
  return part + ((64 - ((part - static_cast<const float*>(ws)) & 63)) & 63);
}

// a2 / a3 of an f32x3 trunk that keeps f32 (TrunkOpts::keep_f32): split3 records -> channel-last f32
void unsplit_s3_a23(const uint8_t* rec2, const uint8_t* rec3, float* a2, float* a3, int N, hipStream_t s) {
  note_launch("unsplit_s3");
  const int64_t p2 = (int64_t)N * 81, p3 = (int64_t)N * 49;
  hipLaunchKernelGGL(s3::unsplit_s3<64>, dim3((unsigned)ceil_div(p2 * 16, 256)), dim3(256), 0, s, rec2, a2, p2);
  hipLaunchKernelGGL(s3::unsplit_s3<64>, dim3((unsigned)ceil_div(p3 * 16, 256)), dim3(256), 0, s, rec3, a3, p3);
}

template <class... Rest>  // a TrunkJob with the weights of `d`
TrunkJob trunk_job_of(const FFNetDev& d, Rest... rest) { return rela_amd::trunk_job(d.W1d, d.s1q, d.b1q, d.B2f, d.b2, d.B3f, d.b3, rest...); }
inline uint8_t* recs(float* p) { return reinterpret_cast<uint8_t*>(p); }  // a tensor's place, holding split records

// ---- the conv trunk: frames u8[N][4][84][84] -> a1 / a2 / a3, in one of three arithmetics (TrunkKind, ffnet_plan.h) ----
struct TrunkLabels {  // per-kernel timing labels (prof.h); conv12: the launch that runs conv1 -> conv2 fused
  const char *conv1, *conv2, *conv3, *conv12;
};
struct TrunkOpts {
  bool keep_f32 = false;          // kTrunkS3: a1 is ALSO written as channel-last f32 (a2 / a3: unsplit_s3_a23, the caller's)
  bool leave_a3_records = false;  // kTrunkBf16: a3 stays in split records instead of going back to f32 in place
  // kTrunkS3 without keep_f32: the frames also go to these rows (conv12_s3_copy; with a second pair, conv12_s3_copy2)
  const FrameRows* store_frames = nullptr;
};
// kTrunkF32:  a1 / a2 / a3 channel-last f32
// kTrunkBf16: a1 is NOT produced; a2 / a3 hold split-bf16 records in the f32 tensors' places (same bytes)
// kTrunkS3:   a2 / a3 as split3 records at rec2 [N][kRec2Bytes] / rec3 [N][kRec3Bytes]; a1 / a2 / a3 themselves are
//             untouched unless keep_f32
void launch_trunk(const FFNetDev& d, TrunkKind kind, int N, const uint8_t* s_dev, float* a1, float* a2, float* a3,
                  uint8_t* rec2, uint8_t* rec3, const TrunkOpts& o, const TrunkLabels& l, hipStream_t s) {
  switch (kind) {
    case kTrunkS3: {
      {
        ProfScope prof(l.conv12, s);
        note_launch("conv12_s3");
        if (o.store_frames && o.store_frames->src2) {
          note_launch("conv12_s3_copy2");  // (counted under both names: it is a conv12_s3 launch that also copies two fields)
          s3::launch_conv12_copy2(s_dev, d.W1d, d.s1q, d.b1q, d.B2e, d.b2, rec2, N, s, persistent_blocks(N), o.store_frames->base,
                                  o.store_frames->first, o.store_frames->ring, o.store_frames->src2, o.store_frames->base2,
                                  o.store_frames->first2);
        } else if (o.store_frames) {
          note_launch("conv12_s3_copy");  // (counted under both names: it is a conv12_s3 launch that also copies)
          s3::launch_conv12_copy(s_dev, d.W1d, d.s1q, d.b1q, d.B2e, d.b2, rec2, N, s, persistent_blocks(N), o.store_frames->base,
                                 o.store_frames->first, o.store_frames->ring);
        } else {
          s3::launch_conv12(s_dev, d.W1d, d.s1q, d.b1q, d.B2e, d.b2, rec2, o.keep_f32 ? a1 : nullptr, N, s, persistent_blocks(N));
        }
      }
      ProfScope prof(l.conv3, s);
      note_launch("conv3_img_s3");
      s3::launch_conv3_img(rec2, d.B3e, d.b3, rec3, N, s, persistent_blocks(N));
      break;
    }
    case kTrunkBf16: {
      {
        ProfScope prof(l.conv12, s);
        launch_conv12_i8(s_dev, d.W1d, d.s1q, d.b1q, d.B2f, d.b2, recs(a2), N, s);
      }
      ProfScope prof(l.conv3, s);
      launch_conv3_bf16s(recs(a2), d.B3f, d.b3, recs(a3), N, s);
      if (!o.leave_a3_records) launch_unsplit_records64(recs(a3), (int64_t)N * 49, s);
      break;
    }
    case kTrunkF32: {
      {
        ProfScope prof(l.conv1, s);
        launch_conv1_bf16x3(s_dev, d.B1, d.b1, a1, N, s);
      }
      {
        ProfScope prof(l.conv2, s);
        launch_conv<Conv2>(a1, d.B2, d.b2, a2, N, s);
      }
      ProfScope prof(l.conv3, s);
      launch_conv<Conv3>(a2, d.B3, d.b3, a3, N, s);
      break;
    }
  }
}

// ---- create / load helpers ---------------------------------------------------------------------------------------------

// THE LAYOUT TABLE: one row per kernel-layout weight copy, in the order of `Layout` (ffnet_plan.h).  A layout is
// `elements` units of `unit` bytes -- one unit per thread of its pack body (weight_pack.h) -- plus `tail` bytes, and is
// packed by a segment of `kind` from the parameters s0 and s1 with the integers a0 and a1.  create allocates it and points
// FFNetDev's field at it, a load makes the segment, rela_*_debug_layout reports the row: no size is written anywhere else.
// Parameters are indices of the load's tensors in state_dict order (conv1_w 0 .. conv3_b 5, then the net's own); both
// nets end in fc_v.weight, fc_v.bias, fc_a.weight, fc_a.bias, which the table counts from the end.
enum { kVw = -4, kVb = -3, kAw = -2, kAb = -1, kNoSrc = 99, kNumAction = -1 /* a0: the net's num_action */ };
struct LayoutRow {
  const char* name;
  size_t field;  // offsetof(FFNetDev, the pointer)
  int64_t elements;
  int unit, tail, kind, s0, s1, a0, a1;
  int64_t bytes() const { return elements * unit + tail; }
};
template <class P>
constexpr int64_t emu_triples() { return f32emu::packed_u4<P>() * 8 / 3; }  // bf16 triples of a gemm_f32emu.h layout
#define RELA_LAYOUT(field, elements, unit, tail, ...) {#field, offsetof(FFNetDev, field), (int64_t)(elements), unit, tail, __VA_ARGS__}
const LayoutRow kLayouts[kLayCount] = {
    RELA_LAYOUT(B1, 2 * 8 * 64 * 8, 6, 0, kPackConv1x3, 0, kNoSrc, 0, 0),  // a thread: one bf16 of each of the three planes
    RELA_LAYOUT(b1, 32, 4, 0, kPackCopy, 1, kNoSrc, 0, 0),
    RELA_LAYOUT(B2, 4 * 128 * 64, 4, 0, kPackFragsConv2, 2, kNoSrc, 4, 128),
    RELA_LAYOUT(b2, 64, 4, 0, kPackCopy, 3, kNoSrc, 0, 0),
    RELA_LAYOUT(B3, 4 * 144 * 64, 4, 0, kPackFragsConv3, 4, kNoSrc, 4, 144),
    RELA_LAYOUT(b3, 64, 4, 0, kPackCopy, 5, kNoSrc, 0, 0),
    RELA_LAYOUT(Bh, kHeadsCT * kHeadsKS * 64, 4, 0, kPackFragsHeads, kAw, kVw, kNumAction, 0),
    RELA_LAYOUT(bh, 32, 4, 0, kPackHeadBias, kAb, kVb, kNumAction, 0),
    RELA_LAYOUT(W1d, kConv1I8Weights, 3, 2 * 32 * 4, kPackConv1I8, 0, 1, 0, 0),  // three int8 digits; tail: s1q [32] | b1q [32]
    RELA_LAYOUT(B2f, Conv2F::CT * Conv2F::KS * 64 * 8, 4, 0, kPackBf16sConv2, 2, kNoSrc, Conv2F::CT, Conv2F::KS),  // a hi and a lo bf16
    RELA_LAYOUT(B3f, Conv3F::CT * Conv3F::KS * 64 * 8, 4, 0, kPackBf16sConv3, 4, kNoSrc, Conv3F::CT, Conv3F::KS),
    RELA_LAYOUT(B2e, emu_triples<f32emu::ProbConv2>(), 6, 0, kPackEmuConv2, 2, kNoSrc, f32emu::ProbConv2::NCG, f32emu::ProbConv2::KS),
    RELA_LAYOUT(B3e, emu_triples<f32emu::ProbConv3>(), 6, 0, kPackEmuConv3, 4, kNoSrc, f32emu::ProbConv3::NCG, f32emu::ProbConv3::KS),
    // AtariFFNet: linear.0.weight 6, linear.0.bias 7
    RELA_LAYOUT(Bf, 32 * 784 * 64, 4, 0, kPackFragsFc, 6, kNoSrc, 32, 784),
    RELA_LAYOUT(BfT, 3136 * 512, 4, 0, kPackFcT, 6, kNoSrc, 0, 0),
    RELA_LAYOUT(bf, 512, 4, 0, kPackCopy, 7, kNoSrc, 0, 0),
    RELA_LAYOUT(Bhp, 2 * 4 * 32 * 64, 4, 0, kPackHeadsPerm, kAw, kVw, kNumAction, 0),
    RELA_LAYOUT(Bff, 32 * FcFast::KS * 64 * 8, 4, 0, kPackBf16sFc, 6, kNoSrc, 32, FcFast::KS),
    RELA_LAYOUT(Bfe, emu_triples<f32emu::ProbFc>(), 6, 0, kPackEmuFc, 6, kNoSrc, f32emu::ProbFc::NCG, f32emu::ProbFc::KS),
    // AtariLSTMNet: weight_ih_l0 6, weight_hh_l0 7, bias_ih_l0 8, bias_hh_l0 9
    RELA_LAYOUT(Bl, (int64_t)GemmLstm::CT * GemmLstm::KS * 64, 4, 0, kPackFragsLstm, 6, 7, GemmLstm::CT, GemmLstm::KS),
    RELA_LAYOUT(bl, 2048, 4, 0, kPackLstmBias, 8, 9, 0, 0),
    RELA_LAYOUT(Wrec, 2048 * 392, 32, 0, kPackWihRec64, 6, kNoSrc, 0, 0),  // 8 channels of a rec64 row: 16 B of hi, 16 B of lo
    RELA_LAYOUT(Wx3, emu_triples<f32emu::ProbGateX>(), 6, 0, kPackEmuGatesPerm, 6, kNoSrc, f32emu::ProbGateX::NCG, f32emu::ProbGateX::KS),
};
#undef RELA_LAYOUT
static_assert(2 * 8 * 64 * 8 * 6 == sizeof(uint4) * Conv1B::FRAG_UINT4 && kConv1I8Weights * 3 == sizeof(uint4) * Conv12I::W1_UINT4,
              "the layout table and the conv1 kernels disagree about their fragments");
constexpr uint32_t kLstmNetLayouts = (lay_bit(kLayShared) - 1) | (lay_bit(kLayCount) - lay_bit(kLayBl));

void*& layout_ptr(FFNetDev& d, int layout) {
  return *reinterpret_cast<void**>(reinterpret_cast<uint8_t*>(&d) + kLayouts[layout].field);
}
// the rows in `set`, owned by `mem`
int alloc_layouts(FFNetDev& d, DevBuffers& mem, uint32_t set) {
  for (int l = 0; l < kLayCount; ++l) {
    uint8_t* p = nullptr;
    if (!(set & lay_bit(l))) continue;
    if (int rc = mem.alloc(&p, (size_t)kLayouts[l].bytes(), false)) return rc;
    layout_ptr(d, l) = p;
  }
  d.s1q = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(d.W1d) + kConv1I8Weights * 3);
  d.b1q = d.s1q + 32;
  return RELA_OK;
}

// ONE launch packs the layouts in `set` from the load's n tensors dv[] and, where `extra` has pointers, the learners'
// dgrad operand copies (ffnet_layout.h) of conv2 / conv3 / fc_w (NULL: the net has none)
int pack_layouts(FFNetDev& d, uint32_t set, const float* const* dv, int n, int A, const ExtraPacks& extra, const float* fc_w,
                 hipStream_t s) {
  PackList list;
  const auto src = [&](int i) { return i == kNoSrc ? nullptr : dv[i < 0 ? n + i : i]; };
  for (int l = 0; l < kLayCount; ++l) {
    const LayoutRow& r = kLayouts[l];
    if (set & lay_bit(l)) list.add(r.kind, src(r.s0), src(r.s1), layout_ptr(d, l), r.a0 == kNumAction ? A : r.a0, r.a1, r.elements);
  }
  float* const copy[3] = {extra.w2p, extra.w3p, fc_w ? extra.wfcp : nullptr};
  const float* const from[3] = {dv[2], dv[4], fc_w};
  for (int mode = 0; mode < 3; ++mode)
    if (copy[mode]) list.add(kPackPermute, from[mode], nullptr, copy[mode], mode, 0, kPermFloats[mode]);
  return launch_weight_pack(list, s);
}

// rela_*_debug_layout: one row of the table
int report_layout(FFNetDev& d, int layout, uint32_t packed_set, const char** name, int64_t* bytes, int* packed, void* host_dst) {
  const LayoutRow& row = kLayouts[layout];
  const bool is_packed = (packed_set & lay_bit(layout)) != 0;
  if (name) *name = row.name;
  if (bytes) *bytes = row.bytes();
  if (packed) *packed = is_packed;
  if (host_dst && is_packed) {
    RELA_HIP(hipDeviceSynchronize());
    RELA_HIP(hipMemcpy(host_dst, layout_ptr(d, layout), (size_t)row.bytes(), hipMemcpyDeviceToHost));
  }
  return RELA_OK;
}

// the trunk kernels' opt-in to > 64 KB of dynamic LDS, once per net: each family lists its own kernels (the stamps
// variants opt in where they are launched)
int opt_in_dynamic_lds() {
  for (int (*family)() : {opt_in_lds_conv12_i8, s3::opt_in_lds_conv12, opt_in_lds_conv_f32, opt_in_lds_conv_bf16s})
    if (int rc = family()) return rc;
  return RELA_OK;
}

// rela_*_create: a net with the rows `layouts` of the table, opted in to its kernels' dynamic LDS (own: the family only
// this net launches, or NULL); a failure frees what was allocated and the net.  rela_*_destroy: free_all.
template <class Net>
int create_net(Net** out, int num_action, int device, const char* who, uint32_t layouts, int (*own)()) {
  RELA_CHECK(out && num_action >= 1 && num_action <= 31, RELA_EINVAL, "%s: num_action must be in 1..31 (got %d)", who, num_action);
  if (int rc = check_device(device, who)) return rc;
  DeviceGuard g(device);
  auto* n = new Net();
  n->device = device;
  n->num_action = num_action;
  int rc = alloc_layouts(n->d, n->mem, layouts);
  if (rc == RELA_OK) rc = opt_in_dynamic_lds();
  if (rc == RELA_OK && own) rc = own();
  if (rc != RELA_OK) {
    n->mem.free_all();
    delete n;
    return rc;
  }
  *out = n;
  return RELA_OK;
}
template <class Net>
void destroy_net(Net* n) {
  if (!n) return;
  DeviceGuard g(n->device);
  (void)hipDeviceSynchronize();
  n->mem.free_all();
  delete n;
}

// The n parameter tensors of a load as device pointers dv[]: the caller's own (on_device), or copies in ONE staging
// buffer *tmp, which the caller hands to free_staging once its pack kernels are on the stream.
int stage_params(const float* const* src, const int64_t* cnt, int n, int on_device, const char* what, float** tmp,
                 const float** dv, hipStream_t s) {
  for (int i = 0; i < n; ++i) RELA_CHECK(src[i], RELA_EINVAL, "%s: parameter %d is NULL", what, i);
  if (on_device) {
    for (int i = 0; i < n; ++i) dv[i] = src[i];
    return RELA_OK;
  }
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += cnt[i];
  RELA_HIP(hipMalloc(tmp, sizeof(float) * total));
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    RELA_HIP(hipMemcpyAsync(*tmp + off, src[i], sizeof(float) * cnt[i], hipMemcpyHostToDevice, s));
    dv[i] = *tmp + off;
    off += cnt[i];
  }
  return RELA_OK;
}
int free_staging(float* tmp, hipStream_t s) {
  if (tmp) {
    RELA_HIP(hipStreamSynchronize(s));
    (void)hipFree(tmp);
  }
  return RELA_OK;
}

// The body of both nets' loads: the n tensors src[] (state_dict order, cnt[] floats each) become device pointers dv[],
// pack(dv) puts the net's one pack launch on the stream, and the net counts as loaded
template <class Pack>
int load_net(NetBase* net, const float* const* src, const int64_t* cnt, int n, int on_device, const char* who, hipStream_t s,
             Pack pack) {
  const float* dv[kLstmNetSegs];
  float* tmp = nullptr;
  if (int rc = stage_params(src, cnt, n, on_device, who, &tmp, dv, s)) return rc;
  if (int rc = pack(dv)) return rc;
  if (int rc = free_staging(tmp, s)) return rc;
  net->loaded = true;
  net->version += 1;
  return RELA_OK;
}

// A diagnostic kernel with shader-clock stamps: launch(out, stamps) writes its ordinary output to `out_bytes` bytes of
// scratch and its stamps to [2][kStampFrames][kStampPoints] u64, which come back in out_host.
template <class Launch>
int run_stamped(size_t out_bytes, Launch launch, unsigned long long* out_host, hipStream_t s) {
  uint8_t* out = nullptr;
  unsigned long long* st = nullptr;
  const size_t nst = (size_t)2 * kStampFrames * kStampPoints;
  RELA_HIP(hipMalloc(&out, out_bytes));
  RELA_HIP(hipMalloc(&st, nst * 8));
  RELA_HIP(hipMemsetAsync(st, 0, nst * 8, s));
  launch(out, st);
  RELA_HIP(hipStreamSynchronize(s));
  RELA_HIP(hipMemcpy(out_host, st, nst * 8, hipMemcpyDeviceToHost));
  (void)hipFree(out);
  (void)hipFree(st);
  return RELA_OK;
}

// rela_*_debug_workspace: the formats `trunk` leaves a1 / a2 / a3 in (keep_f32: TrunkOpts'; a3_unsplit: a kTrunkBf16
// trunk turns a3 back into f32)
void ws_view_formats(rela_debug_workspace_view* v, TrunkKind trunk, bool keep_f32, bool a3_unsplit) {
  const int fmt = trunk == kTrunkF32 ? RELA_WS_F32 : (trunk == kTrunkBf16 ? RELA_WS_SPLIT_BF16 : RELA_WS_SPLIT3);
  v->a1_format = trunk == kTrunkF32 || (trunk == kTrunkS3 && keep_f32) ? RELA_WS_F32 : RELA_WS_NOT_WRITTEN;
  v->a2_format = fmt;
  v->a3_format = trunk == kTrunkBf16 && a3_unsplit ? RELA_WS_F32 : fmt;
}
}  // namespace

struct rela_ffnet : NetBase {
  const char* const* prof_names = nullptr;  // per-kernel timing labels (actor-side by default)
  // precision: 0 = exact f32 MFMA | 1 = split-bf16 MFMA for conv2 / conv3 / fc (two bf16 parts per operand: 16-bit
  // significands, the "fast" mode) | 2 = f32 operands as THREE bf16 parts on the bf16 MFMA (gemm_f32emu.h: f32 accuracy)
  int max_rows = 0;  // > 0: the owner never runs more rows (a learner's batch): layouts only larger batches read are not packed
  // the layouts the last load packed (ffnet_pack_set, ffnet_plan.h); bft_src: the owner's fc weight where that load
  // left BfT to be packed on demand -- by the forward that reads it, which then adds it to the set
  mutable uint32_t packed = 0;
  const float* bft_src = nullptr;
};

extern "C" int rela_ffnet_create(rela_ffnet** out, int num_action, int device) {
  return create_net(out, num_action, device, "rela_ffnet_create", lay_bit(kLayFFNetEnd) - 1, opt_in_lds_fc_bf16s);
}
extern "C" void rela_ffnet_destroy(rela_ffnet* n) { destroy_net(n); }

extern "C" int rela_ffnet_debug_layout(const rela_ffnet* n, int index, const char** name, int64_t* bytes, int* packed,
                                       void* host_dst) {
  RELA_CHECK(n && index >= 0 && index < kLayFFNetEnd, RELA_EINVAL, "rela_ffnet_debug_layout: an AtariFFNet has %d layouts (index %d)",
             (int)kLayFFNetEnd, index);
  DeviceGuard g(n->device);
  return report_layout(const_cast<FFNetDev&>(n->d), index, n->packed, name, bytes, packed, host_dst);
}

// Diagnostic: the fused conv1 -> conv2 kernel (conv12_i8) with shader-clock stamps at its phase boundaries (block 0,
// waves 0 and 7, first 8 frames): out_host receives [2][8][12] u64.  Points: 0 frame start | 1 conv1 done | 2 barrier |
// 3 conv2 MFMAs done | 4 epilogue | 5 barrier.
extern "C" int rela_ffnet_debug_conv12_stamps(const rela_ffnet* n, int N, const uint8_t* s_dev, unsigned long long* out_host,
                                              void* stream_) {
  RELA_CHECK(n && n->loaded && N >= 1 && s_dev && out_host, RELA_EINVAL, "rela_ffnet_debug_conv12_stamps: bad arguments");
  DeviceGuard g(n->device);
  hipStream_t s = (hipStream_t)stream_;
  const hipError_t attr = opt_in_conv12_i8_stamps();
  RELA_HIP(attr);
  const FFNetDev& d = n->d;
  return run_stamped((size_t)N * 81 * 256, [&](uint8_t* a2, unsigned long long* st) {
    launch_conv12_i8_stamps(s_dev, d.W1d, d.s1q, d.b1q, d.B2f, d.b2, a2, N, st, s);
  }, out_host, s);
}

// Diagnostic: conv3 of the split-bf16 mode with shader-clock stamps (block 0, waves 0 and 7, its first 8 groups of two
// frames): out_host [2][8][12] u64, points 0 group start | 1 MFMA loop (+ staging) done | 2 epilogue stored | 3 barrier |
// 4 copy-out issued.  a2_records: [N][81][hi 64 | lo 64] (any bytes do for timing).
extern "C" int rela_ffnet_debug_conv3_stamps(const rela_ffnet* n, int N, const uint8_t* a2_records, unsigned long long* out_host,
                                             void* stream_) {
  RELA_CHECK(n && n->loaded && N >= 2 && a2_records && out_host, RELA_EINVAL, "rela_ffnet_debug_conv3_stamps: bad arguments");
  DeviceGuard g(n->device);
  hipStream_t s = (hipStream_t)stream_;
  const hipError_t attr = opt_in_conv3_bf16s_stamps();
  RELA_HIP(attr);
  const FFNetDev& d = n->d;
  return run_stamped((size_t)N * 49 * 256, [&](uint8_t* a3, unsigned long long* st) {
    launch_conv3_bf16s_stamps(a2_records, d.B3f, d.b3, a3, N, st, s);
  }, out_host, s);
}

// Diagnostic: fc_bf16s with shader-clock stamps (block 0, waves 0 and 7, positions 8..15): out_host [2][8][12] u64, points
// 0 position start (weight fragments in registers) | 1 MFMA loop done | 2 next tile stored | 3 loads issued | 4 barrier.
// a3_records: [N][49][hi 64 | lo 64] split records (any bytes do for timing).
extern "C" int rela_ffnet_debug_fc_stamps(const rela_ffnet* n, int N, const uint8_t* a3_records, unsigned long long* out_host,
                                          void* stream_) {
  RELA_CHECK(n && n->loaded && N >= FcFast::BM && a3_records && out_host, RELA_EINVAL, "rela_ffnet_debug_fc_stamps: bad arguments");
  DeviceGuard g(n->device);
  hipStream_t s = (hipStream_t)stream_;
  const hipError_t attr = opt_in_fc_bf16s_stamps();
  RELA_HIP(attr);
  const FFNetDev& d = n->d;
  return run_stamped((size_t)N * 512 * 4, [&](uint8_t* h, unsigned long long* st) {
    launch_fc_bf16s_stamps(a3_records, d.Bff, d.bf, reinterpret_cast<float*>(h), N, st, s);
  }, out_host, s);
}

// Diagnostic / test hook: conv1 -> conv2 of the split-bf16 mode for n frames through the job form of the kernel, which
// also copies conv1's records out: a1_records [n][400][hi 32 | lo 32] bf16 (128 B per pixel), a2_records [n][81][hi 64 |
// lo 64] (256 B per pixel), both device pointers; plus the packed conv1 scales and biases (host, 32 floats each) when
// conv1 runs on the int8 matrix cores (zeros otherwise).
extern "C" int rela_ffnet_debug_conv12_records(const rela_ffnet* n, int N, const uint8_t* s_dev, uint8_t* a1_records,
                                               uint8_t* a2_records, float* scale_host, float* bias_host, void* stream_) {
  RELA_CHECK(n && n->loaded && N >= 1 && s_dev && a1_records && a2_records, RELA_EINVAL, "rela_ffnet_debug_conv12_records: bad arguments");
  DeviceGuard g(n->device);
  hipStream_t s = (hipStream_t)stream_;
  const FFNetDev& d = n->d;
  TrunkJobs jobs{};
  jobs.n = 1;
  jobs.j[0] = trunk_job_of(d, s_dev, s_dev, N, a1_records, 0, N, a2_records, nullptr, N, 0, std::min(kNumCU, N));
  launch_trunk_jobs(jobs, jobs.j[0].nblocks, "conv12_fused", nullptr, s);  // (no conv3: the job has no a3)
  RELA_HIP(hipStreamSynchronize(s));
  if (scale_host) RELA_HIP(hipMemcpy(scale_host, d.s1q, 32 * sizeof(float), hipMemcpyDeviceToHost));
  if (bias_host) RELA_HIP(hipMemcpy(bias_host, d.b1q, 32 * sizeof(float), hipMemcpyDeviceToHost));
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

extern "C" int rela_runtime_set_cu_reserve(int cus) {
  RELA_CHECK(cus >= 0 && cus <= 128, RELA_EINVAL, "rela_runtime_set_cu_reserve: 0..128 compute units");
  if (!std::getenv("RELA_CU_RESERVE")) rela_amd::g_cu_reserve.store(cus, std::memory_order_relaxed);
  return RELA_OK;
}
extern "C" int rela_ffnet_num_action(const rela_ffnet* n) { return n ? n->num_action : 0; }
namespace rela_amd {
void ffnet_label_as_learner(rela_ffnet* n) { n->prof_names = kProfLearner; }
void ffnet_set_max_rows(rela_ffnet* n, int rows) { n->max_rows = rows; }
}  // namespace rela_amd
extern "C" uint64_t rela_ffnet_version(const rela_ffnet* n) { return n ? n->version : 0; }
extern "C" int rela_ffnet_set_precision(rela_ffnet* n, int mode) {
  RELA_CHECK(n && mode >= 0 && mode <= 2, RELA_EINVAL,
             "rela_ffnet_set_precision: mode must be 0 (f32 MFMA), 1 (split-bf16, 16-bit operands) or 2 (f32 as three bf16 parts)");
  n->precision = mode;
  n->version += 1;  // results of the two modes differ in the last bits: a cached forward must not be reused across them
  return RELA_OK;
}
extern "C" int rela_ffnet_precision(const rela_ffnet* n) { return n ? n->precision : 0; }

// split3 records of a2 / a3 (f32x3 mode, gemm_s3.h) live behind the f32 layout of ffnet_layout.h (and the fc split-K
// partial tiles): 6 bytes per value where the f32 tensors have 4
static inline int64_t ws_records_offset(int batch) {
  const int64_t b = batch > 0 ? batch : 0;
  const int64_t f = (int64_t)sizeof(float) * (kWsFloatsPerSample * b + (b < kFcSplitBelow ? kFcPartFloats : 0)) + 256;
  return (f + 255) & ~(int64_t)255;
}
extern "C" int64_t rela_ffnet_workspace_bytes(const rela_ffnet* n, int batch) {
  (void)n;
  const int64_t b = batch > 0 ? batch : 0;
  return ws_records_offset((int)b) + b * (kRec2Bytes + kRec3Bytes) + 256;
}

static int ffnet_load_impl(rela_ffnet* n, const rela_ffnet_params* p, int on_device, void* stream_, const ExtraPacks& extra) {
  RELA_CHECK(n && p, RELA_EINVAL, "rela_ffnet_load: bad arguments");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(n->device);
  const int A = n->num_action;
  int64_t cnt[kFFNetSegs];
  ffnet_param_counts(A, cnt);
  const float* src[kFFNetSegs] = {p->conv1_w, p->conv1_b, p->conv2_w, p->conv2_b, p->conv3_w, p->conv3_b,
                                  p->fc_w,    p->fc_b,    p->v_w,     p->v_b,     p->a_w,     p->a_b};
  return load_net(n, src, cnt, kFFNetSegs, on_device, "rela_ffnet_load", s, [&](const float* const* dv) -> int {
    // what this load packs: everything, less what a net with a row limit never reads (ffnet_pack_set)
    const uint32_t set = ffnet_pack_set(n->max_rows, n->precision, on_device != 0);
    n->bft_src = ffnet_bft_on_demand(n->max_rows, n->precision, on_device != 0) ? dv[6] : nullptr;  // (the owner's buffer outlives this call)
    if (int rc = pack_layouts(n->d, set, dv, kFFNetSegs, A, extra, dv[6], s)) return rc;
    n->packed = set;
    return RELA_OK;
  });
}
extern "C" int rela_ffnet_load(rela_ffnet* n, const rela_ffnet_params* p, int on_device, void* stream_) {
  return ffnet_load_impl(n, p, on_device, stream_, rela_amd::ExtraPacks{});
}
int rela_amd::ffnet_load_extra(rela_ffnet* n, const rela_ffnet_params* p, void* stream_, const ExtraPacks& extra) {
  return ffnet_load_impl(n, p, 1, stream_, extra);
}

static int forward_impl(const rela_ffnet* n, int N, const uint8_t* s_dev, const float* legal_dev, float* q_dev, void* ws,
                        int64_t ws_bytes, void* stream_, int mode, int rows_limit, const FrameRows* store, int* copied);
extern "C" int rela_ffnet_forward(const rela_ffnet* n, int N, const uint8_t* s_dev, const float* legal_dev,
                                  float* q_dev, void* ws, int64_t ws_bytes, void* stream_) {
  return rela_amd::ffnet_forward_mode(n, N, s_dev, legal_dev, q_dev, ws, ws_bytes, stream_, kModeNet);
}

int rela_amd::ffnet_forward_mode(const rela_ffnet* n, int N, const uint8_t* s_dev, const float* legal_dev, float* q_dev,
                                 void* ws, int64_t ws_bytes, void* stream_, int mode, int rows_limit) {
  return forward_impl(n, N, s_dev, legal_dev, q_dev, ws, ws_bytes, stream_, mode, rows_limit, nullptr, nullptr);
}

bool rela_amd::ffnet_forward_stores_frames(const rela_ffnet* n, int N) {
  return n && N >= 1 && plan_ffnet_forward(kModeNet, n->precision, N, n->max_rows).trunk == kTrunkS3;
}
int rela_amd::ffnet_forward_store_frames(const rela_ffnet* n, int N, const uint8_t* s_dev, const float* legal_dev, float* q_dev,
                                         void* ws, int64_t ws_bytes, void* stream_, const FrameRows& rows, int* copied) {
  RELA_CHECK(copied && rows.base && ((uintptr_t)rows.base & 3) == 0 && rows.first >= 0 && rows.first < rows.ring && N <= rows.ring,
             RELA_EINVAL, "ffnet_forward_store_frames: bad frame rows (first %d, ring %d, %d frames)", rows.first, rows.ring, N);
  if (rows.src2) {  // the second ring lies wholly before or behind the first
    const uint8_t *b1 = rows.base, *b2 = rows.base2;
    const int64_t len = (int64_t)rows.ring * kFrameBytes;
    RELA_CHECK(b2 && (((uintptr_t)b2 | (uintptr_t)rows.src2) & 3) == 0 && rows.first2 >= 0 && rows.first2 < rows.ring &&
                   (b2 + len <= b1 || b1 + len <= b2),
               RELA_EINVAL, "ffnet_forward_store_frames: bad second frame rows (first %d, ring %d)", rows.first2, rows.ring);
  }
  return forward_impl(n, N, s_dev, legal_dev, q_dev, ws, ws_bytes, stream_, kModeNet, -1, &rows, copied);
}

// Test tap: ffnet_forward_store_frames over a caller's ring of frame rows
extern "C" int rela_ffnet_debug_forward_store_frames(const rela_ffnet* n, int N, const uint8_t* s_dev, const float* legal_dev,
                                                     float* q_dev, void* ws, int64_t ws_bytes, void* rows_dev, int first,
                                                     int ring, int* copied, void* stream_) {
  return rela_amd::ffnet_forward_store_frames(n, N, s_dev, legal_dev, q_dev, ws, ws_bytes, stream_,
                                              FrameRows{static_cast<uint8_t*>(rows_dev), first, ring}, copied);
}
// ... with the second pair: the n frames at s2_dev to row (first2 + i) mod ring of rows2_dev
extern "C" int rela_ffnet_debug_forward_store_frames2(const rela_ffnet* n, int N, const uint8_t* s_dev, const float* legal_dev,
                                                      float* q_dev, void* ws, int64_t ws_bytes, void* rows_dev, int first,
                                                      int ring, const uint8_t* s2_dev, void* rows2_dev, int first2, int* copied,
                                                      void* stream_) {
  RELA_CHECK(s2_dev && rows2_dev, RELA_EINVAL, "rela_ffnet_debug_forward_store_frames2: no second source or destination");
  return rela_amd::ffnet_forward_store_frames(
      n, N, s_dev, legal_dev, q_dev, ws, ws_bytes, stream_,
      FrameRows{static_cast<uint8_t*>(rows_dev), first, ring, s2_dev, static_cast<uint8_t*>(rows2_dev), first2}, copied);
}

// store != NULL: a kTrunkS3 plan also stores the frames into *store and sets *copied to the number of fields (1, or 2 with
// the second pair), any other plan clears it
static int forward_impl(const rela_ffnet* n, int N, const uint8_t* s_dev, const float* legal_dev, float* q_dev, void* ws,
                        int64_t ws_bytes, void* stream_, int mode, int rows_limit, const FrameRows* store, int* copied) {
  if (copied) *copied = 0;
  RELA_CHECK(n && n->loaded, RELA_ESTATE, "rela_ffnet_forward: parameters were never loaded");
  const int max_rows = rows_limit < 0 ? n->max_rows : rows_limit;
  RELA_CHECK(N >= 1 && s_dev && legal_dev && q_dev && ws, RELA_EINVAL, "rela_ffnet_forward: bad arguments");
  RELA_CHECK(ws_bytes >= rela_ffnet_workspace_bytes(n, N), RELA_EINVAL,
             "rela_ffnet_forward: workspace of %lld bytes is too small for batch %d", (long long)ws_bytes, N);
  RELA_CHECK(((uintptr_t)s_dev & 15) == 0 && ((uintptr_t)ws & 15) == 0, RELA_EINVAL,
             "rela_ffnet_forward: s_dev and workspace must be 16-byte aligned");
  RELA_CHECK(max_rows <= 0 || N <= max_rows, RELA_EINVAL,
             "rela_ffnet_forward: batch %d on a net whose owner declared at most %d rows", N, max_rows);
  hipStream_t s = (hipStream_t)stream_;
  const FFNetWs w = ffnet_ws(ws, N);
  const FFNetDev& d = n->d;
  const char* const* names = n->prof_names ? n->prof_names : kProfActor;
  const char* name12 = n->prof_names ? "learner_fwd_conv12" : "conv12_fused";  // conv1 -> conv2 in one launch
  const FfnetPlan plan = plan_ffnet_forward(mode, n->precision, N, max_rows);
  uint32_t missing = ffnet_plan_reads(plan) & ~n->packed;
  if (missing == lay_bit(kLayBfT) && n->bft_src) {  // (see rela_ffnet::bft_src)
    if (int rc = pack_one(kLayouts[kLayBfT].kind, n->bft_src, nullptr, n->d.BfT, 0, 0, kLayouts[kLayBfT].elements, s)) return rc;
    n->packed |= lay_bit(kLayBfT);
    missing = 0;
  }
  RELA_CHECK(missing == 0, RELA_ESTATE,
             "rela_ffnet_forward: %d rows in mode %d read layouts (bits 0x%x) the net's last load did not pack (row limit %d)", N,
             plan.precision, missing, n->max_rows);

  // the trunk: a3 as f32, as split-bf16 records in its own place, or as split3 records at rec3 -- whatever plan.fc reads
  uint8_t* rec2 = static_cast<uint8_t*>(ws) + ws_records_offset(N);
  uint8_t* rec3 = rec2 + (int64_t)N * kRec2Bytes;
  TrunkOpts opts;
  opts.keep_f32 = plan.keep_f32;
  opts.leave_a3_records = !plan.unsplit_a3;
  if (store && plan.trunk == kTrunkS3 && !plan.keep_f32) {
    opts.store_frames = store;
    *copied = store->src2 ? 2 : 1;
  }
  launch_trunk(d, plan.trunk, N, s_dev, w.a1, w.a2, w.a3, rec2, rec3, opts, {names[0], names[1], names[2], name12}, s);

  float* const part = fc_part_ptr(ws, w.ha, N);  // (the split-K fcs' partial tiles)
  switch (plan.fc) {
    case kFcBf16: {
      ProfScope prof(names[3], s);
      launch_fc_bf16s(recs(w.a3), d.Bff, d.bf, w.h, N, s);
      break;
    }
    case kFcBf16SplitK:
      launch_fc_bf16_splitk(recs(w.a3), d.Bff, d.bf, part, w.h, N, names[3], s);
      break;
    case kFcS3:
    case kFcS3SplitK: {
      ProfScope prof(names[3], s);
      note_launch("gemm_s3<fc>");
      const s3::Plan pl = s3::plan<s3::ProbFc>(N, plan.fc == kFcS3SplitK);
      if (pl.slices > 1) {  // small batches: the contraction split over blocks, fc_reduce adds slices + bias + ReLU
        s3::launch<s3::ProbFc, s3::kEpiRaw>(rec3, d.Bfe, d.bf, part, N, s, pl);
        launch_fc_reduce(part, pl.slices, N, d.bf, w.h, s);
      } else {
        s3::launch<s3::ProbFc, s3::kEpiRelu>(rec3, d.Bfe, d.bf, w.h, N, s);
      }
      break;
    }
    case kFcF32SplitK:
      launch_fc_f32_splitk(w.a3, d.BfT, d.bf, part, w.h, N, plan.fc_slices, names[3], s);
      break;
    case kFcF32Gemm: {
      ProfScope prof(names[3], s);
      launch_gemm_bm<GemmFc, GemmFc112>("gemm_mfma<GemmFc> (f32)", w.a3, nullptr, d.Bf, d.bf, w.h, nullptr, nullptr, N, s);
      break;
    }
  }
  // the learner's f32x3 pass: a2 / a3 as f32 too, for the backward kernels (a1: conv12_s3 wrote it)
  if (plan.trunk == kTrunkS3 && plan.keep_f32) unsplit_s3_a23(rec2, rec3, w.a2, w.a3, N, s);
  {
    ProfScope prof(names[4], s);
    launch_heads_duel(w.h, d.Bhp, d.bh, legal_dev, w.ha, q_dev, N, n->num_action, s);
  }
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

// Test tap: the workspace offsets and the plan of a forward of N rows at the net's precision, from the helpers the
// forward itself calls (host only)
extern "C" int rela_ffnet_debug_workspace(const rela_ffnet* n, int N, rela_debug_workspace_view* v) {
  RELA_CHECK(n && v && N >= 1, RELA_EINVAL, "rela_ffnet_debug_workspace: bad arguments");
  char* const ws = reinterpret_cast<char*>((uintptr_t)1 << 30);  // (never dereferenced: offsets only)
  auto off = [&](const void* p) { return (int64_t)(static_cast<const char*>(p) - ws); };
  const FFNetWs w = ffnet_ws(ws, N);
  const FfnetPlan plan = plan_ffnet_forward(kModeNet, n->precision, N, n->max_rows);
  *v = rela_debug_workspace_view{};
  v->a1 = off(w.a1), v->a2 = off(w.a2), v->a3 = off(w.a3), v->h = off(w.h), v->ha = off(w.ha), v->gx = -1;
  v->fc_part = off(fc_part_ptr(ws, w.ha, N));
  v->rec2 = ws_records_offset(N), v->rec3 = v->rec2 + (int64_t)N * kRec2Bytes;
  v->precision = plan.precision, v->trunk = plan.trunk, v->fc = plan.fc, v->fc_per = plan.fc_per;
  v->fc_slices = (plan.fc == kFcS3 || plan.fc == kFcS3SplitK) ? s3::plan<s3::ProbFc>(N, plan.fc == kFcS3SplitK).slices : plan.fc_slices;
  ws_view_formats(v, plan.trunk, plan.keep_f32, plan.unsplit_a3);
  v->a3_records = v->a3_format != RELA_WS_F32, v->x_in_gx = 0;
  return RELA_OK;
}

// ---- the Ape-X learner's three forwards in split-bf16, one launch per layer (csrc/learner.hip) ----------------
namespace rela_amd {
bool ffnet_learner_forward_ok(const rela_ffnet* on, const rela_ffnet* tg, int B) {
  return on && tg && on->loaded && tg->loaded && learner_merged_rows(B) && packs_bf16_fc(on->max_rows) &&
         packs_bf16_fc(tg->max_rows);
}

// online over [s ; s'] (2 B rows: rows < B are s) and target over s' (B rows): conv1 -> conv2 of both nets in ONE
// launch (block ranges in proportion to the rows), conv3 likewise, fc as split-K launches of fc_bf16s straight from
// a3's records, the dueling heads per Q table.  ws_on has the ffnet_ws layout for 2 B rows, ws_tg for B rows; a1 (rows
// < B only), a2 and a3 hold split RECORDS: ffnet_learner_unsplit turns the rows < B into f32 for the backward pass.
int ffnet_learner_forward(const rela_ffnet* on, const rela_ffnet* tg, int B, const uint8_t* s_obs, const uint8_t* s_next,
                          const float* legal, const float* nlegal, float* q_on, float* q_no, float* q_nt, void* ws_on,
                          void* ws_tg, int64_t ws_bytes, hipStream_t s) {
  RELA_CHECK(ffnet_learner_forward_ok(on, tg, B), RELA_ESTATE, "ffnet_learner_forward: nets not loaded / batch %d unsupported", B);
  RELA_CHECK(ws_bytes >= rela_ffnet_workspace_bytes(on, 2 * B), RELA_EINVAL, "ffnet_learner_forward: workspace too small");
  RELA_CHECK(((uintptr_t)s_obs & 15) == 0 && ((uintptr_t)s_next & 15) == 0, RELA_EINVAL, "ffnet_learner_forward: frames must be 16-byte aligned");
  const FFNetWs w = ffnet_ws(ws_on, 2 * B), wt = ffnet_ws(ws_tg, B);
  TrunkJobs jobs{};
  jobs.n = 2;
  const int total = std::min(kNumCU, 3 * B);
  const int nb0 = std::max(1, std::min(total - 1, (int)((int64_t)total * 2 / 3)));
  jobs.j[0] = trunk_job_of(on->d, s_obs, s_next, B, recs(w.a1), 0, B, recs(w.a2), recs(w.a3), 2 * B, 0, nb0);
  jobs.j[1] = trunk_job_of(tg->d, s_next, s_next, B, nullptr, 0, 0, recs(wt.a2), recs(wt.a3), B, nb0, total - nb0);
  launch_trunk_jobs(jobs, total, "learner_fwd_conv12", "learner_fwd_conv3", s);
  launch_fc_bf16_splitk(recs(w.a3), on->d.Bff, on->d.bf, fc_part_ptr(ws_on, w.ha, 2 * B), w.h, 2 * B, "learner_fwd_fc", s);
  launch_fc_bf16_splitk(recs(wt.a3), tg->d.Bff, tg->d.bf, fc_part_ptr(ws_tg, wt.ha, B), wt.h, B, "learner_fwd_fc", s);
  {
    ProfScope prof("learner_fwd_heads", s);
    const int nb = ceil_div(B, kHeadRows);
    HeadJobs jb{};
    const float* hs[3] = {w.h, w.h + (size_t)B * kH, wt.h};
    float* has[3] = {w.ha, w.ha + (size_t)B * kHA, wt.ha};
    const rela_ffnet* nets[3] = {on, on, tg};
    const float* legals[3] = {legal, nlegal, nlegal};
    float* qs[3] = {q_on, q_no, q_nt};
    for (int k = 0; k < 3; ++k) {
      jb.h[k] = hs[k], jb.Bhp[k] = nets[k]->d.Bhp, jb.bias[k] = nets[k]->d.bh, jb.legal[k] = legals[k];
      jb.ha[k] = has[k], jb.q[k] = qs[k], jb.N[k] = B, jb.first[k] = k * nb;
    }
    jb.first[3] = 3 * nb;
    launch_heads_duel_jobs(jb, on->num_action, s);
  }
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

int trunk_unsplit_rows(float* a1, float* a2, float* a3, int rows, hipStream_t s) {
  ProfScope prof("learner_unsplit", s);
  launch_unsplit_trunk_rows(recs(a1), recs(a2), recs(a3), rows, s);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

int ffnet_learner_unsplit(int B, void* ws_on, hipStream_t s) {
  const FFNetWs w = ffnet_ws(ws_on, 2 * B);
  return trunk_unsplit_rows(w.a1, w.a2, w.a3, B, s);
}
}  // namespace rela_amd

// =====================================================================================
// AtariLSTMNet (pyrela/net.py:58-163): trunk -> LSTM gates + cell (one fused GEMM) -> heads
// =====================================================================================
// precision: 0 = exact f32; 1 = split-bf16 conv trunk and, from kFastMinN rows up, the x part of the gate GEMM on split-bf16
// MFMA too (the recurrent part and the cell stay f32); 2 = f32x3: from 512 rows up the conv trunk AND the x part of the
// gate GEMM (3136 -> 2048: three quarters of the step's FLOPs) with three-part operands on the bf16 matrix cores
// (conv12_s3.h, conv_img_s3.h, gemm_s3.h: f32 accuracy), the recurrent part, the cell and the heads as in mode 0.
// d: the shared layouts (trunk, Bh / bh) and Bl, bl, Wrec, Wx3; the AtariFFNet's own stay NULL
struct rela_lstmnet : NetBase {};

namespace {
constexpr int64_t kLstmWsFloats = kA1 + kA2 + kA3 + kHA + 2048;  // + the x part of the gates (bf16x2 / f32x3 modes)
using ProbGateX3 = s3::ProbFcT<2048>;
// split3 records of a2 / a3 behind the f32 layout (f32x3 mode)
inline int64_t lstm_ws_records_offset(int batch) {
  return (((int64_t)sizeof(float) * kLstmWsFloats * (batch > 0 ? batch : 0) + 256) + 255) & ~(int64_t)255;
}
// the workspace of one rela_lstmnet_step of N rows and what the step runs at `precision` (the step and its test tap)
struct LstmStepWs {
  float *a1, *a2, *a3, *ha, *gx;
  uint8_t *rec2, *rec3;
  LstmTrunkPlan tp;
  bool x_in_gx;  // the x part of the gates is a GEMM of its own over a3's records -> gx (raw sums, permuted gate columns)
};
inline LstmStepWs lstm_step_ws(void* ws, int N, int precision) {
  LstmStepWs w;
  w.a1 = static_cast<float*>(ws);
  w.a2 = w.a1 + kA1 * N;
  w.a3 = w.a2 + kA2 * N;
  w.ha = w.a3 + kA3 * N;
  w.gx = w.ha + kHA * N;
  w.rec2 = static_cast<uint8_t*>(ws) + lstm_ws_records_offset(N);
  w.rec3 = w.rec2 + (int64_t)N * kRec2Bytes;
  // bf16x2 mode from kFastMinN rows up: a3 stays in split records, the x part of the gates is one split-bf16 GEMM
  // (gemm_bf16s.h: 41 GFLOP at 3,200 rows) and the f32 MFMA kernel only adds h x W_hh (K = 512) and runs the cell
  const bool fast_gates = precision == 1 && N >= kFastMinN;
  w.tp = plan_lstm_trunk(precision == 1, precision == 2, /*has_rec_scratch=*/true, N, fast_gates);
  w.x_in_gx = w.tp.trunk == kTrunkS3 || (w.tp.trunk == kTrunkBf16 && w.tp.a3_records);
  return w;
}
const char* const kLstmActorNames[3] = {"conv1_bf16x3", "conv2_mfma", "conv3_mfma"};
// the trunk of an AtariLSTMNet: the fused conv1 -> conv2 launches run under conv2's label
inline TrunkLabels lstm_trunk_labels(const char* const* names) { return {names[0], names[1], names[2], names[1]}; }
}  // namespace

extern "C" int rela_lstmnet_create(rela_lstmnet** out, int num_action, int device) {
  return create_net(out, num_action, device, "rela_lstmnet_create", kLstmNetLayouts, nullptr);
}
extern "C" void rela_lstmnet_destroy(rela_lstmnet* n) { destroy_net(n); }

// (a load of an AtariLSTMNet packs every layout it holds)
extern "C" int rela_lstmnet_debug_layout(const rela_lstmnet* n, int index, const char** name, int64_t* bytes, int* packed,
                                         void* host_dst) {
  constexpr int rows = kLayShared + (kLayCount - kLayBl);
  RELA_CHECK(n && index >= 0 && index < rows, RELA_EINVAL, "rela_lstmnet_debug_layout: an AtariLSTMNet has %d layouts (index %d)", rows,
             index);
  DeviceGuard g(n->device);
  return report_layout(const_cast<FFNetDev&>(n->d), index < kLayShared ? index : kLayBl + (index - kLayShared),
                       n->loaded ? kLstmNetLayouts : 0u, name, bytes, packed, host_dst);
}

extern "C" int rela_lstmnet_set_precision(rela_lstmnet* n, int mode) {
  RELA_CHECK(n && mode >= 0 && mode <= 2, RELA_EINVAL,
             "rela_lstmnet_set_precision: mode must be 0 (f32), 1 (bf16x2) or 2 (f32x3: conv2 / conv3 of the trunk with three-part operands)");
  if (n->precision != mode) n->version += 1;  // cached forwards of the other mode must not be reused
  n->precision = mode;
  return RELA_OK;
}
extern "C" int rela_lstmnet_precision(const rela_lstmnet* n) { return n ? n->precision : 0; }

extern "C" int rela_lstmnet_num_action(const rela_lstmnet* n) { return n ? n->num_action : 0; }
extern "C" uint64_t rela_lstmnet_version(const rela_lstmnet* n) { return n ? n->version : 0; }

extern "C" int64_t rela_lstmnet_workspace_bytes(const rela_lstmnet* n, int batch) {
  (void)n;
  return lstm_ws_records_offset(batch) + (int64_t)(batch > 0 ? batch : 0) * (kRec2Bytes + kRec3Bytes) + 256;
}

static int lstmnet_load_impl(rela_lstmnet* n, const rela_lstmnet_params* p, int on_device, void* stream_, const ExtraPacks& extra) {
  RELA_CHECK(n && p, RELA_EINVAL, "rela_lstmnet_load: bad arguments");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(n->device);
  const int A = n->num_action;
  int64_t cnt[kLstmNetSegs];
  lstmnet_param_counts(A, cnt);
  const float* src[kLstmNetSegs] = {p->conv1_w, p->conv1_b, p->conv2_w, p->conv2_b, p->conv3_w, p->conv3_b, p->w_ih,
                                    p->w_hh,    p->b_ih,    p->b_hh,    p->v_w,     p->v_b,     p->a_w,     p->a_b};
  return load_net(n, src, cnt, kLstmNetSegs, on_device, "rela_lstmnet_load", s, [&](const float* const* dv) {
    return pack_layouts(n->d, kLstmNetLayouts, dv, kLstmNetSegs, A, extra, nullptr, s);
  });
}
extern "C" int rela_lstmnet_load(rela_lstmnet* n, const rela_lstmnet_params* p, int on_device, void* stream_) {
  return lstmnet_load_impl(n, p, on_device, stream_, rela_amd::ExtraPacks{});
}
int rela_amd::lstmnet_load_extra(rela_lstmnet* n, const rela_lstmnet_params* p, void* stream_, const ExtraPacks& extra) {
  return lstmnet_load_impl(n, p, 1, stream_, extra);
}

extern "C" int rela_lstmnet_step(const rela_lstmnet* n, int N, const uint8_t* s_dev, const float* legal_dev,
                                 const float* h_in, const float* c_in, float* h_out, float* c_out, float* q_dev,
                                 float* adv_dev, void* ws, int64_t ws_bytes, void* stream_) {
  RELA_CHECK(n && n->loaded, RELA_ESTATE, "rela_lstmnet_step: parameters were never loaded");
  RELA_CHECK(N >= 1 && s_dev && legal_dev && h_in && c_in && h_out && c_out && ws, RELA_EINVAL,
             "rela_lstmnet_step: bad arguments");
  RELA_CHECK(h_in != h_out && c_in != c_out, RELA_EINVAL, "rela_lstmnet_step: state may not be updated in place");
  RELA_CHECK(ws_bytes >= rela_lstmnet_workspace_bytes(n, N), RELA_EINVAL,
             "rela_lstmnet_step: workspace of %lld bytes is too small for batch %d", (long long)ws_bytes, N);
  RELA_CHECK(((uintptr_t)s_dev & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)h_in & 15) == 0, RELA_EINVAL,
             "rela_lstmnet_step: s_dev, h_in and workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream_;
  const LstmStepWs w = lstm_step_ws(ws, N, n->precision);
  const FFNetDev& d = n->d;
  TrunkOpts opts;
  opts.leave_a3_records = w.tp.a3_records;
  launch_trunk(d, w.tp.trunk, N, s_dev, w.a1, w.a2, w.a3, w.rec2, w.rec3, opts, lstm_trunk_labels(kLstmActorNames), s);
  // the x part of the gates (3136 -> 2048) over a3's records -> gx (raw sums, permuted gate columns), where the trunk
  // left records: as a three-part GEMM (f32x3) or a split-bf16 one (bf16x2)
  if (w.tp.trunk == kTrunkS3) {
    ProfScope prof("lstm_gates_x_f32x3", s);
    note_launch("gemm_s3<gates_x>");
    s3::launch<ProbGateX3, s3::kEpiRaw>(w.rec3, d.Wx3, nullptr, w.gx, N, s);
  } else if (w.x_in_gx) {
    int rc = gemm16::launch_rec64_nt(recs(w.a3), d.Wrec, N, 2048, 49, gemm16::EpiPlain{w.gx, 2048}, s, "lstm_gates_x_bf16");
    if (rc != RELA_OK) return rc;
  }
  {
    ProfScope prof("lstm_gates_mfma", s);
    if (w.x_in_gx)  // the f32 MFMA kernel adds h x W_hh (K = 512) and the bias and runs the cell
      launch_gemm_bm<GemmLstmH, GemmLstmH112>("gemm_mfma<GemmLstmH> (f32)", h_in, w.gx, d.Bl, d.bl, h_out, c_in, c_out, N, s);
    else
      launch_gemm_bm<GemmLstm, GemmLstm112>("gemm_mfma<GemmLstm> (f32)", w.a3, h_in, d.Bl, d.bl, h_out, c_in, c_out, N, s);
  }
  if (q_dev || adv_dev) launch_heads_f32(h_out, d.Bh, d.bh, legal_dev, w.ha, q_dev, adv_dev, N, n->num_action, "heads_mfma", "dueling", s);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

extern "C" int rela_lstmnet_debug_workspace(const rela_lstmnet* n, int N, rela_debug_workspace_view* v) {
  RELA_CHECK(n && v && N >= 1, RELA_EINVAL, "rela_lstmnet_debug_workspace: bad arguments");
  char* const ws = reinterpret_cast<char*>((uintptr_t)1 << 30);  // (never dereferenced: offsets only)
  auto off = [&](const void* p) { return (int64_t)(static_cast<const char*>(p) - ws); };
  const LstmStepWs w = lstm_step_ws(ws, N, n->precision);
  *v = rela_debug_workspace_view{};
  v->a1 = off(w.a1), v->a2 = off(w.a2), v->a3 = off(w.a3), v->h = -1, v->ha = off(w.ha), v->gx = off(w.gx), v->fc_part = -1;
  v->rec2 = off(w.rec2), v->rec3 = off(w.rec3);
  v->precision = n->precision, v->trunk = w.tp.trunk, v->fc = -1, v->fc_slices = 0, v->fc_per = 0;
  ws_view_formats(v, w.tp.trunk, false, !w.tp.a3_records);
  v->a3_records = w.tp.a3_records, v->x_in_gx = w.x_in_gx;
  return RELA_OK;
}

// ---- internal entry points for the R2D2 learner (csrc/learner_r2d2.hip) -------------------------
namespace rela_amd {
// conv trunk only: frames u8[N][4][84][84] -> a1 / a2 / a3 (channel-last, ffnet_layout.h has the contract)
int lstmnet_trunk(const rela_lstmnet* n, int N, const uint8_t* s_dev, float* a1, float* a2, float* a3, hipStream_t s,
                  const char* const* names, bool fast, bool* a3_records, uint8_t* s3_scratch, bool keep_f32) {
  RELA_CHECK(n && n->loaded, RELA_ESTATE, "lstmnet_trunk: parameters were never loaded");
  RELA_CHECK(N >= 1 && s_dev && a1 && a2 && a3, RELA_EINVAL, "lstmnet_trunk: bad arguments");
  const LstmTrunkPlan tp = plan_lstm_trunk(fast, !fast && n->precision == 2, s3_scratch != nullptr, N, a3_records != nullptr);
  uint8_t* rec3 = s3_scratch ? s3_scratch + (int64_t)N * kRec2Bytes : nullptr;
  TrunkOpts opts;
  opts.keep_f32 = keep_f32;
  opts.leave_a3_records = tp.a3_records;
  launch_trunk(n->d, tp.trunk, N, s_dev, a1, a2, a3, s3_scratch, rec3, opts, lstm_trunk_labels(names), s);
  if (tp.trunk == kTrunkS3 && keep_f32) unsplit_s3_a23(s3_scratch, rec3, a2, a3, N, s);
  if (a3_records) *a3_records = tp.a3_records;
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

int64_t gate_x3_packed_bytes() { return kLayouts[kLayWx3].bytes(); }
int pack_gate_x3(const float* w_ih_dev, void* dst, bool permuted, hipStream_t s) {
  RELA_CHECK(w_ih_dev && dst, RELA_EINVAL, "pack_gate_x3: bad arguments");
  return pack_one(permuted ? kPackEmuGatesPerm : kPackEmuFc, w_ih_dev, nullptr, dst, f32emu::ProbGateX::NCG, f32emu::ProbGateX::KS,
                  kLayouts[kLayWx3].elements, s);
}
int gate_x3_gemm(const uint8_t* a3_records, const void* packed, const float* bias, float* gx, int M, hipStream_t s) {
  RELA_CHECK(a3_records && packed && bias && gx && M >= 1, RELA_EINVAL, "gate_x3_gemm: bad arguments");
  note_launch("gemm_s3<gates_x>");
  s3::launch<ProbGateX3, s3::kEpiBias>(a3_records, reinterpret_cast<const uint4*>(packed), bias, gx, M, s);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

// The ONLINE net's conv trunk of the R2D2 learner on split-bf16 MFMA (r3): conv1 -> conv2 fused, with conv1's records
// copied out for the rows [a1_lo, N) -- the training frames, whose a1 the backward kernels read -- and conv3; a1 (those
// rows), a2 and a3 come out as split RECORDS in the f32 tensors' places.  The caller feeds a3's records to the gate GEMM
// and then turns the training rows back into f32 with trunk_unsplit_rows.
int lstmnet_trunk_records(const rela_lstmnet* n, int N, const uint8_t* s_dev, float* a1, float* a2, float* a3, int a1_lo,
                          hipStream_t s, const char* const* names) {
  RELA_CHECK(n && n->loaded, RELA_ESTATE, "lstmnet_trunk_records: parameters were never loaded");
  RELA_CHECK(N >= 1 && s_dev && a1 && a2 && a3 && a1_lo >= 0 && a1_lo <= N, RELA_EINVAL, "lstmnet_trunk_records: bad arguments");
  TrunkJobs jobs{};
  jobs.n = 1;
  const int nblocks = std::min(kNumCU, N);
  jobs.j[0] = trunk_job_of(n->d, s_dev, s_dev, N, recs(a1), a1_lo, N - a1_lo, recs(a2), recs(a3), N, 0, nblocks);
  launch_trunk_jobs(jobs, nblocks, names[1], names[2], s);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

// dueling heads on rows of LSTM outputs: o f32[N][512] -> ha [N][32] (cols 0..A-1 = fc_a, col 31 = fc_v) and q [N][A]
int lstmnet_heads(const rela_lstmnet* n, int N, const float* o, const float* legal, float* ha, float* q, hipStream_t s,
                  const char* name) {
  RELA_CHECK(n && n->loaded, RELA_ESTATE, "lstmnet_heads: parameters were never loaded");
  launch_heads_f32(o, n->d.Bh, n->d.bh, legal, ha, q, nullptr, N, n->num_action, name, nullptr, s);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}
}  // namespace rela_amd
