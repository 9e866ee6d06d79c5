// atari_screen.hip -- GameState::computeFeature (atari/game_state.h:53-82,122-133) on the device, for the envs that render
// raw screens (rela/screen_env.h):
//   rela_atari_features           [rows][2][H][W][3] u8 screen pairs -> [rows][84][84] u8 features, one launch
//   screens_to_stacks (internal)  features -> the actor shards' frame stacks (rela_*_actor_screens_to_stacks)
//
// The arithmetic is atari_screen.h's fixed float32 recipe.  Memory bound: per row, the 2 x 84 = 168 source rows of both
// screens that the 84 output rows interpolate between (80 % of a 210-row screen) are read, 7,056 B are written.  One
// block of 256 threads = one env row x three output rows (252 pixels): it stages the six source rows of both screens
// with 16-byte loads (a wave reads whole 480-byte rows back to back), keeps their element-wise max in LDS, and each
// thread then interpolates one pixel from LDS.  The per-axis tables and the 1/255 table come from the host by value.
#include "atari_screen.h"
#include "common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

using rela_atari::kMaxIn;
using rela_atari::kOut;
using rela_atari::Tables;

constexpr int kRowsPerBlock = 3;                 // output rows per block
constexpr int kTiles = kOut / kRowsPerBlock;     // 28 blocks per env row
constexpr int kSrc = 2 * kRowsPerBlock;          // staged source rows per block
constexpr int kThreads = 256;

__device__ inline uint32_t max_u8x4(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const uint32_t x = (a >> k) & 0xFFu, y = (b >> k) & 0xFFu;
    r |= (x > y ? x : y) << k;
  }
  return r;
}

// kVec: rows are 16-byte aligned (W * 3 % 16 == 0 and an aligned base): 16-byte loads; otherwise byte loads
template <bool kVec>
__global__ __launch_bounds__(kThreads) void atari_features_kernel(const uint8_t* __restrict__ screens, int H, int W,
                                                                  uint8_t* __restrict__ planes, const Tables tab) {
  __shared__ float v[256];
  __shared__ __attribute__((aligned(16))) uint8_t m[kSrc][kMaxIn * 3];
  const int env = blockIdx.x / kTiles, tile = blockIdx.x - env * kTiles;
  const int y0 = tile * kRowsPerBlock;
  const int rb = W * 3;
  const uint8_t* s0 = screens + (size_t)env * 2 * H * rb;  // current screen
  const uint8_t* s1 = s0 + (size_t)H * rb;                  // previous screen
  v[threadIdx.x] = tab.v[threadIdx.x];
  if (kVec) {
    const int n16 = rb >> 4;
    for (int i = threadIdx.x; i < kSrc * n16; i += kThreads) {
      const int r = i / n16, c = i - r * n16;
      const int y = y0 + (r >> 1);
      const int src = (r & 1) ? tab.h.i1[y] : tab.h.i0[y];
      const uint4 a = reinterpret_cast<const uint4*>(s0 + (size_t)src * rb)[c];
      const uint4 b = reinterpret_cast<const uint4*>(s1 + (size_t)src * rb)[c];
      reinterpret_cast<uint4*>(&m[r][0])[c] =
          make_uint4(max_u8x4(a.x, b.x), max_u8x4(a.y, b.y), max_u8x4(a.z, b.z), max_u8x4(a.w, b.w));
    }
  } else {
    for (int i = threadIdx.x; i < kSrc * rb; i += kThreads) {
      const int r = i / rb, c = i - r * rb;
      const int y = y0 + (r >> 1);
      const int src = (r & 1) ? tab.h.i1[y] : tab.h.i0[y];
      const uint8_t a = s0[(size_t)src * rb + c], b = s1[(size_t)src * rb + c];
      m[r][c] = a > b ? a : b;
    }
  }
  __syncthreads();
  if (threadIdx.x >= kRowsPerBlock * kOut) return;
  const int yl = threadIdx.x / kOut, x = threadIdx.x - yl * kOut, y = y0 + yl;
  planes[(size_t)env * kOut * kOut + y * kOut + x] =
      rela_atari::feature_pixel(v, m[2 * yl], m[2 * yl + 1], tab.w.i0[x], tab.w.i1[x], tab.w.l0[x], tab.w.l1[x],
                                tab.h.l0[y], tab.h.l1[y]);
}

}  // namespace

namespace rela_amd {

int atari_features(const uint8_t* screens, int rows, int height, int width, uint8_t* planes, hipStream_t s) {
  RELA_CHECK(screens && planes && rows >= 1 && rows <= (1 << 30) / kTiles, RELA_EINVAL,
             "rela_atari_features: bad arguments (rows=%d)", rows);
  RELA_CHECK(height >= rela_atari::kMinIn && height <= kMaxIn && width >= rela_atari::kMinIn && width <= kMaxIn,
             RELA_EINVAL, "rela_atari_features: screens must be 2..512 x 2..512 (got %d x %d)", height, width);
  Tables tab;
  rela_atari::make_tables(tab, height, width);
  const bool vec = (width * 3) % 16 == 0 && ((uintptr_t)screens & 15) == 0;
  ProfScope prof("atari_features", s);
  note_launch("atari_features");
  if (vec)
    hipLaunchKernelGGL(atari_features_kernel<true>, dim3(rows * kTiles), dim3(kThreads), 0, s, screens, height, width,
                       planes, tab);
  else
    hipLaunchKernelGGL(atari_features_kernel<false>, dim3(rows * kTiles), dim3(kThreads), 0, s, screens, height, width,
                       planes, tab);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

int screens_to_stacks(const uint8_t* screens, int height, int width, uint8_t* fresh_planes, uint8_t** restart_dev,
                      const uint8_t* restart_host, bool first, uint8_t* cur_slot, const uint8_t* prev_slot,
                      uint8_t* prev_copy, int rows, hipStream_t s, const char* who) {
  RELA_CHECK(restart_host, RELA_EINVAL, "%s: bad arguments", who);
  RELA_CHECK(screens && fresh_planes, RELA_ESTATE, "%s: no screen input was set (set_screen_input)", who);
  for (int i = 0; i < rows; ++i) {
    RELA_CHECK(restart_host[i] <= 1, RELA_EINVAL, "%s: restart flags are 0 or 1 (row %d: %d)", who, i, restart_host[i]);
    RELA_CHECK(!first || restart_host[i] == 1, RELA_EINVAL,
               "%s: the first observation has no predecessor: every row must be flagged restart (row %d)", who, i);
  }
  if (!first && prev_slot == cur_slot) {  // an evaluation shard acts on one slot: slide from a copy of it
    RELA_CHECK(prev_copy, RELA_ESTATE, "%s: act() twice without post_step()", who);
    RELA_HIP(hipMemcpyAsync(prev_copy, cur_slot, (size_t)rows * 4 * kOut * kOut, hipMemcpyDeviceToDevice, s));
    prev_slot = prev_copy;
  }
  if (!*restart_dev) RELA_HIP(hipMalloc(restart_dev, (size_t)rows));
  RELA_HIP(hipMemcpyAsync(*restart_dev, restart_host, (size_t)rows, hipMemcpyHostToDevice, s));
  int rc = atari_features(screens, rows, height, width, fresh_planes, s);
  if (rc != RELA_OK) return rc;
  return slide_stacks(cur_slot, prev_slot, fresh_planes, *restart_dev, rows, s);
}

}  // namespace rela_amd

extern "C" int rela_atari_features(const uint8_t* screens_dev, int rows, int height, int width, uint8_t* planes_dev,
                                   void* stream) {
  return rela_amd::atari_features(screens_dev, rows, height, width, planes_dev, (hipStream_t)stream);
}
