// atari_screen.hip -- GameState::computeFeature (atari/game_state.h:53-82,122-133) on the device, for the envs that render
// raw screens (rela/screen_env.h):
//   rela_atari_features           [rows][2][H][W][3] u8 screen pairs -> [rows][84][84] u8 features, one launch
//   rela_atari_features_indexed   [rows][2][H][W] u8 palette indices + [rows][256][3] u8 palettes -> the same features
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

// ---- indexed-colour screens: one palette index per pixel, the lookup done here ----
// Per row 2 x 168 x W index bytes are read (53,760 B at 210 x 160, a third of the RGB kernel's) plus the 768 B palette.
// A block stages its row's palette in LDS as one packed word per entry, loads the source rows' indices of both screens
// (16 per load when kVec), looks both up, and writes the per-channel max into the same m[r][3 W] image the RGB kernel
// interpolates from; the pixels are then computed by the same feature_pixel.  (The indices go from the load through
// registers into that image; they are not kept in LDS themselves.)  A three-row block as above would move under 2 KB, and
// that shape is already short-block bound, so a block takes kIdxRows output rows and its threads loop over the
// kIdxRows x 84 pixels.  Measured on one MI355X, 210 x 160, HIP events, median of 50 launches, three alternating passes
// (profiles/r08_screen_indexed.md), against the RGB kernel's 127-128 us at 2,400 rows and 324-325 us at 6,400:
//   rows per block      3          6          12         14
//   2,400 rows [us]   114-116    101-102    102-103    119-121
//   6,400 rows [us]   340-349    273-276    279-288    342-345
// Six wins at 2,400 rows (and at 6,400) and is kept: 14 blocks per env row, 20.5 KB of LDS, 504 pixels per block in two
// passes of 256 threads.  Three-row blocks lose to the RGB kernel at 6,400 rows; 14 rows leave 4.6 passes over the pixels
// with a part-filled last one and fewer blocks per CU.
#ifndef RELA_ATARI_INDEXED_ROWS
#define RELA_ATARI_INDEXED_ROWS 6
#endif
constexpr int kIdxRows = RELA_ATARI_INDEXED_ROWS;  // output rows per block: measured above
constexpr int kIdxTiles = kOut / kIdxRows;
constexpr int kIdxSrc = 2 * kIdxRows;
static_assert(kOut % kIdxRows == 0, "a block takes whole output rows of one env row");

template <bool kVec>
__global__ __launch_bounds__(kThreads) void atari_features_indexed_kernel(const uint8_t* __restrict__ screens,
                                                                          const uint8_t* __restrict__ palettes, int H, int W,
                                                                          uint8_t* __restrict__ planes, const Tables tab) {
  __shared__ float v[256];
  __shared__ uint32_t pal[256];  // R | G << 8 | B << 16
  __shared__ __attribute__((aligned(16))) uint8_t m[kIdxSrc][kMaxIn * 3];
  const int env = blockIdx.x / kIdxTiles, tile = blockIdx.x - env * kIdxTiles;
  const int y0 = tile * kIdxRows;
  const uint8_t* s0 = screens + (size_t)env * 2 * H * W;  // current screen
  const uint8_t* s1 = s0 + (size_t)H * W;                  // previous screen
  {
    const uint8_t* p = palettes + (size_t)env * 768 + 3 * threadIdx.x;
    v[threadIdx.x] = tab.v[threadIdx.x];
    pal[threadIdx.x] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
  __syncthreads();
  if (kVec) {
    const int n16 = W >> 4;
    for (int i = threadIdx.x; i < kIdxSrc * n16; i += kThreads) {
      const int r = i / n16, c = i - r * n16;
      const int y = y0 + (r >> 1);
      const int src = (r & 1) ? tab.h.i1[y] : tab.h.i0[y];
      const uint4 a = reinterpret_cast<const uint4*>(s0 + (size_t)src * W)[c];
      const uint4 b = reinterpret_cast<const uint4*>(s1 + (size_t)src * W)[c];
      const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
      uint4* dst = reinterpret_cast<uint4*>(&m[r][0]) + 3 * c;  // 16 pixels = 48 bytes
      uint32_t o[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // four pixels = three words
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = max_u8x4(pal[(aw[k] >> (8 * j)) & 0xFFu], pal[(bw[k] >> (8 * j)) & 0xFFu]);
        o[3 * k] = p[0] | (p[1] << 24);
        o[3 * k + 1] = (p[1] >> 8) | (p[2] << 16);
        o[3 * k + 2] = (p[2] >> 16) | (p[3] << 8);
      }
      dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
      dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
      dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
    }
  } else {
    for (int i = threadIdx.x; i < kIdxSrc * W; i += kThreads) {
      const int r = i / W, c = i - r * W;
      const int y = y0 + (r >> 1);
      const int src = (r & 1) ? tab.h.i1[y] : tab.h.i0[y];
      const uint32_t p = max_u8x4(pal[s0[(size_t)src * W + c]], pal[s1[(size_t)src * W + c]]);
      m[r][3 * c] = (uint8_t)p;
      m[r][3 * c + 1] = (uint8_t)(p >> 8);
      m[r][3 * c + 2] = (uint8_t)(p >> 16);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kIdxRows * kOut; i += kThreads) {
    const int yl = i / kOut, x = i - yl * kOut, y = y0 + yl;
    planes[(size_t)env * kOut * kOut + y * kOut + x] =
        rela_atari::feature_pixel(v, m[2 * yl], m[2 * yl + 1], tab.w.i0[x], tab.w.i1[x], tab.w.l0[x], tab.w.l1[x],
                                  tab.h.l0[y], tab.h.l1[y]);
  }
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

int atari_features_indexed(const uint8_t* screens, const uint8_t* palettes, int rows, int height, int width, uint8_t* planes,
                           hipStream_t s) {
  RELA_CHECK(screens && palettes && planes && rows >= 1 && rows <= (1 << 30) / kIdxTiles, RELA_EINVAL,
             "rela_atari_features_indexed: bad arguments (rows=%d)", rows);
  RELA_CHECK(height >= rela_atari::kMinIn && height <= kMaxIn && width >= rela_atari::kMinIn && width <= kMaxIn,
             RELA_EINVAL, "rela_atari_features_indexed: screens must be 2..512 x 2..512 (got %d x %d)", height, width);
  Tables tab;
  rela_atari::make_tables(tab, height, width);
  const bool vec = width % 16 == 0 && ((uintptr_t)screens & 15) == 0;
  ProfScope prof("atari_features_indexed", s);
  note_launch("atari_features_indexed");
  if (vec)
    hipLaunchKernelGGL(atari_features_indexed_kernel<true>, dim3(rows * kIdxTiles), dim3(kThreads), 0, s, screens, palettes,
                       height, width, planes, tab);
  else
    hipLaunchKernelGGL(atari_features_indexed_kernel<false>, dim3(rows * kIdxTiles), dim3(kThreads), 0, s, screens, palettes,
                       height, width, planes, tab);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

int screens_to_stacks(const uint8_t* screens, const uint8_t* palettes, int height, int width, uint8_t* fresh_planes, uint8_t** restart_dev,
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
  const int rc = palettes ? atari_features_indexed(screens, palettes, rows, height, width, fresh_planes, s)
                          : atari_features(screens, rows, height, width, fresh_planes, s);
  if (rc != RELA_OK) return rc;
  return slide_stacks(cur_slot, prev_slot, fresh_planes, *restart_dev, rows, s);
}

}  // namespace rela_amd

extern "C" int rela_atari_features(const uint8_t* screens_dev, int rows, int height, int width, uint8_t* planes_dev,
                                   void* stream) {
  return rela_amd::atari_features(screens_dev, rows, height, width, planes_dev, (hipStream_t)stream);
}
extern "C" int rela_atari_features_indexed(const uint8_t* screens_dev, const uint8_t* palettes_dev, int rows, int height,
                                           int width, uint8_t* planes_dev, void* stream) {
  return rela_amd::atari_features_indexed(screens_dev, palettes_dev, rows, height, width, planes_dev, (hipStream_t)stream);
}
